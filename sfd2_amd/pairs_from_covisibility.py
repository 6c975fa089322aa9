"""hloc/pairs_from_covisibility.py on the device: for every image of a COLMAP model the num_matched images that share the most 3D
points with it (sfd2_amd.pairs.covisibility_topk).  Same main() signature, command line and file format.  Among images of equal
count the reference's order is that of an unstable sort; here it is the model's image order."""
import argparse
import logging
from pathlib import Path

from . import colmap_io, pairs as P


def main(model, output, num_matched):
    logging.info('Reading the COLMAP model...')
    _, images, points3D = colmap_io.read_model(Path(model))

    logging.info('Extracting image pairs from covisibility info...')
    ids, idx, _, n_found = P.covisibility_topk(images, points3D, num_matched)
    for iid, n in zip(ids, n_found):
        if n == 0:
            logging.info(f'Image {iid} does not have any covisibility.')
    names = [images[i].name for i in ids]
    pairs = P.name_pairs(names, names, idx, n_found)

    logging.info(f'Found {len(pairs)} pairs.')
    P.write_pairs(output, pairs)


def make_parser():
    """The reference's command line."""
    parser = argparse.ArgumentParser()
    parser.add_argument('--model', required=True, type=Path)
    parser.add_argument('--output', required=True, type=Path)
    parser.add_argument('--num_matched', required=True, type=int)
    return parser


if __name__ == "__main__":
    args = make_parser().parse_args()
    main(**args.__dict__)
