"""hloc/pairs_from_poses.py on the device: for every image of a COLMAP model the num_matched nearest images whose orientation
differs by less than rotation_threshold degrees (sfd2_amd.pairs.poses_topk).  Same main() signature, command line and file format.
Positions are the reference's (-R t, pairs_from_poses.py:25-26).  Where the reference raises for num_matched >= the number of images,
an image here simply gets every valid other image."""
import argparse
import logging
from pathlib import Path

from . import colmap_io, pairs as P

DEFAULT_ROT_THRESH = 30  # in degrees


def main(model, output, num_matched, rotation_threshold=DEFAULT_ROT_THRESH):
    logging.info('Reading the COLMAP model...')
    images = colmap_io.read_images_binary(Path(model) / 'images.bin')

    logging.info(f'Obtaining pairwise distances between {len(images)} images...')
    ids, idx, _, n_found = P.poses_topk(images, num_matched, rotation_threshold)
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
    parser.add_argument('--rotation_threshold', default=DEFAULT_ROT_THRESH, type=float)
    return parser


if __name__ == "__main__":
    args = make_parser().parse_args()
    main(**args.__dict__)
