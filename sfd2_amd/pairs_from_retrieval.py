"""hloc/pairs_from_retrieval.py on the device: for every query image the num_matched database images of most similar global
descriptor (sfd2_amd.pairs.retrieval_topk).  Same main() signature, command line and file format.  The descriptor file is read
through the project's store reader (h5py where it imports, else sfd2_amd.h5lite).  With prefixes the reference takes the names in
the arbitrary order of list(set(...)); here they are sorted."""
import argparse
import logging
from pathlib import Path

import numpy as np

from . import colmap_io, feature_io, pairs as P
from .parsers import parse_image_lists_with_intrinsics


def select_names(h5_names, prefix, list_path, model, what):
    if prefix:
        prefix = prefix if isinstance(prefix, str) else tuple(prefix)
        names = [n for n in sorted(h5_names) if n.startswith(prefix)]
        assert len(names)
        return names
    if list_path:
        return [n for n, _ in parse_image_lists_with_intrinsics(list_path)]
    if model:
        images = colmap_io.read_images_binary(Path(model) / 'images.bin')
        return [i.name for i in images.values()]
    raise ValueError(f'Provide either prefixes of {what} names, or path to lists of {what} images'
                     + (', or path to a COLMAP model.' if what == 'DB' else '.'))


def main(descriptors, output, num_matched, query_prefix=None, query_list=None, db_prefix=None, db_list=None, db_model=None):
    logging.info('Extracting image pairs from a retrieval database.')
    store = feature_io.open_store(str(descriptors), 'r')
    try:
        h5_names = list(store.keys())
        db_names = select_names(h5_names, db_prefix, db_list, db_model, 'DB')
        query_names = select_names(h5_names, query_prefix, query_list, None, 'query')

        def array_from_names(names):
            return np.stack([np.asarray(store[i]['global_descriptor'].__array__(), dtype=np.float32) for i in names], 0)

        db_desc = array_from_names(db_names)
        query_desc = array_from_names(query_names)
    finally:
        store.close()
    idx, _ = P.retrieval_topk(query_desc, db_desc, num_matched)
    pairs = P.name_pairs(query_names, db_names, idx)

    logging.info(f'Found {len(pairs)} pairs.')
    P.write_pairs(output, pairs)


def make_parser():
    """The reference's command line."""
    parser = argparse.ArgumentParser()
    parser.add_argument('--descriptors', type=Path, required=True)
    parser.add_argument('--output', type=Path, required=True)
    parser.add_argument('--num_matched', type=int, required=True)
    parser.add_argument('--query_prefix', type=str, nargs='+')
    parser.add_argument('--query_list', type=Path)
    parser.add_argument('--db_prefix', type=str, nargs='+')
    parser.add_argument('--db_list', type=Path)
    parser.add_argument('--db_model', type=Path)
    return parser


if __name__ == "__main__":
    args = make_parser().parse_args()
    main(**args.__dict__)
