"""Global descriptors for retrieval: one VLAD vector per image over its SFD2 descriptors (sfd2_amd.vlad), written
as the `global_descriptor` dataset that sfd2_amd.pairs_from_retrieval reads.  The project's own stage, not a port: the reference
takes NetVLAD descriptors extracted by another project.

With --train the k-means vocabulary is learnt from the selected training images and written to --vocabulary (.npz); without it the
vocabulary is loaded.  Names are selected as pairs_from_retrieval.select_names does: prefixes (sorted names), or a list file; with
neither, every image of the store.  The descriptors (float64 [128, N] per image) are read by at most READ_THREADS reader threads
and aggregated in batches of whole images: a batch's fp32 rows plus its output vectors take at most BATCH_BYTES (256 MiB), or it
holds one image."""
import argparse
import logging
from concurrent.futures import ThreadPoolExecutor
from pathlib import Path

import numpy as np

from . import feature_io, vlad
from .pairs_from_retrieval import select_names
from .triangulation import READ_THREADS

BATCH_BYTES = 256 << 20


def _select(h5_names, prefix, list_path):
    if prefix or list_path:
        return select_names(h5_names, prefix, list_path, None, 'image')
    return sorted(h5_names)


def main(features, output, vocabulary, train=False, train_prefix=None, train_list=None, prefix=None, image_list=None, k=64, max_iters=20,
         max_train=1 << 20, seed=0, norm="intra"):
    if norm not in vlad.NORMS:
        raise ValueError(f"norm must be one of {sorted(vlad.NORMS)}, got {norm!r}")
    feats = feature_io.open_store(str(features), 'r')
    try:
        h5_names = list(feats.keys())
        if train:
            train_names = _select(h5_names, train_prefix, train_list)
            logging.info(f'Learning a vocabulary of {k} words from {len(train_names)} images.')
            voc = vlad.train_vocabulary(feats, train_names, k=k, max_train=max_train, max_iters=max_iters, seed=seed)
            vlad.save_vocabulary(vocabulary, voc["centroids"], norm=norm, seed=seed, iters_run=voc["iters_run"])
            centroids = voc["centroids"]
        else:
            voc = vlad.load_vocabulary(vocabulary)
            centroids, norm = voc["centroids"], voc["norm"]
        names = _select(h5_names, prefix, image_list)
        logging.info(f'Aggregating the global descriptors of {len(names)} images.')
        row_bytes = 4 * vlad.DIM
        pend_names, pend_rows, used = [], [], 0

        def flush(out):
            offsets = np.concatenate([[0], np.cumsum([len(r) for r in pend_rows])]).astype(np.int64)
            desc = vlad.aggregate(np.concatenate(pend_rows, 0), offsets, centroids, norm=norm)
            for name, d in zip(pend_names, desc):
                feature_io.write_features(out, name, {"global_descriptor": np.ascontiguousarray(d, dtype=np.float32)})
            pend_names.clear()
            pend_rows.clear()

        with ThreadPoolExecutor(max_workers=READ_THREADS) as pool, feature_io.open_store(str(output), 'w') as out:
            for w in range(0, len(names), 4 * READ_THREADS):         # a window of reads in flight, so memory follows the batch bound
                window = names[w:w + 4 * READ_THREADS]
                for name, rows in zip(window, pool.map(lambda n: vlad._descriptors(feats[n]), window)):
                    need = row_bytes * (len(rows) + len(centroids))
                    if pend_names and used + need > BATCH_BYTES:
                        flush(out)
                        used = 0
                    pend_names.append(name)
                    pend_rows.append(rows)
                    used += need
            if pend_names:
                flush(out)
    finally:
        feats.close()
    logging.info('Finished writing the global descriptors.')


def make_parser():
    parser = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    parser.add_argument('--features', type=Path, required=True, help='feature store with `descriptors` per image')
    parser.add_argument('--output', type=Path, required=True, help='store that receives `global_descriptor` per image')
    parser.add_argument('--vocabulary', type=Path, required=True, help='.npz vocabulary: written with --train, read without')
    parser.add_argument('--train', action='store_true', help='learn the vocabulary before aggregating')
    parser.add_argument('--train_prefix', type=str, nargs='+')
    parser.add_argument('--train_list', type=Path)
    parser.add_argument('--prefix', type=str, nargs='+')
    parser.add_argument('--image_list', type=Path)
    parser.add_argument('--k', type=int, default=64, help=f'words of the vocabulary, 1 .. {vlad.MAX_K}')
    parser.add_argument('--max_iters', type=int, default=20)
    parser.add_argument('--max_train', type=int, default=1 << 20, help='training rows kept (evenly thinned beyond)')
    parser.add_argument('--seed', type=int, default=0)
    parser.add_argument('--norm', type=str, default='intra', choices=sorted(vlad.NORMS))
    return parser


if __name__ == "__main__":
    logging.basicConfig(level=logging.INFO)
    args = make_parser().parse_args()
    main(**args.__dict__)
