"""The text files the localisation commands share (hloc/utils/parsers.py, it_loc/parsers.py, it_loc/loc_tools.py): query lists with
intrinsics and retrieval results."""
import logging
from pathlib import Path

import numpy as np


def parse_image_lists_with_intrinsics(paths):
    """hloc/utils/parsers.py:7-25: the names (first column) of every list file the glob matches, with the rest of each line as
    (camera model, width, height, params)."""
    paths = Path(paths)
    files = list(Path(paths.parent).glob(paths.name))
    assert len(files) > 0
    results = []
    for lfile in files:
        with open(lfile, 'r') as f:
            raw_data = f.readlines()
        logging.info(f'Importing {len(raw_data)} queries in {lfile.name}')
        for data in raw_data:
            data = data.strip('\n').split(' ')
            name, camera_model, width, height = data[:4]
            results.append((name, (camera_model, int(width), int(height), np.array(data[4:], float))))
    assert len(results) > 0
    return results


def camera_dict(qinfo):
    """The dict the pose code takes (it_loc/localize_cv2.py:684-689) from a list entry's (model, width, height, params)."""
    camera_model, width, height, params = qinfo
    return {'model': camera_model, 'width': width, 'height': height, 'params': params}


def query_cameras(paths):
    """[(query name, camera dict)] of a list with intrinsics."""
    return [(name, camera_dict(info)) for name, info in parse_image_lists_with_intrinsics(paths)]


def read_retrieval_results(path):
    """it_loc/loc_tools.py:38-51: query name -> the retrieved names in file order; `name no_match` lines are skipped."""
    output = {}
    with open(path, "r") as f:
        for line in f.readlines():
            p = line.strip("\n").split(" ")
            if p[1] == "no_match":
                continue
            output.setdefault(p[0], []).append(p[1])
    return output
