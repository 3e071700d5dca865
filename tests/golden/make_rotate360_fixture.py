#!/usr/bin/env python
"""Generates tests/golden/rotate360_frames.npz from the reference's camera preset cameras/rotate360.json: the number of
frames and the camera-to-world matrices of every 24th frame (the 30 views of the bench's rotate360 path).  Needs the
reference checkout (oracle/ref_python.py REF); tests/test_oracle_golden.py reads only the fixture.

    python tests/golden/make_rotate360_fixture.py
"""
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

from oracle.ref_python import REF           # noqa: E402

STRIDE, VIEWS = 24, 30


def main():
    frames = json.load(open(os.path.join(REF, "cameras", "rotate360.json")))["frames"]
    c2w = np.array([frames[STRIDE * k]["transform_matrix"] for k in range(VIEWS)], dtype=np.float64)
    path = os.path.join(HERE, "rotate360_frames.npz")
    np.savez_compressed(path, n_frames=np.int64(len(frames)), stride=np.int64(STRIDE), transform_matrix=c2w)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
