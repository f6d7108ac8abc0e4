#!/usr/bin/env python3
"""Generates tests/golden/cube_twist_v.npy (float64) and cube_twist_f.npy (int32) from the reference's data/cube_twist.obj: the mesh of the
reference's own ray test (tests/test_examples.py:570-608). Run where the reference's checkout exists:
    python tests/golden/make_golden_rays.py [path/to/cube_twist.obj]"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))


def main():
    path = sys.argv[1] if len(sys.argv) > 1 else "/root/reference/data/cube_twist.obj"
    v, f = [], []
    with open(path) as fh:
        for line in fh:
            w = line.split()
            if not w:
                continue
            if w[0] == "v":
                v.append([float(x) for x in w[1:4]])
            elif w[0] == "f":
                assert len(w) == 4, "triangles only"
                f.append([int(x.split("/")[0]) - 1 for x in w[1:4]])
    v, f = np.array(v, dtype=np.float64), np.array(f, dtype=np.int32)
    assert v.shape == (6146, 3) and f.shape == (12288, 3) and f.min() == 0 and f.max() == len(v) - 1
    np.save(os.path.join(HERE, "cube_twist_v.npy"), v)
    np.save(os.path.join(HERE, "cube_twist_f.npy"), f)
    print("wrote cube_twist_v.npy", v.shape, "cube_twist_f.npy", f.shape)


if __name__ == "__main__":
    main()
