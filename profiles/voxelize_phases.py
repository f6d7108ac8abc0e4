#!/usr/bin/env python3
"""Phases of one voxelize_triangle_mesh call: a seeded torus of about 1M faces with radial noise at about 512 voxels
across, float32, device-resident torch input. set_timing(2) makes the library bracket its phases with HIP events (last_stats(): ms_index =
extent pass and scan, ms_search = test pass, ms_tie = emit pass, ms_kernel_search = sort and unique); one warm-up call, then the median and
the range of 10 calls, and the candidates tested per second of test-pass time. Needs a GPU; prints one JSON line.

    python profiles/voxelize_phases.py [--quads 708] [--across 512] [--calls 10] [--out FILE]"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def torus(q, seed=20240612):
    """q x q quads, two faces each, on a torus of radii 1 and 0.4 whose tube radius carries seeded noise of 2 %."""
    rng = np.random.default_rng(seed)
    a, b = np.meshgrid(np.arange(q) * (2 * np.pi / q), np.arange(q) * (2 * np.pi / q), indexing="ij")
    r = 0.4 * (1.0 + 0.02 * rng.standard_normal((q, q)))
    v = np.stack([(1.0 + r * np.cos(b)) * np.cos(a), (1.0 + r * np.cos(b)) * np.sin(a), r * np.sin(b)], axis=-1).reshape(-1, 3)
    i, j = np.meshgrid(np.arange(q), np.arange(q), indexing="ij")
    i1, j1 = (i + 1) % q, (j + 1) % q
    p00, p10, p01, p11 = i * q + j, i1 * q + j, i * q + j1, i1 * q + j1
    f = np.concatenate([np.stack([p00, p10, p11], axis=-1).reshape(-1, 3), np.stack([p00, p11, p01], axis=-1).reshape(-1, 3)])
    return v.astype(np.float32), f.astype(np.int64)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--quads", type=int, default=708)
    ap.add_argument("--across", type=int, default=512)
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    import point_cloud_utils_amd as pcu
    v, f = torus(a.quads)
    size = float((v.max(axis=0) - v.min(axis=0)).max()) / a.across
    origin = (v.min(axis=0).astype(np.float64) - size / 4).tolist()
    tv, tf = torch.from_numpy(v).cuda(), torch.from_numpy(f).cuda()
    pcu.set_timing(2)
    rows = []
    for it in range(a.calls + 1):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        ijk = pcu.voxelize_triangle_mesh(tv, tf, size, origin)
        torch.cuda.synchronize()
        wall = (time.perf_counter() - t0) * 1e3
        st = pcu.last_stats()
        if it:                                             # (the first call is the warm-up)
            rows.append([st["ms_index"], st["ms_search"], st["ms_tie"], st["ms_kernel_search"], st["ms_total"], wall])
    rows = np.array(rows)
    med, lo, hi = np.median(rows, axis=0), rows.min(axis=0), rows.max(axis=0)
    names = ["extent_scan", "test", "emit", "sort_unique", "events_total", "wall"]
    res = {"faces": int(len(f)), "across": a.across, "voxel_size": size, "candidates": int(st["n_queries"]), "kept_pairs": int(st["n_escalated"]),
           "voxels": int(ijk.shape[0]), "calls": a.calls,
           "ms_median": {n: round(float(x), 4) for n, x in zip(names, med)},
           "ms_range": {n: [round(float(x), 4), round(float(y), 4)] for n, x, y in zip(names, lo, hi)},
           "candidates_per_second_of_test_pass": float(st["n_queries"]) / (float(med[1]) * 1e-3)}
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        open(a.out, "w").write(line + "\n")


if __name__ == "__main__":
    main()
