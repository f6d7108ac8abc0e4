#!/usr/bin/env python3
"""Phases of sparse_voxel_grid_to_hex_mesh and marching_cubes_sparse_voxel_grid: a full block of 128^3 voxels (2,097,152
cubes, 2,146,689 hex vertices), the field |x - centre| - 0.35 * extent in float32, isovalue 0, device-resident torch input. set_timing(2)
makes the library bracket its phases with HIP events (last_stats(); hex mesh: ms_index = codes, ms_search = sort, ms_tie = unique,
ms_kernel_search = vertices and cubes; marching cubes: ms_index = checks, classification and scan, ms_search = keys, ms_tie = sort,
ms_kernel_search = unique, the wait for #v, vertices and faces); warm-up calls, then the median and the range of the timed calls. Needs a
GPU; prints its lines and writes them to --out.

    python profiles/marching_cubes_phases.py [--side 128] [--out FILE]"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402
import point_cloud_utils_amd as pcu  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--side", type=int, default=128)
ap.add_argument("--out", default=os.devnull)
args = ap.parse_args()
if os.path.dirname(os.path.abspath(args.out)):
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
out = open(args.out, "w")


def say(*a):
    line = " ".join(str(x) for x in a)
    print(line, flush=True)
    out.write(line + "\n")
    out.flush()


def timed(fn, warm=3, reps=10):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    rows, wall = [], []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        wall.append((time.perf_counter() - t0) * 1e3)
        st = pcu.last_stats()
        rows.append([st["ms_index"], st["ms_search"], st["ms_tie"], st["ms_kernel_search"], st["ms_total"]])
    r = np.array(rows)
    return np.median(r, axis=0), r.min(axis=0), r.max(axis=0), float(np.median(wall)), st


def row(names, med, lo, hi):
    return "  ".join(f"{n} {med[i]:.3f} ({lo[i]:.3f}..{hi[i]:.3f})" for i, n in enumerate(names))


n = args.side
ax = torch.arange(n, dtype=torch.int32, device="cuda")
ijk = torch.stack(torch.meshgrid(ax, ax, ax, indexing="ij"), dim=-1).reshape(-1, 3).contiguous()
pcu.set_timing(2)
size = 1.0 / n
med, lo, hi, wall, st = timed(lambda: pcu.sparse_voxel_grid_to_hex_mesh(ijk, size, (0.0, 0.0, 0.0), np.float32))
say(f"sparse_voxel_grid_to_hex_mesh [{n}^3 voxels, int32, float32 vertices]: voxels {st['n_queries']} vertices {st['n_escalated']}")
say("  ms median (min..max) of 10: " + row(["codes", "sort (63 bits)", "unique", "vertices+cubes", "first to last event"], med, lo, hi) + f"  host wall {wall:.3f}")

P, cubes = pcu.sparse_voxel_grid_to_hex_mesh(ijk, size, (0.0, 0.0, 0.0), np.float32)
S = (torch.linalg.norm(P - P.mean(dim=0), dim=1) - 0.35).contiguous()
for name, cc in (("int64 cubes", cubes), ("int32 cubes", cubes.to(torch.int32))):
    med, lo, hi, wall, st = timed(lambda: pcu.marching_cubes_sparse_voxel_grid(S, P, cc, 0.0))
    v, f = pcu.marching_cubes_sparse_voxel_grid(S, P, cc, 0.0)
    say(f"marching_cubes_sparse_voxel_grid [{name}, float32]: cubes {st['n_queries']} faces {st['n_escalated']} vertices {len(v)}")
    say("  ms median (min..max) of 10: " + row(["checks+classify+scan", "keys", "sort", "unique+wait+write", "first to last event"], med, lo, hi)
        + f"  host wall {wall:.3f}")
    nb = cc.element_size()
    must = len(cc) * 8 * nb + len(P) * 16 + len(v) * 12 + len(f) * 3 * nb
    say(f"  bytes by construction: cubes, scalars and coordinates read once, v and f written once: {must / 1e6:.1f} MB")
out.close()
