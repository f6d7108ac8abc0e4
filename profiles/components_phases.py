#!/usr/bin/env python3
"""Phases of connected_components and flood_fill_3d: the golden bunny tiled 174 times (1,003,284 faces; as tiled, and with
vertex ids and face order permuted), int64 and int32 faces; a 512^3 int32 grid holding the bunny's shell at 500 voxels across, filled from
the outside corner and from a shell voxel. Device-resident torch input. set_timing(2) makes the library bracket its phases with HIP events
(last_stats(): ms_index = union / runs and unions, ms_search = flatten (and rank), ms_tie = labels and counts / the filled copy); warm-up
calls, then the median and the range of the timed calls. Needs a GPU; prints its lines and writes them to --out.

    python profiles/components_phases.py [--what cc|fill|both] [--out FILE]"""
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
ap.add_argument("--what", default="both", choices=["cc", "fill", "both"])
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


def timed(fn, warm=5, reps=20):
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
        rows.append([st["ms_index"], st["ms_search"], st["ms_tie"], st["ms_total"]])
    r = np.array(rows)
    return np.median(r, axis=0), r.min(axis=0), r.max(axis=0), float(np.median(wall)), st


v = np.load(os.path.join(ROOT, "tests", "golden", "bunny_v.npy")).astype(np.float32)
f = np.load(os.path.join(ROOT, "tests", "golden", "bunny_f.npy")).astype(np.int64)
pcu.set_timing(2)

# ---- connected_components: 174 bunnies, vertex ids and face order permuted (seed 1) so that neighbours in the mesh are not neighbours in memory
copies = 174
V = np.concatenate([v + k for k in range(copies)])
F = np.concatenate([f + k * len(v) for k in range(copies)])
rng = np.random.default_rng(1)
for name, FF in () if args.what == "fill" else (("tiled", F), ("tiled, ids and faces permuted", rng.permutation(len(V))[F][rng.permutation(len(F))])):
    for dt in (torch.int64, torch.int32):
        tv = torch.from_numpy(V).cuda()
        tf = torch.from_numpy(np.ascontiguousarray(FF)).to(device="cuda", dtype=dt)
        med, lo, hi, wall, st = timed(lambda: pcu.connected_components(tv, tf))
        nb = tf.element_size()
        must = len(F) * 3 * nb + len(F) * nb + len(V) * nb + len(F) * nb        # faces read once by the union, f[:, 0] again, cv and cf written
        parent = len(V) * 4 * 8                                                # parent init, flatten r/w, flag, scan r/w, labels: ~8 passes of 4 B per vertex
        say(f"connected_components [{name}, {str(dt)[6:]}]: faces {len(F)} vertices {len(V)} components {st['n_escalated']}")
        say(f"  ms median (min..max) of 20: union {med[0]:.3f} ({lo[0]:.3f}..{hi[0]:.3f})  flatten+rank {med[1]:.3f} ({lo[1]:.3f}..{hi[1]:.3f})"
            f"  labels+counts {med[2]:.3f} ({lo[2]:.3f}..{hi[2]:.3f})  total {med[3]:.3f}  host wall {wall:.3f}")
        say(f"  bytes by construction: faces and outputs {must / 1e6:.1f} MB, parent / flag / scan passes ~{parent / 1e6:.1f} MB")

if args.what == "cc":
    out.close()
    sys.exit(0)
# ---- flood_fill_3d: the bunny's shell at 500 voxels across in a 512^3 int32 grid, filled from the outside corner
size = float((v.max(axis=0) - v.min(axis=0)).max()) / 500
ijk = pcu.voxelize_triangle_mesh(torch.from_numpy(v).cuda(), torch.from_numpy(f).cuda(), size, v.min(axis=0).astype(np.float64))
lo_ = ijk.min(dim=0).values
assert int((ijk.max(dim=0).values - lo_).max()) < 510
grid = torch.zeros((512, 512, 512), dtype=torch.int32, device="cuda")
idx = (ijk - lo_ + 1).long()
grid[idx[:, 0], idx[:, 1], idx[:, 2]] = 1
N = grid.numel()
for name, seed in (("outside, from corner (0,0,0)", (0, 0, 0)), ("the shell itself", tuple(int(c) for c in idx[0].tolist()))):
    med, lo, hi, wall, st = timed(lambda: pcu.flood_fill_3d(grid, seed, 2), warm=3, reps=10)
    say(f"flood_fill_3d [512^3 int32, bunny shell of {len(ijk)} voxels, seed {name}]: cells {st['n_queries']} region {st['n_escalated']}")
    say(f"  ms median (min..max) of 10: runs+unions {med[0]:.3f} ({lo[0]:.3f}..{hi[0]:.3f})  flatten {med[1]:.3f} ({lo[1]:.3f}..{hi[1]:.3f})"
        f"  filled copy {med[2]:.3f} ({lo[2]:.3f}..{hi[2]:.3f})  total {med[3]:.3f}  host wall {wall:.3f}")
    say(f"  bytes by construction: grid read once + written once {2 * N * 4 / 1e6:.0f} MB; as built the grid is read by three launches and parent "
        f"(4 B per cell) is written by init, read and written by flatten, read by the copy: {(3 + 1 + 4) * N * 4 / 1e6:.0f} MB plus the unions' traffic")
    say(f"  total over those {(3 + 1 + 4) * N * 4 / 1e6:.0f} MB: {(3 + 1 + 4) * N * 4 / med[3] / 1e6:.0f} GB/s")
res = pcu.flood_fill_3d(grid, (0, 0, 0), 2)
say(f"interior cells (neither shell nor reached): {int((res == 0).sum())}")
out.close()
