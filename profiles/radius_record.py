"""The record of DESIGN.md row f18: radius_search / radius_count of 1M uniform float32 queries against 1M uniform float32 points in the unit
cube, both device-resident torch tensors, at the two radii where the mean row length is about 16 and about 64. The radii come from the ball's
volume; the mean row length is then measured on a 1/64 sample of the queries by a brute force written here in torch (separate multiplies and
adds in float32, `d2 < r2`), and the library's counts on that sample must equal it. Device milliseconds between two events around calls on
the current stream, every shape warmed up three times, the median and the range of 15 repeats; then one call per shape with phase timing (device
time between events: ms_index = index, record order, query order; ms_search = count pass; ms_kernel_search = scan, the one wait and the fill
pass; ms_tie = row sort). Beside them, in the same process, k_nearest_neighbors at 1M against 1M with k = 16, which returns the amount of data
of the smaller radius. Writes profiles/radius_record.json (or the path given)."""
import json
import math
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import numpy as np
import torch
import point_cloud_utils_amd as pcu

N = 1_000_000
REPS = 15


def device_ms(fn, reps=REPS, warmup=3):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(); fn(); b.record(); torch.cuda.synchronize()
        ts.append(a.elapsed_time(b))
    return {"ms_median": round(float(np.median(ts)), 3), "ms_min": round(min(ts), 3), "ms_max": round(max(ts), 3)}


def phases(fn):
    pcu.set_timing(2)
    fn(); torch.cuda.synchronize()
    st = pcu.last_stats()
    pcu.set_timing(0)
    return {k: round(v, 3) for k, v in st.items() if k.startswith("ms_") and v}, st


def brute_counts(q, p, radius):
    r2 = torch.tensor(np.float32(radius) * np.float32(radius), device=q.device)
    out = []
    for a in range(0, len(q), 256):
        d = q[a:a + 256, None, :] - p[None, :, :]
        sq = d * d
        d2 = (sq[..., 0] + sq[..., 1]) + sq[..., 2]
        out.append((d2 < r2).sum(1))
    return torch.cat(out)


def main(path):
    q = torch.from_numpy(np.random.default_rng(21).random((N, 3), dtype=np.float32)).cuda()
    p = torch.from_numpy(np.random.default_rng(22).random((N, 3), dtype=np.float32)).cuda()
    out = {"queries": N, "dataset": N, "dtype": "float32", "device": torch.cuda.get_device_name(0), "reps": REPS}
    out["k_nearest_neighbors_k16"] = device_ms(lambda: pcu.k_nearest_neighbors(q, p, 16))
    print("knn16", out["k_nearest_neighbors_k16"], flush=True)
    sample = q[::64].contiguous()
    for want in (16, 64):
        radius = (3.0 * want / (4.0 * math.pi * N)) ** (1.0 / 3.0)
        bc = brute_counts(sample, p, radius)
        lc = pcu.radius_count(sample, p, radius)
        r = {"radius": radius, "sample_mean_row_length": round(float(bc.double().mean()), 3), "sample_counts_equal_brute_force": bool((bc == lc).all())}
        off, idx, d = pcu.radius_search(q, p, radius)
        total = int(off[-1])
        r["neighbours"] = total
        r["max_row_length"] = int((off[1:] - off[:-1]).max())
        r["bytes_returned"] = 8 * (N + 1) + total * (8 + 4)
        del off, idx, d
        r["radius_search_sorted"] = device_ms(lambda: pcu.radius_search(q, p, radius))
        r["radius_search_unsorted"] = device_ms(lambda: pcu.radius_search(q, p, radius, sort_results=False))
        r["radius_count"] = device_ms(lambda: pcu.radius_count(q, p, radius))
        r["phases_sorted"], st = phases(lambda: pcu.radius_search(q, p, radius))
        r["rows_sorted_in_lds"], r["rows_sorted_by_radix"] = int(st["n_tie_flagged"]), int(st["n_tie_true"])
        with pcu.DatasetIndex(p, k_hint=16) as index:
            r["index_k_hint16_radius_search_sorted"] = device_ms(lambda: index.radius_search(q, radius))
            r["index_k_hint16_radius_count"] = device_ms(lambda: index.radius_count(q, radius))
        out["mean_%d" % want] = r
        print(want, r, flush=True)
    with open(path, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else os.path.join(os.path.dirname(os.path.abspath(__file__)), "radius_record.json"))
