"""The record of DESIGN.md row f24 -- a record, not a gate: milliseconds per call of compute_point_cloud_fpfh at 1M shuffled rows of a unit sphere
with outward normals, float32 and float64, at radii that give about 16 and about 64 neighbours, device-resident torch tensors. Beside every
figure, from the same commit and the same cloud: radius_count(P, P, radius) -- the same grid and the same ball walk with nothing to compute
per member --, the ratio to it, the mean neighbour count, the waves of walk 1 that staged their union box, and the call's phases from
set_timing(2) (grid and record order, walk 1, walk 2). Then match_point_features at 100k x 100k rows, D = 33, float32, on FPFH-like rows,
with the achieved share of the vector-ALU peak: 3 n m D operations (a subtract, a multiply, an add per column and pair) over the call's time,
against the 157.3 TFLOP/s the data sheet gives for float32 fused multiply-adds -- separate multiplies and adds can reach half of that.
Device milliseconds between two events around the call on the current stream, two warm-ups, the median and the range of 7 repeats.
Writes profiles/fpfh_record.json (or the path given)."""
import json
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import numpy as np
import torch
import point_cloud_utils_amd as pcu

N = 1_000_000
M = 100_000
REPS = 7
PEAK_F32_TFLOPS = 157.3


def device_ms(fn, reps=REPS, warmup=2):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(); fn(); b.record(); torch.cuda.synchronize()
        ts.append(a.elapsed_time(b))
    return {"ms_median": round(float(np.median(ts)), 3), "ms_min": round(min(ts), 3), "ms_max": round(max(ts), 3)}


def record_fpfh(dtype):
    rng = np.random.default_rng(24)
    v = rng.standard_normal((N, 3))
    v /= np.linalg.norm(v, axis=1, keepdims=True)
    p = torch.from_numpy(v.astype(dtype)).cuda()
    out = {}
    for label, radius in (("about_16_neighbours", 0.008), ("about_64_neighbours", 0.016)):
        feat, cnt = pcu.compute_point_cloud_fpfh(p, p, radius, return_spfh=True)
        st = pcu.last_stats()
        neighbours = float((pcu.radius_count(p, p, radius) - 1).double().mean())
        pairs = float(cnt[:, :11].sum(dim=1).double().mean())
        old = pcu.set_timing(2)
        try:
            phases = []
            for _ in range(3):
                pcu.compute_point_cloud_fpfh(p, p, radius)
                s = pcu.last_stats()
                phases.append((s["ms_index"], s["ms_search"], s["ms_kernel_search"], s["ms_total"]))
        finally:
            pcu.set_timing(old)
        ph = np.median(np.asarray(phases), axis=0)
        call = device_ms(lambda: pcu.compute_point_cloud_fpfh(p, p, radius))
        count = device_ms(lambda: pcu.radius_count(p, p, radius))
        out[label] = {"radius": radius, "call": call, "radius_count": count, "call_over_radius_count": round(call["ms_median"] / count["ms_median"], 2),
                      "mean_neighbours": round(neighbours, 2), "mean_pairs": round(pairs, 2),
                      "walk1_waves_staged": st["n_tie_flagged"], "walk1_waves_per_lane": st["n_tie_true"],
                      "phases_ms": {"index": round(float(ph[0]), 3), "walk1": round(float(ph[1]), 3), "walk2": round(float(ph[2]), 3), "total": round(float(ph[3]), 3)}}
        print(np.dtype(dtype).name, label, out[label], flush=True)
    return out


def record_match():
    rng = np.random.default_rng(25)
    a = torch.from_numpy((rng.random((M, 33)) * 100.0).astype(np.float32)).cuda()
    b = torch.from_numpy((rng.random((M, 33)) * 100.0).astype(np.float32)).cuda()
    one = device_ms(lambda: pcu.match_point_features(a, b))
    both = device_ms(lambda: pcu.match_point_features(a, b, mutual=True))
    ops = 3.0 * M * M * 33
    out = {"rows": [M, M], "D": 33, "dtype": "float32", "call": one, "call_mutual": both, "operations": ops,
           "tflops": round(ops / (one["ms_median"] * 1e-3) / 1e12, 2),
           "share_of_f32_vector_peak": round(ops / (one["ms_median"] * 1e-3) / 1e12 / PEAK_F32_TFLOPS, 3)}
    print("match", out, flush=True)
    return out


def main(path):
    out = {"what": "a record, not a gate: nothing in the tests or the benchmark depends on these figures",
           "points": N, "cloud": "unit sphere, shuffled rows, outward normals", "device": torch.cuda.get_device_name(0), "reps": REPS}
    for dtype in (np.float32, np.float64):
        out[np.dtype(dtype).name] = record_fpfh(dtype)
    out["match_point_features"] = record_match()
    with open(path, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else os.path.join(os.path.dirname(os.path.abspath(__file__)), "fpfh_record.json"))
