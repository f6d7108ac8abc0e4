"""The record of DESIGN.md row f22 -- a record, not a gate: milliseconds per call of segment_point_cloud_plane at 1M points, float32 and
float64, 100, 1000 and 10000 hypotheses, with and without refit, device-resident torch tensors; and the (row, hypothesis) tests per second
these times amount to. The cloud is the planted plane of tests/test_plane_contract.py (60 % of the rows on a noisy plane). Two yardsticks stand
beside every figure. The arithmetic floor: a test is 8 float64 operations (3 multiplies, 2 adds, 1 subtract, 1 multiply, 1 compare), so
n * H * 8 flop over the chip's peak vector float64 rate -- PEAK_FP64_VECTOR below, 78.6 TFLOP/s, the "Peak Double Precision (FP64) vector"
figure of AMD's public MI355X data sheet (half the 157.3 TFLOP/s vector float32 figure); that rate counts a fused multiply-add as two
operations, which the contract forbids, so a kernel of separate multiplies and adds can reach half of it at the most. And radius_count of the
cloud against itself at radius 0.01, the library's familiar fixed-radius pass over the same rows. Device milliseconds between two events
around the call on the current stream, three warm-ups, the median and the range of 15 repeats (5 at 10000 hypotheses). Writes
profiles/plane_record.json (or the path given)."""
import json
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tests"))
import numpy as np
import torch
import point_cloud_utils_amd as pcu
from test_plane_contract import planted

N = 1_000_000
REPS = 15
THR = 0.01
PEAK_FP64_VECTOR = 78.6e12          # flop/s
FLOP_PER_TEST = 8


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


def record(dtype):
    cloud = torch.from_numpy(planted(N, dtype)).cuda()
    out = {"radius_count_self_r0.01": device_ms(lambda: pcu.radius_count(cloud, cloud, THR))}
    for H in (100, 1000, 10000):
        floor_ms = N * H * FLOP_PER_TEST / PEAK_FP64_VECTOR * 1e3
        for refit in (False, True):
            r = pcu.segment_point_cloud_plane(cloud, THR, H, 3, refit)
            launches = pcu.last_stats()["n_passes"]
            t = device_ms(lambda: pcu.segment_point_cloud_plane(cloud, THR, H, 3, refit), reps=REPS if H < 10000 else 5)
            out[f"H{H}_refit_{'on' if refit else 'off'}"] = {
                "call": t, "tests_per_second": round(N * H / (t["ms_median"] * 1e-3), 0), "arithmetic_floor_ms": round(floor_ms, 4),
                "call_over_floor": round(t["ms_median"] / floor_ms, 2), "scoring_launches": launches, "status": r.status,
                "inliers": int(r.inliers.shape[0]), "best_iteration": r.best_iteration}
            print(np.dtype(dtype).name, H, refit, out[f"H{H}_refit_{'on' if refit else 'off'}"], flush=True)
    return out


def main(path):
    out = {"what": "a record, not a gate: nothing in the tests or the benchmark depends on these figures",
           "points": N, "distance_threshold": THR, "device": torch.cuda.get_device_name(0), "reps": REPS,
           "peak_fp64_vector_flops": PEAK_FP64_VECTOR,
           "peak_source": "AMD Instinct MI355X data sheet, peak double precision (FP64) vector: 78.6 TFLOP/s (a fused multiply-add counted as two)",
           "flop_per_test": FLOP_PER_TEST}
    for dtype in (np.float32, np.float64):
        out[np.dtype(dtype).name] = record(dtype)
    with open(path, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else os.path.join(os.path.dirname(os.path.abspath(__file__)), "plane_record.json"))
