"""The record of DESIGN.md row f25 -- a record, not a gate: milliseconds of register_point_clouds_ransac at 2**17 correspondences against
2**17 hypotheses and at 2**20 correspondences against 2**14 hypotheses, float32 and float64 input, with and without refit, device-resident
torch tensors. The input is the planted motion of tests/test_ransac_contract.py (30 % true pairs); the scoring kernel tests every
correspondence against every hypothesis whatever the pre-check decided, so its time does not depend on the data. Two times per case: the whole
call (device events around the call on the current stream, timing off), and the scoring phase (the library's own events around the scoring
launches and the winner kernel: last_stats()["ms_search"] at set_timing(2), in runs of their own). The scoring phase is set beside the
arithmetic floor: a test is 26 float64 operations (9 multiplies and 9 adds of the motion, 3 subtractions, 3 multiplies and 2 adds of the
squared length), so c * H * 26 flop over the chip's peak vector float64 rate -- PEAK_FP64_VECTOR below, the figure of profiles/plane_record.py,
which counts a fused multiply-add as two operations; the contract forbids fusing, so a kernel of separate multiplies and adds can reach half
of it at the most. The share the plane kernel achieved is read from profiles/plane_record.json (its whole call at 10000 hypotheses, where
scoring is all but the whole). Three warm-ups, the median and the range of 9 repeats. Writes profiles/ransac_record.json (or the path given)."""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, ".."))
sys.path.insert(0, os.path.join(HERE, "..", "tests"))
import numpy as np
import torch
import point_cloud_utils_amd as pcu
from test_ransac_contract import THR, planted

SHAPES = ((1 << 17, 1 << 17), (1 << 20, 1 << 14))       # (correspondences, hypotheses)
REPS = 9
PEAK_FP64_VECTOR = 78.6e12          # flop/s
FLOP_PER_TEST = 26


def spread(ts):
    return {"ms_median": round(float(np.median(ts)), 3), "ms_min": round(min(ts), 3), "ms_max": round(max(ts), 3)}


def call_ms(fn, reps=REPS, warmup=3):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(); fn(); b.record(); torch.cuda.synchronize()
        ts.append(a.elapsed_time(b))
    return spread(ts)


def phase_ms(fn, reps=REPS):
    old = pcu.set_timing(2)
    try:
        fn()
        hyp, score, total = [], [], []
        for _ in range(reps):
            fn()
            st = pcu.last_stats()
            hyp.append(st["ms_index"]); score.append(st["ms_search"]); total.append(st["ms_total"])
        return spread(hyp), spread(score), spread(total)
    finally:
        pcu.set_timing(old)


def record(dtype):
    out = {}
    for c, H in SHAPES:
        P = planted(c, dtype)
        A = tuple(torch.from_numpy(x).cuda() for x in (P.source, P.target, P.corr))
        floor_ms = c * H * FLOP_PER_TEST / PEAK_FP64_VECTOR * 1e3
        for refit in (False, True):
            fn = lambda: pcu.register_point_clouds_ransac(*A, THR, H, 3, refit=refit)
            r = fn()
            launches = pcu.last_stats()["n_passes"]
            t = call_ms(fn)
            hyp, score, total = phase_ms(fn)
            key = f"c{c}_H{H}_refit_{'on' if refit else 'off'}"
            out[key] = {"call": t, "gather_and_hypotheses_phase": hyp, "scoring_phase": score, "phases_total": total,
                        "scoring_flops": round(c * H * FLOP_PER_TEST / (score["ms_median"] * 1e-3), 0), "arithmetic_floor_ms": round(floor_ms, 4),
                        "scoring_over_floor": round(score["ms_median"] / floor_ms, 2), "scoring_share_of_peak": round(floor_ms / score["ms_median"], 4),
                        "scoring_launches": launches, "status": r.status, "inliers": int(r.inliers.shape[0]), "planted": int(P.true.sum()),
                        "best_iteration": r.best_iteration, "fitness": r.fitness, "inlier_rmse": r.inlier_rmse}
            print(np.dtype(dtype).name, key, out[key], flush=True)
    return out


def plane_share():
    with open(os.path.join(HERE, "plane_record.json")) as f:
        p = json.load(f)
    return {k: round(1.0 / p[k]["H10000_refit_off"]["call_over_floor"], 4) for k in ("float32", "float64")}


def main(path):
    from point_cloud_utils_amd import _ransac
    rows, launch_tests = _ransac._geometry()
    out = {"what": "a record, not a gate: nothing in the tests or the benchmark depends on these figures",
           "shapes": [list(s) for s in SHAPES], "max_correspondence_distance": THR, "edge_length_ratio": 0.9, "device": torch.cuda.get_device_name(0),
           "reps": REPS, "rows_per_lane": rows, "tests_per_launch": launch_tests, "peak_fp64_vector_flops": PEAK_FP64_VECTOR,
           "peak_source": "AMD Instinct MI355X data sheet, peak double precision (FP64) vector: 78.6 TFLOP/s (a fused multiply-add counted as two)",
           "flop_per_test": FLOP_PER_TEST,
           "plane_kernel_share_of_peak": plane_share(),
           "plane_share_source": "profiles/plane_record.json: 1 / call_over_floor of H10000_refit_off (8 flop per test, the whole call)"}
    for dtype in (np.float32, np.float64):
        out[np.dtype(dtype).name] = record(dtype)
    with open(path, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else os.path.join(HERE, "ransac_record.json"))
