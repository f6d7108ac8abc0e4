"""The record of DESIGN.md row f23 -- a record, not a gate: milliseconds per call of orient_point_cloud_normals at 1M rows of a unit sphere
(true normals with random signs, shuffled rows), float32 and float64, k = 10 and 30, device-resident torch tensors. Beside every figure, from
the same commit and the same cloud: k_nearest_neighbors(P, P, k + 1) alone -- the search the call begins with --,
estimate_point_cloud_normals_knn(P, k), the number of rounds and trees, and the call's phases from set_timing(2) (the search, the rounds, the
outputs). Device milliseconds between two events around the call on the current stream, three warm-ups, the median and
the range of 15 repeats. Writes profiles/orient_record.json (or the path given)."""
import json
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


def record(dtype):
    rng = np.random.default_rng(23)
    true = rng.standard_normal((N, 3))
    true /= np.linalg.norm(true, axis=1, keepdims=True)
    sign = rng.choice([-1.0, 1.0], size=(N, 1))
    p = torch.from_numpy(true.astype(dtype)).cuda()
    nrm = torch.from_numpy((true * sign).astype(dtype)).cuda()
    out = {}
    for k in (10, 30):
        oriented = pcu.orient_point_cloud_normals(p, nrm, k)
        st = pcu.last_stats()
        outward = bool(((oriented * p).sum(dim=1) > 0).all())
        old = pcu.set_timing(2)
        try:
            phases = []
            for _ in range(5):
                pcu.orient_point_cloud_normals(p, nrm, k)
                s = pcu.last_stats()
                phases.append((s["ms_index"], s["ms_search"], s["ms_tie"], s["ms_total"]))
        finally:
            pcu.set_timing(old)
        ph = np.median(np.asarray(phases), axis=0)
        call = device_ms(lambda: pcu.orient_point_cloud_normals(p, nrm, k))
        knn = device_ms(lambda: pcu.k_nearest_neighbors(p, p, k + 1))
        est = device_ms(lambda: pcu.estimate_point_cloud_normals_knn(p, k))
        out[f"k{k}"] = {"call": call, "knn_k_plus_1": knn, "estimate_normals_knn": est, "call_over_knn": round(call["ms_median"] / knn["ms_median"], 2),
                        "rounds": st["n_passes"], "trees": st["n_escalated"], "all_outward": outward,
                        "phases_ms": {"search": round(float(ph[0]), 3), "rounds": round(float(ph[1]), 3), "outputs": round(float(ph[2]), 3),
                                      "total": round(float(ph[3]), 3)}}
        print(np.dtype(dtype).name, k, out[f"k{k}"], flush=True)
    return out


def main(path):
    out = {"what": "a record, not a gate: nothing in the tests or the benchmark depends on these figures",
           "points": N, "cloud": "unit sphere, shuffled rows, true normals with random signs", "device": torch.cuda.get_device_name(0), "reps": REPS}
    for dtype in (np.float32, np.float64):
        out[np.dtype(dtype).name] = record(dtype)
    with open(path, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else os.path.join(os.path.dirname(os.path.abspath(__file__)), "orient_record.json"))
