"""The record of DESIGN.md row f21: milliseconds per evaluation of register_point_clouds_icp at 1M source points against 1M target points,
float32 and float64, point-to-point and point-to-plane, device-resident torch tensors. The clouds are the ellipsoid pair of
tests/test_icp_contract.py: two independent samples of the surface, the source moved back by 0.1 rad and (0.02, -0.01, 0.03). A call with
max_iterations = K and both tolerances 0 makes exactly K + 1 evaluations (pcu.last_stats()["n_passes"] says so), so the time of a call through
DatasetIndex.register_icp -- the target's grid is built once, outside -- divided by K + 1 is the time of an evaluation: transform, k = 1 search,
sums, fold, read-back and the host's solve. The floor is index.k_nearest_neighbors(queries, 1) on the same clouds, the search an evaluation
cannot do without. The search's time depends on where the queries lie (off the target's surface they need wider passes), so both are taken
twice: "aligned" -- the call starts at the transform a default point-to-plane call converged to and the floor's queries are the source under
that transform -- which is like for like and is the ratio DESIGN.md quotes, and "from the identity", where the evaluations of a call walk
from the misaligned to the aligned state and the floor's queries are the misaligned source. Device milliseconds between two events around
the calls on the current stream, three warm-ups, the median and the range of 15 repeats. Writes profiles/icp_record.json (or the path given)."""
import json
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tests"))
import numpy as np
import torch
import point_cloud_utils_amd as pcu
from test_icp_contract import MOTION_R, MOTION_T, ellipsoid

N = 1_000_000
REPS = 15
K = 9                   # updates per timed call: ten evaluations


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
    tgt, nrm = ellipsoid(N, dtype, seed=5)
    on, _ = ellipsoid(N, np.float64, seed=1005)
    src = torch.from_numpy(((on - MOTION_T) @ MOTION_R).astype(dtype)).cuda()
    tgt, nrm = torch.from_numpy(tgt).cuda(), torch.from_numpy(nrm).cuda()
    out = {}
    with pcu.DatasetIndex(tgt, k_hint=1) as index:
        found = index.register_icp(src, nrm)
        M = found.transform.cpu().numpy()
        out["default_plane_call"] = {"status": found.status, "iterations": found.iterations, "fitness": found.fitness, "inlier_rmse": found.inlier_rmse,
                                     "max_entry_error": float(np.abs(M[:3] - np.c_[MOTION_R, MOTION_T]).max())}
        aligned = (src.double() @ torch.from_numpy(M[:3, :3].T.copy()).cuda() + torch.from_numpy(M[:3, 3].copy()).cuda()).to(src.dtype).contiguous()
        floors = {"aligned": device_ms(lambda: index.k_nearest_neighbors(aligned, 1, squared_distances=True)),
                  "from_identity": device_ms(lambda: index.k_nearest_neighbors(src, 1, squared_distances=True))}
        out["index_knn_k1"] = floors
        for mode, normals in (("point", None), ("plane", nrm)):
            out[mode] = {}
            for start, init in (("aligned", M), ("from_identity", None)):
                def call(free=False):
                    kw = dict(init_transform=init, max_iterations=K, relative_fitness=0.0, relative_rmse=0.0)
                    return pcu.register_point_clouds_icp(src, tgt, normals, **kw) if free else index.register_icp(src, normals, **kw)
                r = call()
                evaluations = pcu.last_stats()["n_passes"]
                assert evaluations == r.iterations + 1 == K + 1 and r.status == "max_iterations"
                whole = device_ms(call)
                per = {k: round(v / evaluations, 4) for k, v in whole.items()}
                floor = floors[start]["ms_median"]
                out[mode][start] = {"evaluations_per_call": evaluations, "call": whole, "per_evaluation": per,
                                    "per_evaluation_over_index_knn": round(per["ms_median"] / floor, 3),
                                    "beyond_the_search_ms": round(per["ms_median"] - floor, 4),
                                    "free_function_call": device_ms(lambda: call(free=True))}
            print(np.dtype(dtype).name, mode, out[mode], flush=True)
    return out


def main(path):
    out = {"source_points": N, "target_points": N, "device": torch.cuda.get_device_name(0), "reps": REPS}
    for dtype in (np.float32, np.float64):
        out[np.dtype(dtype).name] = record(dtype)
    with open(path, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else os.path.join(os.path.dirname(os.path.abspath(__file__)), "icp_record.json"))
