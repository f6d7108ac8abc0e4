"""The record of DESIGN.md row f20: cluster_point_cloud_dbscan of 1M float32 points, device-resident torch tensors, min_points 8 -- uniform in
the unit cube at the two radii of profiles/radius_record.py (mean neighbourhood about 16 and about 64), and a clustered cloud of 1,000
Gaussian blobs of 1,000 points. Device milliseconds between two events around calls on the current stream, every shape warmed up three
times, the median and the range of 15 repeats; then one call with phase timing (device time between events: ms_index = index and record
order; ms_search = core pass; ms_kernel_search = union pass, flatten and ranks; ms_tie = border pass and labels). The yardsticks are calls
the library had before, timed in the same process on the same cloud: radius_count(p, p, eps), the cost of a full count pass, and
radius_search(p, p, eps, sort_results=False), what a caller had to run before clustering on the host. The core mask must equal
radius_count >= min_points on the whole cloud. Writes profiles/dbscan_record.json (or the path given)."""
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
MIN_POINTS = 8


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


def record(p, eps):
    labels, core = pcu.cluster_point_cloud_dbscan(p, eps, MIN_POINTS, return_core=True)
    counts = pcu.radius_count(p, p, eps)
    r = {"eps": eps, "min_points": MIN_POINTS, "mean_neighbourhood": round(float(counts.double().mean()), 3), "max_neighbourhood": int(counts.max()),
         "core_equals_radius_count": bool(torch.equal(core, counts >= MIN_POINTS)),
         "clusters": int(labels.max()) + 1, "core": int(core.sum()), "border": int((~core & (labels >= 0)).sum()), "noise": int((labels < 0).sum())}
    del labels, core, counts
    r["dbscan"] = device_ms(lambda: pcu.cluster_point_cloud_dbscan(p, eps, MIN_POINTS, return_core=True))
    r["radius_count"] = device_ms(lambda: pcu.radius_count(p, p, eps))
    r["radius_search_unsorted"] = device_ms(lambda: pcu.radius_search(p, p, eps, sort_results=False))
    r["dbscan_over_radius_count"] = round(r["dbscan"]["ms_median"] / r["radius_count"]["ms_median"], 3)
    r["dbscan_over_radius_search_unsorted"] = round(r["dbscan"]["ms_median"] / r["radius_search_unsorted"]["ms_median"], 3)
    r["phases"], _ = phases(lambda: pcu.cluster_point_cloud_dbscan(p, eps, MIN_POINTS, return_core=True))
    r["phases_radius_count"], _ = phases(lambda: pcu.radius_count(p, p, eps))
    count_pass = r["phases_radius_count"].get("ms_search", 0.0)
    if count_pass:
        r["core_pass_over_count_pass"] = round(r["phases"].get("ms_search", 0.0) / count_pass, 3)
        r["union_pass_over_count_pass"] = round(r["phases"].get("ms_kernel_search", 0.0) / count_pass, 3)
        r["border_pass_over_count_pass"] = round(r["phases"].get("ms_tie", 0.0) / count_pass, 3)
    with pcu.DatasetIndex(p, k_hint=16) as index:
        r["index_k_hint16_dbscan"] = device_ms(lambda: index.cluster_dbscan(eps, MIN_POINTS, return_core=True))
    return r


def main(path):
    rng = np.random.default_rng(31)
    uniform = torch.from_numpy(rng.random((N, 3), dtype=np.float32)).cuda()
    centres = rng.random((1000, 3))
    blobs = (centres[:, None, :] + rng.normal(0.0, 0.004, (1000, N // 1000, 3))).reshape(-1, 3)
    blobs = torch.from_numpy(np.ascontiguousarray(blobs[rng.permutation(N)], dtype=np.float32)).cuda()
    out = {"points": N, "dtype": "float32", "device": torch.cuda.get_device_name(0), "reps": REPS}
    for want in (16, 64):
        eps = (3.0 * want / (4.0 * math.pi * N)) ** (1.0 / 3.0)
        out["uniform_mean_%d" % want] = record(uniform, eps)
        print(want, out["uniform_mean_%d" % want], flush=True)
    out["blobs_1000_sigma_0.004"] = record(blobs, 0.002)
    print("blobs", out["blobs_1000_sigma_0.004"], flush=True)
    with open(path, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else os.path.join(os.path.dirname(os.path.abspath(__file__)), "dbscan_record.json"))
