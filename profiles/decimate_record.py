"""The record of DESIGN.md row f17: decimate_triangle_mesh to a quarter of the faces, float32 vertices and int32 faces as device-resident
torch tensors, for the bunny fixture (2,885 vertices, 5,766 faces) and an icosphere of 7 subdivisions generated here (163,842 vertices,
327,680 faces; stretched, so that edge lengths differ). Host clock around calls that end in a device synchronise; every shape warmed up
once; the median and the range of 21 repeats. Then one call with phase timing: device time between events, summed over the rounds
(ms_index: the sort and the adjacency, ms_search: cost, validity, claims and wins, ms_tie: budget, collapses and face compaction). Both
results are compared with the contract's (tests/decimate_contract.py), byte for byte, at the size timed: the bunny's by running the
contract here, the icosphere's by the SHA-256 of the contract's four arrays, which takes numpy six minutes and was computed beforehand."""
import sys, os, time, json, hashlib
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tests"))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import numpy as np
import torch
import decimate_contract as D
import point_cloud_utils_amd as pcu

ICOSPHERE7_SHA256 = "4a3a8494e98830d55b4a1a10b5bd931e1c23bc6701ad3b2104ce184d07a1e666"
out = {}


def digest(arrays):
    h = hashlib.sha256()
    for a in arrays:
        h.update(np.ascontiguousarray(a).tobytes())
    return h.hexdigest()


def record(name, v, f, contract_sha256=None, reps=21):
    v, f = np.ascontiguousarray(v.astype(np.float32)), np.ascontiguousarray(f.astype(np.int32))
    target = len(f) // 4
    tv, tf = torch.from_numpy(v).cuda(), torch.from_numpy(f).cuda()
    fn = lambda: pcu.decimate_triangle_mesh(tv, tf, target)
    res = fn(); torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        torch.cuda.synchronize(); t = time.perf_counter(); fn(); torch.cuda.synchronize(); ts.append((time.perf_counter() - t) * 1e3)
    st = pcu.last_stats()
    r = {"vertices": len(v), "faces": len(f), "max_faces": target, "faces_out": int(res[1].shape[0]), "vertices_out": int(res[0].shape[0]),
         "rounds": st["n_passes"], "collapses": st["n_escalated"],
         "ms_median": round(float(np.median(ts)), 3), "ms_min": round(min(ts), 3), "ms_max": round(max(ts), 3)}
    r["ms_per_round"] = round(r["ms_median"] / max(1, r["rounds"]), 4)
    pcu.set_timing(2)
    fn(); torch.cuda.synchronize()
    r["phases"] = {k: round(x, 3) for k, x in pcu.last_stats().items() if k.startswith("ms_") and x}
    pcu.set_timing(0)
    r["sha256"] = digest([g.cpu().numpy() for g in res])
    if contract_sha256 is None:
        t = time.perf_counter()
        d = D.Decimation(v, f)
        contract_sha256 = digest(d.decimate(target))
        r["contract_seconds_numpy"] = round(time.perf_counter() - t, 2)
        r["contract_rounds_collapses"] = [d.rounds, d.collapses]
    r["equals_contract"] = r["sha256"] == contract_sha256
    out[name] = r
    print(name, r, flush=True)


record("bunny", *D.bunny())
sv, sf = D.icosphere(7)
record("icosphere7", sv * np.array([1.0, 0.8, 1.3]), sf, ICOSPHERE7_SHA256)
print(json.dumps(out))
json.dump(out, open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "decimate_record.json"), "w"), indent=1)
