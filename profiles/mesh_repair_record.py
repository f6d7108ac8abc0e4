"""The record of DESIGN.md 8.8: a 708 x 708 grid mesh (501,264 vertices, 999,698 faces), float32 vertices and int32 faces as device-resident
torch tensors. Host clock around calls that end in a device synchronise; every shape warmed up once; the median and the range of 21 repeats.
For orient_mesh_faces half of the faces are reversed at random; for remove_mesh_vertices a random mask keeps 70% of the vertices; for
remove_unreferenced_mesh_vertices every fourth face is left out and 10% more vertices that no face lists are appended."""
import sys, os, time, json
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tests"))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import numpy as np
import torch
import mesh_smooth_contract as S
import mesh_repair_contract as R
import point_cloud_utils_amd as pcu

v, f = S.grid(708)
rng = np.random.default_rng(1)
mask = rng.random(len(v)) < 0.7
turned = R.reverse_some(f, 2)
loose_v = np.concatenate([v, rng.random((len(v) // 10, 3))])
tv, tf = torch.from_numpy(v.astype(np.float32)).cuda(), torch.from_numpy(f.astype(np.int32)).cuda()
tmask, tturned = torch.from_numpy(mask).cuda(), torch.from_numpy(turned.astype(np.int32)).cuda()
tloose_v, tloose_f = torch.from_numpy(loose_v.astype(np.float32)).cuda(), tf[torch.arange(len(f), device="cuda") % 4 != 0].contiguous()
out = {"vertices": len(v), "faces": len(f)}


def timed(name, fn, reps=21, phases=True):
    res = fn(); torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        torch.cuda.synchronize(); t = time.perf_counter(); fn(); torch.cuda.synchronize(); ts.append((time.perf_counter() - t) * 1e3)
    out[name] = {"ms_median": round(float(np.median(ts)), 3), "ms_min": round(min(ts), 3), "ms_max": round(max(ts), 3), "rows_out": [int(r.shape[0]) for r in res]}
    if phases:
        out[name]["n_escalated"] = pcu.last_stats()["n_escalated"]
        pcu.set_timing(2)
        fn(); torch.cuda.synchronize()
        out[name]["phases"] = {k: round(x, 3) for k, x in pcu.last_stats().items() if k.startswith("ms_") and x}
        pcu.set_timing(0)
    print(name, out[name], flush=True)
    return res


timed("remove_mesh_vertices", lambda: pcu.remove_mesh_vertices(tv, tf, tmask))
timed("remove_unreferenced_mesh_vertices", lambda: pcu.remove_unreferenced_mesh_vertices(tloose_v, tloose_f))
timed("deduplicate_mesh_vertices_eps0", lambda: pcu.deduplicate_mesh_vertices(tv, tf, 0.0))
timed("deduplicate_point_cloud_eps0", lambda: pcu.deduplicate_point_cloud(tv, 0.0), phases=False)      # (the vertex side alone; it records no statistics)
o, p = timed("orient_mesh_faces_half_reversed", lambda: pcu.orient_mesh_faces(tturned))
timed("orient_mesh_faces_as_generated", lambda: pcu.orient_mesh_faces(tf))
# the oriented result at this size, by the property
out["orient_check_twisted"] = R.check_orientation(turned, o.cpu().numpy(), p.cpu().numpy())
out["orient_patches"] = int(p.max()) + 1
print(json.dumps(out))
json.dump(out, open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "mesh_repair_record.json"), "w"), indent=1)
