"""The record of DESIGN.md 8.7: a 1000 x 1000 grid mesh (1,000,000 vertices, 1,996,002 faces), float32, device-resident tensors.
Host clock around calls that end in a device synchronise; every shape warmed up once; the median and the range of 7 repeats."""
import sys, os, time, json
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tests"))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import numpy as np
import torch
import mesh_smooth_contract as C
import point_cloud_utils_amd as pcu

v, f = C.grid(1000)
tv, tf = torch.from_numpy(v.astype(np.float32)).cuda(), torch.from_numpy(f.astype(np.int32)).cuda()
out = {"vertices": len(v), "faces": len(f)}


def timed(name, fn, reps=7):
    fn(); torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        torch.cuda.synchronize(); t = time.perf_counter(); fn(); torch.cuda.synchronize(); ts.append((time.perf_counter() - t) * 1e3)
    st = pcu.last_stats()
    out[name] = {"ms_median": round(float(np.median(ts)), 3), "ms_min": round(min(ts), 3), "ms_max": round(max(ts), 3), "n_passes": st["n_passes"], "n_escalated": st["n_escalated"]}
    print(name, out[name], flush=True)


timed("adjacency", lambda: pcu.mesh_vertex_adjacency(tf, num_vertices=len(v)))
for w in ("uniform", "area", "angle"):
    timed("normals_" + w, lambda: pcu.estimate_mesh_vertex_normals(tv, tf, w))
for cot in (False, True):
    timed("smooth3_cotan" if cot else "smooth3_uniform", lambda: pcu.laplacian_smooth_mesh(tv, tf, 3, 0.1, cot))
pcu.set_timing(2)
pcu.laplacian_smooth_mesh(tv, tf, 3, 0.1, False); torch.cuda.synchronize()
out["smooth3_uniform_phases"] = {k: round(x, 3) for k, x in pcu.last_stats().items() if k.startswith("ms_")}
pcu.laplacian_smooth_mesh(tv, tf, 3, 0.1, True); torch.cuda.synchronize()
out["smooth3_cotan_phases"] = {k: round(x, 3) for k, x in pcu.last_stats().items() if k.startswith("ms_")}
pcu.set_timing(0)
# the result at this size against the float64 sparse direct solve
u = pcu.laplacian_smooth_mesh(tv, tf, 1, 0.1, False).cpu().numpy()
ref = C.smooth_direct(v.astype(np.float32), f, 1, 0.1, False, sparse=True)
out["smooth1_uniform_err"] = float(np.abs(u - ref).max() / np.abs(ref).max())
print(json.dumps(out))
json.dump(out, open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "mesh_smooth_record.json"), "w"), indent=1)
