"""The workload of profiles/index_frame_refactor.txt, check D.4: on a 72 x 72 grid mesh (5,184 vertices, 10,082 faces) and a 5,000-point
oriented cloud, float32, device-resident tensors: each of the four creates, one query on each handle and each one-shot call of the three tree
families. Run once per library under `rocprofv3 --kernel-trace` (no counters; the library chosen with PCU_HIP_LIBRARY), then

    python profiles/index_frame_record.py compare <trace A>_kernel_trace.csv <trace B>_kernel_trace.csv

requires the same kernels in the same order with the same grid and block sizes."""
import sys, os, csv
HERE = os.path.dirname(os.path.abspath(__file__))


def dispatches(path):
    rows = list(csv.DictReader(open(path)))
    rows.sort(key=lambda r: int(r["Dispatch_Id"]))
    return [(r["Kernel_Name"],) + tuple(int(r[k]) for k in ("Grid_Size_X", "Grid_Size_Y", "Grid_Size_Z", "Workgroup_Size_X", "Workgroup_Size_Y",
                                                             "Workgroup_Size_Z")) for r in rows]


if len(sys.argv) > 1 and sys.argv[1] == "compare":
    a, b = dispatches(sys.argv[2]), dispatches(sys.argv[3])
    ours = [d for d in a if "pcu::" in d[0]]
    print(f"dispatches: {len(a)} and {len(b)}; {len(ours)} of this library's, {len({d[0] for d in ours})} distinct kernels")
    same = a == b
    if not same:
        for i, (x, y) in enumerate(zip(a, b)):
            if x != y:
                print("first difference at dispatch", i, x, y)
                break
    print("RESULT:", "identical" if same else "DIFFERENT")
    sys.exit(0 if same else 1)

sys.path.insert(0, os.path.join(HERE, "..", "tests"))
sys.path.insert(0, os.path.join(HERE, ".."))
import numpy as np
import torch
import mesh_smooth_contract as S
import point_cloud_utils_amd as pcu

v, f = S.grid(72)
rng = np.random.default_rng(3)
p = rng.random((5000, 3))
n = rng.standard_normal((5000, 3))
q = rng.random((4000, 3)) * 1.2 - 0.1
d = rng.standard_normal((4000, 3))
T = lambda a, t=np.float32: torch.from_numpy(np.ascontiguousarray(a.astype(t))).cuda()       # noqa: E731
tv, tf, tp, tn, tq, td = T(v), T(f, np.int32), T(p), T(n), T(q), T(d)
ta, tr = T(rng.random(5000)), T(0.01 + 0.02 * rng.random(5000))

with pcu.DatasetIndex(tp, k_hint=4) as index:
    index.k_nearest_neighbors(tq, 4)
with pcu.MeshIndex(tv, tf, winding_numbers=True) as mesh:
    mesh.closest_points(tq)
    mesh.intersect_rays(tq, td)
    mesh.winding_number(tq)
    mesh.signed_distance(tq)
with pcu.PointCloudWindingIndex(tp, tn, ta) as cloud:
    cloud.winding_number(tq)
with pcu.RaySurfelIntersector(tp, tn, tr, 7) as surfels:
    surfels.intersect_rays(tq, td)
pcu.closest_points_on_mesh(tq, tv, tf)
pcu.ray_mesh_intersection(tv, tf, tq, td)
pcu.triangle_soup_fast_winding_number(tv, tf, tq)
pcu.signed_distance_to_mesh(tq, tv, tf)
pcu.point_cloud_fast_winding_number(tp, tn, ta, tq)
pcu.ray_surfel_intersection(tp, tn, tq, td, tr, 7)
pcu.pointcloud_surfel_geometry(tp, tn, tr, 7)
torch.cuda.synchronize()
print("index_frame_record: done with", os.environ.get("PCU_HIP_LIBRARY", "the package's library"))
