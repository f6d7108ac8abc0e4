"""The workload of profiles/operator_frame_refactor.txt: one call of every operator whose host side goes through the operator frame's way out
(out_room / out_give, stage_faces, the flag word) or whose kernels read integers through csrc/index_kinds.h. A 72 x 72 grid mesh (5,184
vertices, 10,082 faces), a 32^3 scalar block and 5,000 points; float32 and float64; numpy arrays with each of the four integer kinds and
device tensors with the two signed ones. The library is chosen with PCU_HIP_LIBRARY.

    python profiles/operator_frame_record.py run OUT.json         sha256 of every output and every call's time: ms_total of last_stats() at timing
                                                                   level 2 where the call reports one, else the host clock round three more
                                                                   calls that end in a device synchronise (their median)
    python profiles/operator_frame_record.py hashes A.json B.json byte identity: the two runs' digests are equal
    python profiles/operator_frame_record.py compare A_kernel_trace.csv B_kernel_trace.csv
                                                                   dispatch identity of two `rocprofv3 --kernel-trace -- python ... run` traces
    python profiles/operator_frame_record.py speed PARENT.json... -- NEW.json...
                                                                   per operator: the new median of its time against the parent's median +- the
                                                                   parent's own max - min over its runs"""
import sys, os, csv, json, hashlib, time
HERE = os.path.dirname(os.path.abspath(__file__))


def dispatches(path):
    rows = list(csv.DictReader(open(path)))
    rows.sort(key=lambda r: int(r["Dispatch_Id"]))
    return [(r["Kernel_Name"],) + tuple(int(r[k]) for k in ("Grid_Size_X", "Grid_Size_Y", "Grid_Size_Z", "Workgroup_Size_X", "Workgroup_Size_Y",
                                                             "Workgroup_Size_Z")) for r in rows]


def compare(pa, pb):
    """Three readings, strictest first: every dispatch with its full name; names without their parameter lists (a kernel that gained an
    argument keeps its name); this library's kernels alone (the runtime's own copy and fill kernels, which stand for memcpy and memset
    calls and depend on how the runtime chose to move the bytes, left out). The exit status is that of the second."""
    a, b = dispatches(pa), dispatches(pb)
    bare = lambda d: (d[0][:d[0].rfind("(")] if d[0].endswith(")") else d[0],) + d[1:]       # noqa: E731
    ours = lambda ds: [bare(d) for d in ds if "pcu::" in d[0]]                                 # noqa: E731
    print(f"dispatches: {len(a)} and {len(b)}; {len(ours(a))} and {len(ours(b))} of this library's, {len({d[0] for d in ours(a)})} distinct kernels")
    changed = sorted({(x[0], y[0]) for x, y in zip(a, b) if x != y and bare(x) == bare(y)})
    for x, y in changed:
        print("parameter list changed:", x, "->", y)
    results = []
    for what, xs, ys in (("full names", a, b), ("names without parameter lists", [bare(d) for d in a], [bare(d) for d in b]), ("this library's kernels", ours(a), ours(b))):
        same = xs == ys
        results.append(same)
        if not same:
            i = next((i for i, (x, y) in enumerate(zip(xs, ys)) if x != y), min(len(xs), len(ys)))
            print(f"{what}: first difference at {i}:", xs[i - 1:i + 2], "|", ys[i - 1:i + 2])
        print(f"RESULT ({what}):", "identical" if same else "DIFFERENT")
    return 0 if results[1] else 1


def hashes(pa, pb):
    a, b = json.load(open(pa))["sha"], json.load(open(pb))["sha"]
    diff = sorted(k for k in set(a) | set(b) if a.get(k) != b.get(k))
    print(f"{len(a)} and {len(b)} calls; {len(diff)} differ", *diff[:20], sep="\n  ")
    print("RESULT:", "identical" if not diff else "DIFFERENT")
    return 0 if not diff else 1


def speed(parent, new):
    import numpy as np
    P, N = [json.load(open(p)) for p in parent], [json.load(open(p)) for p in new]
    keys = {}
    for k in sorted(set(P[0]["ms"]) | set(P[0]["wall"])):
        keys.setdefault(k.split("|")[0], []).append(k)
    bad = 0
    print(f"{'operator':42s} {'clock':>8s} {'parent median':>14s} {'parent spread':>14s} {'new median':>11s}  (ms summed over the operator's calls; {len(P)} and {len(N)} runs)")
    for op, ks in sorted(keys.items()):
        src = "ms" if all(k in r["ms"] for r in P + N for k in ks) else "wall"       # the device's figure only where every run has a fresh one
        p, n = [sum(r[src][k] for k in ks) for r in P], [sum(r[src][k] for k in ks) for r in N]
        pm, ps, nm = float(np.median(p)), max(p) - min(p), float(np.median(n))
        ok = abs(nm - pm) <= ps
        bad += not ok
        print(f"{op:42s} {'device' if src == 'ms' else 'host':>8s} {pm:14.4f} {ps:14.4f} {nm:11.4f}  {'within' if ok else 'OUTSIDE'}")
    print("RESULT:", "every operator within the parent's spread" if not bad else f"{bad} operators outside the parent's spread")
    return 0 if not bad else 1


if len(sys.argv) > 1 and sys.argv[1] in ("compare", "hashes"):
    sys.exit({"compare": compare, "hashes": hashes}[sys.argv[1]](sys.argv[2], sys.argv[3]))
if len(sys.argv) > 1 and sys.argv[1] == "speed":
    cut = sys.argv.index("--")
    sys.exit(speed(sys.argv[2:cut], sys.argv[cut + 1:]))

sys.path.insert(0, os.path.join(HERE, "..", "tests"))
sys.path.insert(0, os.path.join(HERE, ".."))
import numpy as np
import torch
import mesh_smooth_contract as S
import marching_cubes_contract as MC
import point_cloud_utils_amd as pcu
from point_cloud_utils_amd._call import _last_stats

v64, f64 = S.grid(72)
rng = np.random.default_rng(3)
p64 = rng.random((5000, 3))
n64 = rng.standard_normal((5000, 3))
q64 = rng.random((4000, 3)) * 1.2 - 0.1
d64 = rng.standard_normal((4000, 3))
a64, r64 = rng.random(5000), 0.01 + 0.02 * rng.random(5000)
mask = rng.random(len(v64)) < 0.7
P64, cubes = MC.dense_grid(32)
S64 = np.linalg.norm(P64, axis=1) - 0.7
ijk = np.unique((p64 * 24).astype(np.int64), axis=0)
block = (np.linalg.norm(np.stack(np.meshgrid(*[np.linspace(-1, 1, 32)] * 3, indexing="ij"), -1), axis=-1) < 0.7)
sha, ms, wall = {}, {}, {}


def digest(res):
    h = hashlib.sha256()
    for x in (res if isinstance(res, (tuple, list)) else [res]):
        if isinstance(x, (list, tuple)):
            h.update(digest(x).encode())
            continue
        a = x.cpu().numpy() if isinstance(x, torch.Tensor) else np.asarray(x)
        h.update(str((a.dtype, a.shape)).encode()); h.update(np.ascontiguousarray(a).tobytes())
    return h.hexdigest()


def call(name, cfg, fn):
    key = name + "|" + cfg
    try:
        _last_stats[0] = None                                       # (so that a call that records no statistics cannot show its predecessor's)
        res = fn()
        torch.cuda.synchronize()
        sha[key] = digest(res)
        fresh = float(pcu.last_stats().get("ms_total", 0.0))
        if fresh > 0.0:
            ms[key] = fresh
            return
        ts = []
        for _ in range(3):
            torch.cuda.synchronize(); t = time.perf_counter(); fn(); torch.cuda.synchronize(); ts.append((time.perf_counter() - t) * 1e3)
        wall[key] = float(np.median(ts))
    except (ValueError, TypeError, RuntimeError) as e:            # a combination the wrapper does not take: the same text from either library
        sha[key] = "refused: " + str(e)[:120]


pcu.set_timing(2)
for T in (np.float32, np.float64):
    for where, kinds in (("numpy", (np.int32, np.int64, np.uint32, np.uint64)), ("device", (np.int32, np.int64))):
        to = (lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()) if where == "device" else np.ascontiguousarray
        v, p, n, q, d, a, r = (to(x.astype(T)) for x in (v64, p64, n64, q64, d64, a64, r64))
        Pm, Sm = to(P64.astype(T)), to(S64.astype(T))
        tmask = to(mask)
        for K in kinds:
            cfg = f"{np.dtype(T).name}|{where}|{np.dtype(K).name}"
            f, c, g = to(f64.astype(K)), to(cubes.astype(K)), to(ijk.astype(K))
            call("closest_points_on_mesh", cfg, lambda: pcu.closest_points_on_mesh(q, v, f))
            call("ray_mesh_intersection", cfg, lambda: pcu.ray_mesh_intersection(v, f, q, d))
            call("triangle_soup_fast_winding_number", cfg, lambda: pcu.triangle_soup_fast_winding_number(v, f, q))
            call("signed_distance_to_mesh", cfg, lambda: pcu.signed_distance_to_mesh(q, v, f))
            call("mesh_face_areas", cfg, lambda: pcu.mesh_face_areas(v, f))
            call("sample_mesh_random", cfg, lambda: pcu.sample_mesh_random(v, f, 3000, random_seed=5))
            call("sample_mesh_poisson_disk", cfg, lambda: pcu.sample_mesh_poisson_disk(v, f, 500, random_seed=5))
            call("estimate_mesh_face_normals", cfg, lambda: pcu.estimate_mesh_face_normals(v, f))
            call("voxelize_triangle_mesh", cfg, lambda: pcu.voxelize_triangle_mesh(v, f, 0.02, np.zeros(3)))
            call("sparse_voxel_grid_boundary", cfg, lambda: pcu.sparse_voxel_grid_boundary(g))
            call("voxel_grid_geometry", cfg, lambda: pcu.voxel_grid_geometry(g, gap_fraction=0.1))
            call("connected_components", cfg, lambda: pcu.connected_components(v, f))
            call("marching_cubes_sparse_voxel_grid", cfg, lambda: pcu.marching_cubes_sparse_voxel_grid(Sm, Pm, c, 0.0))
            call("sparse_voxel_grid_to_hex_mesh", cfg, lambda: pcu.sparse_voxel_grid_to_hex_mesh(g, 0.5, (0.0, 0.0, 0.0), dtype=T))
            call("mesh_vertex_adjacency", cfg, lambda: pcu.mesh_vertex_adjacency(f, len(v64)))
            call("estimate_mesh_vertex_normals", cfg, lambda: pcu.estimate_mesh_vertex_normals(v, f, "angle"))
            call("laplacian_smooth_mesh", cfg, lambda: pcu.laplacian_smooth_mesh(v, f, 2, use_cotan_weights=True))
            call("remove_mesh_vertices", cfg, lambda: pcu.remove_mesh_vertices(v, f, tmask))
            call("remove_unreferenced_mesh_vertices", cfg, lambda: pcu.remove_unreferenced_mesh_vertices(v, f[::2]))
            call("deduplicate_mesh_vertices", cfg, lambda: pcu.deduplicate_mesh_vertices(v, f, 1e-2))
            call("orient_mesh_faces", cfg, lambda: pcu.orient_mesh_faces(f))
            call("decimate_triangle_mesh", cfg, lambda: pcu.decimate_triangle_mesh(v, f, 6000))
        cfg = f"{np.dtype(T).name}|{where}|-"
        call("point_cloud_fast_winding_number", cfg, lambda: pcu.point_cloud_fast_winding_number(p, n, a, q))
        call("ray_surfel_intersection", cfg, lambda: pcu.ray_surfel_intersection(p, n, q, d, r, 7))
        call("pointcloud_surfel_geometry", cfg, lambda: pcu.pointcloud_surfel_geometry(p, n, r, 7))
        call("radius_search", cfg, lambda: pcu.radius_search(q, p, 0.08))
        call("radius_count", cfg, lambda: pcu.radius_count(q, p, 0.08))
        call("downsample_point_cloud_farthest_point", cfg, lambda: pcu.downsample_point_cloud_farthest_point(p, 400, return_distances=True))
        call("downsample_point_cloud_poisson_disk", cfg, lambda: pcu.downsample_point_cloud_poisson_disk(p, 0.05, random_seed=5))
        call("downsample_point_cloud_on_voxel_grid", cfg, lambda: pcu.downsample_point_cloud_on_voxel_grid(0.05, p, n))
        call("deduplicate_point_cloud", cfg, lambda: pcu.deduplicate_point_cloud(p, 1e-2))
        call("pairwise_distances", cfg, lambda: pcu.pairwise_distances(p[:300], q[:200]))
        call("flood_fill_3d", cfg, lambda: pcu.flood_fill_3d(to(block.astype(T)), (16, 16, 16), 5.0))
    call("morton_encode", np.dtype(T).name, lambda: pcu.morton_encode((p64 * 1000).astype(np.int32)))
    call("morton_knn", np.dtype(T).name, lambda: pcu.morton_knn(np.sort(pcu.morton_encode((p64 * 1000).astype(np.int32))), pcu.morton_encode((q64.clip(0, 1) * 1000).astype(np.int32)), 4))
torch.cuda.synchronize()
out = sys.argv[2] if len(sys.argv) > 2 and sys.argv[1] == "run" else None
if out:
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    json.dump({"library": os.environ.get("PCU_HIP_LIBRARY", "the package's library"), "sha": sha, "ms": ms, "wall": wall}, open(out, "w"), indent=1, sort_keys=True)
refused = sum(1 for x in sha.values() if x.startswith("refused"))
print(f"operator_frame_record: {len(sha)} calls ({refused} refused by the wrappers) with", os.environ.get("PCU_HIP_LIBRARY", "the package's library"))
