"""Every entry point that reads an integer array "of a kind" (int32, int64, uint32, uint64), through the C entry points as _lib.lib() binds
them (-m gpu): the Python wrappers refuse a bad host array before the device sees it, so only these calls reach the device checks of
csrc/index_kinds.h. One 4-vertex, 2-face mesh, one cube of 2 x 2 x 2 corners, three voxel coordinates, all in device memory. For every entry
point, kind and poison value: the call is refused with the entry point's own text (the literals below were taken from the commit before the
codec existed, not from the code under test), every output buffer still holds the sentinel it was filled with, and the same call with the
poison taken out returns 0 and equals the numpy contract that the operator's own test uses.

The poison values: -1 (signed kinds), the first index past the end, 2^32 (64-bit kinds: truncated it would read as 0), 2^64 - 1 (uint64:
read as signed it would be -1), and for coordinates 2^20, the first value outside the window. A coordinate has no "past the end" and may be
negative: NOT_REFUSED lists, with the reason, the combinations that are no error, and those are held to the contract instead."""
import ctypes

import numpy as np
import pytest

import components_contract as cc
import decimate_contract as dc
import marching_cubes_contract as mc
import mesh_contract as mesh
import mesh_repair_contract as mr
import mesh_smooth_contract as ms
import sampling_contract as sc
import voxelize_contract as vc

pytestmark = pytest.mark.gpu

ON_DEVICE = 1                                                       # PCU_HIP_PTRS_ON_DEVICE
KINDS = {"int32": (0, np.int32), "int64": (1, np.int64), "uint32": (2, np.uint32), "uint64": (3, np.uint64)}
SENTINEL = 0xA5

V = np.array([(0, 0, 0), (1, 0, 0), (0, 1, 0), (1, 1, 0.5)], dtype=np.float32)
F = np.array([(0, 1, 2), (2, 1, 3)], dtype=np.int64)
P = np.array([(0.2, 0.2, 1.0), (2.0, 2.0, 0.0), (0.5, 0.5, -0.25)], dtype=np.float32)
MASK = np.array([1, 1, 1, 0], dtype=np.uint8)
CUBE_V, CUBE_C = mc.hex_mesh(np.zeros((1, 3), dtype=np.int32))      # 8 corners in the marching-cubes order, one cube
CUBE_V = CUBE_V.astype(np.float32)
CUBE_S = np.ascontiguousarray(CUBE_V[:, 0] - 0.25)
IJK = np.array([(0, 0, 0), (1, 0, 0), (0, 1, 0)], dtype=np.int64)
HALF, ONE, ZERO = ((ctypes.c_double * 3)(*([x] * 3)) for x in (0.5, 1.0, 0.0))

FACE_TEXT = "f must hold row indices of v: found a face index outside [0, 4)"
CUBE_TEXT = "cube_indices must hold row indices of grid_coordinates: found an index outside [0, 8)"
COORD_TEXT = "Invalid vertex leads to an overflow integer. Perhaps grid_size is too small."


@pytest.fixture(scope="module")
def gpu():
    from point_cloud_utils_amd import _lib
    assert _lib.device_count() > 0, "no GPU visible: the gfx950 path has no CPU fallback"
    return _lib


def dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).cuda()


class Outs:
    """Device buffers filled with the sentinel: out(name, dtype, *shape) -> pointer; get(name, rows) -> the array (its first rows)."""

    def __init__(self):
        self.bufs = {}

    def __call__(self, name, dtype, *shape):
        import torch
        n = int(np.prod(shape)) * np.dtype(dtype).itemsize
        self.bufs[name] = (torch.full((max(n, 1),), SENTINEL, dtype=torch.uint8, device="cuda"), np.dtype(dtype), shape)
        return self.bufs[name][0].data_ptr()

    def get(self, name, rows=None):
        t, dtype, shape = self.bufs[name]
        a = t.cpu().numpy()[:int(np.prod(shape)) * dtype.itemsize].view(dtype).reshape(shape)
        return a if rows is None else a[:rows]

    def untouched(self):
        return all(bool((t == SENTINEL).all()) for t, _, _ in self.bufs.values())


def same(got, want):
    want = np.asarray(want)
    return got.shape == want.shape and np.array_equal(got, want.astype(got.dtype))


def i64():
    return ctypes.c_int64(-7)


# ---------------------------------------------------------------------------------------------------- the entry points
# Each: run(L, ctx, a, k, D, o) -> (rc, the host counts the call wrote); check(L, ctx, a, D, o, counts) -> the clean call equals the contract.
# a: the integer array (faces, cube, coordinates) as the host knows it, already of dtype D.
def mesh_args(a):
    return dev(V), 4, dev(a), 2


def run_closest(L, ctx, a, k, D, o):
    tv, nv, tf, nf = mesh_args(a)
    tp = dev(P)
    return L.pcu_hip_closest_points_on_mesh_f32(ctx, tv.data_ptr(), nv, tf.data_ptr(), nf, k, tp.data_ptr(), 3, o("d", np.float32, 3), o("fi", np.int64, 3),
                                                o("bc", np.float32, 3, 3), ON_DEVICE, None, None), ()


def check_closest(L, ctx, a, D, o, counts):
    d, fi, bc = mesh.closest_brute(P, V, a.astype(np.int64))
    return same(o.get("d"), d) and same(o.get("fi"), fi) and same(o.get("bc"), bc)


def run_areas(L, ctx, a, k, D, o):
    tv, nv, tf, nf = mesh_args(a)
    return L.pcu_hip_mesh_face_areas_f32(ctx, tv.data_ptr(), nv, tf.data_ptr(), nf, k, o("areas", np.float32, 2), ON_DEVICE, None, None), ()


def check_areas(L, ctx, a, D, o, counts):
    return same(o.get("areas"), sc.face_areas(V, a.astype(np.int64)))


def run_voxelize(L, ctx, a, k, D, o):
    tv, nv, tf, nf = mesh_args(a)
    rows = i64()
    rc = L.pcu_hip_voxelize_triangle_mesh_f32(ctx, tv.data_ptr(), nv, tf.data_ptr(), nf, k, ctypes.addressof(HALF), ctypes.addressof(ZERO), ctypes.addressof(rows),
                                              ON_DEVICE, None, None)
    return rc, (rows.value,)


def check_voxelize(L, ctx, a, D, o, counts):
    want = vc.voxelize(V, a.astype(np.int64), 0.5, (0.0, 0.0, 0.0))
    return counts == (len(want),) and L.pcu_hip_voxelize_take(ctx, len(want), o("ijk", np.int32, len(want), 3), ON_DEVICE, None) == 0 and same(o.get("ijk"), want)


def run_adjacency(L, ctx, a, k, D, o):
    tf = dev(a)
    n = i64()
    return L.pcu_hip_mesh_adjacency(ctx, tf.data_ptr(), 2, k, 4, ctypes.addressof(n), ON_DEVICE, None, None), (n.value,)


def check_adjacency(L, ctx, a, D, o, counts):
    off, nbr = ms.adjacency(a.astype(np.int64), 4)
    return (counts == (len(nbr),) and L.pcu_hip_mesh_adjacency_take(ctx, 4, len(nbr), o("off", np.int64, 5), o("nbr", D, len(nbr)), ON_DEVICE, None) == 0 and
            same(o.get("off"), off) and same(o.get("nbr"), nbr))


def run_vnormals(L, ctx, a, k, D, o):
    tv, nv, tf, nf = mesh_args(a)
    return L.pcu_hip_mesh_vertex_normals_f32(ctx, tv.data_ptr(), nv, tf.data_ptr(), nf, k, 0, o("n", np.float32, 4, 3), ON_DEVICE, None, None), ()


def check_vnormals(L, ctx, a, D, o, counts):
    return same(o.get("n"), ms.vertex_normals(V, a.astype(np.int64), "uniform"))


def run_components(L, ctx, a, k, D, o):
    tf = dev(a)
    n = i64()
    rc = L.pcu_hip_connected_components(ctx, tf.data_ptr(), 2, k, 4, o("cv", D, 4), o("cf", D, 2), o("nv", D, 4), o("nf", D, 4), ctypes.addressof(n), ON_DEVICE,
                                        None, None)
    return rc, (n.value,)


def check_components(L, ctx, a, D, o, counts):
    cv, nv, cf, nf = cc.components(4, a.astype(np.int64))
    return counts == (len(nv),) and same(o.get("cv"), cv) and same(o.get("cf"), cf) and same(o.get("nv", len(nv)), nv) and same(o.get("nf", len(nf)), nf)


def run_remove(L, ctx, a, k, D, o):
    tv, nv, tf, nf = mesh_args(a)
    tm, cv, cf = dev(MASK), i64(), i64()
    rc = L.pcu_hip_remove_mesh_vertices_f32(ctx, tv.data_ptr(), nv, tf.data_ptr(), nf, k, tm.data_ptr(), o("v", np.float32, 4, 3), o("f", D, 2, 3), ctypes.addressof(cv),
                                            ctypes.addressof(cf), ON_DEVICE, None, None)
    return rc, (cv.value, cf.value)


def check_remove(L, ctx, a, D, o, counts):
    v, f = mr.remove_mesh_vertices(V, a, MASK)
    return counts == (len(v), len(f)) and same(o.get("v", len(v)), v) and same(o.get("f", len(f)), f)


def run_unreferenced(L, ctx, a, k, D, o):
    tv, nv, tf, nf = mesh_args(a)
    cv = i64()
    rc = L.pcu_hip_remove_unreferenced_mesh_vertices_f32(ctx, tv.data_ptr(), nv, tf.data_ptr(), nf, k, o("v", np.float32, 4, 3), o("f", D, 2, 3), o("corr_v", D, 4),
                                                         o("corr_f", D, 4), ctypes.addressof(cv), ON_DEVICE, None, None)
    return rc, (cv.value,)


def check_unreferenced(L, ctx, a, D, o, counts):
    v, f, corr_v, corr_f = mr.remove_unreferenced(V, a)
    return (counts == (len(v),) and same(o.get("v", len(v)), v) and same(o.get("f"), f) and same(o.get("corr_v", len(v)), corr_v) and
            same(o.get("corr_f"), corr_f))


def run_dedup(L, ctx, a, k, D, o):
    tv, nv, tf, nf = mesh_args(a)
    cv, cf = i64(), i64()
    rc = L.pcu_hip_deduplicate_mesh_vertices_f32(ctx, tv.data_ptr(), nv, tf.data_ptr(), nf, k, 1e-3, o("v", np.float32, 4, 3), o("f", D, 2, 3), o("svi", np.int32, 4),
                                                 o("svj", np.int32, 4), ctypes.addressof(cv), ctypes.addressof(cf), ON_DEVICE, None, None)
    return rc, (cv.value, cf.value)


def check_dedup(L, ctx, a, D, o, counts):
    v, f, svi, svj = mr.dedup_mesh(V, a, 1e-3)
    return (counts == (len(v), len(f)) and same(o.get("v", len(v)), v) and same(o.get("f", len(f)), f) and same(o.get("svi", len(v)), svi) and
            same(o.get("svj"), svj))


def run_orient(L, ctx, a, k, D, o):
    tf = dev(a)
    n = i64()
    return L.pcu_hip_orient_mesh_faces(ctx, tf.data_ptr(), 2, k, 4, o("f", D, 2, 3), o("c", D, 2), ctypes.addressof(n), ON_DEVICE, None, None), (n.value,)


def check_orient(L, ctx, a, D, o, counts):
    f, patch, _ = mr.orient(a)
    return counts == (int(np.max(patch)) + 1,) and same(o.get("f"), f) and same(o.get("c"), patch)


def run_decimate(L, ctx, a, k, D, o):
    tv, nv, tf, nf = mesh_args(a)
    cv, cf = i64(), i64()
    rc = L.pcu_hip_decimate_triangle_mesh_f32(ctx, tv.data_ptr(), nv, tf.data_ptr(), nf, k, 2, ctypes.addressof(cv), ctypes.addressof(cf), ON_DEVICE, None, None)
    return rc, (cv.value, cf.value)


def check_decimate(L, ctx, a, D, o, counts):
    v, f, corr_v, corr_f = dc.decimate(V, a, 2)
    return (counts == (len(v), len(f)) and
            L.pcu_hip_decimate_triangle_mesh_take(ctx, len(v), len(f), o("v", np.float32, len(v), 3), o("f", D, len(f), 3), o("corr_v", D, len(v)),
                                                  o("corr_f", D, len(f)), ON_DEVICE, None) == 0 and
            same(o.get("v"), v) and same(o.get("f"), f) and same(o.get("corr_v"), corr_v) and same(o.get("corr_f"), corr_f))


def run_marching(L, ctx, a, k, D, o):
    ts, tp, tc = dev(CUBE_S), dev(CUBE_V), dev(a)
    c = (ctypes.c_int64 * 2)(-7, -7)
    rc = L.pcu_hip_marching_cubes_f32(ctx, ts.data_ptr(), tp.data_ptr(), 8, tc.data_ptr(), 1, k, 0.0, ctypes.addressof(c), ON_DEVICE, None, None)
    return rc, (c[0], c[1])


def check_marching(L, ctx, a, D, o, counts):
    v, f = mc.marching_cubes(CUBE_S, CUBE_V, a, 0.0)
    return (counts == (len(v), len(f)) and L.pcu_hip_marching_cubes_take(ctx, len(v), len(f), o("v", np.float32, len(v), 3), o("f", D, len(f), 3), ON_DEVICE, None) == 0 and
            same(o.get("v"), v) and same(o.get("f"), f))


def run_boundary(L, ctx, a, k, D, o):
    t = dev(a)
    n = i64()
    return L.pcu_hip_sparse_voxel_grid_boundary(ctx, t.data_ptr(), 3, k, o("idx", np.int64, 3), ctypes.addressof(n), ON_DEVICE, None), (n.value,)


def check_boundary(L, ctx, a, D, o, counts):
    want = vc.boundary(a.astype(np.int64))
    return counts == (len(want),) and same(o.get("idx", len(want)), want)


def run_hex(L, ctx, a, k, D, o):
    t = dev(a)
    n = i64()
    rc = L.pcu_hip_sparse_voxel_grid_to_hex_mesh(ctx, t.data_ptr(), 3, k, ctypes.addressof(ONE), ctypes.addressof(ZERO), 1, ctypes.addressof(n), ON_DEVICE, None, None)
    return rc, (n.value,)


def check_hex(L, ctx, a, D, o, counts):
    v, cubes = mc.hex_mesh(a.astype(np.int64))
    return (counts == (len(v),) and L.pcu_hip_sparse_voxel_grid_to_hex_mesh_take(ctx, len(v), 3, o("v", np.float64, len(v), 3), o("c", np.int64, 3, 8), ON_DEVICE, None) == 0 and
            same(o.get("v"), v) and same(o.get("c"), cubes))


def run_geometry(L, ctx, a, k, D, o):
    t = dev(a)
    return L.pcu_hip_voxel_grid_geometry(ctx, t.data_ptr(), 3, k, ctypes.addressof(ONE), ctypes.addressof(ZERO), 0.25, o("v", np.float32, 24, 3), o("f", np.int32, 36, 3),
                                         ON_DEVICE, None), ()


def check_geometry(L, ctx, a, D, o, counts):
    v, f = vc.geometry(a, gap_fraction=0.25)
    return same(o.get("v"), v) and same(o.get("f"), f)


# name: (the clean array, the row count that is "past the end", the refusal's text, run, check)
ENTRY_POINTS = {
    "closest_points_on_mesh": (F, 4, FACE_TEXT, run_closest, check_closest),
    "mesh_face_areas": (F, 4, FACE_TEXT, run_areas, check_areas),
    "voxelize_triangle_mesh": (F, 4, FACE_TEXT, run_voxelize, check_voxelize),
    "mesh_adjacency": (F, 4, FACE_TEXT, run_adjacency, check_adjacency),
    "mesh_vertex_normals": (F, 4, FACE_TEXT, run_vnormals, check_vnormals),
    "connected_components": (F, 4, FACE_TEXT, run_components, check_components),
    "remove_mesh_vertices": (F, 4, FACE_TEXT, run_remove, check_remove),
    "remove_unreferenced_mesh_vertices": (F, 4, FACE_TEXT, run_unreferenced, check_unreferenced),
    "deduplicate_mesh_vertices": (F, 4, FACE_TEXT, run_dedup, check_dedup),
    "orient_mesh_faces": (F, 4, FACE_TEXT, run_orient, check_orient),
    "decimate_triangle_mesh": (F, 4, FACE_TEXT, run_decimate, check_decimate),
    "marching_cubes": (CUBE_C, 8, CUBE_TEXT, run_marching, check_marching),
    "sparse_voxel_grid_boundary": (IJK, 3, COORD_TEXT, run_boundary, check_boundary),
    "sparse_voxel_grid_to_hex_mesh": (IJK, 3, COORD_TEXT, run_hex, check_hex),
    "voxel_grid_geometry": (IJK, 3, None, run_geometry, check_geometry),
}
COORDS = ("sparse_voxel_grid_boundary", "sparse_voxel_grid_to_hex_mesh", "voxel_grid_geometry")


def poisons(kind, past_end, coords):
    signed, wide = kind.startswith("int"), kind.endswith("64")
    p = ([("minus_one", -1)] if signed else []) + [("past_end", past_end)] + ([("two_32", 1 << 32)] if wide else []) + ([("all_ones", (1 << 64) - 1)] if kind == "uint64" else [])
    return p + ([("window", 1 << 20)] if coords else [])


# What is no error, by name, and why. Those calls return 0 and are held to the contract with the value in place.
def not_refused(name, kind, poison):
    if name == "voxel_grid_geometry":
        return "voxel_grid_geometry checks no range: every coordinate has a place in space, and the result is float32"
    if name in COORDS and poison == "minus_one":
        return "a voxel coordinate may be negative: the window is [-2^20, 2^20)"
    if name in COORDS and poison == "past_end":
        return "a voxel coordinate is no row index: the number of rows is inside the window"
    return None


CASES = [(name, kind, pname, value) for name, (a, past_end, _, _, _) in ENTRY_POINTS.items() for kind in KINDS for pname, value in poisons(kind, past_end, name in COORDS)]


def test_the_combinations_that_are_no_error_stay_under_one_in_five():
    listed = [c for c in CASES if not_refused(c[0], c[1], c[2])]
    assert len(CASES) == 15 * 9 + 3 * 4 and 5 * len(listed) < len(CASES), (len(listed), len(CASES))


@pytest.mark.parametrize("kind", list(KINDS))
@pytest.mark.parametrize("name", list(ENTRY_POINTS))
def test_every_kind_is_read_whole_and_checked_before_it_is_narrowed(gpu, name, kind):
    L, ctx = gpu.lib(), gpu.ctx()
    clean, past_end, text, run, check = ENTRY_POINTS[name]
    k, D = KINDS[kind]
    clean = np.ascontiguousarray(clean.astype(D))
    for pname, value in poisons(kind, past_end, name in COORDS):
        a = clean.copy()
        a.reshape(-1)[-1] = np.array(value % (1 << 64), dtype=np.uint64).astype(D)         # (wraps: -1 is all ones in every kind)
        o = Outs()
        rc, counts = run(L, ctx, a, k, D, o)
        if not_refused(name, kind, pname):
            assert rc == 0 and check(L, ctx, a, D, o, counts), (name, kind, pname, rc, counts)
            continue
        assert rc == gpu.ERR_INVALID, (name, kind, pname, rc)
        assert gpu.last_error() == text, (name, kind, pname)
        assert o.untouched() and all(c == 0 for c in counts), (name, kind, pname, counts)
    o = Outs()
    rc, counts = run(L, ctx, clean, k, D, o)
    assert rc == 0 and check(L, ctx, clean, D, o, counts), (name, kind, rc, counts, gpu.last_error())
