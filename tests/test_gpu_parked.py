"""The one result a context parks for a _take call (-m gpu), through the C entry points as _lib.lib() binds them: every kind is taken once and
only with its own counts, any later use of the context's auxiliary block drops it, operators that do not use the block leave it alone, and a
result larger than the block makes the block grow. Expected bytes come from the contract modules, never from the library."""
import ctypes

import numpy as np
import pytest

import decimate_contract as dc
import marching_cubes_contract as mc
import mesh_smooth_contract as ms
import radius_contract as rc
import voxelize_contract as vc

pytestmark = pytest.mark.gpu

ON_DEVICE = 1                       # PCU_HIP_PTRS_ON_DEVICE
INT32, INT64 = 0, 1                 # PCU_HIP_FACE_*


@pytest.fixture(scope="module")
def gpu():
    from point_cloud_utils_amd import _lib
    assert _lib.device_count() > 0, "no GPU visible: the gfx950 path has no CPU fallback"
    return _lib


# ---------------------------------------------------------------------------------------------------- the smallest input of every kind
TET_V, TET_F = (a.astype(t) for a, t in zip(ms.tetrahedron(), (np.float32, np.int32)))
VOX_SIZE, VOX_ORIGIN = (ctypes.c_double * 3)(0.25, 0.25, 0.25), (ctypes.c_double * 3)(0.0, 0.0, 0.0)      # the unit tetrahedron: about 4 voxels across
TWO_VOXELS = np.array([[0, 0, 0], [1, 0, 0]], dtype=np.int32)
ONE, ZERO = (ctypes.c_double * 3)(1.0, 1.0, 1.0), (ctypes.c_double * 3)(0.0, 0.0, 0.0)
HEX_V, HEX_C = mc.hex_mesh(TWO_VOXELS)                                                                       # 12 vertices, 2 cubes
MC_S = np.ascontiguousarray(HEX_V[:, 0] - 0.5)
POINTS = np.random.default_rng(11).random((64, 3), dtype=np.float32)


class Kind:
    """One parking operator: park(L, ctx) -> its counts; take(L, ctx, counts, outs, flags) -> rc; want: the contract's arrays."""

    def outs(self, device):
        if not device:
            return [np.empty_like(w) for w in self.want]
        import torch
        return [torch.empty(w.shape, dtype=getattr(torch, w.dtype.name), device="cuda") for w in self.want]

    def take(self, L, ctx, counts, outs, device=False):
        ptrs = [o.data_ptr() if device else o.ctypes.data for o in outs]
        return self.take_fn(L)(ctx, *counts, *ptrs, ON_DEVICE if device else 0, None)

    def matches(self, outs, device=False):
        got = [o.cpu().numpy() if device else o for o in outs]
        return all(g.dtype == w.dtype and g.tobytes() == w.tobytes() for g, w in zip(got, self.want))


class Voxelization(Kind):
    text = "holds no voxelization"
    want = [vc.voxelize(TET_V, TET_F, 0.25, (0.0, 0.0, 0.0))]
    counts = (len(want[0]),)

    def park(self, L, ctx):
        rows = ctypes.c_int64(0)
        rc = L.pcu_hip_voxelize_triangle_mesh_f32(ctx, TET_V.ctypes.data, 4, TET_F.ctypes.data, 4, INT32, ctypes.addressof(VOX_SIZE),
                                                  ctypes.addressof(VOX_ORIGIN), ctypes.addressof(rows), 0, None, None)
        return rc, (rows.value,)

    def take_fn(self, L):
        return L.pcu_hip_voxelize_take


class Surface(Kind):
    text = "holds no surface"
    want = list(mc.marching_cubes(MC_S, HEX_V, HEX_C, 0.0))
    counts = (len(want[0]), len(want[1]))

    def park(self, L, ctx, m=2):
        c = (ctypes.c_int64 * 2)(0, 0)
        rc = L.pcu_hip_marching_cubes_f64(ctx, MC_S.ctypes.data, HEX_V.ctypes.data, 12, HEX_C.ctypes.data, m, INT64, 0.0, ctypes.addressof(c), 0, None, None)
        return rc, (c[0], c[1])

    def take_fn(self, L):
        return L.pcu_hip_marching_cubes_take


class HexMesh(Kind):
    text = "holds no hex mesh"

    def __init__(self, ijk=TWO_VOXELS):
        self.ijk = np.ascontiguousarray(ijk, dtype=np.int32)
        self.want = list(mc.hex_mesh(self.ijk))
        self.counts = (len(self.want[0]), len(self.ijk))

    def park(self, L, ctx):
        nv = ctypes.c_int64(0)
        rc = L.pcu_hip_sparse_voxel_grid_to_hex_mesh(ctx, self.ijk.ctypes.data, len(self.ijk), INT32, ctypes.addressof(ONE), ctypes.addressof(ZERO), 1,
                                                     ctypes.addressof(nv), 0, None, None)
        return rc, (nv.value, len(self.ijk))

    def take_fn(self, L):
        return L.pcu_hip_sparse_voxel_grid_to_hex_mesh_take


class Adjacency(Kind):
    text = "holds no adjacency"
    want = [a.astype(t) for a, t in zip(ms.adjacency(TET_F.astype(np.int64), 4), (np.int64, np.int32))]
    counts = (4, len(want[1]))

    def park(self, L, ctx):
        n = ctypes.c_int64(0)
        rc = L.pcu_hip_mesh_adjacency(ctx, TET_F.ctypes.data, 4, INT32, 4, ctypes.addressof(n), 0, None, None)
        return rc, (4, n.value)

    def take_fn(self, L):
        return L.pcu_hip_mesh_adjacency_take


class Decimated(Kind):
    """Four segments: vertices, faces and the two correspondences. The octahedron, down to four faces."""
    text = "holds no decimated mesh"
    V, F = (a.astype(t) for a, t in zip(dc.mesh("octahedron"), (np.float32, np.int32)))
    want = list(dc.decimate(V, F, 4))
    counts = (len(want[0]), len(want[1]))

    def park(self, L, ctx):
        nv, nf = ctypes.c_int64(0), ctypes.c_int64(0)
        rc_ = L.pcu_hip_decimate_triangle_mesh_f32(ctx, self.V.ctypes.data, len(self.V), self.F.ctypes.data, len(self.F), INT32, 4, ctypes.addressof(nv),
                                                   ctypes.addressof(nf), 0, None, None)
        return rc_, (nv.value, nf.value)

    def take_fn(self, L):
        return L.pcu_hip_decimate_triangle_mesh_take


class RadiusRows(Kind):
    """The rows of a radius search of the 64 points among themselves; the offsets come back with the call that parks them."""
    text = "holds no radius result"
    RADIUS = 0.3
    offsets, *want = rc.radius_search(POINTS, POINTS, RADIUS)
    counts = (64, len(want[0]))

    def park(self, L, ctx):
        off, total = np.empty(65, dtype=np.int64), ctypes.c_int64(0)
        rc_ = L.pcu_hip_radius_search_f32(ctx, POINTS.ctypes.data, 64, POINTS.ctypes.data, 64, self.RADIUS, 1, off.ctypes.data, ctypes.addressof(total), 0, None, None)
        assert rc_ != 0 or np.array_equal(off, self.offsets)
        return rc_, (64, total.value)

    def take_fn(self, L):
        return L.pcu_hip_radius_search_take


KINDS = [Voxelization(), Surface(), HexMesh(), Adjacency(), Decimated(), RadiusRows()]
IDS = [type(k).__name__ for k in KINDS]


def park(kind, L, ctx):
    rc, counts = kind.park(L, ctx)
    assert rc == 0 and tuple(counts) == tuple(kind.counts), (type(kind).__name__, rc, counts, kind.counts)


def normals_knn(L, ctx):
    out_n, keep = np.empty((64, 3), dtype=np.float32), np.empty(64, dtype=np.uint8)
    return L.pcu_hip_normals_knn_f32(ctx, POINTS.ctypes.data, 64, None, 4, 10, np.pi / 2, out_n.ctypes.data, keep.ctypes.data, 0, None, None)


# ---------------------------------------------------------------------------------------------------- 1. taken once, with its own counts
@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
@pytest.mark.parametrize("kind", KINDS, ids=IDS)
def test_every_kind_is_taken_once_and_only_with_its_own_counts(gpu, kind, device):
    L, ctx = gpu.lib(), gpu.ctx()
    park(kind, L, ctx)
    outs = kind.outs(device)
    for i in range(len(kind.counts)):                       # a wrong first count; a wrong second count where there is one
        wrong = tuple(c + (j == i) for j, c in enumerate(kind.counts))
        assert kind.take(L, ctx, wrong, outs, device) == gpu.ERR_INVALID
        assert kind.text in gpu.last_error()
    assert kind.take(L, ctx, kind.counts, outs, device) == 0            # ... which left the result in place
    assert kind.matches(outs, device)
    assert kind.take(L, ctx, kind.counts, outs, device) == gpu.ERR_INVALID
    assert kind.text in gpu.last_error()


# ---------------------------------------------------------------------------------------------------- 2. any other use of the block drops it
def test_every_later_use_of_the_block_drops_the_parked_result(gpu):
    L, ctx = gpu.lib(), gpu.ctx()
    pairs = []
    for a in KINDS:
        later = [b for b in KINDS if b is not a] + ["normals_knn"] + (["refused marching cubes"] if isinstance(a, Voxelization) else [])
        for b in later:
            park(a, L, ctx)
            if b == "normals_knn":
                assert normals_knn(L, ctx) == 0
            elif b == "refused marching cubes":             # every parking entry point drops what is parked when it is entered
                rc, _ = Surface().park(L, ctx, m=0)
                assert rc == gpu.ERR_INVALID and "cube_indices has zero rows" in gpu.last_error()
            else:
                park(b, L, ctx)
            assert a.take(L, ctx, a.counts, a.outs(False)) == gpu.ERR_INVALID, (type(a).__name__, b)
            assert a.text in gpu.last_error()
            if isinstance(b, Kind):
                outs = b.outs(False)
                assert b.take(L, ctx, b.counts, outs) == 0 and b.matches(outs), (type(a).__name__, type(b).__name__)
            pairs.append((a, b))
    assert len(pairs) == len(KINDS) * len(KINDS) + 1


# ---------------------------------------------------------------------------------------------------- 3. operators that do not use the block
def test_operators_that_do_not_use_the_block_leave_the_parked_result_alone(gpu):
    L, ctx = gpu.lib(), gpu.ctx()
    vox = KINDS[0]
    park(vox, L, ctx)
    areas = np.empty(4, dtype=np.float32)
    assert L.pcu_hip_mesh_face_areas_f32(ctx, TET_V.ctypes.data, 4, TET_F.ctypes.data, 4, INT32, areas.ctypes.data, 0, None, None) == 0
    ijk = vox.want[0]
    idx, cnt = np.empty(len(ijk), dtype=np.int64), ctypes.c_int64(0)
    assert L.pcu_hip_sparse_voxel_grid_boundary(ctx, ijk.ctypes.data, len(ijk), INT32, idx.ctypes.data, ctypes.addressof(cnt), 0, None) == 0
    assert np.array_equal(idx[:cnt.value], vc.boundary(ijk))
    outs = vox.outs(False)
    assert vox.take(L, ctx, vox.counts, outs) == 0 and vox.matches(outs)


# ---------------------------------------------------------------------------------------------------- 4. a result larger than the block
def test_a_result_larger_than_the_block_replaces_the_smaller_one(gpu):
    """A context of its own, so that the block starts empty and gets the smallest capacity there is (1 MiB) with the first result. The hex
    mesh of 16^3 voxels (0.36 MiB) fits it; that of 24^3 (1.2 MiB) does not, so the block is freed and allocated again."""
    L = gpu.lib()
    ctx = ctypes.c_void_p()
    assert L.pcu_hip_ctx_create(gpu.default_device(), ctypes.byref(ctx)) == 0
    try:
        small = KINDS[2]
        for side in (16, 24):
            big = HexMesh(np.stack(np.meshgrid(*[np.arange(side)] * 3, indexing="ij"), axis=-1).reshape(-1, 3))
            park(small, L, ctx)
            park(big, L, ctx)
            assert small.take(L, ctx, small.counts, small.outs(False)) == gpu.ERR_INVALID
            outs = big.outs(False)
            assert big.take(L, ctx, big.counts, outs) == 0 and big.matches(outs), side
    finally:
        L.pcu_hip_ctx_destroy(ctx)
