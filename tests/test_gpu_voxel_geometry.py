"""voxel_grid_geometry on the GPU (-m gpu): the bits of the float32 vertices and the faces against the numpy restatement of
tests/voxelize_contract.py, and the round trip mesh -> voxels -> cubes -> rays that holds the two origin conventions
together."""
import numpy as np
import pytest

import voxelize_contract as vc
from test_voxelize_contract import grid_for, voxels

pytestmark = pytest.mark.gpu

INT_DTYPES = [np.int32, np.int64, np.uint32, np.uint64]


@pytest.fixture(scope="module")
def pcu():
    import point_cloud_utils_amd as m
    from point_cloud_utils_amd import _lib
    assert _lib.device_count() > 0, "no GPU visible: the gfx950 path has no CPU fallback"
    return m


def to_torch(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def same(got, want, what=""):
    (v, f), (wv, wf) = got, want
    v, f = np.asarray(v), np.asarray(f)
    assert v.dtype == np.float32 and f.dtype == np.int32 and v.shape == wv.shape and f.shape == wf.shape, (what, v.dtype, f.dtype, v.shape, f.shape)
    assert np.array_equal(v.view(np.uint32), wv.view(np.uint32)), what
    assert np.array_equal(f, wf), what


def cells(n, seed, lo=-50, hi=50):
    return np.random.default_rng(seed).integers(lo, hi, (n, 3))


@pytest.mark.parametrize("gap", [0.0, 0.1])
@pytest.mark.parametrize("n", [1, 64, 257, 333])
def test_sizes_and_gaps(pcu, n, gap):
    ijk = cells(n, n).astype(np.int32)                     # (negative coordinates among them)
    size, origin = (0.3, 0.7, 1.9), (-1.25, 0.1, 1e3)
    assert n == 1 or ijk.min() < 0
    same(pcu.voxel_grid_geometry(ijk, size, origin, gap), vc.geometry(ijk, size, origin, gap), (n, gap))


def test_defaults_and_a_scalar_size(pcu):
    ijk = cells(100, 5).astype(np.int64)
    same(pcu.voxel_grid_geometry(ijk), vc.geometry(ijk))
    same(pcu.voxel_grid_geometry(ijk, 0.1), vc.geometry(ijk, 0.1))
    same(pcu.voxel_grid_geometry(ijk, voxel_origin=[1.0, 2.0, 3.0], gap_fraction=0.25), vc.geometry(ijk, 1.0, (1.0, 2.0, 3.0), 0.25))


@pytest.mark.parametrize("dt", INT_DTYPES)
def test_dtypes_and_torch(pcu, dt):
    import torch
    unsigned = np.dtype(dt).kind == "u"
    ijk = cells(300, 9, 0 if unsigned else -2 ** 20, 2 ** 20).astype(dt)
    size, origin = (1e-3, 2e-3, 0.5e-3), (0.1, 0.2, 0.3)
    want = vc.geometry(ijk, size, origin, 0.1)
    same(pcu.voxel_grid_geometry(ijk, size, origin, 0.1), want, dt)
    if not unsigned:
        v, f = pcu.voxel_grid_geometry(to_torch(ijk), size, origin, 0.1)
        assert v.is_cuda and f.is_cuda and v.dtype == torch.float32 and f.dtype == torch.int32
        same((v.cpu().numpy(), f.cpu().numpy()), want, (dt, "torch"))


def test_round_trip_holds_the_two_origin_conventions_together(pcu):
    """The voxels of voxelize_triangle_mesh(v, f, s, o) are centred on o + ijk s; voxel_grid_geometry draws voxel 0 from its corner, so the
    cubes are made with o - s / 2. Then (a) a ray from a voxel's centre along +x leaves its cube after s_x / 2, and (b) every vertex of the
    mesh lies in a box of the restatement, so a ray started there hits a cube within one cube diagonal."""
    v, f = vc.golden_mesh("bunny", np.float32)
    size, origin = grid_for(v, 16)
    ijk = pcu.voxelize_triangle_mesh(v, f, size, origin)
    assert np.array_equal(ijk, voxels("bunny", 16))
    gv, gf = pcu.voxel_grid_geometry(ijk, size, origin - size / 2)
    same((gv, gf), vc.geometry(ijk, size, origin - size / 2))
    eps = 1e-5 * float(np.abs(gv).max())                   # float32 vertices: a few ulps of the largest coordinate
    # (a)
    # (the origins sit off the centre line, so that no ray leaves through the diagonal edge of a cube's side)
    centres = (origin + ijk.astype(np.float64) * size + size * np.array([0.0, 0.1, 0.2])).astype(np.float32)
    d = np.tile(np.array([[1.0, 0.0, 0.0]], dtype=np.float32), (len(ijk), 1))
    fid, _, t = pcu.ray_mesh_intersection(gv, gf, centres, d)
    assert bool((fid >= 0).all())
    assert bool((np.abs(t - size[0] / 2) <= eps).all()), float(np.abs(t - size[0] / 2).max())
    # (b)
    assert bool(vc.inside_boxes(v, ijk, size, origin).all())
    d = np.tile(np.array([[0.3, 0.5, 0.8]], dtype=np.float32), (len(v), 1))
    fid, _, t = pcu.ray_mesh_intersection(gv, gf, v, d)
    diag = float(np.sqrt((size * size).sum())) / float(np.sqrt(0.3 ** 2 + 0.5 ** 2 + 0.8 ** 2))
    assert bool((fid >= 0).all()) and bool((t >= 0).all()) and bool((t <= diag + eps).all()), (int((fid < 0).sum()), float(t.max()), diag)
