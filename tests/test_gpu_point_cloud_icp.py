"""register_point_clouds_icp on the GPU (-m gpu) against tests/icp_contract.py: every field of IcpResult by dtype, shape and bytes (floats by
struct.pack), no tolerance, float32 and float64, point-to-point and point-to-plane, numpy arrays and device tensors, every call made twice with
equal bytes, DatasetIndex.register_icp over two grids. The contract's `nearest` is the library's own k = 1 search, so exact ties are resolved
in the library's order on both sides. The shapes are the smallest that reach each level of the sum tree of csrc/icp.h: one lane, a wave minus
one, a wave, a wave plus one, several waves, a block (4096 rows), a block plus one row, a block plus one wave, and 262145 rows for the fourth
level. The cancellation test is tests/test_gpu_zz_icp_cancel.py, and this file sorts behind tests/test_gpu_mesh_sampling.py."""
import ctypes
import math
import struct

import numpy as np
import pytest

import icp_contract as ic
from test_icp_contract import MOTION_R, MOTION_T, ellipsoid, rotation

pytestmark = pytest.mark.gpu

DTYPES = [np.float32, np.float64]
MODES = ["point", "plane"]


@pytest.fixture(scope="module")
def pcu():
    import point_cloud_utils_amd as m
    from point_cloud_utils_amd import _lib
    assert _lib.device_count() > 0, "no GPU visible: the gfx950 path has no CPU fallback"
    return m


def host(x):
    return x.cpu().numpy() if hasattr(x, "cpu") else x


def same(got, want, like):
    """Every field of IcpResult; arrays are of `like`'s kind."""
    assert type(got).__name__ == "IcpResult" and got._fields == want._fields
    assert type(got.transform) is type(like)
    t = host(got.transform)
    assert t.dtype == np.float64 and t.shape == (4, 4)
    assert t.tobytes() == want.transform.tobytes(), (got.status, want.status, got.iterations, want.iterations, np.abs(t - want.transform).max())
    assert type(got.fitness) is float and struct.pack("d", got.fitness) == struct.pack("d", want.fitness), (got.fitness, want.fitness)
    assert type(got.inlier_rmse) is float and struct.pack("d", got.inlier_rmse) == struct.pack("d", want.inlier_rmse), (got.inlier_rmse, want.inlier_rmse)
    assert type(got.iterations) is int and got.iterations == want.iterations
    assert got.status == want.status
    if want.correspondences is None:
        assert got.correspondences is None
    else:
        assert type(got.correspondences) is type(like)
        c = host(got.correspondences)
        assert c.dtype == np.int64 and c.shape == want.correspondences.shape and c.tobytes() == want.correspondences.tobytes()


def pair(n, m, dtype, seed=5):
    """m target points on the ellipsoid with their normals, and n other points of it moved back by the motion of tests/test_icp_contract.py."""
    tgt, nrm = ellipsoid(m, dtype, seed=seed)
    on, _ = ellipsoid(n, np.float64, seed=seed + 1000)
    src = ((on - MOTION_T) @ MOTION_R).astype(dtype)
    return src, tgt, nrm


def check(pcu, src, tgt, nrm, tensors=False, k_hints=(), **kw):
    """The free function twice on numpy arrays (and on tensors), then an index per k_hint, against the contract over the library's own search.
    Returns the contract's result."""
    want = ic.register_icp(src, tgt, nrm, nearest=lambda p, t: pcu.k_nearest_neighbors(p, t, 1, squared_distances=True), **kw)
    kinds = [(src, tgt, nrm)]
    if tensors:
        import torch
        kinds.append(tuple(None if a is None else torch.from_numpy(a).cuda() for a in (src, tgt, nrm)))
    for s, t, nn in kinds:
        got = pcu.register_point_clouds_icp(s, t, nn, **kw)
        same(got, want, s)
        stats = pcu.last_stats()
        assert stats["n_passes"] == got.iterations + 1 and stats["n_grid_builds"] == got.iterations + 2 and stats["n_queries"] == len(src)
        same(pcu.register_point_clouds_icp(s, t, nn, **kw), want, s)            # equal calls, equal bytes
        for k_hint in k_hints:
            with pcu.DatasetIndex(t, k_hint=k_hint) as index:
                got = index.register_icp(s, nn, **kw)
                same(got, want, s)
                stats = pcu.last_stats()
                assert stats["n_passes"] == got.iterations + 1 and stats["n_grid_builds"] == got.iterations + 1
                same(index.register_icp(s, nn, **kw), want, s)
    return want


def index_contract_agrees(pcu, src, tgt, nrm, **kw):
    """The contract over index.k_nearest_neighbors gives the bytes of the contract over the free search."""
    with pcu.DatasetIndex(tgt, k_hint=16) as index:
        return ic.register_icp(src, tgt, nrm, nearest=lambda p, t: index.k_nearest_neighbors(p, 1, squared_distances=True), **kw)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("m", [1, 300, 5000])
def test_sizes_around_a_wave_and_a_block(pcu, dtype, mode, m):
    for n in (1, 63, 64, 65, 257, 4096, 4097, 4160):
        src, tgt, nrm = pair(n, m, dtype)
        check(pcu, src, tgt, nrm if mode == "plane" else None, tensors=n in (1, 65, 4097), k_hints=(1, 16) if n in (257, 4160) else (),
              max_iterations=5, return_correspondences=True)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("dtype", DTYPES)
def test_the_fourth_fold_level(pcu, dtype, mode):
    src, tgt, nrm = pair(262145, 5000, dtype)
    r = check(pcu, src, tgt, nrm if mode == "plane" else None, tensors=True, k_hints=(16,), max_iterations=3, return_correspondences=True)
    assert r.fitness == 1.0 and r.iterations <= 3 and r.status in ("max_iterations", "converged")


INIT = np.eye(4)
INIT[:3, :3], INIT[:3, 3] = rotation((0.0, 1.0, 1.0), -0.07), (0.01, 0.02, -0.015)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("dtype", DTYPES)
def test_iteration_counts_name_the_step(pcu, dtype, mode):
    """0: transform, search, inliers and the d2 fold; 1 adds one solve; 30 runs to convergence."""
    src, tgt, nrm = pair(1000, 1200, dtype)
    nrm = nrm if mode == "plane" else None
    for init in (None, INIT):
        for max_iterations in (0, 1, 2, 5, 30):
            r = check(pcu, src, tgt, nrm, tensors=max_iterations == 2, k_hints=(1, 16) if max_iterations == 5 else (), init_transform=init,
                      max_iterations=max_iterations, return_correspondences=max_iterations in (0, 30))
            assert r.iterations <= max_iterations and r.fitness == 1.0 and (r.status == "max_iterations" or max_iterations >= 5)
        assert r.status == "converged" or mode == "point"                  # (point-to-point creeps along the surface: 17 to over 30 updates here)
    want = ic.register_icp(src, tgt, nrm, nearest=lambda p, t: pcu.k_nearest_neighbors(p, t, 1, squared_distances=True))
    assert index_contract_agrees(pcu, src, tgt, nrm).transform.tobytes() == want.transform.tobytes()


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("dtype", DTYPES)
def test_far_outliers_take_no_part(pcu, dtype, mode):
    src, tgt, nrm = pair(3000, 3000, dtype)
    out = np.random.default_rng(8).choice(3000, 300, replace=False)
    src[out] += np.asarray([3.0, -2.0, 4.0], dtype)
    r = check(pcu, src, tgt, nrm if mode == "plane" else None, tensors=True, k_hints=(1, 16), max_correspondence_distance=0.1,
              return_correspondences=True)
    assert r.status == ("converged" if mode == "plane" else "max_iterations") and r.fitness == 0.9
    assert (r.correspondences[out] == -1).all() and (np.delete(r.correspondences, out) >= 0).all()


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("dtype", DTYPES)
def test_exact_ties_follow_the_library(pcu, dtype, mode):
    """Every target row twice: each search has an exact tie, resolved in k_nearest_neighbors' order on both sides."""
    src, tgt, nrm = pair(700, 400, dtype)
    tgt, nrm = np.repeat(tgt, 2, axis=0), np.repeat(nrm, 2, axis=0)
    r = check(pcu, src, tgt, nrm if mode == "plane" else None, tensors=True, k_hints=(1, 16), return_correspondences=True)
    assert r.status == "converged"


@pytest.mark.parametrize("dtype", DTYPES)
def test_named_outcomes(pcu, dtype):
    src, tgt, nrm = pair(300, 300, dtype)
    r = check(pcu, src, tgt, None, k_hints=(1,), max_correspondence_distance=0.0, return_correspondences=True)
    assert (r.status, r.fitness, r.inlier_rmse, r.iterations) == ("no_correspondences", 0.0, 0.0, 0) and (r.correspondences == -1).all()
    r = check(pcu, src, tgt, nrm, k_hints=(1,), init_transform=INIT, max_iterations=0)
    assert r.status == "max_iterations" and r.transform.tobytes() == INIT.tobytes()
    flat = np.random.default_rng(3).random((200, 3)).astype(dtype)
    flat[:, 2] = 0
    up = np.zeros((200, 3), dtype)
    up[:, 2] = 1
    r = check(pcu, src, flat, up, tensors=True, k_hints=(1,))
    assert r.status == "degenerate" and r.iterations == 0 and np.array_equal(r.transform, np.eye(4))
    bad = nrm.copy()
    bad[::7, 1] = np.nan
    assert check(pcu, src, tgt, bad).status == "degenerate"
    for normals in (None, nrm):
        r = check(pcu, tgt, tgt, normals, tensors=True, return_correspondences=True)
        assert (r.status, r.iterations, r.inlier_rmse) == ("converged", 1, 0.0) and np.array_equal(r.correspondences, np.arange(300))


@pytest.mark.parametrize("mode", MODES)
def test_float32_far_from_the_origin(pcu, mode):
    """(Bytes only. The plane step linearises the rotation about the origin, as Open3D's does: this far from it the step overshoots and the
    contract itself ends as "degenerate"; the point step does not care. DESIGN.md, f21.)"""
    src, tgt, nrm = pair(2000, 2000, np.float32)
    check(pcu, src + np.float32(1000), tgt + np.float32(1000), nrm if mode == "plane" else None, tensors=True, k_hints=(16,),
          return_correspondences=True)


def test_registration_claims_the_parking_block(pcu):
    """A radius search parks its rows in the context; the registration then uses that block, and the rows' take is refused with its text."""
    from point_cloud_utils_amd import _lib
    L, ctx = _lib.lib(), _lib.ctx()
    p = np.random.default_rng(11).random((64, 3), dtype=np.float32)
    off, total = np.empty(65, dtype=np.int64), ctypes.c_int64(0)
    assert L.pcu_hip_radius_search_f32(ctx, p.ctypes.data, 64, p.ctypes.data, 64, 0.3, 1, off.ctypes.data, ctypes.addressof(total), 0, None, None) == 0
    src, tgt, _ = pair(100, 120, np.float32)
    assert pcu.register_point_clouds_icp(src, tgt).status == "converged"
    idx, d = np.empty(total.value, np.int64), np.empty(total.value, np.float32)
    assert L.pcu_hip_radius_search_take(ctx, 64, total.value, idx.ctypes.data, d.ctypes.data, 0, None) == _lib.ERR_INVALID
    assert "holds no radius result" in _lib.last_error()


def test_refusals_of_the_search_come_through(pcu):
    src, tgt, nrm = pair(100, 120, np.float64)
    tgt[5, 1] = math.nan
    with pytest.raises(ValueError, match="dataset_points contains NaN coordinates"):
        pcu.register_point_clouds_icp(src, tgt)
    with pytest.raises(ValueError, match="dataset_points contains NaN coordinates"):
        ic.register_icp(src, tgt, nearest=lambda p, t: pcu.k_nearest_neighbors(p, t, 1, squared_distances=True))
