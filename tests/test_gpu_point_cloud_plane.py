"""segment_point_cloud_plane on the GPU (-m gpu) against tests/plane_contract.py: every field of PlaneResult by dtype, shape and bytes (floats
by struct.pack), no tolerance, float32 and float64, refit on and off, numpy arrays and device tensors, every call made twice with equal bytes.
The shapes are the smallest that reach each edge of csrc/plane.h: three rows, a wave minus one, a wave, a wave plus one, the 64 * R rows of a
scoring wave and one either side, a block of the sum tree (4096 rows), a block plus one row, a block plus one wave, and 262145 rows for the
fourth level of the sum tree; hypothesis counts around the 64 whose scores leave a wave together; scoring cut into several launches. The
cancellation test is tests/test_gpu_zz_plane_cancel.py, and this file sorts behind tests/test_gpu_mesh_sampling.py."""
import struct

import numpy as np
import pytest

import plane_contract as pc
from test_plane_contract import collinear, coplanar_grid, half_repeated, identical, planted, strictness_grid

pytestmark = pytest.mark.gpu

DTYPES = [np.float32, np.float64]
THR = 0.01


@pytest.fixture(scope="module")
def pcu():
    import point_cloud_utils_amd as m
    from point_cloud_utils_amd import _lib
    assert _lib.device_count() > 0, "no GPU visible: the gfx950 path has no CPU fallback"
    return m


@pytest.fixture(scope="module")
def R(pcu):
    from point_cloud_utils_amd import _plane
    rows, launch_tests = _plane._geometry()
    assert rows >= 1 and launch_tests >= 2 ** 20
    return rows


def host(x):
    return x.cpu().numpy() if hasattr(x, "cpu") else x


def same(got, want, like):
    """Every field of PlaneResult; arrays are of `like`'s kind."""
    assert type(got).__name__ == "PlaneResult" and got._fields == want._fields
    assert got.status == want.status
    assert type(got.best_iteration) is int and got.best_iteration == want.best_iteration
    assert type(got.random_seed) is int and got.random_seed == want.random_seed
    assert type(got.plane) is type(like) and type(got.inliers) is type(like)
    p, i = host(got.plane), host(got.inliers)
    assert p.dtype == np.float64 and p.shape == (4,)
    assert struct.pack("4d", *p.tolist()) == struct.pack("4d", *want.plane.tolist()), (p, want.plane)
    assert i.dtype == np.int64 and i.shape == want.inliers.shape and i.tobytes() == want.inliers.tobytes()


def check(pcu, P, thr, H, seed, tensors=True, call=None):
    """Both refit modes, numpy (and tensors), each call twice, against the contract. Returns the contract's results (refit off, on)."""
    call = call or pcu.segment_point_cloud_plane
    wants = []
    kinds = [P]
    if tensors:
        import torch
        kinds.append(torch.from_numpy(P).cuda())
    for refit in (False, True):
        want = pc.segment_plane(P, thr, H, seed, refit=refit)
        wants.append(want)
        for A in kinds:
            same(call(A, thr, H, seed, refit), want, A)
            assert pcu.last_stats()["n_queries"] == len(P)
            same(call(A, thr, H, seed, refit), want, A)              # equal calls, equal bytes
    return wants


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("n", [3, 63, 64, 65, "64R-1", "64R", "64R+1", 4096, 4097, 4160, 262145])
def test_shapes(pcu, R, dtype, n):
    n = {"64R-1": 64 * R - 1, "64R": 64 * R, "64R+1": 64 * R + 1}.get(n, n)
    off, on = check(pcu, planted(n, dtype), THR, 128, 3)
    assert on.status == "ok" and len(on.inliers) >= 3 and len(off.inliers) >= 3


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("H", [1, 63, 64, 65, 1000])
def test_hypothesis_counts(pcu, dtype, H):
    check(pcu, planted(4097, dtype), THR, H, 3)


@pytest.mark.parametrize("dtype", DTYPES)
def test_scoring_in_several_launches(pcu, dtype):
    """The launch cut at n * 128 tests: 128 hypotheses are one launch, 129 two, 300 three; the bytes are those of the uncut call and the
    contract's. The default cut takes one launch for all of them."""
    from point_cloud_utils_amd import _plane
    P = planted(4097, dtype)
    for H, launches in ((128, 1), (129, 2), (300, 3)):
        def cut(A, thr, H, seed, refit):
            r = _plane._forced(A, thr, H, seed, refit, launch_tests=len(P) * 128)
            assert pcu.last_stats()["n_passes"] == launches
            return r
        check(pcu, P, THR, H, 3, call=cut)
        pcu.segment_point_cloud_plane(P, THR, H, 3)
        assert pcu.last_stats()["n_passes"] == 1
    with pytest.raises(ValueError, match="launch_tests"):
        _plane._forced(P, THR, 64, 3, launch_tests=-1)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("seed", [1, 2 ** 32 - 1])
def test_seeds(pcu, dtype, seed):
    check(pcu, planted(1000, dtype), THR, 128, seed)


@pytest.mark.parametrize("dtype", DTYPES)
def test_strictness_grid(pcu, dtype):
    P = strictness_grid(dtype)
    off, on = check(pcu, P, 0.5, 64, 1)
    assert len(off.inliers) == 65
    pcu.segment_point_cloud_plane(P, 0.5, 64, 1, refit=False)
    assert pcu.last_stats()["n_escalated"] == 65                    # the winner's score


@pytest.mark.parametrize("dtype", DTYPES)
def test_coplanar_grid(pcu, dtype):
    P = coplanar_grid(dtype)
    off, on = check(pcu, P, 0.25, 64, 1)
    assert len(off.inliers) == len(on.inliers) == len(P)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("cloud", [collinear, identical])
def test_no_plane(pcu, dtype, cloud):
    off, on = check(pcu, cloud(dtype), 0.5, 64, 1)
    assert off.status == on.status == "no_plane"


@pytest.mark.parametrize("dtype", DTYPES)
def test_threshold_zero_and_hypotheses_without_a_plane(pcu, dtype):
    off, on = check(pcu, planted(300, dtype), 0.0, 64, 1)
    assert off.status == on.status == "no_plane"
    off, on = check(pcu, half_repeated(dtype), 0.05, 64, 1)
    assert off.status == on.status == "ok"


def test_offset_by_1000_float32(pcu):
    off, on = check(pcu, planted(4097, np.float32, 1000.0), THR, 128, 3)
    assert on.status == "ok"


def test_seed_zero_is_from_the_clock(pcu):
    P = planted(1000, np.float32)
    got = pcu.segment_point_cloud_plane(P, THR, 128)
    assert type(got.random_seed) is int and 1 <= got.random_seed <= 0xFFFFFFFF
    same(got, pc.segment_plane(P, THR, 128, got.random_seed), P)
    same(pcu.segment_point_cloud_plane(P, THR, 128, got.random_seed), got, P)
