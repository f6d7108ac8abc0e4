"""register_point_clouds_ransac on the GPU (-m gpu) against tests/ransac_contract.py: every field of RansacRegistrationResult by type, dtype,
shape and bytes (floats by struct.pack), no tolerance, float32 and float64, refit on and off, numpy arrays and device tensors, every call made
twice with equal bytes. The correspondence counts are the smallest that reach each edge of csrc/ransac.h: three rows, a wave minus one, a wave,
a wave plus one (the single-level case of the sum tree ends at 64), the 64 * R rows of a scoring wave and the 4 * 64 * R of a scoring block
with one either side, a block of the sum tree (4096 rows) with one either side; hypothesis counts around the 64 whose scores leave a wave
together; scoring cut into several launches and several slices of blockIdx.y. The cancellation test is tests/test_gpu_zz_ransac_cancel.py."""
import struct

import numpy as np
import pytest

import ransac_contract as rc
from test_ransac_contract import THR, collinear, lattice, planted, rotation, seed_for

pytestmark = pytest.mark.gpu

DTYPES = [np.float32, np.float64]


@pytest.fixture(scope="module")
def pcu():
    import point_cloud_utils_amd as m
    from point_cloud_utils_amd import _lib
    assert _lib.device_count() > 0, "no GPU visible: the gfx950 path has no CPU fallback"
    return m


@pytest.fixture(scope="module")
def R(pcu):
    from point_cloud_utils_amd import _ransac
    rows, launch_tests = _ransac._geometry()
    assert rows >= 1 and launch_tests >= 2 ** 20
    return rows


def host(x):
    return x.cpu().numpy() if hasattr(x, "cpu") else x


def same(got, want, like):
    """Every field of RansacRegistrationResult; arrays are of `like`'s kind."""
    assert type(got).__name__ == "RansacRegistrationResult" and got._fields == want._fields
    assert got.status == want.status
    assert type(got.best_iteration) is int and got.best_iteration == want.best_iteration
    assert type(got.random_seed) is int and got.random_seed == want.random_seed
    assert type(got.transform) is type(like) and type(got.inliers) is type(like)
    M, i = host(got.transform), host(got.inliers)
    assert M.dtype == np.float64 and M.shape == (4, 4)
    assert struct.pack("16d", *M.reshape(-1).tolist()) == struct.pack("16d", *want.transform.reshape(-1).tolist()), (M, want.transform)
    assert i.dtype == np.int64 and i.shape == want.inliers.shape and i.tobytes() == want.inliers.tobytes()
    assert type(got.fitness) is float and type(got.inlier_rmse) is float
    assert struct.pack("2d", got.fitness, got.inlier_rmse) == struct.pack("2d", want.fitness, want.inlier_rmse), (got.fitness, got.inlier_rmse, want.fitness, want.inlier_rmse)


def check(pcu, S, T, corr, thr, H, seed, ratio=0.9, tensors=True, call=None):
    """Both refit modes, numpy (and tensors), each call twice, against the contract. Returns the contract's results (refit off, on)."""
    call = call or pcu.register_point_clouds_ransac
    wants = []
    kinds = [(S, T, corr)]
    if tensors:
        import torch
        kinds.append(tuple(torch.from_numpy(x).cuda() for x in (S, T, corr)))
    for refit in (False, True):
        want = rc.register_ransac(S, T, corr, thr, H, seed, ratio, refit)
        wants.append(want)
        for A in kinds:
            same(call(*A, thr, H, seed, ratio, refit), want, A[0])
            assert pcu.last_stats()["n_queries"] == len(corr)
            same(call(*A, thr, H, seed, ratio, refit), want, A[0])       # equal calls, equal bytes
    return wants


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("c", [3, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 4095, 4096, 4097])
def test_shapes(pcu, R, dtype, c):
    assert R == 4                                        # (the counts above are 64 * R and 4 * 64 * R with one either side)
    P = planted(c, dtype, share=0.5)
    off, on = check(pcu, P.source, P.target, P.corr, THR, 128, 3)
    assert on.status == off.status == "ok" and len(off.inliers) >= 3
    if c >= 63:
        assert np.array_equal(on.inliers, np.flatnonzero(P.true))


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("H", [1, 63, 64, 65, 1000])
def test_hypothesis_counts(pcu, dtype, H):
    P = planted(1025, dtype, share=0.5)
    check(pcu, P.source, P.target, P.corr, THR, H, 3)


@pytest.mark.parametrize("dtype", DTYPES)
def test_scoring_in_several_launches_and_slices(pcu, dtype):
    """The launch cut at c * 128 tests: 128 hypotheses are one launch, 129 two, 300 three -- and the 17 waves of 4097 correspondences split
    every launch's hypotheses over blockIdx.y --; the bytes are those of the uncut call and the contract's. The default cut takes one launch."""
    from point_cloud_utils_amd import _ransac
    P = planted(4097, dtype, share=0.5)
    for H, launches in ((128, 1), (129, 2), (300, 3)):
        def cut(s, t, corr, thr, H, seed, ratio, refit):
            r = _ransac._forced(s, t, corr, thr, H, seed, ratio, refit, launch_tests=len(P.corr) * 128)
            assert pcu.last_stats()["n_passes"] == launches
            return r
        check(pcu, P.source, P.target, P.corr, THR, H, 3, call=cut)
        pcu.register_point_clouds_ransac(P.source, P.target, P.corr, THR, H, 3)
        assert pcu.last_stats()["n_passes"] == 1
    with pytest.raises(ValueError, match="launch_tests"):
        _ransac._forced(P.source, P.target, P.corr, THR, 64, 3, launch_tests=-1)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("seed", [1, 2 ** 32 - 1])
def test_seeds(pcu, dtype, seed):
    P = planted(1000, dtype)
    check(pcu, P.source, P.target, P.corr, THR, 256, seed)


@pytest.mark.parametrize("dtype", DTYPES)
def test_last_stats(pcu, dtype):
    P = planted(1000, dtype)
    want = rc.register_ransac(P.source, P.target, P.corr, THR, 256, 3, refit=False)
    for refit in (False, True):
        pcu.register_point_clouds_ransac(P.source, P.target, P.corr, THR, 256, 3, refit=refit)
        st = pcu.last_stats()
        assert st["n_queries"] == 1000 and st["n_passes"] == 1 and st["n_escalated"] == len(want.inliers) >= 3          # the winner's score


@pytest.mark.parametrize("dtype", DTYPES)
def test_repeated_correspondences(pcu, dtype):
    P = planted(100, dtype, share=0.5)
    corr, true = np.ascontiguousarray(np.tile(P.corr, (3, 1))), np.tile(P.true, 3)
    off, on = check(pcu, P.source, P.target, corr, THR, 256, 3)
    assert on.status == "ok" and np.array_equal(on.inliers, np.flatnonzero(true))


@pytest.mark.parametrize("dtype", DTYPES)
def test_the_comparison_is_strict(pcu, dtype):
    S, T, corr = lattice(dtype, extra=((0.5, 0.0, 0.0), (0.0, -0.5, 0.0), (0.0, 0.0, 0.25), (0.0, 0.0, 0.5)))
    off, on = check(pcu, S, T, corr, 0.5, 1, seed_for(len(corr), (0, 1, 2)))
    assert off.inliers.tolist() == [0, 1, 2, 5]


@pytest.mark.parametrize("dtype", DTYPES)
def test_edge_length_ratio_and_a_winner_of_two_inliers(pcu, dtype):
    S, T, corr = lattice(dtype)
    T8 = np.ascontiguousarray((T.astype(np.float64) * 0.8).astype(dtype))
    seed = seed_for(3, (0, 1, 2))
    for ratio, status in ((0.9, "no_alignment"), (0.75, "ok"), (0.0, "ok")):
        off, on = check(pcu, S, T8, corr, 1.0, 1, seed, ratio)
        assert off.status == on.status == status
    T2 = T.copy()
    T2[2] += np.array([0.0, 3.0, 0.0], dtype=dtype)
    off, on = check(pcu, S, T2, corr, 1.5, 1, seed, 0.0)
    assert off.inliers.tolist() == on.inliers.tolist() == [0, 1]


@pytest.mark.parametrize("dtype", DTYPES)
def test_no_alignment(pcu, dtype):
    off, on = check(pcu, *collinear(dtype), 0.5, 64, 1)
    assert off.status == on.status == "no_alignment"
    P = planted(300, dtype)
    off, on = check(pcu, P.source, P.target, P.corr, 0.0, 64, 1)
    assert off.status == on.status == "no_alignment"
    S, T, corr = lattice(dtype)
    corr[:, 0] = (0, 0, 2)                               # two equal source points: no frame
    off, on = check(pcu, S, T, corr, 10.0, 4, 1, 0.0)
    assert off.status == on.status == "no_alignment"


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("refit", [False, True])
def test_an_index_outside_its_cloud(pcu, dtype, refit):
    """Found by the gather kernel on the device, for host arrays and for tensors alike; the context then answers the good call."""
    import torch
    P = planted(300, dtype)
    n, m = len(P.source), len(P.target)
    for col, bad, text in ((0, n, f"correspondences[:, 0] must hold rows of source_points: found an entry outside [0, {n})"),
                           (0, -1, f"correspondences[:, 0] must hold rows of source_points: found an entry outside [0, {n})"),
                           (1, m, f"correspondences[:, 1] must hold rows of target_points: found an entry outside [0, {m})"),
                           (1, -2 ** 63, f"correspondences[:, 1] must hold rows of target_points: found an entry outside [0, {m})")):
        corr = P.corr.copy()
        corr[217, col] = bad
        for A in ((P.source, P.target, corr), tuple(torch.from_numpy(x).cuda() for x in (P.source, P.target, corr))):
            with pytest.raises(ValueError) as e:
                pcu.register_point_clouds_ransac(*A, THR, 128, 3, refit=refit)
            assert str(e.value) == text
    same(pcu.register_point_clouds_ransac(P.source, P.target, P.corr, THR, 128, 3, refit=refit), rc.register_ransac(P.source, P.target, P.corr, THR, 128, 3, refit=refit), P.source)


def test_arrays_of_two_kinds_are_refused(pcu):
    import torch
    P = planted(100, np.float32)
    with pytest.raises(ValueError, match="same device"):
        pcu.register_point_clouds_ransac(P.source, P.target, torch.from_numpy(P.corr).cuda(), THR, 16, 1)
    with pytest.raises(ValueError, match="same device"):
        pcu.register_point_clouds_ransac(torch.from_numpy(P.source).cuda(), torch.from_numpy(P.target).cuda(), P.corr, THR, 16, 1)


def test_seed_zero_is_from_the_clock(pcu):
    P = planted(1000, np.float32)
    got = pcu.register_point_clouds_ransac(P.source, P.target, P.corr, THR, 256)
    assert type(got.random_seed) is int and 1 <= got.random_seed <= 0xFFFFFFFF
    same(got, rc.register_ransac(P.source, P.target, P.corr, THR, 256, got.random_seed), P.source)
    same(pcu.register_point_clouds_ransac(P.source, P.target, P.corr, THR, 256, got.random_seed), got, P.source)


# ---------------------------------------------------------------------------------------------- the whole pipeline
def bumpy_surface(n, seed=4):
    """A height field over [-1, 1]^2 without a symmetry: bumps of different heights and widths, and a slope."""
    rng = np.random.default_rng(seed)
    xy = rng.random((n, 2)) * 2.0 - 1.0
    z = 0.15 * xy[:, 0] - 0.1 * xy[:, 1] * xy[:, 1]
    for cx, cy, h, w in ((-0.5, -0.4, 0.5, 0.25), (0.45, 0.1, -0.4, 0.2), (-0.1, 0.55, 0.35, 0.15), (0.6, -0.6, 0.3, 0.3), (-0.65, 0.35, -0.3, 0.18)):
        z = z + h * np.exp(-((xy[:, 0] - cx) ** 2 + (xy[:, 1] - cy) ** 2) / (2.0 * w * w))
    return np.ascontiguousarray(np.column_stack([xy, z]))


def test_the_pipeline_from_normals_to_icp(pcu):
    """A surface sampled twice, the second sample moved by a rotation of 143 degrees and a translation: normals (with the direction to the
    sensor moved along, so that both clouds' normals look the same way), FPFH, mutual matches -- about a thousand, one in twelve of them a
    pair of neighbours on the surface (tried on the contracts of the three calls first) --, RANSAC, equal to the contract on the same
    correspondences and with most of its inliers such pairs, then ICP from its transform against ICP from the identity."""
    n, thr = 3000, 0.05
    S = bumpy_surface(n)
    R0, t0 = rotation([1.0, 2.0, 3.0], 2.5), np.array([0.3, -0.2, 0.5])
    T = np.ascontiguousarray(bumpy_surface(n, seed=5) @ R0.T + t0)
    up = np.array([0.0, 0.0, 1.0])
    i_s, n_s = pcu.estimate_point_cloud_normals_knn(S, 16, view_directions=np.tile(up, (n, 1)))
    i_t, n_t = pcu.estimate_point_cloud_normals_knn(T, 16, view_directions=np.tile(R0 @ up, (n, 1)))
    assert len(i_s) > 0.9 * n and len(i_t) > 0.9 * n
    S1, T1 = np.ascontiguousarray(S[i_s]), np.ascontiguousarray(T[i_t])
    f_s, f_t = pcu.compute_point_cloud_fpfh(S1, n_s, 0.15), pcu.compute_point_cloud_fpfh(T1, n_t, 0.15)
    nearest, _, is_mutual = pcu.match_point_features(f_s, f_t, mutual=True)
    corr = np.ascontiguousarray(np.stack([np.flatnonzero(is_mutual), nearest[is_mutual]], axis=1))
    assert corr.dtype == np.int64 and len(corr) >= 100
    got = pcu.register_point_clouds_ransac(S1, T1, corr, thr, 20000, 11)
    want = rc.register_ransac(S1, T1, corr, thr, 20000, 11)
    same(got, want, S1)
    true = np.linalg.norm(S1[corr[:, 0]] @ R0.T + t0 - T1[corr[:, 1]], axis=1) < thr      # the pair is two neighbours on the surface
    print("correspondences", len(corr), "true", int(true.sum()), "inliers", len(got.inliers), "true inliers", int(true[got.inliers].sum()), "fitness", got.fitness)
    assert got.status == "ok" and 2 * int(true[got.inliers].sum()) > len(got.inliers)
    assert np.abs(got.transform[:3, :3] - R0).max() < 0.1
    from_ransac = pcu.register_point_clouds_icp(S1, T1, init_transform=got.transform, max_correspondence_distance=thr)
    from_identity = pcu.register_point_clouds_icp(S1, T1, max_correspondence_distance=thr)
    print("icp fitness from ransac", from_ransac.fitness, "from the identity", from_identity.fitness)
    assert from_ransac.fitness > from_identity.fitness
