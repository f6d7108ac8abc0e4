"""match_point_features on the GPU (-m gpu) against tests/feature_match_contract.py: dtype, shape and bytes of nearest, d2 and is_mutual, no
tolerance, float32 and float64, numpy arrays and device tensors. The shapes are the smallest that reach each path of csrc/feature_match.h:
D = 33 (the query row in registers) and every other D (in LDS), rows around a wave, around a block of queries and around a dataset tile, a
dataset split over several blocks, ties, NaN rows on either side. Then compute_point_cloud_fpfh of a cloud and of its rigidly moved copy, end
to end. This file sorts behind tests/test_gpu_mesh_sampling.py (Tests)."""
import ctypes

import numpy as np
import pytest

import feature_match_contract as mc

pytestmark = pytest.mark.gpu

DTYPES = [np.float32, np.float64]


@pytest.fixture(scope="module")
def pcu():
    import point_cloud_utils_amd as m
    from point_cloud_utils_amd import _lib
    assert _lib.device_count() > 0, "no GPU visible: the gfx950 path has no CPU fallback"
    return m


@pytest.fixture(scope="module")
def geometry(pcu):
    """(queries per block, dataset rows per tile, rows a lane accumulates at once) of csrc/feature_match.h."""
    from point_cloud_utils_amd import _lib
    out = (ctypes.c_int * 3)()
    assert _lib.lib().pcu_hip_match_features_geometry(out) == 0
    return tuple(out)


def same(got, want):
    got = [g.cpu().numpy() if hasattr(g, "cpu") else g for g in got]
    assert len(got) == len(want)
    for g, w in zip(got, want):
        assert g.dtype == w.dtype and g.shape == w.shape, (g.dtype, g.shape, w.dtype, w.shape)
        assert g.tobytes() == w.tobytes(), (np.nonzero(g != w)[0][:8], g[:8], w[:8])


def check(pcu, a, b, tensors=True):
    want = mc.match(a, b, mutual=True)
    assert want[0].dtype == np.int64 and want[1].dtype == a.dtype and want[2].dtype == np.bool_
    kinds = [(a, b)]
    if tensors:
        import torch
        kinds.append((torch.from_numpy(a).cuda(), torch.from_numpy(b).cuda()))
    for qa, qb in kinds:
        got = pcu.match_point_features(qa, qb, mutual=True)
        assert type(got) is tuple and all(type(g) is type(qa) for g in got)
        same(got, want)
        same(pcu.match_point_features(qa, qb, mutual=True), want)            # equal calls, equal bytes
        two = pcu.match_point_features(qa, qb)
        assert type(two) is tuple and len(two) == 2
        same(two, want[:2])
    return want


def features(rng, n, D, dtype):
    """Random rows on a coarse lattice of values, so that exact ties between different rows happen too."""
    return (rng.integers(-8, 9, (n, D)) * 0.125 + rng.integers(0, 2, (n, 1)) * rng.standard_normal((n, D))).astype(dtype)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("D", [1, 3, 32, 33, 34, 128])
def test_every_width_around_a_wave_and_a_tile(pcu, geometry, dtype, D):
    queries, tile, _ = geometry
    rng = np.random.default_rng(D)
    sizes = sorted({1, 63, 64, 65, tile - 1, tile, tile + 1, queries - 1, queries + 1})
    big = features(rng, max(sizes), D, dtype)
    data = features(rng, max(sizes), D, dtype)
    for n in sizes:
        for m in sizes:
            if n in (1, 65) or m in (1, tile + 1) or n == m:                # (every size on either side, not every pair of them)
                check(pcu, big[:n], data[:m], tensors=(n, m) == (65, tile + 1))


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("D", [33, 20])
def test_a_dataset_split_over_blocks_and_several_query_blocks(pcu, geometry, dtype, D):
    """Few queries against many rows: the dataset is cut along gridDim.y and the parts folded (last_stats()["n_escalated"] parts); many
    queries against few rows: several blocks of queries, the last one partial."""
    queries, tile, rows = geometry
    rng = np.random.default_rng(100 + D)
    a, b = features(rng, 70, D, dtype), features(rng, 40 * tile + 5, D, dtype)
    check(pcu, a, b)
    assert pcu.last_stats()["n_escalated"] > 1
    check(pcu, b, a, tensors=False)
    assert pcu.last_stats()["n_escalated"] >= 1 and pcu.last_stats()["n_passes"] == 1


@pytest.mark.parametrize("dtype", DTYPES)
def test_duplicate_rows_tie_to_the_lower_row(pcu, dtype):
    rng = np.random.default_rng(3)
    base = features(rng, 50, 33, dtype)
    b = np.concatenate([base, base[::-1], base])                               # every row three times, far apart in the dataset
    a = base + dtype(0.001)
    nearest, d2, mutual = check(pcu, a, b)
    assert (nearest < 50).all()
    nearest, _, mutual = check(pcu, b, b, tensors=False)                       # a row's own copy at distance 0: the lowest of its copies
    assert np.array_equal(nearest, np.concatenate([np.arange(50), np.arange(49, -1, -1), np.arange(50)]))
    assert np.array_equal(mutual, np.arange(150) < 50)


@pytest.mark.parametrize("dtype", DTYPES)
def test_nan_rows_on_either_side(pcu, dtype):
    rng = np.random.default_rng(4)
    a, b = features(rng, 130, 33, dtype), features(rng, 90, 33, dtype)
    a[5, 7] = np.nan
    a[64] = np.nan
    b[0, 0] = np.nan
    b[33, 32] = np.nan
    nearest, d2, mutual = check(pcu, a, b)
    assert nearest[5] == -1 and nearest[64] == -1 and np.isposinf(d2[[5, 64]]).all() and not mutual[[5, 64]].any()
    assert not np.isin(nearest, [0, 33]).any()
    nearest, d2, mutual = check(pcu, a[:, :5].copy(), np.full((40, 5), np.nan, dtype), tensors=False)       # nothing to match
    assert (nearest == -1).all() and np.isposinf(d2).all() and not mutual.any()
    big = np.finfo(dtype).max
    nearest, d2, _ = check(pcu, np.full((3, 2), big, dtype), np.array([[np.nan, 0], [-big, 0], [-big, -big]], dtype), tensors=False)
    assert nearest.tolist() == [1, 1, 1] and np.isposinf(d2).all()              # +inf is a candidate, the lower row of two


@pytest.mark.parametrize("dtype", DTYPES)
def test_mutual_matches(pcu, dtype):
    rng = np.random.default_rng(5)
    b = rng.standard_normal((300, 33)).astype(dtype)
    perm = rng.permutation(300)
    nearest, d2, mutual = check(pcu, np.ascontiguousarray(b[perm]), b)          # a permuted copy: every row finds itself, both ways
    assert np.array_equal(nearest, perm) and not d2.any() and mutual.all()
    a = np.zeros((3, 4), dtype)
    a[:, 0] = (1.0, 2.0, 4.0)
    hub = np.zeros((2, 4), dtype)
    hub[1, 0] = 100.0
    nearest, _, mutual = check(pcu, a, hub, tensors=False)                      # three queries share dataset row 0, which prefers the first
    assert nearest.tolist() == [0, 0, 0] and mutual.tolist() == [True, False, False]


@pytest.mark.parametrize("dtype", DTYPES)
def test_fpfh_of_a_cloud_and_of_its_rigidly_moved_copy(pcu, dtype):
    """End to end. The moved copy is a rotation by a quarter turn about z and a translation by small integers on coordinates that are multiples
    of 2^-10: the move is exact in both dtypes, so every d2, every pair and every count of the copy equals the cloud's, and the two descriptors
    of a row differ only by the order of the sums W -- each entry within the entry bound of compute_point_cloud_fpfh, (2 m + 8) * 2^-52 * 200 in
    float64, one float32 spacing in float32. A row's image is therefore within 33 * bound^2 of it, and it has to be the nearest: descriptors
    of different rows of this cloud are farther apart than that."""
    rng = np.random.default_rng(6)
    n = 1500
    p = (np.round(rng.random((n, 3)) * 1024.0) / 1024.0).astype(dtype)
    p = np.unique(p, axis=0)
    n = len(p)
    nrm = rng.standard_normal((n, 3))
    nrm = (np.round(nrm / np.linalg.norm(nrm, axis=1)[:, None] * 1024.0) / 1024.0).astype(dtype)
    q = np.stack([-p[:, 1] + 3.0, p[:, 0] - 2.0, p[:, 2] + 1.0], axis=1).astype(dtype)
    qn = np.stack([-nrm[:, 1], nrm[:, 0], nrm[:, 2]], axis=1).astype(dtype)
    radius = 0.15
    fa, ca = pcu.compute_point_cloud_fpfh(p, nrm, radius, return_spfh=True)
    fb, cb = pcu.compute_point_cloud_fpfh(q, qn, radius, return_spfh=True)
    assert np.array_equal(ca, cb)
    m = pcu.radius_count(p, p, radius) - 1
    if dtype == np.float64:
        entry = 2.0 * (2.0 * m + 8.0) * 2.0 ** -52 * 200.0                      # (each of the two is within the bound of the contract)
    else:
        entry = np.full(n, 2.0 * float(np.spacing(np.float32(200.0))))
    has = ca[:, :11].sum(axis=1) > 0
    assert has.mean() > 0.95
    assert (np.abs(fa.astype(np.float64) - fb.astype(np.float64)) <= entry[:, None]).all()
    nearest, d2, mutual = pcu.match_point_features(fa[has], fb[has], mutual=True)
    same((nearest, d2, mutual), mc.match(fa[has], fb[has], mutual=True))
    assert np.array_equal(nearest, np.arange(int(has.sum()))) and mutual.all()
    assert (d2.astype(np.float64) <= 33.0 * entry[has] ** 2 * 1.001).all()
