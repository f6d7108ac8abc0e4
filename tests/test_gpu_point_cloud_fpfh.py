"""compute_point_cloud_fpfh on the GPU (-m gpu) against tests/fpfh_contract.py, float32 and float64, numpy arrays and device tensors.
spfh_counts equal the contract exactly. features are held to the derived bounds of DESIGN.md f24, not to measured ones: the sums W and G have
non-negative terms, so against the contract's ascending j each differs by at most m_i * 2^-52 relative (m_i: the row's neighbours), which
gives |F_gpu - F_contract| <= (2 m_i + 8) * 2^-52 * 200 in float64 and one float32 spacing at max(|a|, |b|) in float32. Two equal calls give
equal bytes, numpy and tensor calls give equal bytes. The shapes are the smallest that reach each path of csrc/fpfh.h. This file sorts behind
tests/test_gpu_mesh_sampling.py (Tests); the cancellation test is tests/test_gpu_zz_fpfh_cancel.py."""
import numpy as np
import pytest

import fpfh_contract as fc

pytestmark = pytest.mark.gpu

DTYPES = [np.float32, np.float64]
U = 2.0 ** -52


@pytest.fixture(scope="module")
def pcu():
    import point_cloud_utils_amd as m
    from point_cloud_utils_amd import _lib
    assert _lib.device_count() > 0, "no GPU visible: the gfx950 path has no CPU fallback"
    return m


def host(x):
    return x.cpu().numpy() if hasattr(x, "cpu") else x


def within_bound(got, want, m, dtype):
    """got, want: (rows, 33) features; m: (rows,) neighbour counts."""
    assert got.dtype == dtype and want.dtype == dtype and got.shape == want.shape
    g, w = got.astype(np.float64), want.astype(np.float64)
    if dtype == np.float64:
        tol = ((2.0 * m + 8.0) * U * 200.0)[:, None] * np.ones_like(g)
    else:
        tol = np.spacing(np.maximum(np.abs(got), np.abs(want)).astype(np.float32)).astype(np.float64)
    err = np.abs(g - w)
    bad = ~(err <= tol)
    print("max |F_gpu - F_contract| / bound:", float((err / np.maximum(tol, 1e-300)).max()) if err.size else 0.0)
    assert not bad.any(), (np.argwhere(bad)[:5], got[bad][:5], want[bad][:5], tol[bad][:5])


def group_sums_are_200(features, counts, m, dtype, has_weight):
    """Every group of a row with pairs (k > 0) and weights (G > 0) sums to 200. Each of its 11 entries is within the entry bound of the contract's,
    whose own sum is within 40 * 2^-52 * 200 of 200 (two roundings per S_b and per 100 W_b / G, ten in G, one per final sum); a float32 entry adds
    half a spacing at 200 for its rounding."""
    f = features.astype(np.float64).reshape(len(features), 3, 11).sum(axis=2)
    k = counts.reshape(len(counts), 3, 11).sum(axis=2)
    assert (k == k[:, :1]).all()                                            # every pair adds one count to each of the three groups
    tol = (11.0 * (2.0 * m + 8.0) + 40.0) * U * 200.0
    if dtype == np.float32:
        tol = tol + 11.0 * 0.5 * float(np.spacing(np.float32(200.0)))
    rows = (k[:, 0] > 0) & has_weight
    assert (np.abs(f[rows] - 200.0) <= tol[rows, None]).all(), np.abs(f[rows] - 200.0).max()
    return int(rows.sum())


def check(pcu, p, nrm, radius, rows=None, tensors=True):
    """The call twice with numpy arrays, once with tensors and once without spfh_counts, against the contract on `rows` (all of them by default).
    Returns the GPU's features and spfh_counts, the contract object and the rows' neighbour counts m."""
    dtype = p.dtype.type
    idx = np.arange(len(p)) if rows is None else np.asarray(rows)
    one = fc.Fpfh(p, nrm, radius)
    want_f, want_c, m = fc.rows_of(one, idx)
    got = pcu.compute_point_cloud_fpfh(p, nrm, radius, return_spfh=True)
    assert type(got) is tuple and len(got) == 2 and all(type(g) is np.ndarray for g in got)
    feat, cnt = got
    assert feat.dtype == dtype and feat.shape == (len(p), 33) and cnt.dtype == np.int32 and cnt.shape == (len(p), 33)
    assert np.array_equal(cnt[idx], want_c), np.argwhere(cnt[idx] != want_c)[:5]
    within_bound(feat[idx], want_f, m, dtype)
    again = pcu.compute_point_cloud_fpfh(p, nrm, radius, return_spfh=True)
    assert again[0].tobytes() == feat.tobytes() and again[1].tobytes() == cnt.tobytes()          # equal calls, equal bytes
    alone = pcu.compute_point_cloud_fpfh(p, nrm, radius)
    assert type(alone) is np.ndarray and alone.tobytes() == feat.tobytes()
    if tensors:
        import torch
        tp, tn = torch.from_numpy(p).cuda(), torch.from_numpy(nrm).cuda()
        tf, tc = pcu.compute_point_cloud_fpfh(tp, tn, radius, return_spfh=True)
        assert tf.device == tp.device and tc.device == tp.device and tc.dtype == torch.int32
        assert host(tf).tobytes() == feat.tobytes() and host(tc).tobytes() == cnt.tobytes()      # numpy and tensors, equal bytes
    valid = fc.valid_rows(nrm)
    assert not feat[~valid].any() and not cnt[~valid].any()
    return feat, cnt, one, m


def unit(v):
    return v / np.linalg.norm(v, axis=1)[:, None]


def weights_of(one, rows):
    """Which of `rows` have G > 0 by the contract object `one`: a neighbour at d2 > 0 that has pairs of its own."""
    out = []
    for i in rows:
        nb, d2 = one.neighbours(int(i))
        out.append(bool(one.valid[i]) and any(dd > 0 and sum(one.counts(int(j))[0][:11]) > 0 for j, dd in zip(nb, d2)))
    return np.array(out, dtype=bool)


@pytest.mark.parametrize("dtype", DTYPES)
def test_one_and_two_rows(pcu, dtype):
    p = np.array([[0.25, 0.5, 0.75]], dtype)
    n = np.array([[0.0, 0.0, 1.0]], dtype)
    feat, cnt, *_ = check(pcu, p, n, 1.0)
    assert not feat.any() and not cnt.any()
    p = np.array([[0.0, 0.0, 0.0], [0.5, 0.25, 0.125]], dtype)
    n = unit(np.array([[0.0, 0.2, 1.0], [1.0, -0.3, 0.1]])).astype(dtype)
    feat, cnt, one, m = check(pcu, p, n, 1.0)
    assert cnt.reshape(2, 3, 11).sum(axis=2).tolist() == [[1, 1, 1], [1, 1, 1]]
    assert group_sums_are_200(feat, cnt, m, dtype, np.ones(2, bool)) == 2                         # S = 100 in one bin, 100 W / G = 100 in one bin
    feat, cnt, *_ = check(pcu, p, n, 0.25, tensors=False)                                        # out of reach of each other
    assert not feat.any() and not cnt.any()


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("n", [63, 64, 65])
def test_the_wave_edge(pcu, dtype, n):
    rng = np.random.default_rng(n)
    p = rng.random((n, 3)).astype(dtype)
    nrm = unit(rng.standard_normal((n, 3))).astype(dtype)
    feat, cnt, one, m = check(pcu, p, nrm, 0.35, tensors=n == 65)
    assert group_sums_are_200(feat, cnt, m, dtype, weights_of(one, range(n))) >= n - 5


@pytest.mark.parametrize("dtype", DTYPES)
def test_a_lattice_with_axis_normals_and_the_radius_on_a_lattice_distance(pcu, dtype):
    """5 x 5 x 5 integer points, normals along +-x, +-y, +-z, radius 2: d2 is 1, 2 or 3 inside and exactly 4 = r2 just outside (strict <), and every
    feature sits on a bin edge or a bin middle (f = 0, +-1, +-1/sqrt 2, ...; theta a multiple of pi / 4)."""
    g = np.arange(5)
    p = np.stack(np.meshgrid(g, g, g, indexing="ij"), axis=-1).reshape(-1, 3).astype(dtype)
    axes = np.array([[1, 0, 0], [0, 1, 0], [0, 0, 1], [-1, 0, 0], [0, -1, 0], [0, 0, -1]], dtype)
    nrm = axes[(p[:, 0] + 2 * p[:, 1] + 3 * p[:, 2]).astype(int) % 6]
    order = np.random.default_rng(5).permutation(len(p))
    p, nrm = np.ascontiguousarray(p[order]), np.ascontiguousarray(nrm[order])
    feat, cnt, one, m = check(pcu, p, nrm, 2.0)
    inner = (p == 2).all(axis=1)
    assert m[inner].tolist() == [6 + 12 + 8] and m.min() == 3 + 3 + 1                            # (the 6 rows at distance 2 are out)
    assert group_sums_are_200(feat, cnt, m, dtype, weights_of(one, range(len(p)))) == len(p)


@pytest.mark.parametrize("dtype", DTYPES)
def test_coincident_copies(pcu, dtype):
    """Every place three times with three normals: the copies are neighbours at d2 = 0 -- no pair (len = 0) and no weight (d2 > 0 fails)."""
    rng = np.random.default_rng(6)
    base = rng.random((100, 3))
    p = np.concatenate([base, base, base]).astype(dtype)
    nrm = unit(rng.standard_normal((300, 3))).astype(dtype)
    order = rng.permutation(300)
    p, nrm = np.ascontiguousarray(p[order]), np.ascontiguousarray(nrm[order])
    feat, cnt, one, m = check(pcu, p, nrm, 0.3)
    assert (m >= 2).all() and (cnt[:, :11].sum(axis=1) <= m - 2).all()
    check(pcu, np.zeros((70, 3), dtype), nrm[:70], 0.5, tensors=False)                           # one place only: neighbours, no pairs at all


@pytest.mark.parametrize("dtype", DTYPES)
def test_rows_with_nan_inf_and_zero_normals(pcu, dtype):
    rng = np.random.default_rng(7)
    p = rng.random((200, 3)).astype(dtype)
    nrm = unit(rng.standard_normal((200, 3))).astype(dtype)
    nrm[3] = np.nan
    nrm[10, 1] = np.nan
    nrm[64, 2] = np.inf
    nrm[65, 0] = -np.inf
    nrm[100] = 0.0
    nrm[101] = (0.0, -0.0, 0.0)
    nrm[150] = (0.0, 0.0, 1e-30)                                                                  # tiny is not zero: a valid row
    feat, cnt, *_ = check(pcu, p, nrm, 0.3)
    assert cnt[150].any() and not cnt[[3, 10, 64, 65, 100, 101]].any()
    check(pcu, p, np.full_like(nrm, np.nan), 0.3, tensors=False)                                  # nobody is valid


@pytest.mark.parametrize("dtype", DTYPES)
def test_radius_zero_and_a_radius_that_holds_the_cloud(pcu, dtype):
    rng = np.random.default_rng(8)
    p = rng.random((150, 3)).astype(dtype)
    nrm = unit(rng.standard_normal((150, 3))).astype(dtype)
    feat, cnt, *_ = check(pcu, p, nrm, 0.0)
    assert not feat.any() and not cnt.any()
    feat, cnt, one, m = check(pcu, p, nrm, 2.0)
    assert (m == 149).all()
    assert group_sums_are_200(feat, cnt, m, dtype, np.ones(150, bool)) == 150


@pytest.mark.parametrize("dtype", DTYPES)
def test_a_tight_cluster_and_far_outliers_take_both_walks(pcu, dtype):
    """600 rows in a cube of 0.1 at the origin and 40 outliers in a cube of 0.05 at (50, 50, 50): two corner cells of a grid of some 160 cells.
    The records lie in cell order, so the first nine waves hold cluster rows only and stage their (one) box; the tenth holds the cluster's last 24
    records and the 40 outliers: the union of its lanes' boxes is the whole grid, more than kRadUnionFactor = 8 times a corner's box of 8 cells,
    and its lanes walk their own boxes. Which walk ran is also a statistic of the call: last_stats() counts the waves of either kind."""
    rng = np.random.default_rng(9)
    blob = rng.random((600, 3)) * 0.1
    far = rng.random((40, 3)) * 0.05 + 50.0
    p = np.concatenate([blob, far])
    order = rng.permutation(len(p))
    p = np.ascontiguousarray(p[order]).astype(dtype)
    nrm = unit(rng.standard_normal(p.shape)).astype(dtype)
    feat, cnt, one, m = check(pcu, p, nrm, 0.02)
    st = pcu.last_stats()
    print("waves that staged / that did not:", st["n_tie_flagged"], st["n_tie_true"])
    assert st["n_tie_flagged"] > 0 and st["n_tie_true"] > 0, st
    assert st["n_tie_flagged"] + st["n_tie_true"] == (len(p) + 63) // 64 and st["n_passes"] == 2
    outlier = order >= 600                                                   # (rows of p that came from the far cube)
    assert cnt[outlier].any() and cnt[~outlier].any()


@pytest.mark.parametrize("dtype", DTYPES)
def test_a_sphere_of_twenty_thousand_rows_on_a_subset_of_queries(pcu, dtype):
    rng = np.random.default_rng(10)
    p = unit(rng.standard_normal((20000, 3))).astype(dtype)
    nrm = p.copy()                                                           # outward
    rows = np.sort(rng.choice(20000, 500, replace=False))
    feat, cnt, one, m = check(pcu, p, nrm, 0.04, rows=rows)
    assert 4 <= m.mean() <= 16
    n200 = group_sums_are_200(feat[rows], cnt[rows], m, dtype, weights_of(one, rows))
    assert n200 >= 450


def test_a_million_device_resident_rows(pcu):
    """2^20 rows, checked by what is known without the contract: every pair adds one count to each group; a row with pairs has group sums of 200
    (or of 100 where none of its neighbours has pairs: G = 0), all three groups alike; a second call gives equal bytes."""
    import torch
    dtype = np.float32
    rng = np.random.default_rng(11)
    p = unit(rng.standard_normal((1 << 20, 3))).astype(dtype)
    tp = torch.from_numpy(p).cuda()
    radius = 0.007
    feat, cnt = pcu.compute_point_cloud_fpfh(tp, tp, radius, return_spfh=True)
    again = pcu.compute_point_cloud_fpfh(tp, tp, radius, return_spfh=True)
    assert torch.equal(feat, again[0]) and torch.equal(cnt, again[1])
    m = host(pcu.radius_count(tp, tp, radius)) - 1                           # (radius_count counts the row itself)
    feat, cnt = host(feat), host(cnt)
    k = cnt.reshape(-1, 3, 11).sum(axis=2)
    assert (k == k[:, :1]).all() and (k[:, 0] <= m).all() and 8 <= m.mean() <= 20
    sums = feat.astype(np.float64).reshape(-1, 3, 11).sum(axis=2)
    tol = ((11.0 * (2.0 * m + 8.0) + 40.0) * U * 200.0 + 11.0 * 0.5 * float(np.spacing(np.float32(200.0))))[:, None]
    is200, is100 = np.abs(sums - 200.0) <= tol, np.abs(sums - 100.0) <= tol
    has = k[:, 0] > 0
    assert (is200[has].all(axis=1) | is100[has].all(axis=1)).all()
    assert is200[has].all(axis=1).mean() > 0.99 and has.mean() > 0.99
    assert not feat[~has].any()
