"""tests/fpfh_contract.py, the definition of compute_point_cloud_fpfh, against cases worked out by hand and against an independent numpy
formulation (np.arctan2, vectorised dots). No GPU."""
import math

import numpy as np
import pytest

import fpfh_contract as fc

X, Y, Z = (1.0, 0.0, 0.0), (0.0, 1.0, 0.0), (0.0, 0.0, 1.0)


def test_the_edge_table_is_the_nearest_float64():
    mp = pytest.importorskip("mpmath")
    mp.mp.prec = 200
    for b, (c, s) in enumerate(fc.EDGES, start=1):
        t = -mp.pi + 2 * mp.pi * b / 11
        assert c == float(mp.cos(t)) and s == float(mp.sin(t)), b


def test_bins_of_the_unit_features():
    assert fc.unit_bin(-1.0) == 0 and fc.unit_bin(0.0) == 5 and fc.unit_bin(1.0) == 10          # f = 0 in bin 5, f = 1 in bin 10
    assert fc.unit_bin(-1.5) == 0 and fc.unit_bin(7.0) == 10 and fc.unit_bin(float("nan")) == 0
    assert fc.unit_bin(math.nextafter(0.0, -1.0)) == 5                                          # (f + 1 rounds to 1)
    for b in range(11):
        f = -1.0 + 2.0 * (b + 0.5) / 11.0
        assert fc.unit_bin(f) == b


def test_bins_of_theta():
    assert fc.theta_bin(0.0, 0.0) == 10                    # stated: x = y = 0
    assert fc.theta_bin(-1.0, -0.0) == 10                  # stated: y = -0.0 with x < 0 is the upper end, not the lower
    assert fc.theta_bin(-1.0, 0.0) == 10 and fc.theta_bin(1.0, 0.0) == 5 and fc.theta_bin(1.0, -0.0) == 5
    assert fc.theta_bin(-1.0, -1e-300) == 0
    for b in range(11):                                    # the middle of every bin
        t = -math.pi + 2.0 * math.pi * (b + 0.5) / 11.0
        assert fc.theta_bin(math.cos(t), math.sin(t)) == b, b
    for b in range(1, 11):                                 # either side of every inner edge
        for db, want in ((-1e-9, b - 1), (1e-9, b)):
            t = -math.pi + 2.0 * math.pi * b / 11.0 + db
            assert fc.theta_bin(3.0 * math.cos(t), 3.0 * math.sin(t)) == want, (b, db)


def test_two_points_with_parallel_normals_are_skipped():
    """dp = (1, 0, 0) and both normals along dp: u x n1 = 0, so the pair is no pair and everything is zero."""
    assert fc.pair_bins((0.0, 0.0, 0.0), X, (1.0, 0.0, 0.0), X) is None
    p = np.array([[0, 0, 0], [1, 0, 0]], dtype=np.float64)
    n = np.array([X, X], dtype=np.float64)
    f, c, m = fc.fpfh(p, n, 1.5)
    assert m.tolist() == [1, 1] and not c.any() and not f.any()


def test_three_lattice_points_with_axis_normals():
    """p0 = origin, p1 = (1, 0, 0), p2 = (0, 1, 0), normals z, z, x, radius 1.2: the pairs (0, 1), (0, 2) and their mirrors; |p1 - p2| = sqrt 2 is out.
    Pair (0, 1): dp = x, a1 = a2 = 0: no swap, n1 = z, f3 = 0 (bin 5); v = x cross z = -y, w = z cross (-y) = x; f2 = v.z = 0 (bin 5); y = w.z = 0, x = 1:
    theta = 0, bin 5. Pair (0, 2): dp = y, a1 = z.y = 0, a2 = x.y = 0: no swap, n1 = z, n2 = x, f3 = 0 (bin 5); v = y cross z = x, w = z cross x = y;
    f2 = v.x = 1 (bin 10); y = w.x = 0, x = z.x = 0: the stated corner, bin 10."""
    assert fc.pair_bins((0.0, 0.0, 0.0), Z, (1.0, 0.0, 0.0), Z) == (5, 5, 5)
    assert fc.pair_bins((0.0, 0.0, 0.0), Z, (0.0, 1.0, 0.0), X) == (10, 10, 5)
    p = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0]], dtype=np.float32)
    n = np.array([Z, Z, X], dtype=np.float32)
    f, c, m = fc.fpfh(p, n, 1.2)
    assert m.tolist() == [2, 1, 1] and f.dtype == np.float32
    want0 = np.zeros(33, np.int32)
    want0[[5, 10]] = 1; want0[[11 + 5, 11 + 10]] = 1; want0[22 + 5] = 2
    assert c[0].tolist() == want0.tolist()
    assert c[1].tolist() == np.bincount([5, 11 + 5, 22 + 5], minlength=33).tolist()            # (1, 0): the same frame seen from the other end
    # S_0 = 50 in four bins and 100 in one; row 0's neighbours are at d2 = 1: W_0 = S_1 + S_2, and every group of F sums to 200
    assert np.allclose(f.reshape(3, 3, 11).sum(axis=2), 200.0)
    assert f[0, 5] == 50.0 + 100.0 * (100.0 / 200.0) and f[0, 22 + 5] == 100.0 + 100.0 * (200.0 / 200.0)


def test_a_duplicate_point_is_a_neighbour_without_a_pair():
    """Two rows at one place: d2 = 0 < r2, so they are neighbours (m counts them), but len = 0 skips the pair and d2 > 0 keeps it out of W."""
    p = np.array([[0, 0, 0], [0, 0, 0], [1, 0, 0]], dtype=np.float64)
    n = np.array([Z, Y, Z], dtype=np.float64)
    f, c, m = fc.fpfh(p, n, 1.5)
    assert m.tolist() == [2, 2, 2]
    assert c[:, :11].sum(axis=1).tolist() == [1, 1, 2]
    one = fc.Fpfh(p, n, 1.5)
    assert one.row(0)[:11] == [s + 100.0 * w / 100.0 for s, w in zip(one.counts(0)[1][:11], one.counts(2)[1][:11])]      # W_0 = S_2 / 1 alone


def test_a_point_exactly_at_the_radius_is_out():
    p = np.array([[0, 0, 0], [2, 0, 0]], dtype=np.float32)
    n = np.array([Z, Y], dtype=np.float32)
    assert fc.fpfh(p, n, 2.0)[2].tolist() == [0, 0] and not fc.fpfh(p, n, 2.0)[0].any()
    assert fc.fpfh(p, n, float(np.nextafter(np.float32(2.0), np.float32(3.0))))[2].tolist() == [1, 1]
    assert not fc.fpfh(p, n, 0.0)[0].any()


def test_invalid_rows_take_part_in_no_pair():
    p = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [0, 0, 1]], dtype=np.float64)
    n = np.array([Z, (np.nan, 0, 0), (0, 0, 0), (np.inf, 0, 1)], dtype=np.float64)
    f, c, m = fc.fpfh(p, n, 5.0)
    assert m.tolist() == [3, 3, 3, 3] and not c.any() and not f.any()
    n[2] = X
    f, c, m = fc.fpfh(p, n, 5.0)
    assert c[0, :11].sum() == 1 and c[2, :11].sum() == 1 and not c[1].any() and not c[3].any() and not f[1].any() and not f[3].any()


def _independent_pairs(p, n, i, j):
    """The features of the pairs (i[k], j[k]) with vectorised numpy and arctan2: (theta, f2, f3) as float64 arrays."""
    dp = p[j] - p[i]
    ln = np.sqrt(np.einsum("ij,ij->i", dp, dp))
    a1 = np.einsum("ij,ij->i", n[i], dp) / ln
    a2 = np.einsum("ij,ij->i", n[j], dp) / ln
    sw = np.abs(a1) < np.abs(a2)
    n1 = np.where(sw[:, None], n[j], n[i]); n2 = np.where(sw[:, None], n[i], n[j])
    dp = np.where(sw[:, None], -dp, dp); f3 = np.where(sw, -a2, a1)
    v = np.cross(dp / ln[:, None], n1)
    v = v / np.linalg.norm(v, axis=1)[:, None]
    w = np.cross(n1, v)
    return np.arctan2(np.einsum("ij,ij->i", w, n2), np.einsum("ij,ij->i", n1, n2)), np.einsum("ij,ij->i", v, n2), f3


def test_against_arctan2_and_vectorised_dots():
    rng = np.random.default_rng(24)
    p = rng.random((2000, 3))
    n = rng.standard_normal((2000, 3)); n /= np.linalg.norm(n, axis=1)[:, None]
    radius = 0.12
    one = fc.Fpfh(p, n, radius)
    ii, jj = [], []
    for i in range(len(p)):
        rows = one.neighbours(i)[0]
        ii += [i] * len(rows); jj += rows.tolist()
    ii, jj = np.array(ii), np.array(jj)
    assert len(ii) > 20000
    theta, f2, f3 = _independent_pairs(p, n, ii, jj)
    pos = np.stack([11.0 * (theta + np.pi) / (2.0 * np.pi), 11.0 * (f2 + 1.0) * 0.5, 11.0 * (f3 + 1.0) * 0.5], axis=1)
    near_edge = (np.abs(pos - np.rint(pos)) < 11.0 * 1e-12).any(axis=1)         # a feature within 1e-12 of a bin edge (the bins are 2 pi / 11 and 2 / 11 wide)
    assert near_edge.sum() <= 1e-4 * len(ii), near_edge.sum()                   # the cap: above it the test fails, it does not pass on less
    want = np.clip(np.floor(pos), 0, 10).astype(int)
    for k in np.flatnonzero(~near_edge):
        got = fc.pair_bins(one.P[ii[k]], one.N[ii[k]], one.P[jj[k]], one.N[jj[k]])
        assert got == tuple(want[k]), (k, got, want[k])
    # and the counts are those pairs, added up
    keep = ~near_edge
    hist = np.zeros((len(p), 33), dtype=np.int64)
    for g in range(3):
        np.add.at(hist, (ii[keep], g * 11 + want[keep, g]), 1)
    clean = np.setdiff1d(np.arange(len(p)), ii[near_edge])
    for i in clean[:300]:
        assert one.counts(int(i))[0] == hist[i].tolist(), i
