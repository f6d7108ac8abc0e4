"""The contract of compute_point_cloud_fpfh in numpy and plain Python floats. With T the input dtype:
  j is a neighbour of i iff j != i and d2(i, j) < r2: radius_contract's arithmetic, d2 in T, r2 = T(radius) * T(radius), strict;
  a row is VALID iff the three components of its normal are finite and not all zero; an invalid row takes part in no pair and its rows of both
  outputs are zero; normals are used as given.
Everything else is float64 on values promoted from T, written with Python floats in plain loops so that no BLAS and no FMA enters: every
product and sum is an operation of its own, dot products are ((x*x) + (y*y)) + (z*z), cross components a*b - c*d, division and math.sqrt are
correctly rounded (pair_bins below is the definition of a pair; theta_bin and unit_bin of the bins).
  spfh_counts[i] counts, over the valid neighbours j of i, the three bins of every pair (i, j) that is not skipped; k_i is the sum of a group;
  S_i[b] = 100 * c_i[b] / k_i (0 where k_i == 0); W_i[b] = the sum, in ascending j, over the neighbours j with d2 > 0 of S_j[b] / float64(d2);
  G_i[g] = the sum of W_i over group g, left to right; F_i[b] = S_i[b] + 100 * W_i[b] / G_i[g] (S_i[b] alone where G_i[g] == 0); features = T(F).
The library sums W in another order (its grid walk's): spfh_counts are equal, features within the bound stated in its docstring. What the
library refuses is not this module's business."""
import math

import numpy as np

from radius_contract import r2_of, squared_distances

BINS = 11
# (C_b, S_b) for b = 1 .. 10: the float64 nearest the cosine and sine of -pi + 2 pi b / 11 (csrc/fpfh.h holds the same literals)
EDGES = ((-0.8412535328311812, -0.5406408174555976), (-0.41541501300188644, -0.9096319953545183), (0.14231483827328514, -0.9898214418809327),
         (0.6548607339452851, -0.7557495743542583), (0.9594929736144974, -0.28173255684142967), (0.9594929736144974, 0.28173255684142967),
         (0.6548607339452851, 0.7557495743542583), (0.14231483827328514, 0.9898214418809327), (-0.41541501300188644, 0.9096319953545183),
         (-0.8412535328311812, 0.5406408174555976))


def theta_bin(x, y):
    """The bin of atan2(y, x) among 11 over [-pi, pi], from * - >= alone. x = y = 0 lands in bin 10; so does y = -0.0 with x < 0."""
    if y < 0.0:
        return sum(1 for c, s in EDGES[0:5] if c * y - s * x >= 0.0)
    return 5 + sum(1 for c, s in EDGES[5:10] if c * y - s * x >= 0.0)


def unit_bin(f):
    """min(max(floor(11 * ((f + 1) * 0.5)), 0), 10), said with comparisons so that a NaN has a bin too: 0."""
    t = 11.0 * ((f + 1.0) * 0.5)
    if not t >= 1.0:
        return 0
    return 10 if t >= 10.0 else int(t)


def _dot(a, b):
    return ((a[0] * b[0]) + (a[1] * b[1])) + (a[2] * b[2])


def pair_bins(pi, ni, pj, nj):
    """(theta bin, f2 bin, f3 bin) of the pair (i, j), or None where it is skipped. Arguments: 3-tuples of Python floats."""
    dp = (pj[0] - pi[0], pj[1] - pi[1], pj[2] - pi[2])
    ln = math.sqrt(_dot(dp, dp))
    if ln == 0.0:
        return None
    a1 = _dot(ni, dp) / ln
    a2 = _dot(nj, dp) / ln
    if abs(a1) < abs(a2):
        n1, n2, dp, f3 = nj, ni, (-dp[0], -dp[1], -dp[2]), -a2
    else:
        n1, n2, f3 = ni, nj, a1
    u = (dp[0] / ln, dp[1] / ln, dp[2] / ln)
    v = (u[1] * n1[2] - u[2] * n1[1], u[2] * n1[0] - u[0] * n1[2], u[0] * n1[1] - u[1] * n1[0])
    vl = math.sqrt(_dot(v, v))
    if vl == 0.0:
        return None
    v = (v[0] / vl, v[1] / vl, v[2] / vl)
    w = (n1[1] * v[2] - n1[2] * v[1], n1[2] * v[0] - n1[0] * v[2], n1[0] * v[1] - n1[1] * v[0])
    f2, y, x = _dot(v, n2), _dot(w, n2), _dot(n1, n2)
    return theta_bin(x, y), unit_bin(f2), unit_bin(f3)


def valid_rows(normals):
    nrm = np.asarray(normals)
    return np.isfinite(nrm).all(axis=1) & (nrm != 0).any(axis=1)


class Fpfh:
    """The contract over one cloud, row by row and on demand (a test of a large cloud asks for a few hundred rows)."""

    def __init__(self, points, normals, radius):
        self.p = np.ascontiguousarray(points)
        self.nrm = np.ascontiguousarray(normals)
        assert self.p.dtype == self.nrm.dtype and self.p.dtype in (np.float32, np.float64)
        self.r2 = r2_of(radius, self.p.dtype)
        self.valid = valid_rows(self.nrm)
        self.P = [tuple(float(v) for v in row) for row in self.p]          # exact promotions
        self.N = [tuple(float(v) for v in row) for row in self.nrm]
        self._nbr, self._spfh = {}, {}

    def neighbours(self, i):
        """(rows ascending, their d2 in T) of the neighbours of row i: valid or not, i itself left out."""
        got = self._nbr.get(i)
        if got is None:
            d2 = squared_distances(self.p[i:i + 1], self.p)[0]
            with np.errstate(all="ignore"):
                member = d2 < self.r2
            member[i] = False
            rows = np.flatnonzero(member)
            got = self._nbr[i] = (rows, d2[rows])
        return got

    def counts(self, i):
        """The 33 counts of row i and, from them, S_i as a list of 33 floats."""
        got = self._spfh.get(i)
        if got is None:
            c = [0] * (3 * BINS)
            if self.valid[i]:
                for j in self.neighbours(i)[0]:
                    if not self.valid[j]:
                        continue
                    bins = pair_bins(self.P[i], self.N[i], self.P[j], self.N[j])
                    if bins is not None:
                        for g in range(3):
                            c[g * BINS + bins[g]] += 1
            k = sum(c[:BINS])
            s = [(100.0 * float(v)) / float(k) if k > 0 else 0.0 for v in c]
            got = self._spfh[i] = (c, s)
        return got

    def row(self, i):
        """F_i as a list of 33 floats (before the rounding to T)."""
        if not self.valid[i]:
            return [0.0] * (3 * BINS)
        s_i = self.counts(i)[1]
        w = [0.0] * (3 * BINS)
        rows, d2 = self.neighbours(i)
        for j, dd in zip(rows, d2):
            dd = float(dd)
            if not dd > 0.0:
                continue
            s_j = self.counts(int(j))[1]
            for b in range(3 * BINS):
                w[b] = w[b] + s_j[b] / dd
        out = []
        for g in range(3):
            tot = 0.0
            for b in range(BINS):
                tot = tot + w[g * BINS + b]
            for b in range(BINS):
                s = s_i[g * BINS + b]
                out.append(s if tot == 0.0 else s + (100.0 * w[g * BINS + b]) / tot)
        return out


def rows_of(f, rows=None):
    """features (len(rows), 33) in the input dtype, spfh_counts (len(rows), 33) int32, neighbour counts m (len(rows),) int64 of the listed rows
    (all of them by default) of the Fpfh object f."""
    rows = range(len(f.p)) if rows is None else [int(r) for r in rows]
    feats = np.array([f.row(i) for i in rows], dtype=np.float64).reshape(len(rows), 3 * BINS)
    counts = np.array([f.counts(i)[0] for i in rows], dtype=np.int32).reshape(len(rows), 3 * BINS)
    m = np.array([len(f.neighbours(i)[0]) for i in rows], dtype=np.int64)
    with np.errstate(all="ignore"):
        return feats.astype(f.p.dtype), counts, m


def fpfh(points, normals, radius, rows=None):
    """rows_of a fresh contract object: (features, spfh_counts, m) of all rows, or of the listed ones."""
    return rows_of(Fpfh(points, normals, radius), rows)
