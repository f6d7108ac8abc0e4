"""The contract of register_point_clouds_ransac in numpy and plain Python floats. This module is the definition; the GPU
path (csrc/ransac.h, csrc/ransac_host.h) equals it to the byte. All arithmetic is float64, every operation rounded on its own (no FMA), division
and square root are IEEE; coordinates of the input dtype T are converted exactly. S and T are the source and target clouds, corr the (c, 2)
int64 correspondences [source row, target row].

  draws       hypothesis h of [0, H): (j0, j1, j2) = plane_contract.triples(seed, c, H)[h], three distinct rows of corr;
              s_k = S[corr[j_k, 0]], t_k = T[corr[j_k, 1]].
  pre-check   for the pairs (0,1), (0,2), (1,2): ls = |s_a - s_b|^2, lt = |t_a - t_b|^2, each as (x*x + y*y) + z*z; passes iff ls >= r2*lt and
              lt >= r2*ls for all three, r2 = ratio*ratio. No square root; any NaN fails. (ratio = 0: every triple of finite lengths passes.)
  frame       of (p0, p1, p2): a = p1 - p0, b = p2 - p0, nn = a x b; la = sqrt((a0*a0 + a1*a1) + a2*a2), ln likewise of nn; usable iff la and ln
              are finite and > 0; e1 = a / la, e3 = nn / ln, e2 = e3 x e1.
  hypothesis  R[i][j] = (e1t[i]*e1s[j] + e2t[i]*e2s[j]) + e3t[i]*e3s[j]; ms = ((s0 + s1) + s2) / 3.0, mt likewise;
              tr[i] = mt[i] - ((R[i][0]*ms0 + R[i][1]*ms1) + R[i][2]*ms2); bound = thr*thr if the pre-check passes and both frames are usable,
              else 0.0.
  test        correspondence i is an inlier of (R, tr, bound) iff d2 < bound with x'_a = ((R[a][0]*x + R[a][1]*y) + R[a][2]*z) + tr[a] (the form of
              icp_contract.transform, not rounded to T), d = x' - q, d2 = (d0*d0 + d1*d1) + d2*d2: strict, false for any NaN.
  winner      the lowest h of the largest score (inlier count); a largest score of 0 is "no_alignment": the identity, no inliers, fitness and
              rmse 0.0.
  refit=False the transform is the winner's, and the inliers are the winner's.
  refit=True  and a winner's count >= 3: the 17 sums of icp_contract's point mode [count, d2, p(3), q(3), p_u*q_v (9)] with p the source row as
              float64, untransformed, q the target row, +0.0 for a non-inlier (a select), each by icp_contract.fold64 in correspondence order;
              icp_contract.horn on them gives (R, t) outright; the inliers are the test under it with bound = thr*thr. A count below 3: the
              winner's transform stands.
  fitness     the final inliers (k of them) under the final transform: S = fold64 of their d2, +0.0 elsewhere; inlier_rmse = sqrt(S / k), or 0.0
              when k == 0; fitness = k / c."""
import collections
import math

import numpy as np

from icp_contract import fold64, horn
from plane_contract import triples

RansacRegistrationResult = collections.namedtuple("RansacRegistrationResult", "transform inliers fitness inlier_rmse best_iteration status random_seed")

PAIRS = ((0, 1), (0, 2), (1, 2))


def packed(source, target, corr):
    """(p, q): the (c, 3) float64 source and target points of the correspondences."""
    corr = np.asarray(corr, dtype=np.int64)
    return np.ascontiguousarray(source).astype(np.float64)[corr[:, 0]], np.ascontiguousarray(target).astype(np.float64)[corr[:, 1]]


def _len2(d):
    return (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]


def _cross(a, b):
    return np.stack([a[:, 1] * b[:, 2] - a[:, 2] * b[:, 1], a[:, 2] * b[:, 0] - a[:, 0] * b[:, 2], a[:, 0] * b[:, 1] - a[:, 1] * b[:, 0]], axis=1)


def precheck(s, t, ratio):
    """s, t: three (H, 3) arrays each. The (H,) mask of the hypotheses whose triangles have edges of like length."""
    r2 = np.float64(ratio) * np.float64(ratio)
    ok = np.ones(len(s[0]), dtype=bool)
    for a, b in PAIRS:
        ls, lt = _len2(s[a] - s[b]), _len2(t[a] - t[b])
        ok &= (ls >= r2 * lt) & (lt >= r2 * ls)
    return ok


def frames(p0, p1, p2):
    """(e1, e2, e3, usable) of H triples: (H, 3) arrays and an (H,) mask."""
    a, b = p1 - p0, p2 - p0
    nn = _cross(a, b)
    la, ln = np.sqrt(_len2(a)), np.sqrt(_len2(nn))
    e1, e3 = a / la[:, None], nn / ln[:, None]
    e2 = _cross(e3, e1)
    return e1, e2, e3, np.isfinite(la) & (la > 0) & np.isfinite(ln) & (ln > 0)


def hypotheses(p, q, thr, seed, H, ratio):
    """(R (H, 3, 3), tr (H, 3), bound (H,)) of the H hypotheses over the packed points p, q, float64."""
    j = triples(seed, len(p), H)
    s, t = [p[jk] for jk in j], [q[jk] for jk in j]
    thr = np.float64(thr)
    with np.errstate(all="ignore"):
        ok = precheck(s, t, ratio)
        e1s, e2s, e3s, us = frames(*s)
        e1t, e2t, e3t, ut = frames(*t)
        R = np.empty((H, 3, 3), np.float64)
        for i in range(3):
            for k in range(3):
                R[:, i, k] = (e1t[:, i] * e1s[:, k] + e2t[:, i] * e2s[:, k]) + e3t[:, i] * e3s[:, k]
        ms, mt = ((s[0] + s[1]) + s[2]) / 3.0, ((t[0] + t[1]) + t[2]) / 3.0
        tr = np.stack([mt[:, i] - ((R[:, i, 0] * ms[:, 0] + R[:, i, 1] * ms[:, 1]) + R[:, i, 2] * ms[:, 2]) for i in range(3)], axis=1)
        bound = np.where(ok & us & ut, thr * thr, 0.0)
    return R, tr, bound


def squared_distances(p, q, R, tr):
    """d2 of every correspondence under (R, tr): R a 3x3 and tr a 3-vector of floats."""
    with np.errstate(all="ignore"):
        d = [(((R[a][0] * p[:, 0] + R[a][1] * p[:, 1]) + R[a][2] * p[:, 2]) + tr[a]) - q[:, a] for a in range(3)]
        return (d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]


def inlier_mask(p, q, R, tr, bound, strict=True):
    """strict=False is `<=`: for the tests of the strictness alone."""
    d2 = squared_distances(p, q, R, tr)
    with np.errstate(all="ignore"):
        return (d2 < bound) if strict else (d2 <= bound)


def scores(p, q, R, tr, bound):
    """The inlier counts of the hypotheses. (A bound of 0.0 is not evaluated: no d2 is < 0.0.)"""
    return np.array([int(np.count_nonzero(inlier_mask(p, q, R[h], tr[h], bound[h]))) if bound[h] > 0.0 else 0 for h in range(len(bound))], dtype=np.int64)


def refit_sums(p, q, inl, d2):
    """The 17 sums of icp_contract's point mode over the inliers `inl` (a mask)."""
    with np.errstate(all="ignore"):
        terms = [np.ones(len(p)), d2] + [p[:, a] for a in range(3)] + [q[:, a] for a in range(3)] + [p[:, a] * q[:, b] for a in range(3) for b in range(3)]
        return [fold64(np.where(inl, t, 0.0)) for t in terms]


def register_ransac(source, target, correspondences, max_correspondence_distance, num_iterations=100000, random_seed=1, edge_length_ratio=0.9, refit=True):
    """The contract on numpy clouds; random_seed is the seed actually used (never 0)."""
    source, target = np.ascontiguousarray(source), np.ascontiguousarray(target)
    corr = np.ascontiguousarray(correspondences)
    assert source.dtype == target.dtype and source.dtype in (np.float32, np.float64)
    assert corr.dtype == np.int64 and corr.ndim == 2 and corr.shape[1] == 2 and len(corr) >= 3
    assert 1 <= random_seed <= 0xFFFFFFFF and 0.0 <= edge_length_ratio <= 1.0
    H, c = int(num_iterations), len(corr)
    thr = float(max_correspondence_distance)
    p, q = packed(source, target, corr)
    R, tr, bound = hypotheses(p, q, thr, random_seed, H, edge_length_ratio)
    sc = scores(p, q, R, tr, bound)
    best = int(np.argmax(sc))                            # the first of the largest
    if sc[best] == 0:
        return RansacRegistrationResult(np.eye(4), np.zeros(0, np.int64), 0.0, 0.0, 0, "no_alignment", random_seed)
    Rb, tb, bb = [[float(x) for x in row] for row in R[best]], [float(x) for x in tr[best]], float(bound[best])
    if refit and sc[best] >= 3:
        d2 = squared_distances(p, q, Rb, tb)
        S = refit_sums(p, q, d2 < bb, d2)
        assert int(S[0]) == sc[best]
        Rb, tb = horn(S, int(S[0]))
        bb = thr * thr
    d2 = squared_distances(p, q, Rb, tb)
    with np.errstate(all="ignore"):
        inl = d2 < bb
    k = int(np.count_nonzero(inl))
    rmse = math.sqrt(fold64(np.where(inl, d2, 0.0)) / k) if k else 0.0
    M = np.eye(4)
    M[:3, :3], M[:3, 3] = np.array(Rb, dtype=np.float64), np.array(tb, dtype=np.float64)
    return RansacRegistrationResult(M, np.flatnonzero(inl).astype(np.int64), k / c, rmse, best, "ok", random_seed)
