"""The contract of segment_point_cloud_plane in numpy and plain Python floats. This module is the definition; the GPU path
(csrc/plane.h, csrc/plane_host.h) equals it to the byte. All arithmetic is float64, every operation rounded on its own (no FMA); coordinates
of the input dtype T are converted exactly. `mix`, GOLDEN_GAMMA and `priority` are sampling_contract's (csrc/poisson.h: pd_mix, pd_priority).

  draws       hypothesis h of [0, H): p = priority(seed, h), h_j = mix(p + (j + 1) * GAMMA mod 2^64), j = 0, 1, 2 (csrc/mesh_sample.h: ms_draw);
              i0 = h_0 mod n; i1 = h_1 mod (n - 1), plus 1 if >= i0; i2 = h_2 mod (n - 2), plus 1 if >= min(i0, i1), then plus 1 if
              >= max(i0, i1): three distinct rows, a function of (seed, h, n) alone.
  hypothesis  a = p1 - p0, b = p2 - p0, c = a x b, l2 = (c0*c0 + c1*c1) + c2*c2, k = (c0*p0x + c1*p0y) + c2*p0z, t2 = thr*thr,
              bound = t2*l2 if l2 is finite and > 0, else 0.0. No square root, no division.
  test        row i is an inlier of (c, k, bound) iff e*e < bound with e = ((c0*x + c1*y) + c2*z) - k: strict, false for any NaN.
  winner      the lowest h of the largest score (inlier count); a largest score of 0 is "no_plane": a zero plane, no inliers.
  refit=False plane = [c0/l, c1/l, c2/l, -k/l] with l = sqrt(l2); the inliers are the winner's.
  refit=True  o = p0 of the winner; u = row - o for its inliers, +0.0 elsewhere (a select); ten sums, each by icp_contract.fold64 in row order:
              [count, u0, u1, u2, u0u0, u0u1, u0u2, u1u1, u1u2, u2u2]; mu = S_u / count; C[a][b] = S_uaub - S_ua * mu[b] (a <= b, mirrored);
              cyclic Jacobi on C (`jacobi3`); nv = the eigenvector of the first smallest diagonal entry over its length; m = o + mu;
              kk = (nv0*m0 + nv1*m1) + nv2*m2; ll = (nv0*nv0 + nv1*nv1) + nv2*nv2; the inliers are the test with (nv, kk, t2*ll);
              plane = [nv0, nv1, nv2, -kk].
  sign        in both modes the plane is negated if the first of a, b, c that is not zero is negative."""
import collections
import math

import numpy as np

from icp_contract import JACOBI_SWEEPS, fold64
from sampling_contract import GOLDEN_GAMMA, M64, mix, priority

PlaneResult = collections.namedtuple("PlaneResult", "plane inliers best_iteration status random_seed")

JACOBI3_PAIRS = ((0, 1), (0, 2), (1, 2))
N_SUMS = 10


def triples(seed, n, H):
    """(i0, i1, i2): int64 arrays of H rows each."""
    assert n >= 3
    p = priority(seed, H)
    h0, h1, h2 = (mix(p + np.uint64(((j + 1) * GOLDEN_GAMMA) & M64)) for j in range(3))
    i0 = (h0 % np.uint64(n)).astype(np.int64)
    i1 = (h1 % np.uint64(n - 1)).astype(np.int64)
    i1 = i1 + (i1 >= i0)
    lo, hi = np.minimum(i0, i1), np.maximum(i0, i1)
    i2 = (h2 % np.uint64(n - 2)).astype(np.int64)
    i2 = i2 + (i2 >= lo)
    i2 = i2 + (i2 >= hi)
    return i0, i1, i2


def hypotheses(points, thr, seed, H):
    """(c (H, 3), k (H,), bound (H,), i0 (H,)) of the H hypotheses, float64."""
    P = np.ascontiguousarray(points).astype(np.float64)
    i0, i1, i2 = triples(seed, len(P), H)
    p0, p1, p2 = P[i0], P[i1], P[i2]
    thr = np.float64(thr)
    with np.errstate(all="ignore"):
        a, b = p1 - p0, p2 - p0
        c0 = a[:, 1] * b[:, 2] - a[:, 2] * b[:, 1]
        c1 = a[:, 2] * b[:, 0] - a[:, 0] * b[:, 2]
        c2 = a[:, 0] * b[:, 1] - a[:, 1] * b[:, 0]
        l2 = (c0 * c0 + c1 * c1) + c2 * c2
        k = (c0 * p0[:, 0] + c1 * p0[:, 1]) + c2 * p0[:, 2]
        t2 = thr * thr
        bound = np.where(np.isfinite(l2) & (l2 > 0), t2 * l2, 0.0)
    return np.stack([c0, c1, c2], axis=1), k, bound, i0


def inlier_mask(P64, c, k, bound, strict=True):
    """The test of one (c, k, bound) against every row of P64 (float64). strict=False is `<=`: for the tests of the strictness alone."""
    with np.errstate(all="ignore"):
        e = ((c[0] * P64[:, 0] + c[1] * P64[:, 1]) + c[2] * P64[:, 2]) - k
        return (e * e < bound) if strict else (e * e <= bound)


def scores(points, thr, seed, H, strict=True):
    P = np.ascontiguousarray(points).astype(np.float64)
    c, k, bound, _ = hypotheses(points, thr, seed, H)
    return np.array([int(np.count_nonzero(inlier_mask(P, c[h], k[h], bound[h], strict))) for h in range(H)], dtype=np.int64)


def jacobi3(C):
    """Cyclic Jacobi on the symmetric 3x3 C (list of lists): (diagonal, V) with the eigenvectors in V's columns. The rotations are written
    exactly as icp_contract.jacobi4 writes them."""
    A = [row[:] for row in C]
    V = [[1.0 if i == k else 0.0 for k in range(3)] for i in range(3)]
    for _ in range(JACOBI_SWEEPS):
        for (p, q) in JACOBI3_PAIRS:
            apq = A[p][q]
            if apq == 0.0:
                continue
            theta = (A[q][q] - A[p][p]) / (2.0 * apq)
            den = abs(theta) + math.sqrt(theta * theta + 1.0)
            t = (1.0 / den) if theta >= 0.0 else (-1.0 / den)
            c = 1.0 / math.sqrt(t * t + 1.0)
            s = t * c
            for k in range(3):
                akp, akq = A[k][p], A[k][q]
                A[k][p] = c * akp - s * akq
                A[k][q] = s * akp + c * akq
            for k in range(3):
                apk, aqk = A[p][k], A[q][k]
                A[p][k] = c * apk - s * aqk
                A[q][k] = s * apk + c * aqk
            A[p][q] = A[q][p] = 0.0
            for k in range(3):
                vkp, vkq = V[k][p], V[k][q]
                V[k][p] = c * vkp - s * vkq
                V[k][q] = s * vkp + c * vkq
    return [A[i][i] for i in range(3)], V


def refit_sums(P64, inl, o):
    """The ten sums of the inliers `inl` (a mask) about the origin o."""
    with np.errstate(all="ignore"):
        u = [np.where(inl, P64[:, a] - o[a], 0.0) for a in range(3)]
        terms = [np.where(inl, 1.0, 0.0), u[0], u[1], u[2], u[0] * u[0], u[0] * u[1], u[0] * u[2], u[1] * u[1], u[1] * u[2], u[2] * u[2]]
        return [fold64(t) for t in terms]


def _sqrt(x):
    return math.sqrt(x) if x >= 0.0 else math.nan        # (x is NaN or negative only through overflow or NaN upstream: IEEE sqrt gives NaN)


def _div(a, b):
    with np.errstate(all="ignore"):
        return float(np.float64(a) / np.float64(b))      # IEEE division: x / 0 is inf or NaN, never an exception


def refit_plane(S, o):
    """(nv, kk, ll) from the ten sums and the origin o: Python floats."""
    cnt = S[0]
    mu = [_div(S[1 + a], cnt) for a in range(3)]
    Suu = {(0, 0): S[4], (0, 1): S[5], (0, 2): S[6], (1, 1): S[7], (1, 2): S[8], (2, 2): S[9]}
    C = [[0.0] * 3 for _ in range(3)]
    for a in range(3):
        for b in range(a, 3):
            C[a][b] = C[b][a] = Suu[(a, b)] - S[1 + a] * mu[b]
    diag, V = jacobi3(C)
    best = 0
    for i in range(1, 3):
        if diag[i] < diag[best]:
            best = i
    v = [V[0][best], V[1][best], V[2][best]]
    ln = _sqrt((v[0] * v[0] + v[1] * v[1]) + v[2] * v[2])
    nv = [_div(v[a], ln) for a in range(3)]
    m = [o[a] + mu[a] for a in range(3)]
    kk = (nv[0] * m[0] + nv[1] * m[1]) + nv[2] * m[2]
    ll = (nv[0] * nv[0] + nv[1] * nv[1]) + nv[2] * nv[2]
    return nv, kk, ll


def signed(plane):
    for v in plane[:3]:
        if v != 0.0:                                     # (a NaN is "not zero" and not negative)
            return [-x for x in plane] if v < 0.0 else plane
    return plane


def segment_plane(points, distance_threshold, num_iterations=1000, random_seed=1, refit=True):
    """The contract on a numpy cloud; random_seed is the seed actually used (never 0)."""
    points = np.ascontiguousarray(points)
    assert points.dtype in (np.float32, np.float64) and points.ndim == 2 and points.shape[1] == 3 and len(points) >= 3
    assert 1 <= random_seed <= 0xFFFFFFFF
    H = int(num_iterations)
    P = points.astype(np.float64)
    thr = float(distance_threshold)
    c, k, bound, i0 = hypotheses(points, thr, random_seed, H)
    sc = np.array([int(np.count_nonzero(inlier_mask(P, c[h], k[h], bound[h]))) for h in range(H)], dtype=np.int64)
    best = int(np.argmax(sc))                            # the first of the largest
    if sc[best] == 0:
        return PlaneResult(np.zeros(4, np.float64), np.zeros(0, np.int64), 0, "no_plane", random_seed)
    cb = [float(x) for x in c[best]]
    kb = float(k[best])
    inl = inlier_mask(P, cb, kb, bound[best])
    if not refit:
        l = _sqrt((cb[0] * cb[0] + cb[1] * cb[1]) + cb[2] * cb[2])
        plane = [_div(cb[0], l), _div(cb[1], l), _div(cb[2], l), _div(-kb, l)]
    else:
        o = [float(x) for x in P[i0[best]]]
        nv, kk, ll = refit_plane(refit_sums(P, inl, o), o)
        t2 = thr * thr
        inl = inlier_mask(P, nv, kk, t2 * ll)
        plane = [nv[0], nv[1], nv[2], -kk]
    return PlaneResult(np.array(signed(plane), dtype=np.float64), np.flatnonzero(inl).astype(np.int64), best, "ok", random_seed)
