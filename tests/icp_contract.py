"""The contract of register_point_clouds_icp in numpy and plain Python floats. This module is the definition; the GPU path
(csrc/icp.h, csrc/icp_host.h) equals it to the byte. With T the input dtype and M the current 4x4 float64 transform:

  evaluate(M)  p = T(M * source) with every product and sum rounded in float64 in the order written in `transform`; (d2, j) = nearest(p, target),
               this library's k = 1 search with squared distances; row i is an inlier iff d2 < T(max_correspondence_distance)^2 (strict, false
               for a non-finite d2); every row contributes float64 terms that are +0.0 for a non-inlier (a select, no multiplication by a mask);
               each sum is taken in the fixed order of `fold64`.
  solve        float64, only + - * /, sqrt and comparisons in a fixed order (no libm beyond sqrt, no BLAS / LAPACK), so that this Python and the
               C++ of csrc/icp_host.h round alike: Horn's closed form with a cyclic Jacobi iteration (point-to-point), a 6x6 Cholesky solve
               (point-to-plane).
  loop         Open3D's registration_icp: evaluate, stop on no correspondences / on small absolute changes of fitness and rmse / at
               max_iterations / on a degenerate system, else M = D o M.

The order of the sums (S_*): POINT mode  [count, d2, p0 p1 p2, q0 q1 q2, p0q0 p0q1 p0q2 p1q0 ... p2q2]                       (17)
                             PLANE mode  [count, d2, J_u J_v for u <= v row by row (21), J_u r (6), r r]                         (30)
`count` is the sum of 1.0 per inlier, folded like the rest: exact for every row count this library accepts."""
import collections
import math

import numpy as np

IcpResult = collections.namedtuple("IcpResult", "transform fitness inlier_rmse iterations status correspondences")

# Cyclic Jacobi on Horn's symmetric 4x4 matrix: the pairs in this order, this many sweeps. The iteration converges quadratically once the
# off-diagonal mass is small: of 20,000 symmetric 4x4 matrices -- Gaussian entries, entries spread over sixteen decades, two eigenvalues 1e-9
# apart, Horn matrices of a near-identity motion -- every one had its largest off-diagonal entry below 1e-17 of its largest entry after 2 to 6
# sweeps (most after 4). A rotation by an already-zero entry is skipped, so the spare sweeps of a converged matrix cost next to nothing and
# change nothing; 16 leaves a margin of ten and keeps the count a constant of the contract.
JACOBI_SWEEPS = 16
JACOBI_PAIRS = ((0, 1), (0, 2), (0, 3), (1, 2), (1, 3), (2, 3))

N_SUMS_POINT, N_SUMS_PLANE = 17, 30


def fold64(terms):
    """The sum of `terms` (1-D, float64) in the contract's order: pad with +0.0 to rows of 64, add the upper half of every row to its lower half
    six times (w = 32 .. 1), the row results are the next level's terms; until one value remains. At least one level is always taken."""
    y = np.ascontiguousarray(terms, dtype=np.float64).reshape(-1)
    assert y.size > 0
    with np.errstate(all="ignore"):
        while True:
            pad = (-y.size) % 64
            if pad:
                y = np.concatenate([y, np.zeros(pad, np.float64)])
            y = y.reshape(-1, 64)
            for w in (32, 16, 8, 4, 2, 1):
                y = y[:, :w] + y[:, w:2 * w]
            y = y.reshape(-1)
            if y.size == 1:
                return float(y[0])


def transform(M, source):
    """p = T(M * source): float64, x' = ((M00*x + M01*y) + M02*z) + M03, one rounding per operation, then one rounding to T."""
    T = source.dtype.type
    s = source.astype(np.float64)
    x, y, z = s[:, 0], s[:, 1], s[:, 2]
    with np.errstate(all="ignore"):
        cols = [((M[a][0] * x + M[a][1] * y) + M[a][2] * z) + M[a][3] for a in range(3)]
        return np.stack(cols, axis=1).astype(T)


def brute_nearest(p, target):
    """The CPU tests' search: the first minimum of radius_contract.squared_distances. (Exact ties are the library's business: the callers
    assert that there are none.)"""
    import radius_contract as rc
    d2 = rc.squared_distances(p, target)
    j = np.argmin(d2, axis=1)
    return d2[np.arange(len(p)), j], j.astype(np.int64)


def terms_point(p, q):
    return [p[:, a] for a in range(3)] + [q[:, a] for a in range(3)] + [p[:, a] * q[:, b] for a in range(3) for b in range(3)]


def plane_rows(p, q, nrm):
    """J (6 columns) and r of every row, float64."""
    e = p - q
    r = ((e[:, 0] * nrm[:, 0]) + (e[:, 1] * nrm[:, 1])) + (e[:, 2] * nrm[:, 2])
    a0 = p[:, 1] * nrm[:, 2] - p[:, 2] * nrm[:, 1]
    a1 = p[:, 2] * nrm[:, 0] - p[:, 0] * nrm[:, 2]
    a2 = p[:, 0] * nrm[:, 1] - p[:, 1] * nrm[:, 0]
    return [a0, a1, a2, nrm[:, 0], nrm[:, 1], nrm[:, 2]], r


def terms_plane(p, q, nrm):
    J, r = plane_rows(p, q, nrm)
    return [J[u] * J[v] for u in range(6) for v in range(u, 6)] + [J[u] * r for u in range(6)] + [r * r]


Evaluation = collections.namedtuple("Evaluation", "count fitness rmse sums correspondences")


def evaluate(M, source, target, normals, max_correspondence_distance, nearest):
    T = source.dtype.type
    n = len(source)
    p = transform(M, source)
    d2, j = nearest(p, target)
    d2, j = np.asarray(d2).reshape(-1), np.asarray(j).reshape(-1).astype(np.int64)
    assert d2.dtype == source.dtype and d2.shape == (n,) and j.shape == (n,)
    with np.errstate(all="ignore"):
        r2 = T(T(max_correspondence_distance) * T(max_correspondence_distance))
        inlier = d2 < r2
        jj = np.where(inlier, j, 0)
        p64, q64 = p.astype(np.float64), target[jj].astype(np.float64)
        terms = [np.ones(n), d2.astype(np.float64)]
        terms += terms_point(p64, q64) if normals is None else terms_plane(p64, q64, normals[jj].astype(np.float64))
        sums = [fold64(np.where(inlier, t, 0.0)) for t in terms]
    count = int(sums[0])
    assert count == int(np.count_nonzero(inlier))
    rmse = math.sqrt(sums[1] / count) if count else 0.0
    return Evaluation(count, count / n, rmse, sums, np.where(inlier, j, -1).astype(np.int64))


def quat_to_rot(w, x, y, z):
    """The rotation matrix of a unit quaternion, every product and sum in this order (the doublings are exact)."""
    xx, yy, zz = x * x, y * y, z * z
    xy, xz, yz = x * y, x * z, y * z
    wx, wy, wz = w * x, w * y, w * z
    return [[1.0 - 2.0 * (yy + zz), 2.0 * (xy - wz), 2.0 * (xz + wy)],
            [2.0 * (xy + wz), 1.0 - 2.0 * (xx + zz), 2.0 * (yz - wx)],
            [2.0 * (xz - wy), 2.0 * (yz + wx), 1.0 - 2.0 * (xx + yy)]]


def jacobi4(N):
    """Cyclic Jacobi on the symmetric 4x4 N (list of lists): (diagonal, V) with the eigenvectors in V's columns."""
    A = [row[:] for row in N]
    V = [[1.0 if i == k else 0.0 for k in range(4)] for i in range(4)]
    for _ in range(JACOBI_SWEEPS):
        for (p, q) in JACOBI_PAIRS:
            apq = A[p][q]
            if apq == 0.0:
                continue
            theta = (A[q][q] - A[p][p]) / (2.0 * apq)
            den = abs(theta) + math.sqrt(theta * theta + 1.0)
            t = (1.0 / den) if theta >= 0.0 else (-1.0 / den)
            c = 1.0 / math.sqrt(t * t + 1.0)
            s = t * c
            for k in range(4):                      # columns p and q: A <- A G
                akp, akq = A[k][p], A[k][q]
                A[k][p] = c * akp - s * akq
                A[k][q] = s * akp + c * akq
            for k in range(4):                      # rows p and q: A <- G^T A
                apk, aqk = A[p][k], A[q][k]
                A[p][k] = c * apk - s * aqk
                A[q][k] = s * apk + c * aqk
            A[p][q] = A[q][p] = 0.0                 # (what the rotation is chosen for; the rounding left 1e-17 of it)
            for k in range(4):
                vkp, vkq = V[k][p], V[k][q]
                V[k][p] = c * vkp - s * vkq
                V[k][q] = s * vkp + c * vkq
    return [A[i][i] for i in range(4)], V


def horn(S, count):
    """Point-to-point step from the 17 sums: (R, t) with target ~ R source + t. Never None."""
    c = float(count)
    Sp, Sq, Spq = S[2:5], S[5:8], S[8:17]
    mp = [Sp[a] / c for a in range(3)]
    mq = [Sq[a] / c for a in range(3)]
    H = [[Spq[3 * a + b] - Sp[a] * mq[b] for b in range(3)] for a in range(3)]
    (Sxx, Sxy, Sxz), (Syx, Syy, Syz), (Szx, Szy, Szz) = H
    N = [[(Sxx + Syy) + Szz, Syz - Szy, Szx - Sxz, Sxy - Syx],
         [Syz - Szy, (Sxx - Syy) - Szz, Sxy + Syx, Szx + Sxz],
         [Szx - Sxz, Sxy + Syx, (Syy - Sxx) - Szz, Syz + Szy],
         [Sxy - Syx, Szx + Sxz, Syz + Szy, (Szz - Sxx) - Syy]]
    diag, V = jacobi4(N)
    best = 0
    for i in range(1, 4):
        if diag[i] > diag[best]:
            best = i
    w, x, y, z = V[0][best], V[1][best], V[2][best], V[3][best]
    nrm = math.sqrt(((w * w + x * x) + y * y) + z * z)
    R = quat_to_rot(w / nrm, x / nrm, y / nrm, z / nrm)
    t = [mq[a] - (((R[a][0] * mp[0]) + (R[a][1] * mp[1])) + (R[a][2] * mp[2])) for a in range(3)]
    return R, t


def plane_system(S):
    """(A, b) of the point-to-plane step from the 30 sums: A = sum J J^T (6x6, symmetric), b = sum J r."""
    A = [[0.0] * 6 for _ in range(6)]
    k = 2
    for u in range(6):
        for v in range(u, 6):
            A[u][v] = A[v][u] = S[k]
            k += 1
    return A, list(S[23:29])


def cholesky_solve(A, b):
    """x with A x = -b, or None when a pivot is not > 0 (NaN fails that test too)."""
    L = [[0.0] * 6 for _ in range(6)]
    for i in range(6):
        for j in range(i + 1):
            s = A[i][j]
            for k in range(j):
                s = s - L[i][k] * L[j][k]
            if i == j:
                if not s > 0.0:
                    return None
                L[i][i] = math.sqrt(s)
            else:
                L[i][j] = s / L[j][j]
    y = [0.0] * 6
    for i in range(6):
        s = -b[i]
        for k in range(i):
            s = s - L[i][k] * y[k]
        y[i] = s / L[i][i]
    x = [0.0] * 6
    for i in range(5, -1, -1):
        s = y[i]
        for k in range(i + 1, 6):
            s = s - L[k][i] * x[k]
        x[i] = s / L[i][i]
    return x


def plane_step(S):
    A, b = plane_system(S)
    x = cholesky_solve(A, b)
    if x is None:
        return None
    hx, hy, hz = x[0] / 2.0, x[1] / 2.0, x[2] / 2.0
    nrm = math.sqrt(((1.0 + hx * hx) + hy * hy) + hz * hz)
    return quat_to_rot(1.0 / nrm, hx / nrm, hy / nrm, hz / nrm), [x[3], x[4], x[5]]


def compose(R, t, M):
    """D o M for D = (R, t): R_new = R M_R, t_new = R M_t + t, every sum left to right."""
    out = [[0.0] * 4 for _ in range(4)]
    for a in range(3):
        for b in range(3):
            out[a][b] = ((R[a][0] * M[0][b]) + (R[a][1] * M[1][b])) + (R[a][2] * M[2][b])
        out[a][3] = (((R[a][0] * M[0][3]) + (R[a][1] * M[1][3])) + (R[a][2] * M[2][3])) + t[a]
    out[3] = [0.0, 0.0, 0.0, 1.0]
    return out


def register_icp(source, target, target_normals=None, init_transform=None, max_correspondence_distance=math.inf, max_iterations=30,
                 relative_fitness=1e-6, relative_rmse=1e-6, return_correspondences=False, nearest=brute_nearest):
    source, target = np.ascontiguousarray(source), np.ascontiguousarray(target)
    assert source.dtype == target.dtype and source.dtype in (np.float32, np.float64)
    normals = None if target_normals is None else np.ascontiguousarray(target_normals)
    M = np.eye(4) if init_transform is None else np.array(init_transform, dtype=np.float64).reshape(4, 4)
    M = [[float(v) for v in row] for row in M]
    prev, it = None, 0
    while True:
        E = evaluate(M, source, target, normals, max_correspondence_distance, nearest)
        if E.count == 0:
            status = "no_correspondences"
            break
        if it > 0 and abs(E.fitness - prev.fitness) < relative_fitness and abs(E.rmse - prev.rmse) < relative_rmse:
            status = "converged"
            break
        if it == max_iterations:
            status = "max_iterations"
            break
        D = horn(E.sums, E.count) if normals is None else plane_step(E.sums)
        if D is None:
            status = "degenerate"
            break
        M = compose(D[0], D[1], M)
        prev = E
        it += 1
    return IcpResult(np.array(M, dtype=np.float64), E.fitness, E.rmse, it, status, E.correspondences if return_correspondences else None)
