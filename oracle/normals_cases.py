"""Inputs and the judging rule of the normals tests. TEST INFRASTRUCTURE ONLY (tests/test_oracle.py holds the inputs and the rule to what
they claim without a GPU; tests/test_gpu_normals_fits.py runs the library on them). Every generator is deterministic and returns a
C-contiguous (n, 3) array of the asked dtype."""
import numpy as np

from . import fit_excess

DTYPES = (np.float32, np.float64)


def sheet(n, dtype, seed=3):
    """A wavy sheet with noise in [-1, 1]^2: well-defined normals, varied orientations (the cloud of tests/test_gpu_normals.py)."""
    rng = np.random.default_rng(seed)
    xy = rng.random((n, 2)) * 2 - 1
    z = 0.3 * np.sin(3 * xy[:, 0]) * np.cos(2 * xy[:, 1]) + rng.normal(0, 0.002, n)
    return np.ascontiguousarray(np.concatenate([xy, z[:, None]], 1).astype(dtype))


def sheet_on_lattice(n, dtype, seed=3):
    """The sheet with every coordinate rounded to a multiple of 2^-16 (float32) / 2^-30 (float64): every coordinate difference is then such a
    multiple, so after a scaling by 2^+-20 / 2^+-300 no non-zero squared difference leaves the normal range of the type."""
    q = 2.0 ** (16 if np.dtype(dtype) == np.float32 else 30)
    return np.ascontiguousarray((np.round(sheet(n, np.float64, seed) * q) / q).astype(dtype))


SCALE_EXP = {np.float32: 20, np.float64: 300}
OFFSET = {np.float32: 1000.0, np.float64: 2.0 ** 40}


def rotation(seed):
    return np.linalg.qr(np.random.default_rng(seed).normal(size=(3, 3)))[0]


def line(n, dtype, seed=11):
    """Points on a straight line, not axis-aligned: rank-1 offset matrices up to the rounding of the coordinates."""
    t = np.random.default_rng(seed).random(n)
    return np.ascontiguousarray((t[:, None] * rotation(seed)[:, 0][None, :]).astype(dtype))


def ribbon(n, dtype, seed=17):
    """Extent 1 x 1e-7 x 1e-11, rotated (the ribbon of test_normals_thin_neighbourhoods_f64)."""
    rng = np.random.default_rng(seed)
    p = np.stack([rng.random(n), 1e-7 * rng.random(n), 1e-11 * rng.normal(size=n)], 1)
    return np.ascontiguousarray((p @ rotation(seed).T).astype(dtype))


def tilted_plane(n, dtype, seed=5):
    """An exact plane z = x / 2 + y / 4 over x, y multiples of 2^-10: exact in both dtypes, rank-2 offset matrices."""
    xy = np.random.default_rng(seed).integers(0, 1024, (n, 2)) / 1024.0
    return np.ascontiguousarray(np.stack([xy[:, 0], xy[:, 1], xy[:, 0] / 2 + xy[:, 1] / 4], 1).astype(dtype))


def flat_plane(n, dtype, seed=6, z=0.25):
    """Exactly planar, z constant: a grid with one flat axis."""
    xy = np.random.default_rng(seed).integers(0, 4096, (n, 2)) / 4096.0
    return np.ascontiguousarray(np.stack([xy[:, 0], xy[:, 1], np.full(n, z)], 1).astype(dtype))


def axis_line(n, dtype, seed=7):
    """Points on the x axis through (., 0.5, -0.25): a grid with two flat axes."""
    x = np.random.default_rng(seed).permutation(n) / float(n)
    return np.ascontiguousarray(np.stack([x, np.full(n, 0.5), np.full(n, -0.25)], 1).astype(dtype))


def duplicates(dtype, m=600, times=8, seed=13):
    """Every point of a small sheet `times` times: with k <= times all offsets are zero."""
    p = np.tile(sheet(m, dtype, seed), (times, 1))
    return np.ascontiguousarray(p[np.random.default_rng(seed).permutation(len(p))])


def lattice(dtype, g=16, displaced=False, flat=False):
    """The integer lattice g^3 (g^2 with z = 0 if flat), shuffled. displaced: z += 2^-10 ((7 x + 3 y) mod 5), exact in both dtypes; it makes the
    exactly tied candidates of a neighbourhood differ in their contribution to A^T A."""
    ax = np.arange(g)
    x, y, z = np.meshgrid(ax, ax, ax[:1] if flat else ax, indexing="ij")
    p = np.stack([x.ravel(), y.ravel(), z.ravel()], 1).astype(np.float64)
    if displaced:
        p[:, 2] += 2.0 ** -10 * ((7 * p[:, 0] + 3 * p[:, 1]) % 5)
    return np.ascontiguousarray(p[np.random.default_rng(g).permutation(len(p))].astype(dtype))


def blob_clusters(dtype, n=3000, clusters=4, per=250, seed=19):
    """A Gaussian blob and tight clusters (1 000 points within 1e-4 of four centres): skewed density, isotropic fits."""
    rng = np.random.default_rng(seed)
    b = rng.normal(size=(n, 3))
    c = np.concatenate([b[i] + 1e-4 * (rng.random((per, 3)) - 0.5) for i in range(clusters)])
    p = np.concatenate([b, c])
    return np.ascontiguousarray(p[rng.permutation(len(p))].astype(dtype))


def with_outliers(p, count, seed=23):
    """count far points (extent >> any ball radius used on p) appended."""
    far = 1000.0 + 5000.0 * np.random.default_rng(seed).random((count, 3))
    return np.ascontiguousarray(np.concatenate([p, far.astype(p.dtype)]))


def view_directions(n, dtype, seed=29, odd=True):
    """One random unit direction per row; with odd, every 50th row is zero, every 50th + 1 has length 0.5 and every 50th + 2 length 2."""
    v = np.random.default_rng(seed).normal(size=(n, 3))
    v /= np.linalg.norm(v, axis=1)[:, None]
    if odd:
        v[0::50] = 0.0; v[1::50] *= 0.5; v[2::50] *= 2.0
    return np.ascontiguousarray(v.astype(dtype))


def unit(n, dtype):
    """Rows of n scaled to unit length in np.longdouble, then rounded to dtype (numpy's singular vectors are unit to a few ulps only)."""
    nl = np.asarray(n).astype(np.longdouble)
    ln = np.sqrt((nl * nl).sum(-1))
    return (nl / np.where(ln == 0, 1, ln)[..., None]).astype(dtype)          # (a zero row stays zero)


THRESHOLDS = (np.pi / 2, np.deg2rad(40.0), 0.0)
ANGLE_SLACK = 1e-6             # rad: the kept sets may differ only where the checker's angle is this close to the threshold


def ambiguous_rows(info, thr, dirs):
    """The fitted rows (positions in info["rows"]) whose angle lies within ANGLE_SLACK of the threshold, judged from the checker alone. Rows with a
    zero view direction are never among them: their cosine is an exact 0 and their angle acos(0) for every implementation."""
    nz = np.any(np.asarray(dirs)[info["rows"]] != 0, axis=1)
    return nz & (np.abs(info["ang"] - thr) <= ANGLE_SLACK)


def ambiguous_share(info, thr, dirs):
    return float(np.mean(ambiguous_rows(info, thr, dirs))) if len(info["rows"]) else 0.0


def unseparated_share(gap):
    return float(np.mean(~(gap > 1e-2))) if len(gap) else 0.0


def judge(idx, nrm, idx0, info, dtype, dirs=None, thr=None, separated=False):
    """The contract of one call: (idx, nrm) = the answer under test, (idx0, info) = oracle.normals_*(..., fits=True).
    * the kept rows equal the checker's; with view directions they may differ where the checker's angle is within ANGLE_SLACK of thr;
    * EVERY kept fit meets the residual contract (oracle.fit_excess) against the checker's offset matrix of that row; a kept row whose
      view direction is zero has a zero normal (sign(0) = 0, as the reference);
    * separated cases: where (s1 - s2) / s0 > 1e-2 the direction equals the checker's, 1 - |n . n0| <= 1e-8 (float64) / 1e-6 (float32),
      n . n0 signed when view directions fix the sign; at most 10 % of the fits may be left out of THIS comparison (never of the residual).
    Returns the largest excess (units of fit_excess). Raises AssertionError."""
    idx = np.asarray(idx); nrm = np.asarray(nrm)
    assert idx.dtype == np.int64 and nrm.dtype == np.dtype(dtype) and nrm.shape == (len(idx), 3), (idx.dtype, nrm.dtype, nrm.shape)
    rows = info["rows"]
    if dirs is None:
        assert np.array_equal(idx, idx0), "kept rows differ: %d vs %d, first %s" % (len(idx), len(idx0), np.setxor1d(idx, idx0)[:5])
    else:
        diff = np.setxor1d(idx, idx0)
        pos = np.searchsorted(rows, diff)
        assert np.all(pos < len(rows)) and np.array_equal(rows[pos], diff), "rows without a fit were kept"
        assert np.all(ambiguous_rows(info, thr, dirs)[pos]), "kept rows differ away from the threshold: %s" % diff[:5]
    pos = np.searchsorted(rows, idx)
    assert np.all(pos < len(rows)) and np.array_equal(rows[pos], idx), "rows without a fit were kept"
    assert np.all(np.isfinite(nrm))
    zdir = np.zeros(len(idx), bool)
    if dirs is not None:
        zdir = ~np.any(np.asarray(dirs)[idx] != 0, axis=1)
        assert not np.any(nrm[zdir] != 0), "a zero view direction must give a zero normal"
    A = info["A"]
    sel = np.flatnonzero(~zdir)
    Asel = A[pos[sel]] if isinstance(A, np.ndarray) else [A[j] for j in pos[sel]]
    ok, excess, _, nerr = fit_excess(Asel, nrm[sel], dtype)
    worst = float(excess.max()) if len(excess) else 0.0
    assert ok.all(), "%d of %d fits break the residual contract; largest excess %.3g units, largest | |n| - 1 | %.3g; first rows %s" % (
        (~ok).sum(), len(ok), worst, float(nerr.max()), idx[sel][~ok][:5])
    if separated:
        gap = info["gap"][pos[sel]]
        good = gap > 1e-2
        assert unseparated_share(gap) <= 0.10, unseparated_share(gap)
        dot = np.einsum("ij,ij->i", nrm[sel].astype(np.float64), info["normals"][pos[sel]])
        if dirs is None:
            dot = np.abs(dot)
        tol = 1e-8 if np.dtype(dtype) == np.float64 else 1e-6
        assert np.all(1.0 - dot[good] <= tol), "direction off by %.3g" % float((1.0 - dot[good]).max())
    return worst


def knn_cases():
    """(id, cloud maker(dtype), num_neighbors, max_points_per_leaf, separated) of the _knn table."""
    c = []
    for k in (1, 2, 3, 4, 127, 128, 200):           # m < 3; the grid search's limit (127) and the kd path beyond it
        c.append(("sheet-k%d" % k, lambda t: sheet(5000, t), k, 10, k >= 4))
    c.append(("k=n", lambda t: sheet(300, t, 4), 300, 10, True))
    c.append(("k=n+1", lambda t: sheet(300, t, 4), 301, 10, False))
    c.append(("offset", lambda t: (sheet(5000, t) + np.dtype(t).type(OFFSET[t])).astype(t), 12, 10, True))
    c.append(("line", lambda t: line(3000, t), 12, 10, False))
    c.append(("ribbon", lambda t: ribbon(3000, t), 12, 10, False))
    c.append(("tilted-plane", lambda t: tilted_plane(4000, t), 12, 10, True))
    for k in (4, 8, 12):
        c.append(("duplicates-k%d" % k, lambda t: duplicates(t), k, 10, False))
    for leaf in (1, 10, 33):
        for k in (4, 5):
            c.append(("lattice-displaced-k%d-leaf%d" % (k, leaf), lambda t: lattice(t, displaced=True), k, leaf, False))
        for k in (7, 19):
            c.append(("lattice-k%d-leaf%d" % (k, leaf), lambda t: lattice(t), k, leaf, False))
    c.append(("blob-clusters", lambda t: blob_clusters(t), 12, 10, False))
    return c


def ball_cases():
    """(id, cloud maker(dtype), ball_radius, min_pts_per_ball, separated, sample) of the _ball table that is judged by residual; sample: brute-force
    only that many rows (0: all)."""
    c = []
    c.append(("sheet", lambda t: sheet(2500, t, 5), 0.012, 5, True, 0))
    c.append(("sheet-x20", lambda t: (sheet(2500, t, 5) * np.dtype(t).type(20)).astype(t), 4.0, 5, True, 0))        # d / ball_radius < 1 here, > 1 above
    c.append(("flat-plane", lambda t: flat_plane(1200, t), 0.01, 3, True, 0))
    c.append(("axis-line", lambda t: axis_line(1000, t), 0.0004, 3, False, 0))
    c.append(("identical", lambda t: np.ascontiguousarray(np.tile(np.array([[0.5, -1.25, 3.0]], dtype=t), (50, 1))), 0.01, 3, False, 0))
    c.append(("sees-all", lambda t: blob_clusters(t, n=500, clusters=2, per=50), 1.0e4, 3, False, 0))
    c.append(("one-outlier", lambda t: with_outliers(sheet(1200, t, 5), 1), 0.04, 5, True, 0))
    c.append(("100-outliers", lambda t: with_outliers(sheet(1200, t, 5), 100), 0.04, 5, True, 0))
    c.append(("blob-clusters", lambda t: blob_clusters(t, n=1200, clusters=3, per=100), 0.1, 3, False, 0))
    c.append(("sheet-200k", lambda t: sheet(200000, t, 9), 0.0004, 5, True, 500))
    return c


def sample_rows(n, count, seed=31):
    return np.sort(np.random.default_rng(seed).choice(n, count, replace=False))
