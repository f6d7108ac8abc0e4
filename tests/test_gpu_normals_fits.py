"""GPU tests (-m gpu) of estimate_point_cloud_normals_knn / _ball that judge EVERY fit ("Normals"): the kept rows equal the
checker's (oracle.normals_*: the reference's neighbour sets, brute-force balls), and every returned normal n meets the residual contract against
the checker's offset matrix A of its row (oracle.fit_excess: |A n|^2 <= s2^2 + (4 m + 64) 2^-53 s0^2, one more 2^-24 s0 on |A n| for float32
clouds; unit length to 8 2^-53 / 2^-23). No fit is left out for being ill-conditioned: where the smallest direction is not separated any unit
vector of the near-null space is as right as Eigen's, and the residual says exactly that. The direction comparison of tests/test_gpu_normals.py is
kept on top for the cases marked separated. Inputs and rule live in oracle/normals_cases.py; tests/test_oracle.py holds both to what they claim
without a GPU (the rule fails a swapped neighbour, two Jacobi sweeps, `<=` in the ball test, `>` for `>=` on min_pts, view directions or normals
of the wrong rows, a leaf size that is not forwarded)."""
import numpy as np
import pytest

import oracle
from oracle import normals_cases as nc

pytestmark = pytest.mark.gpu
_IDS = ["f32", "f64"]
_KNN = nc.knn_cases()
_BALL = nc.ball_cases()
NONFINITE = "contains NaN coordinates, or both \\+inf and -inf along one axis"


@pytest.fixture(scope="module")
def pcu():
    import point_cloud_utils_amd as m
    from point_cloud_utils_amd import _lib
    assert _lib.device_count() > 0
    return m


def _report(name, dtype, worst):
    print("normals excess %-40s %s %.4g" % (name, np.dtype(dtype).name, worst))


@pytest.mark.parametrize("dtype", nc.DTYPES, ids=_IDS)
@pytest.mark.parametrize("case", _KNN, ids=[c[0] for c in _KNN])
def test_normals_knn_every_fit(pcu, oracle_kind, case, dtype):
    name, make, k, leaf, separated = case
    p = make(dtype)
    idx, nrm = pcu.estimate_point_cloud_normals_knn(p, k, max_points_per_leaf=leaf)
    idx0, _, _, info = oracle.normals_knn(p, k, max_points_per_leaf=leaf, kind=oracle_kind, fits=True)
    assert len(idx0) == (0 if name == "k=n+1" else len(p))
    assert nrm.shape == (len(idx0), 3)
    _report("knn " + name, dtype, nc.judge(idx, nrm, idx0, info, dtype, separated=separated))


@pytest.mark.parametrize("dtype", nc.DTYPES, ids=_IDS)
def test_normals_knn_power_of_two_scaling_is_exact(pcu, oracle_kind, dtype):
    """Scaling the cloud by 2^+-20 (float32) / 2^+-300 (float64) leaves idx and every bit of the normals unchanged: squared distances in T, A^T A,
    the trace normalisation and the Jacobi thresholds (applied after it) all scale exactly while no square leaves the normal range."""
    p = nc.sheet_on_lattice(5000, dtype)
    idx, nrm = pcu.estimate_point_cloud_normals_knn(p, 12)
    idx0, _, _, info = oracle.normals_knn(p, 12, kind=oracle_kind, fits=True)
    _report("knn sheet-on-lattice", dtype, nc.judge(idx, nrm, idx0, info, dtype, separated=True))
    for sgn in (1, -1):
        q = (p * dtype(2.0) ** (sgn * nc.SCALE_EXP[dtype])).astype(dtype)
        idx1, nrm1 = pcu.estimate_point_cloud_normals_knn(q, 12)
        assert np.array_equal(idx1, idx) and np.array_equal(nrm1, nrm), sgn


@pytest.mark.parametrize("dtype", nc.DTYPES, ids=_IDS)
@pytest.mark.parametrize("which", ["knn", "ball"])
def test_normals_per_row_view_directions(pcu, oracle_kind, which, dtype):
    """One random direction per row (zero rows, lengths 0.5 and 2 among them), thresholds pi / 2 (the default), 40 degrees and 0: the sign is fixed, so
    n . n0 is compared signed; the kept rows may differ from the checker's only within 1e-6 rad of the threshold. _ball runs in cell order and must read
    the directions and write its results at the point's own row."""
    p = nc.sheet(3000 if which == "knn" else 1500, dtype)
    dirs = nc.view_directions(len(p), dtype)
    for thr in nc.THRESHOLDS:
        kw = {} if thr == np.pi / 2 else {"drop_angle_threshold": thr}
        if which == "knn":
            idx, nrm = pcu.estimate_point_cloud_normals_knn(p, 12, view_directions=dirs, **kw)
            idx0, _, _, info = oracle.normals_knn(p, 12, view_directions=dirs, drop_angle_threshold=thr, kind=oracle_kind, fits=True)
        else:
            idx, nrm = pcu.estimate_point_cloud_normals_ball(p, 0.03, view_directions=dirs, min_pts_per_ball=5, **kw)
            idx0, _, _, info = oracle.normals_ball(p, 0.03, view_directions=dirs, drop_angle_threshold=thr, min_pts_per_ball=5, fits=True)
        assert nc.ambiguous_share(info, thr, dirs) <= 1e-3
        _report("%s dirs thr %.3f" % (which, thr), dtype, nc.judge(idx, nrm, idx0, info, dtype, dirs=dirs, thr=thr, separated=True))


@pytest.mark.parametrize("dtype", nc.DTYPES, ids=_IDS)
def test_normals_ball_membership_on_lattice(pcu, dtype):
    """Strict `d2 < radius` (in the cloud's dtype) and `count >= min_pts`, where they decide: see tests/test_oracle.py::test_normals_ball_lattice_membership."""
    p = nc.lattice(dtype, g=12)
    up = float(np.nextafter(dtype(4), dtype(5)))
    for radius, min_pts in ((4.0, 27), (4.0, 28), (3.0, 19), (3.0, 20), (up, 28), (up, 33), (up, 34)):
        idx, nrm = pcu.estimate_point_cloud_normals_ball(p, radius, min_pts_per_ball=min_pts)
        idx0 = oracle.normals_ball(p, radius, min_pts_per_ball=min_pts)[0]
        assert np.array_equal(idx, idx0), (radius, min_pts, len(idx), len(idx0))
        assert np.allclose(np.linalg.norm(nrm.astype(np.float64), axis=1), 1.0, atol=1e-6)
    assert len(pcu.estimate_point_cloud_normals_ball(p, 4.0, min_pts_per_ball=27)[0]) == 1000
    assert len(pcu.estimate_point_cloud_normals_ball(p, 4.0, min_pts_per_ball=28)[0]) == 0
    flat = nc.lattice(dtype, g=12, flat=True)
    for min_pts, kept in ((9, 100), (10, 0)):
        idx, nrm = pcu.estimate_point_cloud_normals_ball(flat, 4.0, min_pts_per_ball=min_pts)
        assert np.array_equal(idx, oracle.normals_ball(flat, 4.0, min_pts_per_ball=min_pts)[0]) and len(idx) == kept
        assert np.array_equal(np.abs(nrm), np.tile(np.array([0, 0, 1], dtype), (kept, 1)))          # exactly


@pytest.mark.parametrize("dtype", nc.DTYPES, ids=_IDS)
@pytest.mark.parametrize("weight", ["constant", "rbf"])
@pytest.mark.parametrize("case", _BALL, ids=[c[0] for c in _BALL])
def test_normals_ball_every_fit(pcu, case, weight, dtype):
    name, make, radius, min_pts, separated, sample = case
    p = make(dtype)
    idx, nrm = pcu.estimate_point_cloud_normals_ball(p, radius, min_pts_per_ball=min_pts, weight_function=weight)
    rows = nc.sample_rows(len(p), sample) if sample else None
    idx0, _, _, info = oracle.normals_ball(p, radius, min_pts_per_ball=min_pts, weight_function=weight, rows=rows, fits=True)
    assert len(idx0) > 0
    if sample:                                   # the brute-forced sample of a large cloud
        pick = np.isin(idx, rows)
        assert len(idx) > 0.99 * len(p)
        idx, nrm = idx[pick], nrm[pick]
    _report("ball %s %s" % (name, weight), dtype, nc.judge(idx, nrm, idx0, info, dtype, separated=separated))


@pytest.mark.parametrize("dtype", nc.DTYPES, ids=_IDS)
def test_normals_ball_nobody_has_three_members(pcu, dtype):
    p = nc.sheet(3000, dtype, 5)
    idx, nrm = pcu.estimate_point_cloud_normals_ball(p, 1e-12)
    assert idx.shape == (0,) and idx.dtype == np.int64 and nrm.shape == (0, 3) and nrm.dtype == dtype
    dirs = nc.view_directions(len(p), dtype)
    idx, nrm = pcu.estimate_point_cloud_normals_ball(p, 1e-12, view_directions=dirs)
    assert idx.shape == (0,) and idx.dtype == np.int64 and nrm.shape == (0, 3) and nrm.dtype == dtype


@pytest.mark.parametrize("dtype", nc.DTYPES, ids=_IDS)
def test_normals_ball_max_pts(pcu, dtype):
    """max_pts_per_ball at and above the largest ball count fits every member (strict `total > max_pts`): bit-identical to the unlimited call; two calls
    are bit-identical; on an exact plane every subset of >= 3 members gives (0, 0, +-1) exactly."""
    p = nc.sheet(2000, dtype, 5)
    r = 0.03
    d = p[:, None, :] - p[None, :, :]
    largest = int(((d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2] < dtype(r)).sum(1).max())      # members of the fullest ball
    assert largest > 30
    idx_a, nrm_a = pcu.estimate_point_cloud_normals_ball(p, r)
    for cap in (-1, 0, largest, largest + 1, 10 * largest):
        idx_c, nrm_c = pcu.estimate_point_cloud_normals_ball(p, r, max_pts_per_ball=cap)
        assert np.array_equal(idx_c, idx_a) and np.array_equal(nrm_c, nrm_a), cap
    idx_s, nrm_s = pcu.estimate_point_cloud_normals_ball(p, r, max_pts_per_ball=largest - 1)            # the fullest balls are now subsets
    assert np.array_equal(idx_s, idx_a) and not np.array_equal(nrm_s, nrm_a)
    for cap in (3, 7, 20):
        one = pcu.estimate_point_cloud_normals_ball(p, r, max_pts_per_ball=cap)
        two = pcu.estimate_point_cloud_normals_ball(p, r, max_pts_per_ball=cap)
        assert np.array_equal(one[0], idx_a) and np.array_equal(one[0], two[0]) and np.array_equal(one[1], two[1]), cap
    assert np.median(np.abs(np.einsum("ij,ij->i", one[1].astype(np.float64), nrm_a.astype(np.float64)))) > 0.995
    plane = nc.flat_plane(1200, dtype)
    idx0 = oracle.normals_ball(plane, 0.01)[0]
    assert len(idx0) > 1000
    for cap in (3, 4, 5, 11, 64):
        idx, nrm = pcu.estimate_point_cloud_normals_ball(plane, 0.01, max_pts_per_ball=cap)
        assert np.array_equal(idx, idx0)
        assert np.array_equal(np.abs(nrm), np.tile(np.array([0, 0, 1], dtype), (len(idx), 1))), cap


@pytest.mark.parametrize("dtype", nc.DTYPES, ids=_IDS)
def test_normals_input_layouts(pcu, dtype):
    """C-ordered, Fortran-ordered and strided-slice numpy inputs, and torch device tensors (points and view directions), give the same bits."""
    import torch
    p = nc.sheet(3000, dtype, 5)
    dirs = nc.view_directions(len(p), dtype, odd=False)
    wide = np.zeros((2 * len(p), 5), dtype); wide[::2, 1:4] = p
    wdir = np.zeros((len(p), 6), dtype); wdir[:, ::2] = dirs
    forms = [(np.asfortranarray(p), np.asfortranarray(dirs)), (wide[::2, 1:4], wdir[:, ::2])]
    assert not forms[0][0].flags.c_contiguous and not forms[1][0].flags.c_contiguous and np.array_equal(forms[1][0], p) and np.array_equal(forms[1][1], dirs)
    thr = np.deg2rad(40.0)
    for fn, args, kw in ((pcu.estimate_point_cloud_normals_knn, (12,), {}),
                         (pcu.estimate_point_cloud_normals_ball, (0.02,), {"weight_function": "rbf", "min_pts_per_ball": 5})):
        for use_dirs in (False, True):
            vd = lambda d: {"view_directions": d, "drop_angle_threshold": thr} if use_dirs else {}
            idx, nrm = fn(p, *args, **vd(dirs), **kw)
            assert 0 < len(idx) <= len(p)
            for pp, dd in forms:
                i2, n2 = fn(pp, *args, **vd(dd), **kw)
                assert np.array_equal(i2, idx) and np.array_equal(n2, nrm)
            ti, tn = fn(torch.from_numpy(p).cuda(), *args, **vd(torch.from_numpy(dirs).cuda()), **kw)
            assert ti.is_cuda and tn.is_cuda and ti.dtype == torch.int64 and tn.dtype == torch.from_numpy(p).dtype
            assert np.array_equal(ti.cpu().numpy(), idx) and np.array_equal(tn.cpu().numpy(), nrm)


def test_normals_argument_errors(pcu):
    """The reference's texts (point_cloud_utils/_pointcloud_normals.py, src/point_cloud_normals.cpp) for input the wrappers refuse."""
    p = nc.sheet(100, np.float64)
    for fn, arg in ((pcu.estimate_point_cloud_normals_knn, 5), (pcu.estimate_point_cloud_normals_ball, 0.1)):
        with pytest.raises(ValueError, match=r"Invalid scalar type \(float16\) for argument 'points'. Expected one of \['float32', 'float64'\]"):
            fn(p.astype(np.float16), arg)
        with pytest.raises(ValueError, match=r"Invalid scalar type \(int64\) for argument 'points'"):
            fn((p * 100).astype(np.int64), arg)
        with pytest.raises(ValueError, match=r"Invalid scalar type \(float32\) for argument 'view_dirs'. Expected it to match argument 'points' which is of type float64"):
            fn(p, arg, view_directions=np.ones((100, 3), np.float32))
        with pytest.raises(ValueError, match=r"Invalid view directions does not match the number of points.*view_dirs.shape = \(100, 2\)"):
            fn(p, arg, view_directions=np.ones((100, 2)))
        with pytest.raises(ValueError, match=r"Invalid shape for view_directions, must be \(n, 3\)"):
            fn(p, arg, view_directions=np.ones(300))
        with pytest.raises(ValueError, match=r"Invalid shape for points, must be \(n, 3\) but got \(100, 2\)"):
            fn(p[:, :2], arg)
        with pytest.raises(ValueError, match="Invalid type for view_directions, must be None or a NumPy array"):
            fn(p, arg, view_directions=[[0.0, 0.0, 1.0]] * 100)


@pytest.mark.parametrize("dtype", nc.DTYPES, ids=_IDS)
@pytest.mark.parametrize("which", ["knn", "ball"])
def test_normals_nonfinite_input(pcu, oracle_kind, which, dtype):
    """The rule of every cloud that is searched in (README "Limits"): NaN, or +inf and -inf along one axis, is a ValueError; a row with infinities of one
    sign per axis is dropped, is nobody's neighbour / member, and every other row's result is what the cloud without it gives -- bit for bit: _knn adds
    its neighbours up in order of distance; _ball in the order of its grid's cells, rows ascending inside a cell, and the grid is laid over the finite
    values with cells of ball_radius^(1/2) / 1.98 (a ball this large against the cloud's density fixes the cell size, so the three extra rows do not move it)."""
    p = nc.sheet(3000 if which == "knn" else 1200, dtype, 5)
    if which == "knn":
        run = lambda c: pcu.estimate_point_cloud_normals_knn(c, 12)
        idx0, _, _, info = oracle.normals_knn(p, 12, kind=oracle_kind, fits=True)
    else:
        run = lambda c: pcu.estimate_point_cloud_normals_ball(c, 0.3, min_pts_per_ball=5)
        idx0, _, _, info = oracle.normals_ball(p, 0.3, min_pts_per_ball=5, fits=True)
    bad = p.copy(); bad[1034, 1] = np.nan
    with pytest.raises(ValueError, match=NONFINITE):
        run(bad)
    bad = p.copy(); bad[5, 2] = np.inf; bad[1100, 2] = -np.inf
    with pytest.raises(ValueError, match=NONFINITE):
        run(bad)
    idx, nrm = run(p)
    for extra in ([[np.inf, 0.0, 0.0]], [[np.inf, 0.0, -np.inf], [0.1, np.inf, 0.2], [np.inf, np.inf, -np.inf]]):
        q = np.ascontiguousarray(np.concatenate([p, np.array(extra, dtype)]))
        idx1, nrm1 = run(q)
        assert np.array_equal(idx1, idx) and idx1.max() < len(p)
        nc.judge(idx1, nrm1, idx0, info, dtype, separated=True)
        assert np.array_equal(nrm1, nrm)
