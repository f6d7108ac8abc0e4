"""GPU tests (-m gpu) of the dense transport family (csrc/sinkhorn.h: pairwise_distances, sinkhorn, earth_movers_distance) on every
kernel path, against numpy and the numpy restatement of the reference module (oracle.sinkhorn, pinned to the reference by
tests/test_oracle.py).

* pairwise_distances: numpy's bytes for ord None / 2 / 1 / +-inf / 0 (k_pairwise sums in numpy's pairwise order), within ULP_POW ulps
  per entry for the other ords (the powers are taken in double there, in T by numpy), numpy's NaN / inf pattern on non-finite input.
* sinkhorn: every dispatch path (k_sink_iter<T, 4>, k_sink_iter<T, 16>, the two-pass k_sink_rows / k_sink_cols / k_sink_cols_finish;
  each also under PCU_HIP_SINK_TWO_PASS=1 in a child process) at nb = 1 and 4, held per entry to the reference in the same dtype and
  to a float64 truth within C_PLAN u_T S (u_T: unit roundoff of T, S = max|M| / eps + 8), and the column marginal sum_i P_ij = b_j to the
  same kind of bound; the stopping rule lands on the reference's iteration on both sides of the host's every-8th poll.
* earth_movers_distance: past one grid-stride pass of k_dot_partial; the scalar within 1 ulp of T of math.fsum of the products."""
import ctypes
import json
import math
import os
import subprocess
import sys

import numpy as np
import pytest

import oracle

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

ULP_POW = 8             # general ord: |got - numpy| <= ULP_POW ulps of numpy's value, per entry
C_PLAN = 8              # Sinkhorn: |P - P_ref| <= C_PLAN u_T S P_ref + tiny_T per entry; |sum_i P_ij - b_j| <= C_PLAN u_T S b_j


@pytest.fixture(scope="module")
def pcu():
    import point_cloud_utils_amd as m
    from point_cloud_utils_amd import _lib
    assert _lib.device_count() > 0
    return m


def _u(dt):
    return float(np.finfo(dt).eps) / 2


def _same_bits(got, ref, what):
    assert got.dtype == ref.dtype and got.shape == ref.shape, what
    if got.tobytes() != ref.tobytes():
        bad = np.argwhere(got != ref)
        raise AssertionError(f"{what}: {len(bad)} entries differ, first {tuple(bad[0])}: {got[tuple(bad[0])]!r} vs {ref[tuple(bad[0])]!r}")


def _same_nonfinite(got, ref, what):
    assert np.array_equal(np.isnan(got), np.isnan(ref)), what
    inf = np.isinf(ref)
    assert np.array_equal(np.isinf(got), inf) and np.array_equal(got[inf], ref[inf]), what


def _within_ulps(got, ref, k, what):
    assert got.dtype == ref.dtype and got.shape == ref.shape, what
    _same_nonfinite(got, ref, what)
    f = np.isfinite(ref)
    err = np.abs(got[f].astype(np.float64) - ref[f]) / np.spacing(np.abs(ref[f]))
    assert err.size == 0 or err.max() <= k, (what, float(err.max()))


# ---- pairwise_distances ------------------------------------------------------------------------------------------------------

EXACT_ORDS = (None, 2, 1, np.inf, -np.inf, 0)
GENERAL_ORDS = (3, 0.5, -1, -2, 2.5)
# m / n around the 4 x 64 tiles of k_pairwise; the widest shapes only at small d (numpy's (nb, m, n, d) temporary)
SHAPES = ((1, 1), (3, 63), (4, 64), (5, 65), (1, 1000), (257, 1))
D_ALL = (1, 2, 3, 7, 8, 9, 16, 17, 64, 129, 300)


def _points(rng, shape, dt):
    x = rng.standard_normal(shape) * 10.0 ** rng.uniform(-2, 2, shape)
    return x.astype(dt)


def _pair_inputs(rng, nb, m, n, d, dt):
    a = _points(rng, (nb, m, d), dt); b = _points(rng, (nb, n, d), dt)
    k = min(m, n)
    b[:, :k, : d // 2] = a[:, :k, : d // 2]             # exact zero components (ord 0; 0 ** negative ord = inf)
    if k > 1:
        b[:, 1] = a[:, 1]                               # an exact zero distance
    return a, b


@pytest.mark.parametrize("dt", [np.float32, np.float64])
def test_pairwise_bits_equal_numpy(pcu, dt):
    """ord None / 2 / 1 / +-inf / 0: numpy's result byte for byte, every d around numpy's 8-term and 128-term summation blocks, nb 1 and 3,
    and m / n on both sides of the 4 x 64 tile edges. Before k_pairwise summed in numpy's order, d >= 8 failed here."""
    rng = np.random.default_rng(101)
    for d in D_ALL:
        shapes = SHAPES + (((257, 1000),) if d <= 9 else ((257, 65),))
        for nb in (1, 3):
            for m, n in shapes:
                a, b = _pair_inputs(rng, nb, m, n, d, dt)
                for o in EXACT_ORDS:
                    ref = np.linalg.norm(a[:, :, None, :] - b[:, None, :, :], axis=-1, ord=o)
                    _same_bits(pcu.pairwise_distances(a, b, o), ref, (dt.__name__, d, nb, m, n, o))


@pytest.mark.parametrize("dt", [np.float32, np.float64])
def test_pairwise_general_ord_within_ulps(pcu, dt):
    """ord 3 / 0.5 / -1 / -2 / 2.5: within ULP_POW ulps of numpy per entry (not relative to the matrix maximum), d = 1 and zero
    differences included (0 ** -1 = inf, inf ** -1 = 0: exactly numpy's 0)."""
    rng = np.random.default_rng(102)
    for d in (1, 3, 8, 17, 129):
        for nb in (1, 3):
            for m, n in ((5, 65), (64, 63), (1, 1)):
                a, b = _pair_inputs(rng, nb, m, n, d, dt)
                for o in GENERAL_ORDS:
                    with np.errstate(divide="ignore"):
                        ref = np.linalg.norm(a[:, :, None, :] - b[:, None, :, :], axis=-1, ord=o)
                    got = pcu.pairwise_distances(a, b, o)
                    _within_ulps(got, ref, ULP_POW, (dt.__name__, d, nb, m, n, o))
                    if o < 0 and min(m, n) > 1:
                        assert (ref[:, 1, 1] == 0).all() and (got[:, 1, 1] == 0).all()


@pytest.mark.parametrize("dt", [np.float32, np.float64])
def test_pairwise_non_finite_coordinates(pcu, dt):
    """NaN, +inf, -inf and inf - inf in the coordinates: numpy's value at every ord, NaN positions included. Before the fix, ord = +-inf
    dropped the NaN (a NaN lost every comparison of the running max / min)."""
    rng = np.random.default_rng(103)
    for d in (3, 9, 130):
        a = _points(rng, (2, 6, d), dt); b = _points(rng, (2, 70, d), dt)
        a[0, 0, d - 1] = np.nan                         # a NaN last: after the running max has a finite value
        a[0, 1, 0] = np.nan                             # and first
        a[1, 2, d // 2] = np.inf
        a[1, 3, 1] = -np.inf
        b[1, 5, d // 2] = np.inf                        # with a[1, 2]: inf - inf = NaN
        b[0, 7, 2] = -np.inf
        b[1, 9, 0] = np.nan
        for o in EXACT_ORDS + GENERAL_ORDS:
            with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
                ref = np.linalg.norm(a[:, :, None, :] - b[:, None, :, :], axis=-1, ord=o)
            got = pcu.pairwise_distances(a, b, o)
            what = (dt.__name__, d, o)
            assert o == 0 or np.isnan(ref).any(), what        # (ord 0 counts NaN != 0 as one)
            if o in EXACT_ORDS:
                _same_nonfinite(got, ref, what)
                f = np.isfinite(ref)
                assert got[f].tobytes() == ref[f].tobytes(), what
            else:
                _within_ulps(got, ref, ULP_POW, what)


def test_pairwise_batch_limit(pcu):
    """65535 batches (gridDim.y) run and match numpy; 65536 are refused with the library's error."""
    rng = np.random.default_rng(104)
    a = rng.random((65535, 1, 3), dtype=np.float32); b = rng.random((65535, 2, 3), dtype=np.float32)
    _same_bits(pcu.pairwise_distances(a, b), np.linalg.norm(a[:, :, None, :] - b[:, None, :, :], axis=-1), "nb = 65535")
    a = np.zeros((65536, 1, 3), np.float32); b = np.zeros((65536, 2, 3), np.float32)
    with pytest.raises(ValueError, match="more than 65535 batches"):
        pcu.pairwise_distances(a, b)


# ---- sinkhorn --------------------------------------------------------------------------------------------------------------

def _sinkhorn_raw(a, b, M, eps, max_iters, stop_thresh):
    """The native entry point on (nb, m), (nb, n), (nb, m, n) as they are: the reference's squeeze leaves the Python API no way to
    pass m = 1 or n = 1. Returns (P, iterations)."""
    from point_cloud_utils_amd import _lib
    from point_cloud_utils_amd._sinkhorn import _prep
    from point_cloud_utils_amd._voxel import _ptr
    (a, b, M), (ctx, flags, stream, _, _), suf, npd = _prep([a, b, M])
    nb, m, n = M.shape
    P = np.empty((nb, m, n), npd)
    it = ctypes.c_int(-1)
    _lib.check(getattr(_lib.lib(), "pcu_hip_sinkhorn_" + suf)(ctx, _ptr(a), _ptr(b), _ptr(M), nb, m, n, float(eps), int(max_iters),
                                                              float(stop_thresh), _ptr(P), ctypes.byref(it), flags, stream))
    return P, it.value


_CHILD = r"""
import json, sys
import numpy as np
sys.path.insert(0, sys.argv[3]); sys.path.insert(0, sys.argv[4])
from test_gpu_dense import _sinkhorn_raw
z = np.load(sys.argv[1])
out = {}
for k, (eps, iters, thresh) in enumerate(json.loads(str(z["cases"]))):
    out[f"P{k}"], it = _sinkhorn_raw(z[f"a{k}"], z[f"b{k}"], z[f"M{k}"], eps, iters, thresh)
    out[f"it{k}"] = np.array(it)
np.savez(sys.argv[2], **out)
"""


def _two_pass(tmp_path, cases):
    """[(a, b, M, eps, max_iters, stop_thresh)] through a child process with PCU_HIP_SINK_TWO_PASS=1 (read once per process)."""
    inp, outp = str(tmp_path / "in.npz"), str(tmp_path / "out.npz")
    arrs = {"cases": np.array(json.dumps([[float(c[3]), int(c[4]), float(c[5])] for c in cases]))}
    for k, c in enumerate(cases):
        arrs[f"a{k}"], arrs[f"b{k}"], arrs[f"M{k}"] = c[0], c[1], c[2]
    np.savez(inp, **arrs)
    env = dict(os.environ, PCU_HIP_SINK_TWO_PASS="1")
    r = subprocess.run([sys.executable, "-c", _CHILD, inp, outp, ROOT, os.path.dirname(os.path.abspath(__file__))], env=env,
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    z = np.load(outp)
    return [(z[f"P{k}"], int(z[f"it{k}"])) for k in range(len(cases))]


def _scale(M, eps):
    """S = max|M| / eps (the exponents' magnitude: an absolute error of u_T S in them is a relative u_T S in P) + 8 (the ulps of exp,
    log and the divisions themselves, which dominate at a large eps)"""
    f = np.isfinite(M)
    return (float(np.abs(M[f]).max()) / eps if f.any() else 0.0) + 8.0


def _plan_close(P, P0, dt, S, what):
    """|P - P0| <= C_PLAN u_T S P0 + tiny_T per entry, NaN where P0 is NaN."""
    assert P.shape == P0.shape, what
    assert np.array_equal(np.isnan(P), np.isnan(P0)), (what, np.argwhere(np.isnan(P) != np.isnan(P0))[:5].tolist(), int(np.isnan(P).sum()), int(np.isnan(P0).sum()))
    f = ~np.isnan(P0)
    err = np.abs(P[f].astype(np.float64) - P0[f].astype(np.float64))
    lim = C_PLAN * _u(dt) * S * np.abs(P0[f].astype(np.float64)) + float(np.finfo(dt).tiny)
    ratio = float((err / lim).max()) if err.size else 0.0
    assert ratio <= 1.0, (what, ratio)
    return ratio


def _marginal_close(P, b, dt, S, what):
    cs = P.astype(np.float64).sum(axis=1)
    bb = b.astype(np.float64)
    lim = C_PLAN * _u(dt) * S * bb + P.shape[1] * float(np.finfo(dt).tiny)
    assert (np.abs(cs - bb) <= lim).all(), (what, float((np.abs(cs - bb) / lim).max()))


def _problem(rng, nb, m, n, dt):
    M = oracle.pairwise_distances(rng.random((nb, m, 3)), rng.random((nb, n, 3))).astype(dt)
    wa = rng.random((nb, m)) + 0.5; wa /= wa.sum(1, keepdims=True)
    wb = rng.random((nb, n)) + 0.5; wb /= wb.sum(1, keepdims=True)
    return wa.astype(dt), wb.astype(dt), M


# (nb, m, n): k_sink_iter<T, 4> (n <= 1024), <T, 16> (n <= 4096), two-pass (n > 4096). m < 8, m = 1, partial last row slabs (37 rows:
# slabs of 8; 301 rows: two-pass slabs of 151), and m = 2000 x n = 4100: 8 column-pass slabs at nb = 1, 2 at nb = 4.
SINK_CASES = ((1, 5, 1), (4, 1, 1), (1, 37, 255), (4, 5, 255), (1, 300, 1024), (4, 37, 1024), (1, 5, 1025), (4, 37, 1025),
              (1, 37, 4096), (4, 5, 4096), (1, 1, 4097), (4, 37, 4097), (1, 301, 6000), (4, 5, 6000), (1, 2000, 4100), (4, 2000, 4100),
              (4, 300, 1024))


@pytest.mark.parametrize("dt", [np.float32, np.float64])
def test_sinkhorn_every_path_against_reference_and_float64(pcu, dt, tmp_path):
    """Fixed iteration count (stop_thresh = 0): P per entry against the reference module in T and against a float64 truth, and the
    column marginal, on the single-launch pipeline and (child process) the two-pass one. eps = 1e-4 (the EMD default) included."""
    rng = np.random.default_rng(200)
    cases, runs = [], []
    for nb, m, n in SINK_CASES:
        big = nb * m * n > 1_000_000
        for eps in ((1e-2, 1e-4) if (m, n) in ((300, 1024), (301, 6000)) else (1e-2,)):
            wa, wb, M = _problem(rng, nb, m, n, dt)
            iters = 3 if big else 10
            cases.append((wa, wb, M, eps, iters, 0.0))
            runs.append(_sinkhorn_raw(wa, wb, M, eps, iters, 0.0))
    worst = 0.0
    for c, (P, it), (P2, it2) in zip(cases, runs, _two_pass(tmp_path, cases)):
        wa, wb, M, eps, iters, _ = c
        what = (dt.__name__, M.shape, eps)
        assert it == it2 == iters, what
        P0, it0 = oracle.sinkhorn(wa, wb, M, eps, iters, 0.0, squeeze=False)
        assert it0 == iters
        S = _scale(M, eps)
        for tag, Q in (("single-read", P), ("two-pass", P2)):
            assert Q.dtype == dt
            worst = max(worst, _plan_close(Q, P0, dt, S, what + (tag, "reference")))
            if dt == np.float32:
                Pt, _ = oracle.sinkhorn(wa.astype(np.float64), wb.astype(np.float64), M.astype(np.float64), eps, iters, 0.0, squeeze=False)
                worst = max(worst, _plan_close(Q, Pt, dt, S, what + (tag, "float64 truth")))
            _marginal_close(Q, wb, dt, S, what + (tag,))
    print(f"sinkhorn {dt.__name__}: worst |P - P_ref| / (u_T S P_ref) = {worst * C_PLAN:.2f}")


def _stop_threshold(trajs, t):
    """A threshold at least 1.5x away from max(err_u, err_v) of iteration t (below) and of every earlier iteration (above) in every
    trajectory: the rule fires at t in each of them, and in the kernel's own (differently rounded) errors."""
    lo = 1.5 * max(max(tr[t - 1]) for tr in trajs)
    hi = min(max(tr[s]) for tr in trajs for s in range(t - 1)) / 1.5 if t > 1 else np.inf
    assert lo < hi, (t, lo, hi)
    return math.sqrt(lo * hi) if t > 1 else 2 * lo


@pytest.mark.parametrize("dt", [np.float32, np.float64])
def test_sinkhorn_stops_on_the_reference_iteration(pcu, dt):
    """stop_thresh placed so that the reference stops after t iterations, t = 1 .. 8 (both sides of the host's poll every 8th
    iteration): last_iterations == t exactly, and P as the reference's. Also max_iters reached, max_iters = 0 and 1."""
    rng = np.random.default_rng(300)
    eps = 0.3
    wa, wb, M = _problem(rng, 2, 64, 48, dt)
    S = _scale(M, eps)
    trajs = []
    for x in (dt, np.float64):
        e = []
        oracle.sinkhorn(wa.astype(x), wb.astype(x), M.astype(x), eps, 12, 0.0, errors=e, squeeze=False)
        trajs.append(e)
    for t in range(1, 9):
        th = _stop_threshold(trajs, t)
        P0, it0 = oracle.sinkhorn(wa, wb, M, eps, 50, th, squeeze=False)
        assert it0 == t
        P = pcu.sinkhorn(wa, wb, M, eps=eps, max_iters=50, stop_thresh=th)
        assert pcu.sinkhorn.last_iterations == t, (t, pcu.sinkhorn.last_iterations)
        _plan_close(P, P0, dt, S, ("stop", t))
    for iters in (0, 1, 13):
        P0, it0 = oracle.sinkhorn(wa, wb, M, eps, iters, 0.0, squeeze=False)
        P = pcu.sinkhorn(wa, wb, M, eps=eps, max_iters=iters, stop_thresh=0.0)
        assert it0 == iters and pcu.sinkhorn.last_iterations == iters
        _plan_close(P, P0, dt, S, ("max_iters", iters))
    P = pcu.sinkhorn(wa, wb, M, eps=eps, max_iters=0)
    _plan_close(P, np.exp(-M / dt(eps)), dt, S, "max_iters = 0: exp(-M / eps)")


@pytest.mark.parametrize("dt", [np.float32, np.float64])
def test_sinkhorn_forbidden_row_and_column(pcu, dt, tmp_path):
    """An entirely +inf row, and separately an entirely +inf column, after 1 and 3 iterations on both pipelines: the reference's NaN
    pattern (the NaN spreads from the forbidden line to the whole plan) and its finite values."""
    rng = np.random.default_rng(400)
    cases = []
    for m, n in ((37, 40), (9, 4097)):
        for line in ("row", "col"):
            wa, wb, M = _problem(rng, 1, m, n, dt)
            if line == "row":
                M[0, 5, :] = np.inf
            else:
                M[0, :, 7] = np.inf
            for iters in (1, 3):
                cases.append((wa, wb, M, 1e-2, iters, 0.0))
    for c, (P2, it2) in zip(cases, _two_pass(tmp_path, cases)):
        wa, wb, M, eps, iters, _ = c
        with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
            P0, _ = oracle.sinkhorn(wa, wb, M, eps, iters, 0.0, squeeze=False)
        assert np.isnan(P0).any()
        P, it = _sinkhorn_raw(wa, wb, M, eps, iters, 0.0)
        assert it == it2 == iters
        for tag, Q in (("single-read", P), ("two-pass", P2)):
            _plan_close(Q, P0, dt, _scale(M, eps), (dt.__name__, M.shape, iters, tag))


# ---- earth_movers_distance ---------------------------------------------------------------------------------------------------

def _dot_raw(x, y):
    from point_cloud_utils_amd import _lib
    from point_cloud_utils_amd._sinkhorn import _prep
    from point_cloud_utils_amd._voxel import _ptr
    (x, y), (ctx, flags, stream, _, _), suf, npd = _prep([x, y])
    out = ctypes.c_double(0.0)
    _lib.check(getattr(_lib.lib(), "pcu_hip_dot_" + suf)(ctx, _ptr(x), _ptr(y), int(x.size), ctypes.byref(out), flags, stream))
    return npd(out.value)


def _one_ulp_of_fsum(got, P, M, dt, what):
    prod = (P * M).astype(dt)                           # each product rounded to T, as k_dot_partial takes it
    ref = dt(math.fsum(prod.astype(np.float64).ravel()))
    assert abs(float(got) - float(ref)) <= float(np.spacing(ref)), (what, float(got), float(ref))


def test_emd_past_one_grid_stride_pass(pcu):
    """700 x 600 and 1500 x 1200 (one pass of k_dot_partial's grid is 262144 products), p_norm 2 / 1 / inf: the scalar within 1 ulp of
    math.fsum of the products, P as the reference's, torch inputs giving the same bits. float32 is refused as by the reference (its
    weights are float64); its plan and dot are checked through the native entry points at the EMD default eps = 1e-4."""
    import torch
    rng = np.random.default_rng(500)
    eps, iters = 1e-4, 5
    for n1, n2 in ((700, 600), (1500, 1200)):
        p, q = rng.random((n1, 3)), rng.random((n2, 3))
        for pn in (2, 1, np.inf):
            emd, P = pcu.earth_movers_distance(p, q, pn, eps=eps, max_iters=iters, stop_thresh=0.0)
            M = pcu.pairwise_distances(p, q, pn)
            _, P0 = oracle.earth_movers_distance(p, q, pn, eps, iters, 0.0)
            _plan_close(P, P0, np.float64, _scale(M, eps), ("emd", n1, n2, pn))
            _one_ulp_of_fsum(emd, P, M, np.float64, ("emd f64", n1, n2, pn))
            emd_t, P_t = pcu.earth_movers_distance(torch.from_numpy(p).cuda(), torch.from_numpy(q).cuda(), pn, eps=eps, max_iters=iters,
                                                   stop_thresh=0.0)
            assert float(emd_t) == float(emd) and np.array_equal(P_t.cpu().numpy(), P)
        p32, q32 = p.astype(np.float32), q.astype(np.float32)
        with pytest.raises(ValueError, match="must have the same dtype"):
            pcu.earth_movers_distance(p32, q32)
        M = pcu.pairwise_distances(p32, q32)
        wa = np.full((1, n1), 1 / n1, np.float32); wb = np.full((1, n2), 1 / n2, np.float32)
        P, _ = _sinkhorn_raw(wa, wb, M[None], eps, iters, 0.0)
        P0, _ = oracle.sinkhorn(wa, wb, M[None], eps, iters, 0.0, squeeze=False)
        _plan_close(P, P0, np.float32, _scale(M, eps), ("emd f32 plan", n1, n2))
        _one_ulp_of_fsum(_dot_raw(P[0], M), P[0], M, np.float32, ("emd f32", n1, n2))
