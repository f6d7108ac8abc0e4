"""The batch entry points (-m gpu): pcu_hip_hausdorff_batch_* / pcu_hip_chamfer_batch_* through point_cloud_utils_amd.batched, whose contract
(include/pcu_hip.h) is one sentence: per-pair results are identical to the single-pair calls. A batch keeps up to 16 pairs in flight, each on a
lane -- a full context with every piece of sticky cross-call state (occupancy scale, two-pass build, eager placement, fill-word parity, the
handed-down grid layout, the cached tie-order graph) -- and lane l runs pairs l, l + L, l + 2L, ...: it meets those states in a sequence the
caller does not see. Here: mixed sizes and dtypes, every norm and flag, every rung of the fused ladder (restarts by a stale layout and by an
occupancy rescale, refits, a slot overflow, exact ties), errors and an abandoned batch in the middle, lane counts, chunking, side streams.

Every row is held to two references (check): the oracle on the same arrays -- Hausdorff (d, i, j) equal as tuples, Chamfer within the
documented contract of test_gpu_parity.py (1e-4 relative for float32, 1e-6 for float64), NaN equal to NaN -- and the single-pair call with the
same arguments made afterwards on the same thread: Hausdorff tuples equal; Chamfer float32 within one float32 ulp (both values are float64
sums of the same terms in possibly different order, rounded once to float32), float64 within 1e-10 relative (the bound of the
fused sum against the fp64 sum of the rows).

A test that depends on what a lane has seen before runs on a thread of its own: _lib.ctx is per thread, so that is a fresh context with fresh
lanes. The statistics of a batch are the sums over its pairs, restarts included."""
import os
import threading
import time

import numpy as np
import pytest

import oracle
from test_gpu_parity import _fuzz_cloud

pytestmark = pytest.mark.gpu

DTYPES = [np.float32, np.float64]


@pytest.fixture(scope="module")
def pcu():
    import point_cloud_utils_amd as m
    from point_cloud_utils_amd import _lib
    assert _lib.device_count() > 0, "no GPU visible: the gfx950 path has no CPU fallback"
    return m


def _fresh_thread(fn):
    """fn() on a new thread (a fresh context and fresh lanes); what it raises is re-raised here."""
    err = []
    def body():
        try:
            fn()
        except BaseException as e:          # noqa: BLE001 -- re-raised on the test's thread
            err.append(e)
    th = threading.Thread(target=body); th.start(); th.join()
    if err:
        raise err[0]


def _host(a):
    return a if isinstance(a, np.ndarray) else a.cpu().numpy()


def _same(a, b):
    """tuples / scalars equal, NaN == NaN"""
    a, b = np.atleast_1d(np.asarray(a, np.float64)), np.atleast_1d(np.asarray(b, np.float64))
    return a.shape == b.shape and bool(np.all((a == b) | (np.isnan(a) & np.isnan(b))))


_ORACLE = {}        # (key, op, arguments) -> the oracle's rows: computed once, shared by every test that runs the same pairs, never changed


def _oracle_rows(op, pairs, kind, key, skip, kw):
    k = (key, op, tuple(sorted(kw.items())))
    if key is None or k not in _ORACLE:
        rows = []
        for p, (x, y) in enumerate(pairs):
            if p in skip:
                rows.append(None)
            elif op == "hausdorff":
                rows.append(oracle.hausdorff_distance(_host(x), _host(y), return_index=True, kind=kind, **kw))
            else:
                rows.append(float(oracle.chamfer_distance(_host(x), _host(y), kind=kind, **kw)))
        if key is None:
            return rows
        _ORACLE[k] = rows
    return _ORACLE[k]


def check(pcu, op, pairs, kind, workers, key=None, nan_rows=(), **kw):
    """One batched call over `pairs` (in pair order), every row against the oracle and against the single-pair call (module docstring). key: names
    the pairs for the shared oracle rows. nan_rows (Chamfer): pairs with a NaN coordinate -- the value is NaN in the batch and in the single call;
    the oracle's kd-tree over such a cloud has no stable correspondences and is not asked. Returns the statistics of the batch."""
    from point_cloud_utils_amd import batched
    n = len(pairs)
    f32 = _host(pairs[0][0][:1]).dtype == np.float32
    if op == "hausdorff":
        res = batched.batched_hausdorff(lambda p: pairs[p], n, workers=workers, **kw)
        assert res.shape == (n, 3) and res.dtype == np.float64
    else:
        res = batched.batched_chamfer(lambda p: pairs[p], n, workers=workers, **kw)
        assert res.shape == (n,) and res.dtype == np.float64
    st = pcu.last_stats()
    ref = _oracle_rows(op, pairs, kind, key, set(nan_rows), kw)
    for p, (x, y) in enumerate(pairs):
        what = (op, p, tuple(x.shape), tuple(y.shape), workers, kw)
        if op == "hausdorff":
            assert _same(tuple(res[p]), ref[p]), (what, tuple(res[p]), ref[p])
            one = pcu.hausdorff_distance(x, y, return_index=True, **kw)
            assert _same(tuple(res[p]), one), (what, tuple(res[p]), one)
            continue
        v, one = float(res[p]), float(pcu.chamfer_distance(x, y, **kw))
        if p in nan_rows:
            assert np.isnan(v) and np.isnan(one), (what, v, one)
            continue
        v0 = ref[p]
        if np.isnan(v0) or np.isinf(v0):
            assert _same(v, v0), (what, v, v0)
        else:
            assert abs(v - v0) <= (1e-4 if f32 else 1e-6) * abs(v0), (what, v, v0)
        if np.isnan(one) or np.isinf(one):
            assert _same(v, one), (what, v, one)
        elif f32:
            assert abs(v - one) <= float(np.spacing(np.float32(max(abs(v), abs(one))))), (what, v, one)
        else:
            assert abs(v - one) <= 1e-10 * abs(one), (what, v, one)
    return st


def _n_points(pairs):
    return sum(int(x.shape[0]) + int(y.shape[0]) for x, y in pairs)


# ---- 1. mixed sizes and shapes in one call ---------------------------------------------------------------------------------------------
# 1 row; below 64 rows (atomic build, wave-only search); below 1024 (no shared grid, no hand-down); size ratio above 2 (no shared grid);
# equal sizes (a lane keys the next such pair on this one's layout); distributions that leave the fused attempt on every rung.
MIXED = [((1, 1), "uniform", "uniform"), ((1, 5000), "sphere", "plane"), ((40, 63), "lattice", "dups"), ((63, 64), "line", "uniform"),
         ((64, 1023), "clusters", "aniso"), ((1023, 1024), "offset", "offset"), ((1024, 2049), "plane", "sphere"), ((3000, 700), "dups", "lattice"),
         ((20000, 20000), "uniform", "uniform"), ((20000, 9000), "clusters", "uniform"), ((60000, 50000), "sphere", "sphere"),
         ((5000, 1), "aniso", "line"), ((20000, 20000), "lattice", "lattice"), ((9000, 20000), "dups", "clusters")]
_MIXED_PAIRS = {}


def _mixed_pairs(dtype):
    """The pairs of MIXED, shuffled once with a fixed seed: long and short pairs alternate on a lane and the lanes finish out of order."""
    name = np.dtype(dtype).name
    if name not in _MIXED_PAIRS:
        rng = np.random.default_rng(7001)
        pairs = [(_fuzz_cloud(rng, n, dx, dtype), _fuzz_cloud(rng, m, dy, dtype)) for (n, m), dx, dy in MIXED]
        _MIXED_PAIRS[name] = [pairs[i] for i in np.random.default_rng(7002).permutation(len(pairs))]
    return _MIXED_PAIRS[name]


def _check_mixed(pcu, op, dtype, kind, workers):
    pairs = _mixed_pairs(dtype)
    st = check(pcu, op, pairs, kind, workers, key="mixed-" + np.dtype(dtype).name)
    assert st["n_queries"] == _n_points(pairs), st
    return st


@pytest.mark.parametrize("workers", [1, 3, 5])
@pytest.mark.parametrize("op", ["hausdorff", "chamfer"])
@pytest.mark.parametrize("dtype", DTYPES)
def test_mixed_sizes_and_shapes_in_one_call(pcu, oracle_kind, dtype, op, workers):
    _fresh_thread(lambda: _check_mixed(pcu, op, dtype, oracle_kind, workers))


# ---- 2. every Chamfer norm and every Hausdorff flag ------------------------------------------------------------------------------------
def _flag_pairs(dtype):
    rng = np.random.default_rng(7010)
    lat = np.stack(np.meshgrid(*[np.arange(11)] * 3, indexing="ij"), -1).reshape(-1, 3).astype(dtype)       # (test_metrics_under_exact_ties)
    half = (np.random.default_rng(4).integers(0, 22, (3000, 3)) / 2).astype(dtype)
    return [(_fuzz_cloud(rng, 20000, "uniform", dtype), _fuzz_cloud(rng, 15000, "uniform", dtype)),
            (half, lat),
            (_fuzz_cloud(rng, 9000, "dups", dtype), _fuzz_cloud(rng, 6000, "dups", dtype)),
            (_fuzz_cloud(rng, 7000, "uniform", dtype), _fuzz_cloud(rng, 12000, "uniform", dtype)),
            (_fuzz_cloud(rng, 12000, "sphere", dtype), _fuzz_cloud(rng, 10000, "sphere", dtype)),
            (_fuzz_cloud(rng, 8000, "clusters", dtype), _fuzz_cloud(rng, 8000, "clusters", dtype))]


@pytest.mark.parametrize("dtype", DTYPES)
def test_every_chamfer_norm_through_the_batch(pcu, oracle_kind, dtype):
    """p != 2 is row-based from its begin, with the tie order of every row resolved on the lane (the difference vector of a tied neighbour
    depends on which one is picked): the rows follow the oracle built with the same leaf size."""
    pairs = _flag_pairs(dtype)
    def body():
        for leaf in (10, 1):
            for p in (2, 1, 3, 0.5, np.inf, -np.inf, 0):
                st = check(pcu, "chamfer", pairs, oracle_kind, 3, key="flags-" + np.dtype(dtype).name, p_norm=p, max_points_per_leaf=leaf)
                assert st["n_queries"] == _n_points(pairs), (p, leaf, st)
    _fresh_thread(body)


@pytest.mark.parametrize("dtype", DTYPES)
def test_every_hausdorff_flag_through_the_batch(pcu, oracle_kind, dtype):
    """squared_distances and max_points_per_leaf in a batch; on the lattice pair the arg-max row has exactly tied neighbours, so j is re-read in
    the tie order of the oracle's tree with the same leaf size (witness: n_tie_true > 0 with one lane)."""
    pairs = _flag_pairs(dtype)
    def body():
        for workers in (1, 3):
            for squared in (False, True):
                for leaf in (10, 1, 33):
                    st = check(pcu, "hausdorff", pairs, oracle_kind, workers, key="flags-" + np.dtype(dtype).name, squared_distances=squared,
                               max_points_per_leaf=leaf)
                    assert st["n_queries"] == _n_points(pairs), (squared, leaf, st)
                    if workers == 1:
                        assert st["n_tie_true"] > 0, (squared, leaf, st)
    _fresh_thread(body)


# ---- 3. restarts inside the batch: stale handed-down layout -----------------------------------------------------------------------------
LAYOUT_N, LAYOUT_M = 20_000, 18_000      # (the smallest size tried: the three jumps restart there; _layout_sequence itself uses 180 000 / 150 000)


def _layout_pairs(dtype, n=LAYOUT_N, m=LAYOUT_M):
    """The steps of test_gpu_parity._layout_sequence as eight pairs of one size: same, same, 1 % jitter, x3, +10, x0.1, back, a Gaussian blob."""
    rng = np.random.default_rng(606)
    bx, by = rng.random((n, 3)).astype(dtype), rng.random((m, 3)).astype(dtype)
    steps = [(1.0, 0.0), (1.0, 0.0), (1.01, 0.002), (3.0, 0.0), (3.0, 10.0), (0.1, 10.0), (1.0, 0.0)]
    pairs = [((bx * dtype(sc) + dtype(off)).astype(dtype), (by * dtype(sc) + dtype(off)).astype(dtype)) for sc, off in steps]
    pairs.append((rng.normal(0.5, 0.05, (n, 3)).astype(dtype), rng.normal(0.5, 0.05, (m, 3)).astype(dtype)))
    return pairs


# The layout is handed down by the staged one-pass build of a fused call, between calls whose two clouds share one bucket plan -- clouds of
# different sizes do only on a shared grid: none of these may be set for the restarts to be witnessed.
_NO_HAND_DOWN = ("PCU_HIP_NO_GEO_CACHE", "PCU_HIP_NO_FUSE", "PCU_HIP_BUILD_V1", "PCU_HIP_TWO_PASS", "PCU_HIP_NO_SHARED_GRID")


@pytest.mark.parametrize("dtype", DTYPES)
def test_stale_layout_restarts_inside_the_batch(pcu, oracle_kind, dtype):
    """Eight pairs of 20 000 against 18 000 points whose geometry jumps from pair to pair. With one lane every pair keys its points on its
    predecessor's layout; the three jumps (x3, +10, x0.1) are refused as stale and the pair restarts inside batch_run -- its own restart loop,
    not with_restarts. The restarted attempt reports into the lane's statistics: n_queries counts every pair, n_grid_builds the abandoned
    attempts too (>= 2 per pair + 2 per restart). Then three lanes: every lane sees another subsequence. Every batch on a thread of its own:
    the blob that ends the sequence overflows a slot of the one-pass build, after which its lane builds two-pass and hands no layout down."""
    pairs = _layout_pairs(dtype)
    key = "layout-" + np.dtype(dtype).name
    witnessed = all(os.environ.get(v) is None for v in _NO_HAND_DOWN)
    def run(op, workers):
        st = check(pcu, op, pairs, oracle_kind, workers, key=key)
        assert st["n_queries"] == _n_points(pairs), (op, workers, st)
        if workers == 1 and witnessed:
            assert st["n_grid_builds"] >= 2 * len(pairs) + 2 * 3, (op, st)
    for workers in (1, 3):
        for op in ("hausdorff", "chamfer"):
            _fresh_thread(lambda: run(op, workers))


# ---- 4. restarts inside the batch: occupancy rescale, and sticky lane state -------------------------------------------------------------
SURF_N, SURF_M = 100_000, 80_000         # (the smallest size tried: a fresh context restarts the first pair on a finer grid; the single-call test uses 400 000 / 300 000)
REFIT_N = 60_000
OVERFLOW_N, OVERFLOW_M = 100_000, 80_000


def _sphere(rng, n):
    v = rng.normal(size=(n, 3)); v /= np.linalg.norm(v, axis=1, keepdims=True)
    return v.astype(np.float32)


def _surface_pairs():
    """The sequence of test_surface_clouds_take_the_finer_grid_and_stay_exact: surfaces make the passes give up on the balance check and the call
    restart on a finer grid, which the context keeps; a volume-filling cloud afterwards switches back."""
    rng = np.random.default_rng(41)
    sx, sy = _sphere(rng, SURF_N), _sphere(rng, SURF_M)
    ux, uy = rng.random((SURF_M, 3), dtype=np.float32), rng.random((SURF_M, 3), dtype=np.float32)
    return [(sx, sy), (sx, sy), (ux, uy), (sx, uy), (ux, uy)]


def test_occupancy_rescale_restarts_inside_the_batch(pcu, oracle_kind):
    """One lane meets the whole sequence, two lanes diverge in their occupancy scale. Witness (sizes: 100 000 / 80 000): the single-pair call
    on a fresh context restarts on the first pair (more than 2 index builds), and so does the one-lane batch."""
    pairs = _surface_pairs()
    def single():
        assert _same(pcu.hausdorff_distance(*pairs[0], return_index=True), oracle.hausdorff_distance(*pairs[0], return_index=True, kind=oracle_kind))
        assert pcu.last_stats()["n_grid_builds"] > 2, pcu.last_stats()
    def run(workers):
        for op in ("hausdorff", "chamfer"):
            st = check(pcu, op, pairs, oracle_kind, workers, key="surface")
            assert st["n_queries"] == _n_points(pairs), (op, workers, st)
            if workers == 1 and op == "hausdorff":
                assert st["n_grid_builds"] > 2 * len(pairs), st
    _fresh_thread(single)
    _fresh_thread(lambda: run(1))
    _fresh_thread(lambda: run(2))


def _uniform_pairs(seed, count, n, m, dtype=np.float32):
    rng = np.random.default_rng(seed)
    return [(rng.random((n, 3)).astype(dtype), rng.random((m, 3)).astype(dtype)) for _ in range(count)]


def test_refit_pair_among_uniform_pairs(pcu, oracle_kind):
    """The pair of test_unbalanced_clouds_refit_path (a far outlier and a tight cluster: every direction stops at the balance check, finer grids
    are refitted over the core -- Rows / RowsGiven) at n = 60 000, in one batch with uniform pairs. Witness: more than 2 builds per pair."""
    rng = np.random.default_rng(11)
    n = REFIT_N
    r = np.concatenate([rng.random((n * 9 // 10, 3)), rng.normal(0.5, 0.002, (n // 10, 3))]).astype(np.float32)
    r[0] = [900.0, -700.0, 800.0]
    q = np.concatenate([rng.random((n // 2, 3)), rng.normal(0.5, 0.002, (n // 2, 3))]).astype(np.float32)
    q[1] = [-500.0, 500.0, 0.0]
    u = _uniform_pairs(7040, 4, n, n)
    pairs = [u[0], (q, r), u[1], u[2], (r, q), u[3]]
    def body():
        for op in ("hausdorff", "chamfer"):
            st = check(pcu, op, pairs, oracle_kind, 2, key="refit")
            assert st["n_queries"] == _n_points(pairs), (op, st)
            assert st["n_grid_builds"] > 2 * len(pairs), (op, st)
    _fresh_thread(body)


def test_slot_overflow_pair_among_uniform_pairs(pcu, oracle_kind):
    """The pair of test_one_pass_build_overflow_falls_back (Gaussian clouds overflow the fixed bucket slots of the one-pass build: every pass
    gives up, the index is rebuilt by the two-pass pipeline) in one batch with uniform pairs; the lane that met it builds two-pass from then on,
    the other does not. The same batch again runs on those lanes. Witness (100 000 / 80 000 points, unless PCU_HIP_TWO_PASS rules the one-pass
    build out): more than 2 builds per pair in the first batch."""
    rng = np.random.default_rng(31)
    g = (rng.normal(0.5, 0.05, (OVERFLOW_N, 3)).astype(np.float32), rng.normal(0.5, 0.05, (OVERFLOW_M, 3)).astype(np.float32))
    u = _uniform_pairs(7050, 4, OVERFLOW_N, OVERFLOW_M)
    pairs = [u[0], g, u[1], u[2], u[3]]
    def body():
        for rep in range(2):
            for op in ("hausdorff", "chamfer"):
                st = check(pcu, op, pairs, oracle_kind, 2, key="overflow")
                assert st["n_queries"] == _n_points(pairs), (op, st)
                if rep == 0 and op == "hausdorff" and os.environ.get("PCU_HIP_TWO_PASS") is None:
                    assert st["n_grid_builds"] > 2 * len(pairs), st
    _fresh_thread(body)


# ---- 5. an error in the middle, and the lanes afterwards --------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
def test_error_in_the_middle_and_the_lanes_afterwards(pcu, oracle_kind, dtype):
    """Pair 2 of six has one NaN in its target. Hausdorff refuses the batch (and Chamfer with p_norm = 0, where NaN counts as a non-zero and the
    value depends on correspondences that do not exist); Chamfer returns NaN for that pair and the values of the others. The lanes -- two pairs
    each, the other lanes' pairs were in flight when the error came -- then run the batch without the bad pair twice (both parities of the
    staged build's fill words) and the mixed batch of test 1. batched.py's own refusals leave the lanes alone."""
    from point_cloud_utils_amd import batched
    name = np.dtype(dtype).name
    good = _uniform_pairs(7060, 6, 20_000, 19_000, dtype)
    bad = list(good)
    yb = good[2][1].copy(); yb[1234, 1] = np.nan
    bad[2] = (good[2][0], yb)
    rest = good[:2] + good[3:]
    def afterwards(op, **kw):
        for _ in range(2):
            check(pcu, op, rest, oracle_kind, 3, key="rest-" + name, **kw)
        _check_mixed(pcu, op, dtype, oracle_kind, 3)
    def body():
        with pytest.raises(ValueError, match="non-finite"):
            batched.batched_hausdorff(lambda p: bad[p], 6, workers=3)
        afterwards("hausdorff")
        st = check(pcu, "chamfer", bad, oracle_kind, 3, key="bad-" + name, nan_rows=(2,))
        assert st["n_queries"] == _n_points(bad), st
        with pytest.raises(ValueError, match="non-finite"):
            batched.batched_chamfer(lambda p: bad[p], 6, p_norm=0, workers=3)
        afterwards("chamfer", p_norm=0)
        afterwards("chamfer")
        # what batched.py refuses before the library sees the chunk
        other = np.float64 if dtype == np.float32 else np.float32
        mixed = list(good); mixed[4] = tuple(a.astype(other) for a in good[4])
        import torch
        beside = list(good); beside[1] = tuple(torch.from_numpy(a).cuda() for a in good[1])
        empty = list(good); empty[3] = (good[3][0], good[3][1][:0])
        for fn in (batched.batched_hausdorff, batched.batched_chamfer):
            with pytest.raises(ValueError, match="must share dtype, device and array kind"):
                fn(lambda p: mixed[p], 6)
            with pytest.raises(ValueError, match="must share dtype, device and array kind"):
                fn(lambda p: beside[p], 6)
            with pytest.raises(ValueError, match="Invalid input set with zero elements"):
                fn(lambda p: empty[p], 6)
        none = batched.batched_hausdorff(lambda p: good[p], 0)
        assert none.shape == (0, 3) and none.dtype == np.float64
        none = batched.batched_chamfer(lambda p: good[p], 0)
        assert none.shape == (0,) and none.dtype == np.float64
        check(pcu, "hausdorff", rest, oracle_kind, 3, key="rest-" + name)
    _fresh_thread(body)


# ---- 6. lane count and chunking ---------------------------------------------------------------------------------------------------------
def test_lane_count_changes_and_chunking(pcu, oracle_kind):
    """The same twelve pairs at 4, 1, 3, 20 (12 lanes: one per pair; batch_lanes caps at 16) and 2 lanes on one thread: lanes are created on
    demand and kept, the results are equal each time. Then 130 pairs of 300 to 800 points: three library calls (CHUNK = 64), the last with two
    pairs, rows in pair order."""
    from point_cloud_utils_amd import batched
    assert batched.CHUNK == 64
    twelve = _uniform_pairs(7070, 12, 5000, 5000)
    rng = np.random.default_rng(7071)
    many = [(rng.random((int(rng.integers(300, 801)), 3)).astype(np.float32), rng.random((int(rng.integers(300, 801)), 3)).astype(np.float32)) for _ in range(130)]
    def body():
        for op in ("hausdorff", "chamfer"):
            first = None
            for workers in (4, 1, 3, 20, 2):
                if first is None:
                    check(pcu, op, twelve, oracle_kind, workers, key="twelve")
                fn = batched.batched_hausdorff if op == "hausdorff" else batched.batched_chamfer
                res = fn(lambda p: twelve[p], 12, workers=workers)
                assert pcu.last_stats()["n_queries"] == _n_points(twelve)
                first = res if first is None else first
                assert np.array_equal(res, first), (op, workers)
            check(pcu, op, many, oracle_kind, 4, key="many")
    _fresh_thread(body)


# ---- 7. device tensors produced on a side stream ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
def test_device_tensors_produced_on_a_side_stream(pcu, oracle_kind, dtype):
    """Six pairs of device tensors whose producer kernels are still queued on a side stream (torch's current one) behind something slow when the
    batch is called, without a synchronisation: the lanes run on streams of their own and wait for an event recorded on the caller's stream
    (batch_lanes). Compared with the oracle on host copies taken afterwards."""
    import torch
    tdt = torch.float32 if dtype == np.float32 else torch.float64
    side = torch.cuda.Stream()
    gen = torch.Generator(device="cuda"); gen.manual_seed(11)
    def body():
        for op in ("hausdorff", "chamfer"):
            with torch.cuda.stream(side):
                big = torch.rand((4096, 4096), device="cuda", generator=gen)
                for _ in range(8):                      # something slow first ...
                    big = (big @ big).clamp(0.0, 1.0)
                pairs = []
                for p in range(6):
                    a = torch.rand((30000 + 1000 * p, 3), device="cuda", generator=gen, dtype=tdt)
                    b = torch.rand((25000, 3), device="cuda", generator=gen, dtype=tdt)
                    for _ in range(20):                 # ... then a queue of dependent producer kernels
                        a = (a * 1.0000001).clamp(0.0, 1.0); b = (b * 0.9999999).clamp(0.0, 1.0)
                    pairs.append((a, b))
                check(pcu, op, pairs, oracle_kind, 3)   # enqueued behind the producers, no host sync in between
            torch.cuda.synchronize()
    _fresh_thread(body)


# ---- 8. a batch abandoned by cancel() ---------------------------------------------------------------------------------------------------
def test_abandoned_batch_and_its_lanes_afterwards(pcu, oracle_kind):
    """tests/test_gpu_cancel.py::test_cancel_from_another_thread for a batch: 32 device-resident pairs of 100 000 points in a loop until a
    helper thread's pcu.cancel() (every 20 ms) lands: KeyboardInterrupt, with pairs in flight on every lane. The same lanes then run the same
    pairs three times (both fill-word parities, the layouts and graphs of the abandoned pairs dropped) and the mixed batch of test 1."""
    import torch
    from point_cloud_utils_amd import batched
    host = _uniform_pairs(7080, 32, 100_000, 100_000)
    def body():
        pairs = [tuple(torch.from_numpy(a).cuda() for a in pr) for pr in host]
        started, done = threading.Event(), threading.Event()
        def canceller():
            started.wait()
            while not done.wait(0.02):          # keep asking until the caller has left the loop (a request made between two calls is dropped)
                pcu.cancel()
        th = threading.Thread(target=canceller); th.start()
        t0 = time.perf_counter()
        try:
            with pytest.raises(KeyboardInterrupt):
                started.set()
                while time.perf_counter() - t0 < 60.0:
                    batched.batched_hausdorff(lambda p: pairs[p], 32)
        finally:
            done.set(); th.join()
        assert time.perf_counter() - t0 < 60.0
        for _ in range(3):
            st = check(pcu, "hausdorff", pairs, oracle_kind, 4, key="abandoned")
            assert st["n_queries"] == _n_points(host), st
        _check_mixed(pcu, "hausdorff", np.float32, oracle_kind, 4)
        _check_mixed(pcu, "chamfer", np.float32, oracle_kind, 4)
    _fresh_thread(body)
