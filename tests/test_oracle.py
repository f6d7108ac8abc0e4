"""CPU tests: the oracle (plain-C restatement) against the golden vectors generated from the reference's own
nanoflann, against oracle/_ref when present, and against exact brute force."""
import glob
import json
import os

import numpy as np
import pytest

import oracle
from conftest import cloud, digest

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
with open(os.path.join(GOLD, "ref_pins.json")) as _f:
    REF_PINS = json.load(_f)
CASES = sorted(p for p in glob.glob(os.path.join(GOLD, "*.npz")) if not p.endswith(("metrics.npz", "sinkhorn.npz", "config1.npz")))


@pytest.mark.parametrize("path", CASES, ids=[os.path.basename(p)[:-4] for p in CASES])
def test_port_matches_golden(path):
    g = np.load(path)
    d, c = oracle.knn(g["q"], g["r"], int(g["k"]), squared_distances=bool(g["squared"]), kind="port")
    assert np.array_equal(c, g["c"])
    assert np.array_equal(d.view(np.uint8), g["d"].view(np.uint8))   # bit-exact distances


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("leaf", [1, 10, 37])
def test_port_matches_ref_when_present(dtype, leaf):
    """The port against the reference's own nanoflann: its answers pinned in tests/golden/ref_pins.json (make_golden.py
    --only-ref-pins), and live as well where oracle/_ref is built."""
    q, r = cloud(1, 3000, dtype), cloud(2, 2500, dtype)
    r = np.concatenate([r, r[:500]])      # duplicates: tie order depends on the tree
    tag = "f32" if dtype == np.float32 else "f64"
    for k in (1, 6):
        d1, c1 = oracle.knn(q, r, k, max_points_per_leaf=leaf, kind="port")
        assert digest(c1) == REF_PINS[f"knn_{tag}_leaf{leaf}_k{k}_c"] and digest(d1) == REF_PINS[f"knn_{tag}_leaf{leaf}_k{k}_d"]
        if oracle.have_ref():
            d0, c0 = oracle.knn(q, r, k, max_points_per_leaf=leaf, kind="ref")
            assert np.array_equal(c0, c1) and np.array_equal(d0, d1)


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_port_matches_brute_without_ties(dtype):
    q, r = cloud(3, 1500, dtype), cloud(4, 2000, dtype)
    for k in (1, 9):
        d0, c0, tie = oracle.brute_knn_with_ties(q, r, k)
        d1, c1 = oracle.knn(q, r, k, kind="port")
        ok = ~tie
        assert ok.sum() > 1400
        assert np.array_equal(c0[ok], c1[ok]) and np.array_equal(d0[ok], d1[ok])
        assert np.array_equal(d0, d1)         # distances are unique even under ties


def test_metrics_golden():
    g = np.load(os.path.join(GOLD, "metrics.npz"))
    for tag in ("f32", "f64"):
        a, b = g[f"a_{tag}"], g[f"b_{tag}"]
        h = oracle.hausdorff_distance(a, b, return_index=True, kind="port")
        assert list(g[f"hausdorff_{tag}"]) == [h[0], h[1], h[2]]
        assert tuple(g[f"one_sided_ab_{tag}"]) == oracle.one_sided_hausdorff_distance(a, b, kind="port")
        assert tuple(g[f"one_sided_ba_sq_{tag}"]) == oracle.one_sided_hausdorff_distance(b, a, squared_distances=True, kind="port")
        ch, cxy, cyx = oracle.chamfer_distance(a, b, return_index=True, kind="port")
        assert float(ch) == g[f"chamfer_{tag}"][0]
        assert np.array_equal(cxy, g[f"cxy_{tag}"]) and np.array_equal(cyx, g[f"cyx_{tag}"])


def test_nonfinite_metrics_golden():
    """tests/golden/nf_*_metrics.npz (generated from the reference's own nanoflann): the C port and the restated Python tails give the
    same answers on clouds with non-finite rows -- unmatched source rows are -1 / -1.0, Chamfer gathers through index -1."""
    import warnings
    for tag in ("f32", "f64"):
        g = np.load(os.path.join(GOLD, f"nf_{tag}_metrics.npz"))
        same = lambda a, b: np.array_equal(np.asarray(a, np.float64), np.asarray(b, np.float64), equal_nan=True)
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            for name in ("inf", "mixed", "last"):
                x, y = g[f"{name}_x"], g[f"{name}_y"]
                assert same(oracle.one_sided_hausdorff_distance(x, y, kind="port"), g[f"{name}_os_xy"])
                assert same(oracle.one_sided_hausdorff_distance(y, x, kind="port"), g[f"{name}_os_yx"])
                assert same(oracle.hausdorff_distance(x, y, True, kind="port"), g[f"{name}_h"])
                ch, cxy, cyx = oracle.chamfer_distance(x, y, return_index=True, kind="port")
                assert np.array_equal(cxy, g[f"{name}_cxy"]) and np.array_equal(cyx, g[f"{name}_cyx"])
                assert same([oracle.chamfer_distance(x, y, p_norm=p, kind="port") for p in (2, 1, np.inf, -np.inf, 0, 3)], g[f"{name}_ch"])
            assert same(oracle.one_sided_hausdorff_distance(g["nan_x"], g["nan_y"], kind="port"), g["nan_os_xy"])
            assert np.isnan(oracle.chamfer_distance(g["nan_x"], g["nan_y"], kind="port"))


def test_reference_test_knn_body_on_oracle():
    """tests/test_examples.py:349-396 of the reference, with the oracle standing in for pcu."""
    rng = np.random.default_rng(0)
    for _ in range(3):
        a, b = rng.random((1000, 3)), rng.random((500, 3))
        k = int(rng.integers(10)) + 1
        d, c = oracle.k_nearest_neighbors(a, b, k)
        assert d.shape == ((1000, k) if k > 1 else (1000,))
        if k == 1:
            d, c = d[:, None], c[:, None]
        assert np.all(np.abs(np.linalg.norm(a[:, None, :] - b[c], axis=-1) - d) < 1e-5)
    with pytest.raises(ValueError):
        oracle.k_nearest_neighbors(a, b, 0)


def test_oracle_normals_on_planes():
    """The numpy restatement of the normals path: exact planes give the plane normal, the view direction fixes the sign and
    filters (src/point_cloud_normals.cpp:115-173)."""
    rng = np.random.default_rng(2)
    xy = rng.random((500, 2))
    p = np.concatenate([xy, (0.5 * xy[:, :1] + 0.25 * xy[:, 1:2])], 1)           # plane z = 0.5 x + 0.25 y
    n0 = np.array([-0.5, -0.25, 1.0]); n0 /= np.linalg.norm(n0)
    idx, nrm, gap = oracle.normals_knn(p, 8)
    assert len(idx) == 500 and np.allclose(np.abs(nrm @ n0), 1.0, atol=1e-9)
    dirs = np.tile(-n0, (500, 1))
    idx, nrm, _ = oracle.normals_knn(p, 8, view_directions=dirs)
    assert len(idx) == 500 and np.allclose(nrm @ n0, -1.0, atol=1e-9)
    idx, _, _ = oracle.normals_knn(p, 8, view_directions=np.tile(np.array([1.0, 0, 0]), (500, 1)), drop_angle_threshold=np.deg2rad(20))
    assert len(idx) == 0                                                       # the normal is ~64 degrees off the x axis
    idx, nrm, _ = oracle.normals_ball(p[:200], 0.05)
    assert np.allclose(np.abs(nrm @ n0), 1.0, atol=1e-9)
    assert len(oracle.normals_knn(p[:5], 9)[0]) == 0                           # fewer points than neighbours: dropped


def test_oracle_morton_port_pinned_to_reference():
    """The numpy restatement of MortonCode64 against the reference's own class (src/common/morton_code.cpp compiled in place
    into oracle/_ref/libpcu_ref_morton.so): its answers pinned in tests/golden/ref_pins.json (make_golden.py --only-ref-pins,
    which also checks that the class decodes its codes back to the points), and live as well where that library is built."""
    rng = np.random.default_rng(0)
    p = rng.integers(-(1 << 20), 1 << 20, (50000, 3)).astype(np.int32)
    p[:4] = [[0, 0, 0], [-1, -1, -1], [(1 << 20) - 1] * 3, [-(1 << 20)] * 3]
    c = oracle.morton_encode(p, "port")
    assert digest(c) == REF_PINS["morton_c"]
    assert np.array_equal(oracle.morton_decode(c, "port"), p)
    c2 = oracle.morton_encode(rng.integers(-2000, 2000, (50000, 3)).astype(np.int32), "port")
    assert digest(c2) == REF_PINS["morton_c2"]
    for sub, name in ((False, "morton_add"), (True, "morton_sub")):
        assert digest(oracle.morton_addsub(c, c2, sub, "port")) == REF_PINS[name]
    cs = np.sort(c)
    for k in (1, 7, 16):
        assert digest(oracle.morton_knn_window(cs, c2[:2000], k, "port")) == REF_PINS[f"morton_knn_{k}"]
    assert digest(oracle.morton_knn_window(cs[:10], c2[:100], 15, "port")) == REF_PINS["morton_knn_short"]
    if oracle.have_ref_morton():
        assert np.array_equal(c, oracle.morton_encode(p, "ref"))
        assert np.array_equal(oracle.morton_decode(c, "ref"), p)
        for sub in (False, True):
            assert np.array_equal(oracle.morton_addsub(c, c2, sub, "ref"), oracle.morton_addsub(c, c2, sub, "port"))
        for k in (1, 7, 16):
            assert np.array_equal(oracle.morton_knn_window(cs, c2[:2000], k, "ref"), oracle.morton_knn_window(cs, c2[:2000], k, "port"))
        assert np.array_equal(oracle.morton_knn_window(cs[:10], c2[:100], 15, "ref"), oracle.morton_knn_window(cs[:10], c2[:100], 15, "port"))


def test_oracle_voxel_and_dedup_restatements():
    rng = np.random.default_rng(1)
    p = rng.random((2000, 3)).astype(np.float32)
    v, a = oracle.voxel_downsample(p, p * 2, [0.25] * 3, [0, 0, 0])
    assert len(v) == 64 and np.allclose(a, v * 2, rtol=1e-6)
    key = np.floor(p / np.float32(0.25)).astype(int)
    m = np.all(key == 0, axis=1)
    assert np.allclose(v[0], p[m].mean(0), rtol=1e-5)
    x = np.concatenate([p[:100], p[:100]])
    u, svi, svj = oracle.deduplicate_point_cloud(x, 1e-7)
    assert len(u) == 100 and np.array_equal(x[svi], u) and np.array_equal(u[svj], x) and np.all(svi < 100)
    assert np.array_equal(oracle.deduplicate_point_cloud(np.array([[0.5, 1.5, -0.5], [2.5, -1.5, 0.49999997]], np.float32), 1.0)[0],
                          np.array([[0.5, 1.5, -0.5], [2.5, -1.5, 0.49999997]], np.float32)[[0, 1]])


def test_oracle_voxel_downsample_fast_pinned_to_dict_restatement():
    """oracle.voxel_downsample_fast (lexsort + np.add.at, for the size sweeps of tests/test_gpu_voxel_edges.py) is bit-equal to the
    dict restatement of the reference loop: both point dtypes with the other dtype's attributes, signed coordinates, anisotropic
    voxels, min_points_per_voxel, one voxel holding every point, an empty result."""
    rng = np.random.default_rng(11)

    def same(p, a, vs, mb, mp=1):
        v0, a0 = oracle.voxel_downsample(p, a, vs, mb, mp)
        v1, a1 = oracle.voxel_downsample_fast(p, a, vs, mb, mp)
        assert v1.dtype == v0.dtype and v1.shape == v0.shape and np.array_equal(v0, v1)
        if a is None:
            assert a0 is None and a1 is None
        else:
            assert a1.dtype == a0.dtype and a1.shape == a0.shape and np.array_equal(a0, a1)
        return len(v0)

    for dt, adt in ((np.float32, np.float64), (np.float64, np.float32)):
        p = ((rng.random((30000, 3)) - 0.5) * 3).astype(dt)                      # signed: negative voxel indices on every axis
        a = rng.normal(size=(30000, 2)).astype(adt)
        assert same(p, a, [0.125] * 3, [-0.4, 0.1, -1.0]) > 5000
        assert same(p, a, (0.3, 0.07, 0.9), [-1.6, -1.6, -1.6]) > 500           # anisotropic
        assert 0 < same(p, a, [0.125] * 3, [-1.5] * 3, 3) < same(p, a, [0.125] * 3, [-1.5] * 3, 1)
        assert same(p, None, [0.25] * 3, [-1.5] * 3, 0) == same(p, None, [0.25] * 3, [-1.5] * 3, -4)
        assert same(p, a, [10.0] * 3, [-2.0] * 3) == 1                           # one voxel holds all 30 000 points
        assert same(p, a, [0.25] * 3, [-1.5] * 3, 10 ** 6) == 0                  # nothing kept: (0, 3) and (0, 2)
        assert same(p[:1], a[:1], [0.25] * 3, [-1.5] * 3) == 1


def test_oracle_sinkhorn_pinned_to_reference_module_and_golden():
    """The numpy restatement of point_cloud_utils/_sinkhorn.py against tests/golden/sinkhorn.npz (generated from the reference's
    own module) and, where /root/reference exists, against that module itself on fresh inputs: bit-equal (same numpy calls)."""
    import os
    g = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "sinkhorn.npz"))
    for tag in ("f32", "f64"):
        a, b = g[f"a_{tag}"], g[f"b_{tag}"]
        for p in (None, 1, np.inf, 3):
            assert np.array_equal(oracle.pairwise_distances(a, b, p), g[f"M_{tag}_p{p}"])
        dt = a.dtype.type
        P, _ = oracle.sinkhorn(np.full(96, 1.0 / 96, dt), np.full(80, 1.0 / 80, dt), g[f"M_{tag}_pNone"], eps=1e-2, max_iters=60)
        assert np.array_equal(P, g[f"P_{tag}"])
        Pb, _ = oracle.sinkhorn(g[f"wab_{tag}"], g[f"wbb_{tag}"], g[f"Mb_{tag}"], eps=5e-2, max_iters=100, stop_thresh=1e-4)
        assert np.array_equal(Pb, g[f"Pb_{tag}"])
    emd, P = oracle.earth_movers_distance(g["emd_p"], g["emd_q"], eps=1e-2)
    assert emd == g["emd"] and np.array_equal(P, g["emd_P"])
    ref = oracle.reference_sinkhorn_module()
    if ref is not None:
        rng = np.random.default_rng(5)
        x = rng.random((2, 30, 4)).astype(np.float32); y = rng.random((2, 25, 4)).astype(np.float32)
        M = ref.pairwise_distances(x, y, 2)
        assert np.array_equal(M, oracle.pairwise_distances(x, y, 2))
        wa = np.full((2, 30), 1 / 30, np.float32); wb = np.full((2, 25), 1 / 25, np.float32)
        assert np.array_equal(ref.sinkhorn(wa, wb, M, 1e-2), oracle.sinkhorn(wa, wb, M, 1e-2)[0])


def test_config1_cpu():
    """BASELINE config 1 ("chamfer_distance on two 10k-point fp64 random clouds via reference nanoflann CPU path; plumbing, no GPU"):
    the reference's nanoflann (oracle/_ref, where built) and the restatement agree bit for bit on value and correspondences, and a
    golden scalar generated from the reference (tests/golden/make_golden.py) pins both."""
    x, y = cloud(1000, 10_000, np.float64), cloud(1001, 10_000, np.float64)
    ch, cxy, cyx = oracle.chamfer_distance(x, y, return_index=True, kind="port")
    g = np.load(os.path.join(GOLD, "config1.npz"))
    assert float(ch) == float(g["chamfer"]) and np.array_equal(cxy, g["cxy"]) and np.array_equal(cyx, g["cyx"])
    if oracle.have_ref():
        ch1, cxy1, cyx1 = oracle.chamfer_distance(x, y, return_index=True, kind="ref")
        assert float(ch1) == float(ch) and np.array_equal(cxy1, cxy) and np.array_equal(cyx1, cyx)


def test_oracle_norm_order_pinned_to_numpy():
    """oracle.vector_norm_numpy_order -- numpy's pairwise summation restated, the order k_pairwise follows -- equals
    np.linalg.norm(..., axis=-1) bit for bit for d = 1 .. 300 at every ord the kernel reproduces exactly (and at the general ords,
    whose powers it also takes as numpy does). If a numpy release changes its summation order, this says so before a GPU test does."""
    rng = np.random.default_rng(17)
    for dt in (np.float32, np.float64):
        for d in range(1, 301):
            x = (rng.standard_normal((3, 4, d)) * 10.0 ** rng.uniform(-3, 3, (3, 4, d))).astype(dt)
            x[0, 0, : d // 2] = 0                       # zero components: ord 0 counts, negative ords meet 0 ** ord = inf
            for o in (None, 2, 1, np.inf, -np.inf, 0, 3, 0.5, -1, 2.5):
                with np.errstate(divide="ignore"):
                    ref = np.linalg.norm(x, ord=o, axis=-1)
                    got = oracle.vector_norm_numpy_order(x, o)
                assert got.dtype == ref.dtype and got.tobytes() == ref.tobytes(), (dt, d, o)
    # the order matters: a left-to-right sum of squares is not numpy's 2-norm once d >= 8
    x = rng.standard_normal((500, 17)).astype(np.float32)
    seq = np.zeros(500, np.float32)
    for c in range(17):
        seq = seq + x[:, c] * x[:, c]
    assert not np.array_equal(np.sqrt(seq), np.linalg.norm(x, axis=-1))
    a, b = rng.random((2, 5, 9)), rng.random((2, 6, 9))
    assert oracle.pairwise_distances_numpy_order(a, b).tobytes() == oracle.pairwise_distances(a, b).tobytes()


# ---- normals: the inputs of tests/test_gpu_normals_fits.py and the rule that judges them, held to what they claim without a GPU -------------------
from oracle import normals_cases as nc

_KNN = nc.knn_cases()
_BALL = nc.ball_cases()


def _knn_kind():
    oracle.build()
    return "ref" if oracle.have_ref() else "port"


@pytest.mark.parametrize("dtype", nc.DTYPES, ids=["f32", "f64"])
@pytest.mark.parametrize("case", _KNN, ids=[c[0] for c in _KNN])
def test_normals_knn_cases_checker_passes_its_own_rule(case, dtype):
    """The checker's own SVD normal, rounded to the cloud's dtype, meets the residual contract on every fit of every _knn case, and the
    'separated' cases leave at most 10 % of their fits out of the direction comparison. With fewer than three neighbours there is no
    checker normal (V(:, 2) of a thin V): the smallest right singular vector of the zero-padded A is used, which is what the contract asks."""
    _, make, k, leaf, separated = case
    p = make(dtype)
    idx0, nrm0, gap, info = oracle.normals_knn(p, k, max_points_per_leaf=leaf, kind=_knn_kind(), fits=True)
    if k < 3:
        a = info["A"]
        nrm0 = np.linalg.svd(np.concatenate([a, np.zeros((len(a), 3 - k, 3))], 1))[2][:, 2, :]
    if case[0] == "k=n+1":
        assert len(idx0) == 0
    elif case[0] != "k=n":
        assert len(idx0) == len(p)
    else:
        assert len(idx0) == 300
    zero = np.flatnonzero(~np.any(info["A"] != 0, axis=(1, 2)))
    nrm0[zero] = (0.0, 0.0, 1.0)                   # no spread at all: the V = I answer
    if case[0] == "duplicates-k4" or case[0] == "duplicates-k8":
        assert len(zero) == len(p)                 # the tr == 0 early-out is all this case reaches
    if case[0] == "duplicates-k12":
        assert len(zero) == 0
    nc.judge(idx0, nc.unit(nrm0, dtype), idx0, info, dtype, separated=separated)


@pytest.mark.parametrize("dtype", nc.DTYPES, ids=["f32", "f64"])
def test_normals_rule_rejects_wrong_variants(dtype):
    """The residual contract fails (i) a neighbour swapped for the (k+1)-th, (iv) a Jacobi loop cut to two sweeps, and an index mix-up of the
    normals; modelled on the CPU: A^T A in neighbour order and the cyclic Jacobi of csrc/normals.h restated in numpy."""
    p = nc.sheet(2000, dtype)
    k = 12
    kind = _knn_kind()
    idx0, nrm0, gap, info = oracle.normals_knn(p, k, kind=kind, fits=True)
    _, c = oracle.knn(p, p, k + 1, True, kind=kind)
    swapped = c[:, list(range(k - 1)) + [k]]
    a_wrong = (p[swapped] - p[:, None, :]).astype(np.float64)
    n_wrong = np.linalg.svd(a_wrong)[2][:, 2, :]
    ok, _, _, _ = oracle.fit_excess(info["A"], nc.unit(n_wrong, dtype), dtype)
    assert (~ok).mean() > 0.9, (~ok).mean()
    with pytest.raises(AssertionError, match="residual contract"):
        nc.judge(idx0, nc.unit(n_wrong, dtype), idx0, info, dtype)

    def jacobi(S, sweeps):
        a = S / np.trace(S); v = np.eye(3)
        for _ in range(sweeps):
            for pi, qi in ((0, 1), (0, 2), (1, 2)):
                apq = a[pi, qi]
                if abs(apq) < 1e-300:
                    continue
                theta = (a[qi, qi] - a[pi, pi]) / (2.0 * apq)
                with np.errstate(over="ignore"):
                    t = (1.0 if theta >= 0 else -1.0) / (abs(theta) + np.sqrt(theta * theta + 1.0))
                cth = 1.0 / np.sqrt(t * t + 1.0); sth = t * cth
                J = np.eye(3); J[pi, pi] = cth; J[qi, qi] = cth; J[pi, qi] = sth; J[qi, pi] = -sth
                a = J.T @ a @ J; v = v @ J
        return v[:, int(np.argmin(np.diag(a)))]

    A = info["A"][:400]
    S = np.einsum("nki,nkj->nij", A, A)
    for sweeps, expect_fail in ((2, True), (8, False)):
        nj = nc.unit(np.stack([jacobi(s, sweeps) for s in S]), dtype)
        ok, _, _, _ = oracle.fit_excess(A, nj, dtype)
        assert (not ok.all()) == expect_fail, (sweeps, int((~ok).sum()))
    with pytest.raises(AssertionError, match="residual contract"):       # normals written at the wrong rows
        nc.judge(idx0, nc.unit(np.roll(nrm0, 1, axis=0), dtype), idx0, info, dtype)
    with pytest.raises(AssertionError, match="kept rows differ"):
        nc.judge(idx0[1:], nc.unit(nrm0[1:], dtype), idx0, info, dtype)


@pytest.mark.parametrize("dtype", nc.DTYPES, ids=["f32", "f64"])
@pytest.mark.parametrize("k", [4, 5])
def test_normals_lattice_tells_leaf_sizes_apart(dtype, k):
    """(v) max_points_per_leaf not forwarded: on the displaced lattice the leaf-33 answer breaks the contract against the leaf-1 matrices on at
    least 100 rows, while each answer passes against its own (test_normals_knn_cases_checker_passes_its_own_rule)."""
    p = nc.lattice(dtype, displaced=True)
    kind = _knn_kind()
    _, _, _, i1 = oracle.normals_knn(p, k, max_points_per_leaf=1, kind=kind, fits=True)
    _, n33, _, _ = oracle.normals_knn(p, k, max_points_per_leaf=33, kind=kind, fits=True)
    ok, _, _, _ = oracle.fit_excess(i1["A"], nc.unit(n33, dtype), dtype)
    assert (~ok).sum() >= 100, int((~ok).sum())


@pytest.mark.parametrize("dtype", nc.DTYPES, ids=["f32", "f64"])
def test_normals_scaling_case_is_exact(dtype):
    """The scaled clouds of the bit-identity case: scaling by 2^+-e is exact, no non-zero squared coordinate difference leaves the normal
    range, and the checker's own neighbour rows do not change."""
    p = nc.sheet_on_lattice(5000, dtype)
    e = nc.SCALE_EXP[dtype]
    tiny = np.finfo(dtype).tiny
    _, c0 = oracle.knn(p, p, 12, True, kind=_knn_kind())
    for sgn in (1, -1):
        q = (p * dtype(2.0) ** (sgn * e)).astype(dtype)
        assert np.array_equal(q.astype(np.longdouble), p.astype(np.longdouble) * np.longdouble(2.0) ** (sgn * e))
        for j in range(3):
            d = np.diff(np.sort(q[:, j])); d = d[d > 0]
            assert d.min() * d.min() >= tiny and np.isfinite((q[:, j].max() - q[:, j].min()) ** 2 * 3)
        _, c1 = oracle.knn(q, q, 12, True, kind=_knn_kind())
        assert np.array_equal(c0, c1)
    idx0, _, gap, _ = oracle.normals_knn(p, 12, kind=_knn_kind(), fits=True)
    assert nc.unseparated_share(gap) <= 0.10


@pytest.mark.parametrize("dtype", nc.DTYPES, ids=["f32", "f64"])
def test_normals_view_direction_cases(dtype):
    """Per-row view directions: at most 1e-3 of the rows lie within 1e-6 rad of a threshold (judged by the checker alone), every threshold keeps
    and drops rows of every kind the case claims, and an answer computed with the directions of the wrong rows is refused."""
    p = nc.sheet(3000, dtype)
    dirs = nc.view_directions(len(p), dtype)
    for thr in nc.THRESHOLDS:
        idx0, nrm0, gap, info = oracle.normals_knn(p, 12, view_directions=dirs, drop_angle_threshold=thr, kind=_knn_kind(), fits=True)
        assert nc.ambiguous_share(info, thr, dirs) <= 1e-3
        kept0 = np.isin(np.arange(0, len(p), 50), idx0)                       # zero directions: angle pi / 2
        assert kept0.all() if thr == np.pi / 2 else not kept0.any()
        assert np.isin(np.arange(2, len(p), 50), idx0).any()                  # length 2: cosines above 1 are kept
        if thr > 0:
            assert 0.05 < len(idx0) / len(p)
        nc.judge(idx0, nc.unit(nrm0, dtype), idx0, info, dtype, dirs=dirs, thr=thr, separated=True)
    thr = nc.THRESHOLDS[1]
    idx0, nrm0, gap, info = oracle.normals_knn(p, 12, view_directions=dirs, drop_angle_threshold=thr, kind=_knn_kind(), fits=True)
    idx1, nrm1, _ = oracle.normals_knn(p, 12, view_directions=np.roll(dirs, 1, axis=0), drop_angle_threshold=thr, kind=_knn_kind())     # (iii) dirs[t] for dirs[q.idx]
    with pytest.raises(AssertionError):
        nc.judge(idx1, nc.unit(nrm1, dtype), idx0, info, dtype, dirs=dirs, thr=thr, separated=True)


@pytest.mark.parametrize("dtype", nc.DTYPES, ids=["f32", "f64"])
def test_normals_ball_lattice_membership(dtype):
    """Strict d2 < radius and count >= min_pts on the 12^3 lattice, ball_radius 4.0: the members of an inner point are its 3 x 3 x 3 block (27; the six
    points at distance 2 are out), so 10^3 rows are kept at min_pts 27 and none at 28; (ii) `<=` would count 33 and keep rows at 28, (vi) `>` for `>=` none at 27.
    The next radius above 4 in the cloud's dtype admits the six."""
    p = nc.lattice(dtype, g=12)
    inner = np.flatnonzero(np.all((p >= 1) & (p <= 10), axis=1))
    idx27, _, _, info = oracle.normals_ball(p, 4.0, min_pts_per_ball=27, fits=True)
    assert np.array_equal(idx27, inner) and len(inner) == 1000
    assert max(len(a) for a in info["A"]) == 27
    assert len(oracle.normals_ball(p, 4.0, min_pts_per_ball=28)[0]) == 0
    up = float(np.nextafter(dtype(4), dtype(5)))
    assert dtype(up) > dtype(4)
    idx33, _, _, info = oracle.normals_ball(p, up, min_pts_per_ball=28, fits=True)
    deep = np.flatnonzero(np.all((p >= 2) & (p <= 9), axis=1))
    assert np.isin(deep, idx33).all() and max(len(a) for a in info["A"]) == 33
    d2 = ((p[inner[0]] - p) ** 2).sum(1)
    assert (d2 <= 4).sum() == 33 and (d2 < 4).sum() == 27 and (d2 < 3).sum() == 19
    assert len(oracle.normals_ball(p, 3.0, min_pts_per_ball=19)[0]) == 1000 and len(oracle.normals_ball(p, 3.0, min_pts_per_ball=20)[0]) == 0
    flat = nc.lattice(dtype, g=12, flat=True)
    idx9, n9, _ = oracle.normals_ball(flat, 4.0, min_pts_per_ball=9)
    assert len(idx9) == 100 and len(oracle.normals_ball(flat, 4.0, min_pts_per_ball=10)[0]) == 0
    assert np.array_equal(np.abs(n9), np.tile([0.0, 0.0, 1.0], (100, 1)))


# (the large sampled cloud once on this side -- float32, constant --; the GPU test runs every combination)
_BALL_RUNS = [(c, w, t) for c in _BALL for w in ("constant", "rbf") for t in nc.DTYPES if not c[5] or (w == "constant" and t == np.float32)]


@pytest.mark.parametrize("case,weight,dtype", _BALL_RUNS, ids=["%s-%s-%s" % (c[0], w, "f32" if t == np.float32 else "f64") for c, w, t in _BALL_RUNS])
def test_normals_ball_cases_checker_passes_its_own_rule(case, weight, dtype):
    """As test_normals_knn_cases_checker_passes_its_own_rule, for the _ball table; and rows= gives what the full run gives on those rows."""
    name, make, radius, min_pts, separated, sample = case
    p = make(dtype)
    rows = nc.sample_rows(len(p), sample) if sample else None
    idx0, nrm0, gap, info = oracle.normals_ball(p, radius, min_pts_per_ball=min_pts, weight_function=weight, rows=rows, fits=True)
    assert len(idx0) > 0
    if name == "identical":
        assert len(idx0) == 50
        nrm0[:] = (0.0, 0.0, 1.0)
    if name == "sees-all":
        assert all(len(a) == len(p) for a in info["A"])
    if name.endswith("outliers") or name == "one-outlier":
        assert idx0.max() < 1200 and len(idx0) > 1150              # the far points are dropped
    nc.judge(idx0, nc.unit(nrm0, dtype), idx0, info, dtype, separated=separated)
    if sample:                                                     # rows= equals the full run on those rows (a smaller cloud: the full run is the cost)
        q = nc.sheet(1500, dtype, 5)
        r = nc.sample_rows(len(q), 200)
        full = oracle.normals_ball(q, 0.02, min_pts_per_ball=5, weight_function=weight)
        part = oracle.normals_ball(q, 0.02, min_pts_per_ball=5, weight_function=weight, rows=r)
        pick = np.isin(full[0], r)
        assert np.array_equal(part[0], full[0][pick]) and np.array_equal(part[1], full[1][pick]) and np.array_equal(part[2], full[2][pick])
