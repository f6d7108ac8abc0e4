"""downsample_point_cloud_poisson_disk on the GPU (-m gpu), against a serial restatement of the contract (csrc/poisson.h, DESIGN.md
"Poisson-disk downsampling"): visit the rows by ascending splitmix64 priority, take a row iff no row taken so far is close to it, close
meaning d2 < r * r with d2 = ((dx*dx)+(dy*dy))+(dz*dz) evaluated in the input type. Candidates come from scipy's cKDTree at a slightly
larger radius; the exact test is then made in the input type."""
import threading
import time

import numpy as np
import pytest

from conftest import cloud, mesh_samples, ROOT

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def pcu():
    import point_cloud_utils_amd as m
    from point_cloud_utils_amd import _lib
    assert _lib.device_count() > 0, "no GPU visible: the gfx950 path has no CPU fallback"
    return m


# ------------------------------------------------------------------------------------------------ restatement of the contract
def priority(n, seed):
    z = (np.uint64(seed) << np.uint64(32)) ^ np.arange(n, dtype=np.uint64)
    z ^= z >> np.uint64(30); z *= np.uint64(0xBF58476D1CE4E5B9)
    z ^= z >> np.uint64(27); z *= np.uint64(0x94D049BB133111EB)
    z ^= z >> np.uint64(31)
    return z


def d2_exact(v, i, j):
    d = v[i] - v[j]                                   # in the input type
    return (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]


def greedy(v, r, seed, tree=None):
    """The serial greedy of the contract: sorted row indices (int32)."""
    from scipy.spatial import cKDTree
    T = v.dtype.type
    rT = T(r)
    r2 = rT * rT
    n = len(v)
    tree = tree if tree is not None else cKDTree(v.astype(np.float64))
    rq = float(rT) * (1 + 1e-5) if np.isfinite(rT) else np.inf
    order = np.argsort(priority(n, seed), kind="stable")
    blocked = np.zeros(n, dtype=bool)
    taken = []
    for i in order:
        if blocked[i]:
            continue
        taken.append(i)
        if np.isinf(rq):
            blocked[:] = True
            continue
        cand = np.asarray(tree.query_ball_point(v[i].astype(np.float64), rq), dtype=np.int64)
        if cand.size:
            blocked[cand[d2_exact(v, cand, np.full(cand.shape, i)) < r2]] = True
    return np.sort(np.asarray(taken, dtype=np.int32))


def greedy_target(v, target, seed, tol=0.04):
    """The reference's radius search (src/sample_point_cloud.cpp:281-329) driving the restated greedy, in the input type."""
    from scipy.spatial import cKDTree
    T = v.dtype.type
    tree = cKDTree(v.astype(np.float64))
    tolf = np.float32(tol)
    nmin = int(T(target) * T(np.float32(1.0) - tolf))
    nmax = int(T(target) * T(np.float32(1.0) + tolf))
    e = v.max(axis=0) - v.min(axis=0)
    bb = np.sqrt((e[0] * e[0] + e[1] * e[1]) + e[2] * e[2])
    rmin = T(float(bb) / 50.0); rmax = rmin
    while True:
        rmin = T(float(rmin) / 2.0)
        s = greedy(v, rmin, seed, tree)
        if len(s) >= target:
            break
    while True:
        rmax = T(float(rmax) * 2.0)
        s = greedy(v, rmax, seed, tree)
        if len(s) <= target:
            break
    it = 0
    while it < 20 and (len(s) < nmin or len(s) > nmax):
        it += 1
        cur = T(float(T(rmin + rmax)) / 2.0)
        s = greedy(v, cur, seed, tree)
        if len(s) > target:
            rmin = cur
        if len(s) < target:
            rmax = cur
    return s


def check_properties(v, idx, r):
    """No two samples are close; every row is a sample or close to one."""
    from scipy.spatial import cKDTree
    T = v.dtype.type
    rT = T(r); r2 = rT * rT
    s = v[idx]
    pairs = cKDTree(s.astype(np.float64)).query_pairs(float(rT) * (1 + 1e-5), output_type="ndarray")
    if len(pairs):
        assert not np.any(d2_exact(s, pairs[:, 0], pairs[:, 1]) < r2), "two samples are close"
    _, nn = cKDTree(s.astype(np.float64)).query(v.astype(np.float64), k=min(4, len(s)))
    nn = nn.reshape(len(v), -1)
    d = (v[:, None, :] - s[nn])
    d2 = (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]
    assert np.all(np.any(d2 < r2, axis=1)), "a row is neither a sample nor close to one"


def bunny_dense(n, dtype):
    v = np.load(f"{ROOT}/tests/golden/bunny_v.npy").astype(np.float64)
    f = np.load(f"{ROOT}/tests/golden/bunny_f.npy")
    return np.ascontiguousarray(mesh_samples(v, f, n).astype(dtype))


def clustered(n, dtype, seed=11):
    rng = np.random.default_rng(seed)
    centres = rng.random((20, 3))
    a = centres[rng.integers(0, 20, n)] + 0.01 * rng.standard_normal((n, 3))
    return np.ascontiguousarray(a.astype(dtype))


# ------------------------------------------------------------------------------------------------ 1. exact equality
DTYPES = [np.float32, np.float64]


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("r", [0.01, 0.025, 0.05, 0.12])
def test_uniform_equals_restatement(pcu, dtype, r):
    v = cloud(101, 50_000, dtype)
    got = pcu.downsample_point_cloud_poisson_disk(v, r, random_seed=12345)
    assert got.dtype == np.int32
    assert np.array_equal(got, greedy(v, r, 12345))


@pytest.mark.parametrize("dtype", DTYPES)
def test_radius_below_spacing_returns_every_row(pcu, dtype):
    v = cloud(102, 50_000, dtype)
    got = pcu.downsample_point_cloud_poisson_disk(v, 1e-7, random_seed=7)
    assert np.array_equal(got, greedy(v, 1e-7, 7))
    assert np.array_equal(got, np.arange(len(v), dtype=np.int32))


@pytest.mark.parametrize("dtype", DTYPES)
def test_radius_above_diagonal_returns_the_first_row(pcu, dtype):
    v = cloud(103, 50_000, dtype)
    for r in (2.0, 2.0 * len(v)):
        got = pcu.downsample_point_cloud_poisson_disk(v, r, random_seed=99)
        assert np.array_equal(got, np.array([np.argmin(priority(len(v), 99))], dtype=np.int32))


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("r", [0.002, 0.01])
def test_clustered_equals_restatement(pcu, dtype, r):
    v = clustered(50_000, dtype)
    got = pcu.downsample_point_cloud_poisson_disk(v, r, random_seed=4242)
    rounds = pcu.last_stats()["n_passes"]
    print(f"clustered {np.dtype(dtype).name} r={r}: {len(got)} samples, {rounds} rounds")
    assert np.array_equal(got, greedy(v, r, 4242))


@pytest.mark.parametrize("dtype", DTYPES)
def test_duplicates_equal_restatement(pcu, dtype):
    base = cloud(104, 10_000, dtype)
    v = np.ascontiguousarray(np.concatenate([base, base[::3], base[::7], base[:50]]))
    for r in (1e-6, 0.03):
        got = pcu.downsample_point_cloud_poisson_disk(v, r, random_seed=31337)
        assert np.array_equal(got, greedy(v, r, 31337))


@pytest.mark.parametrize("dtype", DTYPES)
def test_dense_bunny_equals_restatement(pcu, dtype):
    v = bunny_dense(50_000, dtype)
    diag = float(np.linalg.norm(v.max(0).astype(np.float64) - v.min(0)))
    for frac in (0.004, 0.02):
        got = pcu.downsample_point_cloud_poisson_disk(v, frac * diag, random_seed=1234567)
        assert np.array_equal(got, greedy(v, frac * diag, 1234567))


# ------------------------------------------------------------------------------------------------ 2. properties at 1M points
@pytest.mark.parametrize("dtype", DTYPES)
def test_properties_at_one_million_points(pcu, dtype):
    v = cloud(105, 1_000_000, dtype)
    for r in (0.01, 0.03):
        idx = pcu.downsample_point_cloud_poisson_disk(v, r, random_seed=2024)
        print(f"1M {np.dtype(dtype).name} r={r}: {len(idx)} samples, {pcu.last_stats()['n_passes']} rounds")
        assert np.all(np.diff(idx) > 0)
        check_properties(v, idx, r)


# ------------------------------------------------------------------------------------------------ 3. the reference's own test body
def test_reference_test_body(pcu):
    v = np.load(f"{ROOT}/tests/golden/bunny_v.npy").astype(np.float64)
    f = np.load(f"{ROOT}/tests/golden/bunny_f.npy")
    bbox_diag = np.linalg.norm(v.max(0) - v.min(0))
    v_dense = bunny_dense(v.shape[0] * 4, np.float64)

    s_idx = pcu.downsample_point_cloud_poisson_disk(v_dense, 0.1 * bbox_diag, random_seed=1234567)
    s_idx2 = pcu.downsample_point_cloud_poisson_disk(v_dense, 0.1 * bbox_diag, random_seed=1234567)
    s_idx3 = pcu.downsample_point_cloud_poisson_disk(v_dense, 0.1 * bbox_diag, random_seed=7654321)
    assert np.all(s_idx == s_idx2)
    if s_idx3.shape == s_idx.shape:
        assert not np.all(s_idx == s_idx3)
    else:
        assert not s_idx.shape == s_idx3.shape

    s_idx_0 = pcu.downsample_point_cloud_poisson_disk(v_dense, 2 * v_dense.shape[0], random_seed=1234567)
    assert len(s_idx_0) == 1

    s_idx = pcu.downsample_point_cloud_poisson_disk(v_dense, 0., target_num_samples=1000, random_seed=1234567)
    s_idx2 = pcu.downsample_point_cloud_poisson_disk(v_dense, 0., target_num_samples=1000, random_seed=1234567)
    s_idx3 = pcu.downsample_point_cloud_poisson_disk(v_dense, 0., target_num_samples=1000, random_seed=7654321)
    assert np.all(s_idx == s_idx2)
    if s_idx3.shape == s_idx.shape:
        assert not np.all(s_idx == s_idx3)
    else:
        assert not s_idx.shape == s_idx3.shape


# ------------------------------------------------------------------------------------------------ 4. target mode
@pytest.mark.parametrize("dtype", DTYPES)
def test_target_mode_equals_restated_schedule(pcu, dtype):
    v = cloud(106, 20_000, dtype)
    for target in (500, 3000):
        got = pcu.downsample_point_cloud_poisson_disk(v, 0.0, target_num_samples=target, random_seed=555)
        assert np.array_equal(got, greedy_target(v, target, 555))


@pytest.mark.parametrize("dtype", DTYPES)
def test_target_mode_at_one_million_points(pcu, dtype):
    v = cloud(107, 1_000_000, dtype)
    for target in (1_000, 10_000, 100_000):
        got = pcu.downsample_point_cloud_poisson_disk(v, 0.0, target_num_samples=target, random_seed=77)
        st = pcu.last_stats()
        print(f"target {target} {np.dtype(dtype).name}: {len(got)} samples, {st['n_grid_builds']} radii, {st['n_passes']} rounds")
        assert int(target * 0.96) <= len(got) <= int(target * 1.04)
        assert np.all(np.diff(got) > 0)


def test_target_at_least_n_returns_every_row(pcu):
    v = cloud(108, 1000, np.float32)
    for target in (1000, 5000):
        got = pcu.downsample_point_cloud_poisson_disk(v, 0.0, target_num_samples=target)
        assert got.dtype == np.int32 and np.array_equal(got, np.arange(1000, dtype=np.int32))


def test_all_rows_equal(pcu):
    v = np.full((5000, 3), 0.25, dtype=np.float32)
    got = pcu.downsample_point_cloud_poisson_disk(v, 0.0, target_num_samples=10, random_seed=8)
    assert np.array_equal(got, np.array([np.argmin(priority(5000, 8))], dtype=np.int32))
    got = pcu.downsample_point_cloud_poisson_disk(v, 0.1, random_seed=8)
    assert np.array_equal(got, np.array([np.argmin(priority(5000, 8))], dtype=np.int32))


# ------------------------------------------------------------------------------------------------ 5. torch
@pytest.mark.parametrize("dtype", DTYPES)
def test_torch_input_equals_numpy(pcu, dtype):
    import torch
    v = cloud(109, 200_000, dtype)
    t = torch.from_numpy(v).cuda()
    for kw in (dict(radius=0.02), dict(radius=0.0, target_num_samples=5000)):
        a = pcu.downsample_point_cloud_poisson_disk(v, random_seed=9, **kw)
        b = pcu.downsample_point_cloud_poisson_disk(t, random_seed=9, **kw)
        assert b.dtype == torch.int32 and b.device == t.device
        assert np.array_equal(a, b.cpu().numpy())


# ------------------------------------------------------------------------------------------------ 6. cancellation
def test_cancel_from_another_thread(pcu):
    v = cloud(110, 4_000_000, np.float32)
    started, done = threading.Event(), threading.Event()

    def canceller():
        started.wait()
        for _ in range(500):            # keep asking until the main thread has left its loop (a request made between two calls is dropped)
            time.sleep(0.02)
            pcu.cancel()
            if done.is_set():
                break
    th = threading.Thread(target=canceller); th.start()
    t0 = time.perf_counter()
    try:
        with pytest.raises(KeyboardInterrupt):
            started.set()
            for _ in range(500):
                pcu.downsample_point_cloud_poisson_disk(v, 0.0, target_num_samples=20_000, random_seed=5)
    finally:
        done.set(); th.join()
    assert time.perf_counter() - t0 < 60.0
    w = cloud(111, 20_000, np.float64)
    assert np.array_equal(pcu.downsample_point_cloud_poisson_disk(w, 0.03, random_seed=6), greedy(w, 0.03, 6))


# ------------------------------------------------------------------------------------------------ 7. seeds
def test_seeds(pcu):
    v = cloud(112, 30_000, np.float32)
    a = pcu.downsample_point_cloud_poisson_disk(v, 0.04, random_seed=1)
    b = pcu.downsample_point_cloud_poisson_disk(v, 0.04, random_seed=1)
    c = pcu.downsample_point_cloud_poisson_disk(v, 0.04, random_seed=2)
    assert np.array_equal(a, b) and not (a.shape == c.shape and np.array_equal(a, c))
    for _ in range(2):
        z = pcu.downsample_point_cloud_poisson_disk(v, 0.04)            # random_seed=0: a seed from the clock
        check_properties(v, z, 0.04)
