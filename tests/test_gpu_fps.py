"""downsample_point_cloud_farthest_point on the GPU (-m gpu): idx and dists byte-equal to tests/fps_contract.py in every case, on both kernel
paths wherever a path admits the cloud. The shapes come from the library's own geometry (pcu_hip_fps_geometry): L the one-block row limit
(float32; float64 holds half), B the bucket size, G the blocks of an iteration launch, C the iterations per graph replay. A reference is
computed once per (cloud, start) at the largest size asked for; shorter results are its prefixes (the prefix property is
tests/test_fps_contract.py's)."""
import functools

import numpy as np
import pytest

import fps_contract as fc

pytestmark = pytest.mark.gpu
DTYPES = [np.float32, np.float64]


@pytest.fixture(scope="module")
def pcu():
    import point_cloud_utils_amd as m
    from point_cloud_utils_amd import _lib
    assert _lib.device_count() > 0, "no GPU visible: the gfx950 path has no CPU fallback"
    assert callable(m.downsample_point_cloud_farthest_point)
    return m


def geometry():
    from point_cloud_utils_amd import _fps
    return _fps._geometry()


def block_limit(dtype):
    return geometry()[0] // (np.dtype(dtype).itemsize // 4)


def paths(n, dtype):
    return (["block"] if n <= block_limit(dtype) else []) + ["grid"]


CLOUDS = {}


def lattice(k, dtype, seed):
    g = np.arange(k, dtype=dtype)
    p = np.stack(np.meshgrid(g, g, g, indexing="ij"), -1).reshape(-1, 3)
    return np.ascontiguousarray(p[np.random.default_rng(seed).permutation(len(p))])        # shuffled: the cell order is not the row order


def make(name, dtype):
    """The named inputs, made once per dtype."""
    key = (name, np.dtype(dtype).name)
    if key in CLOUDS:
        return CLOUDS[key]
    rng = np.random.default_rng(sum(map(ord, name)))
    T = dtype
    if name.startswith("uniform"):
        p = rng.random((int(name[7:]), 3)).astype(T)
    elif name == "lattice9":
        p = lattice(9, T, 1)
    elif name == "lattice17":
        p = lattice(17, T, 2)
    elif name == "twice":
        a = rng.random((600, 3)).astype(T); p = np.concatenate([a, a])
    elif name == "identical":
        p = np.broadcast_to(rng.random((1, 3)).astype(T), (1000, 3)).copy()
    elif name == "collinear":
        t = rng.random(3000).astype(T); p = np.stack([t, t * T(0.5), t * T(0.25)], 1)
    elif name == "coplanar":
        p = rng.random((3000, 3)).astype(T); p[:, 2] = T(0.375)
    elif name == "offset":
        p = (rng.random((5000, 3)).astype(T) + T(1e6)).astype(T)
    elif name == "clusters":
        p = (rng.random((70001, 3)) * 1e-3).astype(T); p[35000:] += T(100.0)
    elif name == "huge":                                                          # float32: d2 overflows to +inf for nearly every pair
        p = (rng.integers(-50, 50, (3000, 3)).astype(T) * T(1e20)).astype(T)
    else:
        raise KeyError(name)
    p = np.ascontiguousarray(p, dtype=T); p.setflags(write=False)
    CLOUDS[key] = p
    return p


@functools.lru_cache(maxsize=None)
def reference(name, dtype_name, n, start, m):
    p = make(name, np.dtype(dtype_name).type)[:n]
    idx, d2 = fc.farthest_point_sample(p, m, start, squared_distances=True)
    return idx, d2, np.sqrt(d2)


def same(got, want_idx, want_d):
    idx, d = got
    assert idx.dtype == np.int64 and idx.shape == want_idx.shape and np.array_equal(idx, want_idx), np.flatnonzero(idx != want_idx)[:5]
    assert d.dtype == want_d.dtype and d.tobytes() == want_d.tobytes(), np.flatnonzero(d != want_d)[:5]


def check(name, dtype, n, start, m, m_ref=None, squared=False):
    """Both paths (where admitted) at (n, start, m) against the reference computed at m_ref >= m."""
    from point_cloud_utils_amd import _fps
    p = make(name, dtype)[:n]
    idx, d2, d = reference(name, np.dtype(dtype).name, n, start, m_ref or m)
    for path in paths(n, dtype):
        got = _fps._forced(p, m, start, path=path, squared_distances=squared)
        same(got[:2], idx[:m], (d2 if squared else d)[:m])


def shape_sets():
    L, B, G, C = geometry()
    ns = [1, 2, 63, 64, 65, B - 1, B, B + 1, L - 1, L, L + 1, B * G - 1, B * G + 1, 70001]
    ms = [1, 2, C - 1, C, C + 1, 2 * C + 1]
    return ns, ms


@pytest.mark.parametrize("dtype", DTYPES)
def test_every_shape_on_both_paths(pcu, dtype):
    ns, ms = shape_sets()
    for n in ns:
        top = min(n, 300)
        for m in sorted({m for m in ms if m <= n} | {top}):
            check("uniform70001", dtype, n, 0, m, m_ref=top)
        for start in {n - 1, n // 2} - {0}:                                       # the last row and one in the middle
            check("uniform70001", dtype, n, start, min(n, 65))
    f64_limit = block_limit(np.float64)                                           # the one-block limit of float64 is a threshold of its own
    for n in (f64_limit - 1, f64_limit, f64_limit + 1):
        check("uniform70001", dtype, n, 3, min(n, 65))


@pytest.mark.parametrize("dtype", DTYPES)
def test_every_row_is_taken_once(pcu, dtype):
    L, B, G, C = geometry()
    for n in (1, 2, 63, 64, 65, B - 1, B, B + 1, 4097):
        check("uniform70001", dtype, n, n // 3, n)
        assert sorted(reference("uniform70001", np.dtype(dtype).name, n, n // 3, n)[0].tolist()) == list(range(n))


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name, m", [("lattice9", 729), ("lattice17", 300), ("twice", 1200), ("identical", 1000), ("collinear", 300),
                                     ("coplanar", 300), ("offset", 300)])
def test_inputs_where_ties_and_rounding_decide(pcu, dtype, name, m):
    n = len(make(name, dtype))
    check(name, dtype, n, 0, m)
    check(name, dtype, n, n - 1, min(m, 65), squared=True)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("e", [-20, 30])
def test_power_of_two_scalings_change_nothing_but_the_scale(pcu, dtype, e):
    from point_cloud_utils_amd import _fps
    p = make("uniform5000", dtype)
    q = (p * dtype(2.0 ** e)).astype(dtype)
    idx, d2 = fc.farthest_point_sample(q, 200, 7, squared_distances=True)
    base = reference("uniform5000", np.dtype(dtype).name, 5000, 7, 200)
    assert np.array_equal(idx, base[0]) and np.array_equal(d2[1:], base[1][1:] * dtype(4.0 ** e))
    for path in paths(5000, dtype):
        same(_fps._forced(q, 200, 7, path=path, squared_distances=True)[:2], idx, d2)
        same(_fps._forced(q, 200, 7, path=path)[:2], idx, np.sqrt(d2))


@pytest.mark.parametrize("dtype", DTYPES)
def test_two_tight_clusters_far_apart(pcu, dtype):
    """Most buckets are skipped -- the counters say so -- and the answer is the contract's."""
    from point_cloud_utils_amd import _fps
    p = make("clusters", dtype)
    idx, d2, d = reference("clusters", np.dtype(dtype).name, len(p), 11, 100)
    got = _fps._forced(p, 100, 11, path="grid")
    same(got[:2], idx, d)
    tests, updates = (int(x) for x in got[2])
    nb = -(-len(p) // geometry()[1])
    assert tests == 99 * nb and nb <= updates < tests, (tests, updates, nb)     # (the last sample updates nothing; the first pass touches every bucket)


def test_distances_that_overflow(pcu):
    p = make("huge", np.float32)
    assert np.isinf(reference("huge", "float32", 3000, 5, 100)[1]).sum() > 90
    check("huge", np.float32, 3000, 5, 100)
    check("huge", np.float32, 3000, 2999, 33, squared=True)


@pytest.mark.parametrize("dtype", DTYPES)
def test_call_forms(pcu, dtype):
    import torch
    for n, m in ((3000, 100), (40000, 70)):                                       # the one-block path and the grid path, chosen by the library
        p = make("uniform70001", dtype)[:n]
        idx, d2, d = reference("uniform70001", np.dtype(dtype).name, n, 9, m)
        tp = torch.from_numpy(p.copy()).cuda()
        for a in (p, tp):
            got = pcu.downsample_point_cloud_farthest_point(a, m, 9)
            assert (isinstance(got, torch.Tensor) and got.is_cuda and got.dtype == torch.int64) if a is tp else isinstance(got, np.ndarray)
            assert np.array_equal(got.cpu().numpy() if a is tp else got, idx)
            for squared in (False, True):
                gi, gd = pcu.downsample_point_cloud_farthest_point(a, m, start_index=9, return_distances=True, squared_distances=squared)
                if a is tp:
                    assert gi.device == tp.device and gd.device == tp.device and gd.dtype == tp.dtype
                    gi, gd = gi.cpu().numpy(), gd.cpu().numpy()
                same((gi, gd), idx, d2 if squared else d)
            only = pcu.downsample_point_cloud_farthest_point(a, m, 9, False, True)       # squared_distances without distances: the rows alone
            assert np.array_equal(only.cpu().numpy() if a is tp else only, idx)
        assert pcu.last_stats()["n_queries"] == n


@pytest.mark.parametrize("k_hint", [1, 16])
@pytest.mark.parametrize("dtype", DTYPES)
def test_dataset_index_returns_the_free_functions_bytes(pcu, dtype, k_hint):
    import torch
    for n, m in ((3000, 100), (40000, 70)):
        p = make("uniform70001", dtype)[:n]
        idx, d2, d = reference("uniform70001", np.dtype(dtype).name, n, 9, m)
        with pcu.DatasetIndex(p, k_hint=k_hint) as ix:
            same(ix.farthest_point_sample(m, 9, return_distances=True), idx, d)
            same(ix.farthest_point_sample(m, start_index=9, return_distances=True, squared_distances=True), idx, d2)
            assert np.array_equal(ix.farthest_point_sample(m, 9), idx)
            assert np.array_equal(ix.k_nearest_neighbors(p[:10], 1)[1], np.arange(10))        # the index is as it was
        with pcu.DatasetIndex(torch.from_numpy(p.copy()).cuda(), k_hint=k_hint) as ix:
            gi, gd = ix.farthest_point_sample(m, 9, return_distances=True)
            assert gi.is_cuda and gd.is_cuda
            same((gi.cpu().numpy(), gd.cpu().numpy()), idx, d)


def test_consecutive_calls_and_a_call_after_a_refusal(pcu):
    """One context: sizes that change the bucket layout and the number of replays from call to call (the cached graph, the ping-pong
    partials), both dtypes interleaved, and a refused call in between."""
    for dtype, n, m in ((np.float32, 70001, 65), (np.float32, 20000, 300), (np.float64, 70001, 33), (np.float32, 70001, 2), (np.float64, 9000, 300)):
        check("uniform70001", dtype, n, 0, m, m_ref=min(n, 300))
    import torch
    bad = torch.from_numpy(make("uniform70001", np.float32)[:30000].copy()).cuda()
    with pytest.raises(ValueError, match="Invalid num_samples"):
        pcu.downsample_point_cloud_farthest_point(bad, 30001)
    bad[12345, 1] = float("inf")
    with pytest.raises(ValueError, match="points must not contain NaN or infinite coordinates"):
        pcu.downsample_point_cloud_farthest_point(bad, 10)
    check("uniform70001", np.float32, 70001, 0, 300)
    check("uniform70001", np.float64, 3000, 0, 300)


def test_the_library_refuses_non_finite_rows_itself(pcu):
    """Below the Python checks: the entry point finds NaN and infinities on the device, on both paths, and the context answers afterwards."""
    import ctypes
    from point_cloud_utils_amd import _lib
    from point_cloud_utils_amd._call import _Dev, _call
    for n, bad in ((2000, np.nan), (40000, np.inf)):
        p = make("uniform70001", np.float32)[:n].copy(); p[n // 2, 2] = bad
        d = _Dev(p, p)
        out = np.zeros(5, np.int64)
        with pytest.raises(ValueError, match="points must not contain NaN or infinite coordinates"):
            _call("fps", d, d.pa, n, 5, 0, out.ctypes.data, None, None)
    check("uniform70001", np.float32, 2000, 0, 65)
    assert _lib.lib().pcu_hip_fps_f32(_lib.ctx(), None, 10, 5, 0, None, None, None, 0, None, None) == _lib.ERR_INVALID
    assert ctypes.sizeof(_lib.Stats) == 64
