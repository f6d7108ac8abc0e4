"""radius_search / radius_count on the GPU (-m gpu) against tests/radius_contract.py: dtype, shape and bytes, no tolerance, float32 and
float64, numpy arrays and device tensors. The shapes are the smallest that reach each path of csrc/radius.h: partial and several waves of
queries, the staged and the per-lane walk, every sort tier on both sides of its boundary (rows of 16 | 17: four to a wave or not, 32 | 33: two
to a wave or not, 64 | 65: one or two members to a lane, 128 | 129: registers or LDS, 2048 | 2049: LDS or radix passes), empty rows, one
cell, a degenerate grid."""
import itertools
import threading
import time

import numpy as np
import pytest

import radius_contract as rc

pytestmark = pytest.mark.gpu

DTYPES = [np.float32, np.float64]


@pytest.fixture(scope="module")
def pcu():
    import point_cloud_utils_amd as m
    from point_cloud_utils_amd import _lib
    assert _lib.device_count() > 0, "no GPU visible: the gfx950 path has no CPU fallback"
    return m


def same(got, want):
    """dtype, shape and bytes of every array (tensors are brought to the host first)."""
    got = [g.cpu().numpy() if hasattr(g, "cpu") else g for g in got]
    assert len(got) == len(want)
    for g, w in zip(got, want):
        assert g.dtype == w.dtype and g.shape == w.shape, (g.dtype, g.shape, w.dtype, w.shape)
        assert g.tobytes() == w.tobytes(), (np.nonzero(g != w)[0][:8], g[:8], w[:8])


def check(pcu, q, p, radius, tensors=True):
    """Sorted rows, both kinds of distance, the counts, unsorted rows as sets and twice the same -- numpy, then tensors. Returns the contract's offsets."""
    want = rc.radius_search(q, p, radius)
    want2 = rc.radius_search(q, p, radius, squared_distances_out=True)
    counts = want[0][1:] - want[0][:-1]
    kinds = [(q, p)]
    if tensors:
        import torch
        tq = torch.from_numpy(q).cuda()
        kinds.append((tq, tq if p is q else torch.from_numpy(p).cuda()))
    for a, b in kinds:
        got = pcu.radius_search(a, b, radius)
        assert all(type(g) is type(a) for g in got)
        if hasattr(a, "device"):
            assert all(g.device == a.device for g in got)
        same(got, want)
        same(pcu.radius_search(a, b, radius, squared_distances=True), want2)
        same([pcu.radius_count(a, b, radius)], [counts])
        u1 = pcu.radius_search(a, b, radius, squared_distances=True, sort_results=False)
        u2 = pcu.radius_search(a, b, radius, squared_distances=True, sort_results=False)
        u1, u2 = ([g.cpu().numpy() if hasattr(g, "cpu") else g for g in u] for u in (u1, u2))
        same(u2, u1)                                                     # equal calls, equal bytes
        same(u1[:1], want[:1])
        seg = np.repeat(np.arange(len(q)), counts)
        order = np.lexsort((u1[1], u1[2], seg))                          # every row of the unsorted result, put in the contract's order
        same([u1[1][order], u1[2][order]], want2[1:])
    return want[0]


@pytest.mark.parametrize("dtype", DTYPES)
def test_small_sizes_around_a_wave(pcu, dtype):
    rng = np.random.default_rng(1)
    for n, m in itertools.product((1, 63, 64, 65, 257), repeat=2):
        q, p = rng.random((n, 3)).astype(dtype), rng.random((m, 3)).astype(dtype)
        off = check(pcu, q, p, 0.35, tensors=(n, m) in ((1, 1), (65, 257), (257, 63)))
        assert m < 60 or off[-1] > 0


@pytest.mark.parametrize("dtype", DTYPES)
def test_every_row_is_the_whole_dataset(pcu, dtype):
    p = np.random.default_rng(2).random((4097, 3)).astype(dtype)
    q = np.ascontiguousarray(p[:130])
    off = check(pcu, q, p, 4.0)
    assert np.array_equal(off, np.arange(131) * 4097)


TIERS = (0, 1, 2, 16, 17, 32, 33, 64, 65, 128, 129, 2048, 2049)


def clusters(dtype, tied, seed):
    """One cluster of L dataset points per L of TIERS, ten units apart, a query at each cluster's centre and radius 1: L copies of the centre
    (L tied members, ordered by row) or L points on a ray (L distinct distances); the dataset rows are shuffled. Plus far points."""
    rng = np.random.default_rng(seed)
    pts, q = [], []
    for c, L in enumerate(TIERS):
        centre = np.array([10.0 * c, 3.0, -2.0])
        q.append(centre)
        if tied:
            pts.append(np.repeat(centre[None], L, axis=0))
        else:
            pts.append(centre[None] + np.arange(1, L + 1)[:, None] * (0.9 / (L + 1)) * np.array([[0.6, 0.0, 0.8]]))
    pts.append(np.array([[1e3, 1e3, 1e3], [-500.0, 20.0, 7.0], [55.0, 60.0, 3.0]]))
    p = np.concatenate(pts).astype(dtype)
    return np.array(q, dtype=dtype), np.ascontiguousarray(p[rng.permutation(len(p))])


@pytest.mark.parametrize("tied", [True, False])
@pytest.mark.parametrize("dtype", DTYPES)
def test_row_lengths_on_both_sides_of_every_sort_tier(pcu, dtype, tied):
    q, p = clusters(dtype, tied, 3)
    off = check(pcu, q, p, 1.0)
    assert (off[1:] - off[:-1]).tolist() == list(TIERS)                  # the rows have the intended lengths
    # the same rows in another order of the queries (which four rows share a wave of the register tier), and next to copies of themselves
    order = np.random.default_rng(4).permutation(np.repeat(np.arange(len(q)), 3))
    off = check(pcu, np.ascontiguousarray(q[order]), p, 1.0, tensors=False)
    assert (off[1:] - off[:-1]).tolist() == [TIERS[i] for i in order]
    d = rc.radius_search(q, p, 1.0)[2]
    assert len(np.unique(d[-2049:])) == (1 if tied else 2049)            # the longest row: all tied, or distinct distances on the ray


@pytest.mark.parametrize("dtype", DTYPES)
def test_lattice_strict_boundary_and_ties_by_row(pcu, dtype):
    p = np.array(list(itertools.product(range(9), repeat=3)), dtype=dtype)
    p = np.ascontiguousarray(p[np.random.default_rng(5).permutation(len(p))])
    for radius in (1.0, np.sqrt(2.0), 2.0, 3.0):
        off = check(pcu, p, p, float(radius), tensors=radius == 2.0)
        exact = ((p[:, None, :].astype(np.int64) - p[None, :, :].astype(np.int64)) ** 2).sum(-1)
        r2 = float(rc.r2_of(radius, dtype))
        assert np.array_equal(off[1:] - off[:-1], (exact < r2).sum(1))
        if radius != np.sqrt(2.0):
            assert (exact == int(radius * radius)).sum() > 1000          # pairs at exactly the radius, all left out


@pytest.mark.parametrize("dtype", DTYPES)
def test_duplicates_query_is_dataset_and_one_cell(pcu, dtype):
    rng = np.random.default_rng(6)
    base = rng.random((300, 3)).astype(dtype)
    p = np.ascontiguousarray(np.repeat(base, 3, axis=0)[rng.permutation(900)])       # duplicated dataset rows
    check(pcu, base, p, 0.2)
    check(pcu, p, p, 0.15)                                                 # query is dataset
    one = np.ascontiguousarray(np.repeat(np.array([[0.25, -1.0, 8.0]], dtype=dtype), 700, axis=0))
    off = check(pcu, one[:70], one, 0.5)                                   # all points in one cell
    assert off[-1] == 70 * 700
    assert check(pcu, one[:70], one, 0.0)[-1] == 0                         # radius 0: empty rows for coincident points


@pytest.mark.parametrize("dtype", DTYPES)
def test_line_dataset_and_far_queries(pcu, dtype):
    t = np.random.default_rng(7).random(3000)
    line = np.ascontiguousarray(np.stack([t, 0.5 * t, 0.25 * t], axis=1).astype(dtype))            # a degenerate grid
    q = np.random.default_rng(8).random((500, 3)).astype(dtype)
    assert check(pcu, q, line, 0.1)[-1] > 0
    assert check(pcu, line[:200], line, 0.01)[-1] > 200
    p = np.random.default_rng(9).random((5000, 3)).astype(dtype)
    far = (np.random.default_rng(10).random((300, 3)) * 2000.0 - 1000.0).astype(dtype)             # queries far outside the dataset's box, wide apart
    far[:40] = p[:40]                                                                               # ... some of them inside it
    off = check(pcu, far, p, 0.05)
    assert off[40] > 40 and off[-1] == off[40]
    sparse = np.ascontiguousarray(p[::97])                                                          # a query cloud that is sparse against the dataset
    assert check(pcu, sparse, p, 0.02)[-1] >= len(sparse)


@pytest.mark.parametrize("dtype", DTYPES)
def test_nonfinite_queries_and_datasets(pcu, dtype):
    p = np.random.default_rng(11).random((2000, 3)).astype(dtype)
    q = np.random.default_rng(12).random((200, 3)).astype(dtype)
    q[3, 0] = np.nan; q[70, 1] = np.inf; q[71, 2] = -np.inf; q[199] = np.nan
    off = check(pcu, q, p, 0.3)
    assert all(off[i + 1] == off[i] for i in (3, 70, 71, 199)) and off[-1] > 0
    p2 = p.copy(); p2[5, 0] = np.inf; p2[900, 0] = np.inf                 # single-signed infinities: rows that are nobody's members
    off = check(pcu, q, p2, 0.3, tensors=False)
    assert off[-1] > 0
    for bad in ((5, 0, np.nan, None), (5, 1, np.inf, -np.inf)):
        p3 = p.copy(); p3[bad[0], bad[1]] = bad[2]
        if bad[3] is not None:
            p3[6, bad[1]] = bad[3]
        for call in (lambda: pcu.radius_search(q, p3, 0.3), lambda: pcu.radius_count(q, p3, 0.3)):
            with pytest.raises(ValueError, match="dataset_points contains NaN coordinates, or both"):
                call()
        with pytest.raises(ValueError, match="dataset_points contains NaN coordinates, or both"):
            pcu.DatasetIndex(p3)
    same(pcu.radius_search(q, p, 0.3), rc.radius_search(q, p, 0.3))       # the context answers as before


@pytest.mark.parametrize("k_hint", [1, 16])
@pytest.mark.parametrize("dtype", DTYPES)
def test_dataset_index_returns_the_free_functions_bytes(pcu, dtype, k_hint):
    import torch
    p = np.random.default_rng(13).random((3000, 3)).astype(dtype)
    q = np.random.default_rng(14).random((400, 3)).astype(dtype)
    spacing = (1.0 / len(p)) ** (1.0 / 3.0)
    tq = torch.from_numpy(q).cuda()
    with pcu.DatasetIndex(p, k_hint=k_hint) as index, pcu.DatasetIndex(torch.from_numpy(p).cuda(), k_hint=k_hint) as tindex:
        for radius in (0.1 * spacing, spacing, 3.0 * spacing, 0.3, 1.8):
            want = rc.radius_search(q, p, radius)
            free = pcu.radius_search(q, p, radius)
            same(free, want)
            same(index.radius_search(q, radius), free)
            same(tindex.radius_search(tq, radius), free)
            same(index.radius_search(q, radius, squared_distances=True), pcu.radius_search(q, p, radius, squared_distances=True))
            # unsorted rows: their order follows the grid that is walked (the index's own here), so it is the index's, not the free function's --
            # the same members, and the same bytes from two equal calls
            u1 = index.radius_search(q, radius, squared_distances=True, sort_results=False)
            same(index.radius_search(q, radius, squared_distances=True, sort_results=False), u1)
            same([g.cpu() for g in tindex.radius_search(tq, radius, squared_distances=True, sort_results=False)], u1)
            order = np.lexsort((u1[1], u1[2], np.repeat(np.arange(len(q)), want[0][1:] - want[0][:-1])))
            same([u1[0], u1[1][order], u1[2][order]], rc.radius_search(q, p, radius, squared_distances_out=True))
            same([index.radius_count(q, radius)], [want[0][1:] - want[0][:-1]])
            same([tindex.radius_count(tq, radius)], [want[0][1:] - want[0][:-1]])
        assert want[0][-1] == len(q) * len(p)                             # the last radius is the cloud's diameter
        d, c = index.k_nearest_neighbors(q, 3)                             # the index still answers k-NN
        d0, c0 = pcu.k_nearest_neighbors(q, p, 3)
        assert np.array_equal(c, c0) and np.array_equal(d, d0)
    for method, args in (("radius_search", (q, 0.1)), ("radius_count", (q, 0.1)), ("k_nearest_neighbors", (q, 1))):
        with pytest.raises(ValueError, match="the index has been closed"):
            getattr(index, method)(*args)


def test_the_total_limit(pcu):
    """65,536 copies of one query against 32,768 coincident points: 2^31 neighbours. Refused after the count pass, nothing allocated for the rows."""
    import torch
    q = torch.zeros((65536, 3), dtype=torch.float32, device="cuda")
    p = torch.zeros((32768, 3), dtype=torch.float32, device="cuda")
    pcu.radius_count(q[:64], p[:64], 1.0)
    torch.cuda.synchronize()
    free0 = torch.cuda.mem_get_info()[0]
    with pytest.raises(ValueError, match="2147483648"):
        pcu.radius_search(q, p, 1.0)
    free1 = torch.cuda.mem_get_info()[0]
    assert free0 - free1 < (1 << 30), (free0, free1)                      # (the rows alone would take 32 GiB)
    c = pcu.radius_count(q, p, 1.0)
    assert c.dtype == torch.int64 and c.shape == (65536,) and bool((c == 32768).all())
    same(pcu.radius_search(q[:3].cpu().numpy(), p[:5].cpu().numpy(), 1.0), rc.radius_search(np.zeros((3, 3), np.float32), np.zeros((5, 3), np.float32), 1.0))


def test_cancel_from_another_thread(pcu):
    """A canceller thread asks until the main thread has left its loop of calls (a request made between two calls is dropped): the call in
    flight ends with KeyboardInterrupt, and the context answers as before. Shaped after tests/test_gpu_cancel.py."""
    import torch
    q = torch.from_numpy(np.random.default_rng(15).random((1 << 19, 3), dtype=np.float32)).cuda()
    p = torch.from_numpy(np.random.default_rng(16).random((1 << 19, 3), dtype=np.float32)).cuda()
    started, done = threading.Event(), threading.Event()

    def canceller():
        started.wait()
        for _ in range(2000):
            time.sleep(0.005)
            pcu.cancel()
            if done.is_set():
                break
    th = threading.Thread(target=canceller); th.start()
    t0 = time.perf_counter()
    try:
        with pytest.raises(KeyboardInterrupt):
            started.set()
            for _ in range(400):                                           # (every call walks 2^38 pairs)
                pcu.radius_count(q, p, 2.0)
    finally:
        done.set(); th.join()
    assert time.perf_counter() - t0 < 60.0
    a, b = q[:500].cpu().numpy(), p[:4000].cpu().numpy()
    same(pcu.radius_search(a, b, 0.1), rc.radius_search(a, b, 0.1))
    same(pcu.radius_search(q[:500], p[:4000], 0.1), rc.radius_search(a, b, 0.1))
