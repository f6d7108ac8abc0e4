"""cluster_point_cloud_dbscan on the GPU (-m gpu) against tests/dbscan_contract.py: dtype, shape and bytes of labels and is_core, no tolerance,
float32 and float64, numpy arrays and device tensors, every shape called twice with equal bytes, DatasetIndex.cluster_dbscan over two grids.
The shapes are the smallest that reach each path of csrc/dbscan.h: partial and several waves, everybody core | nobody core, one cell, the
staged and the per-lane walk, union trees thousands of links deep across blocks, border points with tied and with unequal core neighbours.
Then a million-point lattice whose labels are known without a brute force (every compute unit unions at once). The cancellation test is
tests/test_gpu_zz_dbscan_cancel.py, and this file sorts behind tests/test_gpu_mesh_sampling.py (Tests)."""
import numpy as np
import pytest

import dbscan_contract as dc

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


def check(pcu, p, eps, min_points, want=None, tensors=True, k_hints=()):
    """(labels, is_core) twice and labels alone -- numpy, then tensors, then an index per k_hint -- against the contract. Returns the contract's."""
    if want is None:
        want = dc.dbscan(p, eps, min_points)
    assert want[0].dtype == np.int64 and want[1].dtype == np.bool_
    kinds = [p]
    if tensors:
        import torch
        kinds.append(torch.from_numpy(p).cuda())
    calls = [(a, lambda a=a, **kw: pcu.cluster_point_cloud_dbscan(a, eps, min_points, **kw)) for a in kinds]
    for k_hint in k_hints:
        for a in kinds:
            index = pcu.DatasetIndex(a, k_hint=k_hint)
            calls.append((a, lambda index=index, **kw: index.cluster_dbscan(eps, min_points, **kw)))
    for a, call in calls:
        got = call(return_core=True)
        assert type(got) is tuple and all(type(g) is type(a) for g in got)
        if hasattr(a, "device"):
            assert all(g.device == a.device for g in got)
        same(got, want)
        same(call(return_core=True), want)                                  # equal calls, equal bytes
        alone = call()
        assert type(alone) is type(a)
        same([alone], want[:1])
    return want


@pytest.mark.parametrize("dtype", DTYPES)
def test_small_sizes_around_a_wave(pcu, dtype):
    rng = np.random.default_rng(1)
    for n in (1, 63, 64, 65, 257):
        p = rng.random((n, 3)).astype(dtype)
        for min_points in (1, 4, n + 1):
            labels, core = check(pcu, p, 0.35, min_points, tensors=n in (1, 65, 257), k_hints=(1, 16) if n == 257 else ())
            if min_points == 1:
                assert core.all() and (labels >= 0).all()
            if min_points == n + 1:
                assert not core.any() and (labels == -1).all()


@pytest.mark.parametrize("dtype", DTYPES)
def test_a_uniform_cloud_with_cores_borders_and_noise(pcu, dtype):
    """Several clusters, a few hundred border points and noise at once; through two index grids too."""
    p = np.random.default_rng(2).random((3000, 3)).astype(dtype)
    labels, core = check(pcu, p, 0.05, 3, k_hints=(1, 16))
    border = ~core & (labels >= 0)
    assert labels.max() >= 10 and border.sum() >= 100 and (labels == -1).sum() >= 100 and core.sum() >= 100


@pytest.mark.parametrize("dtype", DTYPES)
def test_one_cluster_with_every_point_core(pcu, dtype):
    p = np.random.default_rng(3).random((4097, 3)).astype(dtype)
    want = (np.zeros(4097, np.int64), np.ones(4097, bool))
    check(pcu, p, 4.0, 4097, want=want)
    check(pcu, p, 4.0, 7, want=want, tensors=False)                          # (the core pass stops counting at 7)
    check(pcu, p, 4.0, 4098, want=(np.full(4097, -1, np.int64), np.zeros(4097, bool)), tensors=False)


@pytest.mark.parametrize("dtype", DTYPES)
def test_all_noise(pcu, dtype):
    p = np.random.default_rng(4).random((1000, 3)).astype(dtype)
    noise = (np.full(1000, -1, np.int64), np.zeros(1000, bool))
    same(check(pcu, p, 1e-4, 2), noise)
    same(check(pcu, p, 0.0, 1), noise)
    same(check(pcu, np.zeros((70, 3), dtype), 0.0, 1), (np.full(70, -1, np.int64), np.zeros(70, bool)))     # not even coincident points


def chain(n, spacing, seed, dtype, offset=(0.0, 0.0, 0.0)):
    """n points along x, `spacing` apart, in shuffled rows."""
    p = np.zeros((n, 3), dtype)
    p[:, 0] = np.random.default_rng(seed).permutation(n) * spacing
    return p + np.asarray(offset, dtype)


@pytest.mark.parametrize("dtype", DTYPES)
def test_a_thin_chain_of_five_thousand_points(pcu, dtype):
    """Links of 0.9 eps across hundreds of cells, rows shuffled: union trees as deep as the chain is long, hooked from every block."""
    eps, n = 0.5, 5000
    p = chain(n, 0.9 * eps, 7, dtype)
    check(pcu, p, eps, 2, want=(np.zeros(n, np.int64), np.ones(n, bool)), k_hints=(1,))
    # min_points 3: the two ends are border points of the one cluster
    ends = (p[:, 0] == p[:, 0].min()) | (p[:, 0] == p[:, 0].max())
    check(pcu, p, eps, 3, want=(np.zeros(n, np.int64), ~ends), tensors=False)


@pytest.mark.parametrize("dtype", DTYPES)
def test_two_interleaved_chains(pcu, dtype):
    """Two chains side by side, 2 eps apart, their rows interleaved at random: exactly two clusters, numbered by who holds row 0."""
    eps, n = 0.5, 2500
    both = np.concatenate([chain(n, 0.9 * eps, 8, dtype), chain(n, 0.9 * eps, 9, dtype, offset=(0.0, 2.0 * eps, 0.0))])
    order = np.random.default_rng(10).permutation(2 * n)
    p = np.ascontiguousarray(both[order])
    second = order >= n
    labels = np.where(second == second[0], 0, 1).astype(np.int64)
    got = check(pcu, p, eps, 2, want=(labels, np.ones(2 * n, bool)))
    same(got, dc.dbscan(p, eps, 2))                                          # (the analytic answer is the contract's)


def _hub(x, sign):
    """A core point at x and three more 0.9 beyond it (tests/test_dbscan_contract.py): four cores with min_points = 4."""
    return [[x, 0.0, 0.0], [x + sign * 0.9, 0.0, 0.0], [x + sign * 0.9, 0.1, 0.0], [x + sign * 0.9, -0.1, 0.0]]


@pytest.mark.parametrize("dtype", DTYPES)
def test_border_points_tied_and_nearer(pcu, dtype):
    left, right = _hub(-1.0, -1.0), _hub(1.0, 1.0)
    core = np.array([True] * 8 + [False])
    # exactly equidistant from the two hubs: the lower row wins, here the hub of the higher-numbered cluster
    p = np.array(left[1:] + right + left[:1] + [[0.0, 0.0, 0.0]], dtype)
    check(pcu, p, 1.05, 4, want=(np.array([0, 0, 0, 1, 1, 1, 1, 0, 1], np.int64), core))
    p = np.array(left[1:] + left[:1] + right[1:] + right[:1] + [[0.0, 0.0, 0.0]], dtype)
    check(pcu, p, 1.05, 4, want=(np.array([0, 0, 0, 0, 1, 1, 1, 1, 0], np.int64), core))
    # nearer to the hub of the higher-numbered cluster, which has the higher row as well
    p = np.array(left + right + [[0.125, 0.0, 0.0]], dtype)
    check(pcu, p, 1.2, 4, want=(np.array([0] * 4 + [1] * 4 + [1], np.int64), core))
    p = np.array(left + right + [[-0.125, 0.0, 0.0]], dtype)
    check(pcu, p, 1.2, 4, want=(np.array([0] * 4 + [1] * 4 + [0], np.int64), core))
    # the same with the two hubs' members in other waves and other cells than the border point: 200 far noise rows in between
    far = np.random.default_rng(11).random((200, 3)) * 1000.0 + 100.0
    p = np.concatenate([left, far, right, far + 2000.0, [[0.125, 0.0, 0.0]]]).astype(dtype)
    labels, _ = check(pcu, p, 1.2, 4)
    assert labels[-1] == 1 and labels[:4].tolist() == [0] * 4 and labels[204:208].tolist() == [1] * 4 and (labels[4:204] == -1).all()


@pytest.mark.parametrize("dtype", DTYPES)
def test_coincident_copies(pcu, dtype):
    for min_points in (2, 5, 70):                                           # (70 copies: more than a tile of one wave)
        far = np.array([[50.0, 0.0, 0.0]], dtype)
        few = np.concatenate([np.full((min_points - 1, 3), 0.25, dtype), far])
        check(pcu, few, 0.1, min_points, want=(np.full(min_points, -1, np.int64), np.zeros(min_points, bool)), tensors=False)
        enough = np.concatenate([far, np.full((min_points, 3), 0.25, dtype)])
        check(pcu, enough, 0.1, min_points, want=(np.array([-1] + [0] * min_points, np.int64), np.array([False] + [True] * min_points)), tensors=False)


@pytest.mark.parametrize("dtype", DTYPES)
def test_a_dense_blob_and_far_sparse_outliers(pcu, dtype):
    """The blob's waves stage their union box; a wave of outliers has its 64 records in cells far apart and walks per lane. The outliers come
    in tight groups of one to four: the groups of four are small clusters, the others noise."""
    rng = np.random.default_rng(12)
    blob = rng.random((3000, 3)) * 0.1
    centres = rng.random((150, 3)) * 50.0 + 1.0
    groups = [c + rng.random((1 + i % 4, 3)) * 0.01 for i, c in enumerate(centres)]
    p = np.concatenate([blob] + groups)
    p = np.ascontiguousarray(p[rng.permutation(len(p))]).astype(dtype)
    labels, core = check(pcu, p, 0.01, 4, k_hints=(4,))
    assert labels.max() >= 30 and (labels == -1).sum() >= 100 and (~core & (labels >= 0)).sum() >= 20


@pytest.mark.parametrize("dtype", DTYPES)
def test_degenerate_clouds_in_one_cell(pcu, dtype):
    rng = np.random.default_rng(13)
    line = np.zeros((300, 3), dtype)
    line[:, 1] = rng.random(300) * 0.5
    plane = np.zeros((300, 3), dtype)
    plane[:, [0, 2]] = rng.random((300, 2)) * 0.5
    for p, eps in ((line, 0.004), (plane, 0.03), (line + np.asarray([3.0, -2.0, 1.0], dtype), 0.004)):
        check(pcu, p, 1.0, 4, want=(np.zeros(300, np.int64), np.ones(300, bool)), tensors=False)       # one cell holds the cloud
        labels, core = check(pcu, p, eps, 4, tensors=False)
        assert core.sum() >= 30 and (~core).sum() >= 30 and labels.max() >= 3


@pytest.mark.parametrize("dtype", DTYPES)
def test_non_finite_rows(pcu, dtype):
    """A row of +inf is noise and nobody's neighbour, the rest is as without it; NaN, or +inf and -inf on one axis, is refused."""
    p = np.random.default_rng(14).random((257, 3)).astype(dtype)
    labels, core = check(pcu, p, 0.2, 4)
    assert core.any() and not core.all()
    for at, row in ((10, [np.inf] * 3), (0, [np.inf, 0.5, 0.5]), (256, [0.5, -np.inf, 0.5])):
        p2 = np.insert(p, at, np.asarray(row, dtype), axis=0)
        labels2, core2 = check(pcu, p2, 0.2, 4, k_hints=(1,))
        assert labels2[at] == -1 and not core2[at]
        assert np.array_equal(np.delete(labels2, at), labels) and np.array_equal(np.delete(core2, at), core)
    import torch
    for bad in ((5, 0, np.nan, None), (5, 1, np.inf, -np.inf)):
        p3 = p.copy()
        p3[bad[0], bad[1]] = bad[2]
        if bad[3] is not None:
            p3[200, bad[1]] = bad[3]
        for a in (p3, torch.from_numpy(p3).cuda()):
            with pytest.raises(ValueError, match="dataset_points contains NaN coordinates, or both"):
                pcu.cluster_point_cloud_dbscan(a, 0.2, 4)
    check(pcu, p, 0.2, 4, want=(labels, core), tensors=False)                # the context answers as before


def test_stats_and_the_c_entry_point(pcu):
    """The cluster count comes back with the call; a null core output is allowed; what the C side refuses."""
    import ctypes
    from point_cloud_utils_amd import _lib
    p = np.random.default_rng(2).random((3000, 3)).astype(np.float32)
    labels, core = dc.dbscan(p, 0.05, 3)
    L, ctx, st = _lib.lib(), _lib.ctx(), _lib.Stats()
    out, count = np.full(3000, -7, np.int64), ctypes.c_int64(-1)
    rc = L.pcu_hip_dbscan_f32(ctx, p.ctypes.data, 3000, 0.05, 3, out.ctypes.data, None, ctypes.addressof(count), 0, None, ctypes.addressof(st))
    assert rc == 0 and count.value == labels.max() + 1 and np.array_equal(out, labels)
    assert st.n_queries == 3000 and st.n_escalated == count.value and st.n_grid_builds == 1
    for args, text in (((p.ctypes.data, 3000, -1.0, 3), "Invalid radius"), ((p.ctypes.data, 3000, 0.05, 0), "Invalid min_points"),
                       ((p.ctypes.data, 0, 0.05, 3), "zero elements"), ((None, 3000, 0.05, 3), "null points")):
        rc = L.pcu_hip_dbscan_f32(ctx, *args, out.ctypes.data, None, ctypes.addressof(count), 0, None, ctypes.addressof(st))
        assert rc == _lib.ERR_INVALID and count.value == 0
        with pytest.raises(ValueError, match=text):
            _lib.check(rc)
    # more min_points than an int holds: nobody is core
    assert not pcu.cluster_point_cloud_dbscan(p, 0.05, 2 ** 40, return_core=True)[1].any()


# ---------------------------------------------------------------------------------------------------- scale: an analytic answer
@pytest.mark.parametrize("cut", [None, 37])
def test_a_shuffled_lattice_of_a_million_points(pcu, cut):
    """100 x 100 x 100 points of spacing h in shuffled rows, eps = 1.01 h, min_points 4: a corner has itself and three neighbours, so every
    point is core and the lattice is one cluster. With one plane removed the two slabs are 2 h apart: labels 0 and 1, 0 on the side that holds
    row 0. A million records union at once, from every compute unit; the expected labels need no brute force."""
    import torch
    h, m = 0.25, 100
    i = np.arange(m)
    ijk = np.stack(np.meshgrid(i, i, i, indexing="ij"), axis=-1).reshape(-1, 3)
    if cut is not None:
        ijk = ijk[ijk[:, 0] != cut]
    ijk = ijk[np.random.default_rng(16).permutation(len(ijk))]
    p = np.ascontiguousarray(ijk * h, dtype=np.float32)
    n = len(p)
    assert n == (m ** 3 if cut is None else m ** 3 - m * m)
    if cut is None:
        labels = np.zeros(n, np.int64)
    else:
        high = ijk[:, 0] > cut
        labels = np.where(high == high[0], 0, 1).astype(np.int64)
        assert 0 < labels.sum() < n
    want = (labels, np.ones(n, bool))
    t = torch.from_numpy(p).cuda()
    got = pcu.cluster_point_cloud_dbscan(t, 1.01 * h, 4, return_core=True)
    same(got, want)
    same(pcu.cluster_point_cloud_dbscan(t, 1.01 * h, 4, return_core=True), want)
    assert pcu.last_stats()["n_escalated"] == (1 if cut is None else 2)
    if cut is not None:
        same(pcu.cluster_point_cloud_dbscan(p, 1.01 * h, 4, return_core=True), want)
