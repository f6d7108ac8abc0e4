"""GPU tests of connected_components and flood_fill_3d with the whole chip racing on one parent array: a million faces or
four million cells per call -- one to two full rounds of 256 CUs x 2,048 threads --, hooks that all end at one word, roots that change under every
thread's feet, scattered ids, forests half a million trees wide, paths half a million cells long. Everything is compared exactly with
components_fast() / flood_fill_fast() of tests/components_contract.py (scipy's labelling, held to the plain restatements by
tests/test_components_contract.py); what is said "of the input" is asserted from the reference before the library is called. Then the small
shapes at which one wave spans several z rows and x slabs, the scan's carry, the count's runs, producers on a side stream, and the two C entry
points called directly with what the Python layer never lets through."""
import ctypes
import functools

import numpy as np
import pytest

import components_contract as cc

pytestmark = pytest.mark.gpu

NAMES = ("cv", "nv", "cf", "nf")


@pytest.fixture(scope="module")
def pcu():
    import point_cloud_utils_amd as m
    return m


def frozen(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays


def check(pcu, nv, f, want=None):
    """All four outputs of two calls against the reference (computed here unless given): values, dtypes, and equal bytes call to call."""
    if want is None:
        want = cc.components_fast(nv, f)
    v = np.zeros((nv, 3), dtype=np.float32)
    got = pcu.connected_components(v, f)
    for g, w, name in zip(got, want, NAMES):
        assert isinstance(g, np.ndarray) and g.dtype == f.dtype and g.ndim == 1, name
        assert np.array_equal(g, w), (name, int((g != w).sum()) if g.shape == w.shape else (g.shape, w.shape))
    again = pcu.connected_components(v, f)
    assert all(a.tobytes() == b.tobytes() for a, b in zip(got, again))
    return want


def permuted(nv, f, seed):
    """Vertex ids, then the face order, permuted."""
    rng = np.random.default_rng(seed)
    return np.ascontiguousarray(rng.permutation(nv)[f][rng.permutation(len(f))])


# ---------------------------------------------------------------------------------------------------- connected_components: the inputs
GRID_N = 724                                       # vertices per side: 724^2 = 524,176 vertices, 2 * 723^2 = 1,045,458 faces


def grid_mesh(n):
    i, j = np.meshgrid(np.arange(n - 1), np.arange(n - 1), indexing="ij")
    a = (i * n + j).ravel()
    return np.stack([np.stack([a, a + 1, a + n], axis=1), np.stack([a + 1, a + n + 1, a + n], axis=1)], axis=1).reshape(-1, 3)


def hub_faces(hub, nv, m, seed):
    """m faces (hub, a_i, b_i): a and b from two permutations of the other vertices."""
    rng = np.random.default_rng(seed)
    others = np.delete(np.arange(nv), hub)
    return np.stack([np.full(m, hub), rng.permutation(others)[:m], rng.permutation(others)[:m]], axis=1)


@functools.lru_cache(maxsize=1)
def hub_case(hub):
    nv = 1_000_001
    f = hub_faces(hub, nv, 500_000, 21)
    want = cc.components_fast(nv, f)
    return (nv,) + frozen(f, *want)


@functools.lru_cache(maxsize=None)
def one_face_case():
    nv = 300_000
    f = np.tile(np.array([[7, nv - 1, nv // 2]]), (500_000, 1))
    return (nv,) + frozen(f, *cc.components_fast(nv, f))


@functools.lru_cache(maxsize=None)
def tiled_bunny():
    v, f = cc.golden_mesh("bunny")
    copies = 174
    nv = copies * len(v)
    f = permuted(nv, (f[None, :, :] + (np.arange(copies) * len(v))[:, None, None]).reshape(-1, 3), 23)
    return (nv, len(v), len(f) // copies, copies) + frozen(f, *cc.components_fast(nv, f))


# ---------------------------------------------------------------------------------------------------- connected_components: every CU hooking
@pytest.mark.parametrize("scattered", [True, False])
def test_a_grid_mesh_of_a_million_faces_is_one_component(pcu, scattered):
    """Scattered: every find is a scattered read and every chain of hooks ends at one word. In order: consecutive lanes hook consecutive words."""
    nv, f = GRID_N * GRID_N, grid_mesh(GRID_N)
    assert nv == 524_176 and f.shape == (1_045_458, 3)
    if scattered:
        f = permuted(nv, f, 20)
    want = cc.components_fast(nv, f)
    assert want[1].tolist() == [524_176] and want[3].tolist() == [1_045_458]
    check(pcu, nv, f, want)


@pytest.mark.parametrize("hub, dtype", [(0, np.int64), (500_000, np.int64), (1_000_000, np.int64), (1_000_000, np.int32)])
def test_half_a_million_faces_around_one_hub(pcu, hub, dtype):
    """Every face unions the hub's tree. With the hub at nv - 1 the tree's root changes under every thread's feet: every CAS on the hub but the
    first fails and must carry on from the value returned."""
    nv, f, *want = hub_case(hub)
    assert nv == 1_000_001 and hub in (0, nv - 1, nv // 2) and (f[:, 0] == hub).all() and not (f[:, 1:] == hub).any()
    cv, cnv = want[0], want[1]
    assert cnv[cv[hub]] > 700_000 and cnv[cv[hub]] == cnv.max() and (cnv == 1).sum() > 200_000
    check(pcu, nv, f.astype(dtype), want)


@pytest.mark.parametrize("dtype", [np.int64, np.uint32])
def test_one_face_half_a_million_times(pcu, dtype):
    """Every thread of the launch CASes the same two words."""
    nv, f, *want = one_face_case()
    cv, cnv, cf, cnf = want
    assert len(cnv) == nv - 2 and cnv[7] == 3 and cnf[7] == 500_000 and (np.delete(cnv, 7) == 1).all() and not np.delete(cnf, 7).any()
    assert cv[7] == cv[nv - 1] == cv[nv // 2] == 7 and (cf == 7).all()
    check(pcu, nv, f.astype(dtype), want)


def test_a_random_sparse_soup(pcu):
    """The hooks of a deep random forest, ranks up to half a million through the scan, counts with the labels scattered over the lanes."""
    nv = 1_500_000
    f = np.random.default_rng(22).integers(0, nv, (500_000, 3))
    want = cc.components_fast(nv, f)
    assert len(want[1]) >= 100_000 and want[1].max() >= nv // 2
    check(pcu, nv, f, want)


@pytest.mark.parametrize("ids", ["identity", "reversed", "permuted"])
def test_a_strip_of_a_million_triangles(pcu, ids):
    """Identity: every union hooks i + 1 under i, the longest chains before halving. Reversed: every hook lowers an existing root."""
    n = 1_000_000
    i = np.arange(n)
    f = np.stack([i, i + 1, i + 2], axis=1)
    if ids == "reversed":
        f = n + 1 - f
    elif ids == "permuted":
        f = permuted(n + 2, f, 24)
    want = cc.components_fast(n + 2, f)
    assert want[1].tolist() == [1_000_002] and want[3].tolist() == [n]
    check(pcu, n + 2, f, want)


def test_many_equal_components_scattered(pcu):
    """The bunny 174 times, ids and faces permuted: 174 components in the order of their smallest vertex."""
    nv, per_v, per_f, copies, f, *want = tiled_bunny()
    assert (nv, len(f), per_v, per_f) == (501_990, 1_003_284, 2_885, 5_766)
    assert want[1].tolist() == [per_v] * copies and want[3].tolist() == [per_f] * copies
    smallest = np.full(copies, nv)
    np.minimum.at(smallest, want[0], np.arange(nv))
    assert (np.diff(smallest) > 0).all()
    check(pcu, nv, f, want)


def test_many_equal_components_device_resident(pcu):
    import torch
    nv, per_v, per_f, copies, f, *want = tiled_bunny()
    tv = torch.zeros((nv, 3), dtype=torch.float32, device="cuda")
    tf = torch.from_numpy(f.copy()).to(device="cuda")
    assert tf.dtype == torch.int64
    got = pcu.connected_components(tv, tf)
    host = pcu.connected_components(np.zeros((nv, 3), dtype=np.float32), f)
    for g, h, w, name in zip(got, host, want, NAMES):
        assert g.is_cuda and g.device == tf.device and g.dtype == tf.dtype and g.dim() == 1, name
        assert np.array_equal(g.cpu().numpy(), h) and np.array_equal(h, w), name
    again = pcu.connected_components(tv, tf)
    assert all(torch.equal(a, b) for a, b in zip(got, again))


# ---------------------------------------------------------------------------------------------------- the root scan and the counts
def by_hand(nv, faces):
    """The expected arrays of a few disjoint faces, without a reference: cv is arange less the merges."""
    root = np.arange(nv)
    for face in faces:
        root[list(face)] = min(face)
    rank = np.cumsum(root == np.arange(nv)) - 1
    cv = rank[root]
    cf = cv[[face[0] for face in faces]]
    cnv = np.bincount(cv)
    return cv, cnv, cf, np.bincount(cf, minlength=len(cnv))


def test_the_root_scan_carries_from_chunk_to_chunk(pcu):
    """own_inclusive_scan scans the tile sums in chunks of 1,024 tiles of 4,096 with a carry between the chunks: 1,026 tiles here. One face in the
    first tile, one across the boundary between chunk 0 and chunk 1, one that ends in the last tile (which holds the last vertex alone)."""
    edge = cc.SC_TILE * 1024
    nv = edge + cc.SC_TILE + 1
    faces = [(1, 5, 9), (edge - 1, edge, edge + 1), (nv - 3, nv - 2, nv - 1)]
    want = by_hand(nv, faces)
    assert len(want[1]) == nv - 6 and want[0][-1] == nv - 7 and want[2].tolist() == [1, edge - 1 - 2, nv - 3 - 4]
    f = np.array(faces)
    check(pcu, nv, f, want)
    assert all(np.array_equal(a, b) for a, b in zip(want, cc.components_fast(nv, f)))


@pytest.mark.parametrize("nv", [4095, 4096, 4097, 8191, 8193])
def test_the_count_is_read_from_the_last_scan_word(pcu, nv):
    for face in ((nv - 3, nv - 2, nv - 1), (0, nv // 2, nv - 1)):
        want = by_hand(nv, [face])
        assert len(want[1]) == nv - 2
        check(pcu, nv, np.array([face]), want)


@pytest.mark.parametrize("r", [0, 1, 63, 64, 65, 255])
def test_count_runs_at_wave_and_block_edges(pcu, r):
    """cc_count makes one add per run of equal labels among consecutive lanes and closes a wave's last run with the popcount of its active lanes.
    Components are fans over consecutive vertex ranges, so a run of labels is a range: 2,000 of them, of lengths around the wave (64) and the
    block (256) in a shuffled order, the last one lengthened until #v = 256 q + r."""
    rng = np.random.default_rng(30 + r)
    lengths = np.tile([1, 2, 3, 63, 64, 65, 130, 257], 250)
    rng.shuffle(lengths)
    lengths[-1] += (r - lengths.sum()) % 256
    nv = int(lengths.sum())
    assert nv % 256 == r and len(lengths) == 2000
    faces = []
    for start, n in zip((np.cumsum(lengths) - lengths).tolist(), lengths.tolist()):
        j = np.arange(1, max(n - 1, min(n, 2)))              # n >= 3: a fan of n - 2 faces; n == 2: the face (s, s + 1, s + 1); n == 1: none
        faces.append(np.stack([np.full(len(j), start), start + j, start + np.minimum(j + 1, n - 1)], axis=1))
    f = np.concatenate(faces)
    cv, cnv, cf, cnf = want = cc.components_fast(nv, f)
    assert np.array_equal(cnv, lengths) and np.array_equal(cnf, np.where(lengths == 1, 0, np.maximum(lengths - 2, 1)))
    check(pcu, nv, f, want)


def test_faces_produced_on_a_side_stream(pcu):
    """The permuted grid mesh made by torch kernels that are still queued on a side stream when connected_components is called there, without a
    synchronisation: the call must be ordered after its producers."""
    import torch
    n = GRID_N
    side = torch.cuda.Stream()
    gen = torch.Generator(device="cuda")
    gen.manual_seed(25)
    with torch.cuda.stream(side):
        a = (torch.arange(n - 1, device="cuda")[:, None] * n + torch.arange(n - 1, device="cuda")[None, :]).reshape(-1)
        tf = torch.stack([torch.stack([a, a + 1, a + n], dim=1), torch.stack([a + 1, a + n + 1, a + n], dim=1)], dim=1).reshape(-1, 3)
        tf = torch.randperm(n * n, device="cuda", generator=gen)[tf][torch.randperm(len(tf), device="cuda", generator=gen)]
        tv = torch.zeros((n * n, 3), dtype=torch.float32, device="cuda")
        got = pcu.connected_components(tv, tf)            # enqueued behind the producers, no host sync in between
    side.synchronize()
    f = tf.cpu().numpy()
    assert f.dtype == np.int64 and f.shape == (1_045_458, 3) and np.array_equal(np.unique(f), np.arange(n * n))
    want = cc.components_fast(n * n, f)
    assert want[1].tolist() == [n * n]
    for g, w, name in zip(got, want, NAMES):
        assert g.is_cuda and g.dtype == torch.int64 and np.array_equal(g.cpu().numpy(), w), name


# ---------------------------------------------------------------------------------------------------- flood_fill_3d: 160^3, 16,000 workgroups
def check_fill(pcu, grid, seed, fill, reference=cc.flood_fill_fast):
    before = grid.copy()
    want = reference(grid, seed, fill)
    got = pcu.flood_fill_3d(grid, seed, fill)
    assert isinstance(got, np.ndarray) and got.dtype == grid.dtype and got.shape == grid.shape and got.flags.c_contiguous
    assert np.array_equal(got, want), np.argwhere(got != want)[:5]
    assert np.array_equal(grid, before) and got is not grid
    assert pcu.flood_fill_3d(grid, seed, fill).tobytes() == got.tobytes()
    return got


@functools.lru_cache(maxsize=None)
def percolation():
    """Site percolation just above the threshold (0.3116 for the cubic lattice): the largest cluster is a fractal that wanders through the whole
    grid. Returns the grid, the clusters' sizes (index = label - 1), and one cell each of the largest cluster, the zeros, and a one-cell cluster."""
    from scipy import ndimage
    g = (np.random.default_rng(11).random((160, 160, 160)) < 0.32).astype(np.int32)
    label, count = ndimage.label(g)
    sizes = np.bincount(label.ravel())[1:]
    assert len(sizes) == count
    flat = label.ravel()
    cell = lambda at: tuple(int(c) for c in np.unravel_index(at, g.shape))
    big = cell(np.flatnonzero(flat == 1 + int(sizes.argmax()))[0])
    single = cell(np.flatnonzero(flat == 1 + int(np.flatnonzero(sizes == 1)[0]))[0])
    zero = cell(np.flatnonzero(flat == 0)[0])
    frozen(g, sizes)
    return g, sizes, big, zero, single


def test_the_percolation_grid_is_what_the_cases_below_need():
    g, sizes, big, zero, single = percolation()
    assert g.size == 4_096_000 and sizes.sum() == g.sum() and len(sizes) > 100_000
    assert 400_000 <= sizes.max() < g.sum() // 2
    assert g[big] == 1 and g[single] == 1 and g[zero] == 0


def test_fill_the_largest_percolation_cluster(pcu):
    g, sizes, big, zero, single = percolation()
    assert 400_000 <= sizes.max() < g.sum() // 2
    out = check_fill(pcu, g, big, 2)
    assert (out == 2).sum() == sizes.max() and (out == 1).sum() == g.sum() - sizes.max()
    st = pcu.last_stats()
    assert st["n_queries"] == g.size and st["n_escalated"] == sizes.max()


def test_fill_the_zeros_around_the_percolation_clusters(pcu):
    g, sizes, big, zero, single = percolation()
    out = check_fill(pcu, g, zero, 2)
    assert (out == 2).sum() > 0.99 * (g == 0).sum() and (out == 1).sum() == g.sum()


def test_fill_a_cluster_of_one_cell(pcu):
    g, sizes, big, zero, single = percolation()
    out = check_fill(pcu, g, single, 2)
    assert (out == 2).sum() == 1 and out[single] == 2


def test_fill_the_largest_percolation_cluster_as_float64_on_the_device(pcu):
    import torch
    g, sizes, big, zero, single = percolation()
    want = cc.flood_fill_fast(g.astype(np.float64), big, 2.5)
    assert (want == 2.5).sum() == sizes.max()
    t = torch.from_numpy(g.copy()).to(device="cuda", dtype=torch.float64)
    keep = t.clone()
    out = pcu.flood_fill_3d(t, big, 2.5)
    assert out.is_cuda and out.device == t.device and out.dtype == torch.float64 and tuple(out.shape) == g.shape
    assert np.array_equal(out.cpu().numpy(), want) and torch.equal(t, keep) and out.data_ptr() != t.data_ptr()


# ---------------------------------------------------------------------------------------------------- flood_fill_3d: a path of half a million cells
@functools.lru_cache(maxsize=None)
def corridor():
    g, first, cells = cc.serpentine(129)
    # the walk's two ends are the corridor cells with one corridor neighbour
    near = np.zeros(g.shape, dtype=np.int32)
    for axis in range(3):
        lo, hi = [slice(None)] * 3, [slice(None)] * 3
        lo[axis], hi[axis] = slice(0, -1), slice(1, None)
        near[tuple(lo)] += g[tuple(hi)]
        near[tuple(hi)] += g[tuple(lo)]
    ends = [tuple(int(c) for c in e) for e in np.argwhere((g == 1) & (near == 1))]
    assert np.array_equal(np.unique(near[g == 1]), [1, 2]) and len(ends) == 2 and ends[0] == first
    frozen(g)
    return g, ends, cells


def test_a_corridor_of_half_a_million_cells(pcu):
    g, ends, cells = corridor()
    assert g.size == 2_146_689 and cells == 549_249
    for seed in ends:
        out = check_fill(pcu, g, seed, 2)
        assert (out == 2).sum() == cells and not (out == 1).any()


def test_the_corridor_cut_at_its_middle_cell(pcu):
    g, ends, cells = corridor()
    cut = g.copy()
    middle = (64, 64, 64)                                   # the middle cell of the middle row of the middle slab
    assert cut[middle] == 1
    cut[middle] = 0
    a, b = (check_fill(pcu, cut, seed, 2) == 2 for seed in ends)
    assert a.sum() == b.sum() == cells // 2                 # (the walk is symmetric about that cell)
    assert not (a & b).any() and np.array_equal(a | b, cut == 1)


# ---------------------------------------------------------------------------------------------------- flood_fill_3d: a wave across rows and slabs
@pytest.mark.parametrize("shape", [(40, 3, 5), (64, 2, 1), (30, 30, 1), (50, 1, 3), (2, 2, 64), (3, 3, 63), (3, 3, 65), (2, 3, 128), (2, 2, 256)])
def test_shapes_in_which_a_wave_spans_rows_and_slabs(pcu, shape):
    """Where the i % d, row % h and row >= h tests of k_fill_init / k_fill_union change inside a wave of 64 consecutive cells, and where rows start
    exactly on wave and block boundaries. Compared with the plain walk of cc.flood_fill."""
    for p in (0.5, 0.7):
        g = (np.random.default_rng(int(p * 10) + sum(shape)).random(shape) < p).astype(np.int32)
        for value in (1, 0):
            cells = np.argwhere(g == value)
            for seed in (cells[0].tolist(), cells[-1].tolist()):
                check_fill(pcu, g, seed, 3, cc.flood_fill)
    g = np.full(shape, 4, dtype=np.int32)
    for seed in ((0, 0, 0), tuple(s - 1 for s in shape)):
        assert (check_fill(pcu, g, seed, 3, cc.flood_fill) == 3).all()


def test_a_grid_produced_on_a_side_stream(pcu):
    """A grid made by a queue of torch kernels on a side stream and filled there without a synchronisation in between."""
    import torch
    side = torch.cuda.Stream()
    gen = torch.Generator(device="cuda")
    gen.manual_seed(26)
    with torch.cuda.stream(side):
        x = torch.rand((128, 128, 128), device="cuda", generator=gen)
        for _ in range(20):                                # a queue of dependent producer kernels
            x = (x * 1.0000001).clamp(0.0, 1.0)
        t = (x < 0.32).to(torch.int32)
        t[0, 0, :] = 0                                     # the seed's value, and a way from it into the zeros around the clusters
        t[0, :, 0] = 0
        t[:, 0, 0] = 0
        out = pcu.flood_fill_3d(t, (0, 0, 0), 9)           # enqueued behind the producers, no host sync in between
    side.synchronize()
    g = t.cpu().numpy()
    want = cc.flood_fill_fast(g, (0, 0, 0), 9)
    assert g.dtype == np.int32 and 0.25 * g.size < g.sum() < 0.4 * g.size and (want == 9).sum() > 0.9 * (g == 0).sum()
    assert out.is_cuda and out.dtype == torch.int32 and np.array_equal(out.cpu().numpy(), want)


# ---------------------------------------------------------------------------------------------------- the two C entry points, called directly
class Direct:
    """pcu_hip_connected_components / pcu_hip_flood_fill_3d over host arrays, with every argument replaceable."""

    def __init__(self):
        from point_cloud_utils_amd import _lib
        self.lib, self.L, self.ctx = _lib, _lib.lib(), _lib.ctx()
        self.st = _lib.Stats()

    def workspace(self):
        return int(self.L.pcu_hip_ctx_workspace_bytes(self.ctx))

    def components(self, f, nv, **over):
        nf, rows = len(f), nv if 0 < nv < 10 ** 6 else 1       # (a call with another nv is refused before anything is written)
        self.out = [np.full(n, -1, dtype=f.dtype) for n in (rows, nf, rows, rows)]
        self.count = ctypes.c_int64(77)
        a = dict(f_ptr=f.ctypes.data, nf=nf, f_kind={"int32": 0, "int64": 1, "uint32": 2, "uint64": 3}[f.dtype.name], nv=nv, cv=self.out[0].ctypes.data,
                 cf=self.out[1].ctypes.data, cnv=self.out[2].ctypes.data, cnf=self.out[3].ctypes.data)
        a.update(over)
        return self.L.pcu_hip_connected_components(self.ctx, a["f_ptr"], a["nf"], a["f_kind"], a["nv"], a["cv"], a["cf"], a["cnv"], a["cnf"],
                                                   ctypes.addressof(self.count), 0, None, ctypes.addressof(self.st))

    def fill(self, g, seed, fill, **over):
        self.grid_out = np.full(g.shape, -1, dtype=g.dtype)
        self.filled = ctypes.c_int64(77)
        seed3 = (ctypes.c_int64 * 3)(*seed)
        a = dict(grid=g.ctypes.data, out=self.grid_out.ctypes.data, sx=g.shape[0], sy=g.shape[1], sz=g.shape[2], seed3=ctypes.addressof(seed3),
                 kind={"int32": 0, "int64": 1, "float32": 2, "float64": 3}[g.dtype.name])
        a.update(over)
        return self.L.pcu_hip_flood_fill_3d(self.ctx, a["grid"], a["out"], a["sx"], a["sy"], a["sz"], a["seed3"], a["kind"], float(fill),
                                            ctypes.addressof(self.filled), 0, None, ctypes.addressof(self.st))

    def refused(self, rc, counter, message, workspace):
        assert rc == self.lib.ERR_INVALID and counter.value == 0, (rc, counter.value)
        with pytest.raises(ValueError, match=message):
            self.lib.check(rc)
        assert self.workspace() == workspace


def test_what_the_c_side_of_connected_components_refuses(pcu):
    d = Direct()
    f = np.array([[0, 1, 2], [2, 3, 4], [6, 7, 5]])
    cc_valid = lambda: (d.components(f, 9), [o.copy() for o in d.out], d.count.value)
    rc, out, count = cc_valid()                             # (first: whatever this small call needs is allocated before the refusals)
    assert rc == 0
    ws = d.workspace()
    nulls = "^null f / out_cv / out_cf / out_nv / out_nf$"
    for name in ("f_ptr", "cv", "cf", "cnv", "cnf"):
        d.refused(d.components(f, 9, **{name: None}), d.count, nulls, ws)
    d.refused(d.components(f, 9, f_kind=4), d.count, "^f_kind must be one of PCU_HIP_FACE_INT32 / INT64 / UINT32 / UINT64$", ws)
    d.refused(d.components(f, 9, f_kind=-1), d.count, "^f_kind must be one of", ws)
    for nv in (2 ** 27 - 15, 2 ** 27, 2 ** 40):
        d.refused(d.components(f, nv), d.count, r"^meshes and point clouds with more than 2\^27-16 rows are not supported$", ws)
    d.refused(d.components(f, 9, nf=2 ** 27 - 15), d.count, r"more than 2\^27-16 rows", ws)
    for nv, nf in ((0, 3), (9, 0), (-1, 3)):
        d.refused(d.components(f, nv, nf=nf), d.count, "^Invalid input mesh with zero elements", ws)
    d.refused(d.components(f, 7), d.count, r"found a face index outside \[0, 7\)$", d.workspace())      # (found on the device: this one may allocate)
    rc, out, count = cc_valid()                             # the context works on
    want = cc.components(9, f)
    assert rc == 0 and count == len(want[1]) == 3
    assert np.array_equal(out[0], want[0]) and np.array_equal(out[1], want[2])
    assert np.array_equal(out[2][:3], want[1]) and np.array_equal(out[3][:3], want[3]) and (out[2][3:] == -1).all() and (out[3][3:] == -1).all()
    assert d.st.n_queries == 3 and d.st.n_escalated == 3


def test_what_the_c_side_of_flood_fill_refuses(pcu):
    d = Direct()
    g = (np.random.default_rng(40).random((5, 6, 70)) < 0.7).astype(np.float32)
    seed = np.argwhere(g == 1)[0].tolist()
    assert d.fill(g, seed, 2.5) == 0                        # (first: whatever this small call needs is allocated before the refusals)
    ws = d.workspace()
    for name in ("grid", "out", "seed3"):
        d.refused(d.fill(g, seed, 2.5, **{name: None}), d.filled, "^null grid / out / seed3$", ws)
    for kind in (-1, 4):
        d.refused(d.fill(g, seed, 2.5, kind=kind), d.filled, "^kind must be one of PCU_HIP_GRID_INT32 / INT64 / FLOAT32 / FLOAT64$", ws)
    for bad in ((5, 0, 0), (0, 6, 0), (0, 0, 70), (-1, 0, 0), (0, 0, -1), (2 ** 40, 0, 0)):
        d.refused(d.fill(g, bad, 2.5), d.filled, "^seed point must be inside grid$", ws)
    for axis in ("sx", "sy", "sz"):
        d.refused(d.fill(g, (0, 0, 0), 2.5, **{axis: 0}), d.filled, "^seed point must be inside grid$", ws)
        d.refused(d.fill(g, (0, 0, 0), 2.5, **{axis: -3}), d.filled, "^seed point must be inside grid$", ws)
    too_many = r"^grids with more than 2\^31-16 cells are not supported$"
    # 2^21 in each axis: the product is 2^63, which wraps; the check divides instead
    d.refused(d.fill(g, (0, 0, 0), 2.5, sx=2 ** 21, sy=2 ** 21, sz=2 ** 21), d.filled, too_many, ws)
    d.refused(d.fill(g, (0, 0, 0), 2.5, sx=2 ** 32, sy=2 ** 32, sz=1), d.filled, too_many, ws)
    d.refused(d.fill(g, (0, 0, 0), 2.5, sx=2 ** 31 - 15, sy=1, sz=1), d.filled, too_many, ws)
    d.refused(d.fill(g, (0, 0, 0), 2.5, sx=2 ** 11, sy=2 ** 10, sz=2 ** 10), d.filled, too_many, ws)
    assert d.fill(g, seed, 2.5) == 0                        # the context works on
    want = cc.flood_fill(g, seed, 2.5)
    assert np.array_equal(d.grid_out, want) and d.filled.value == (want == 2.5).sum() > 1
    assert d.st.n_queries == g.size and d.st.n_escalated == d.filled.value
