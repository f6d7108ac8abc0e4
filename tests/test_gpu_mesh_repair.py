"""remove_mesh_vertices, remove_unreferenced_mesh_vertices, deduplicate_mesh_vertices and orient_mesh_faces on the GPU (-m gpu) against
tests/mesh_repair_contract.py. Every expected value is an integer or a copy of input bits, so every comparison is of
dtype, shape and bytes; nothing takes a tolerance. References are computed once per mesh (in float64 / int64: the calls only select and
re-index rows, so the expected arrays of another dtype are casts) and shared."""
import functools

import numpy as np
import pytest

import mesh_repair_contract as R

pytestmark = pytest.mark.gpu

FLOATS = [np.float32, np.float64]
SIGNED = [np.int32, np.int64]
KINDS = [np.int32, np.int64, np.uint32, np.uint64]
EDGES = [1, 63, 64, 65, 255, 256, 257]


@pytest.fixture(scope="module")
def pcu():
    import point_cloud_utils_amd as m
    from point_cloud_utils_amd import _lib
    assert _lib.device_count() > 0, "no GPU visible: the gfx950 path has no CPU fallback"
    return m


def to_torch(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def host(a):
    return a.cpu().numpy() if hasattr(a, "is_cuda") else a


def same(got, want, on_device=False):
    """dtype, shape and bytes; a tensor on the device where one is expected, else numpy."""
    if on_device:
        assert got.is_cuda, type(got)
    else:
        assert isinstance(got, np.ndarray), type(got)
    g = host(got)
    assert g.dtype == want.dtype and g.shape == want.shape, (g.dtype, want.dtype, g.shape, want.shape)
    assert g.tobytes() == np.ascontiguousarray(want).tobytes(), int((g != want).sum())


def all_same(got, want, on_device=False):
    assert len(got) == len(want)
    for g, w in zip(got, want):
        same(g, w, on_device)


def stats_are(pcu, nf, escalated):
    st = pcu.last_stats()
    assert st["n_queries"] == nf and st["n_passes"] == 1 and st["n_escalated"] == escalated, st


# ---------------------------------------------------------------------------------------------------- the shared cases
@functools.lru_cache(maxsize=None)
def case(name):
    """The named mesh with vertices that no face lists added in the middle and at the end, a mask that keeps about 70% of the vertices, and
    what the contract makes of them."""
    v, f = R.mesh(name)
    v, f, ids = R.with_unreferenced(v, f, 11)
    mask = np.random.default_rng(12).random(len(v)) < 0.7
    out = dict(v=v, f=f, mask=mask, masked=R.remove_mesh_vertices(v, f, mask), unref=R.remove_unreferenced(v, f))
    for a in (v, f, mask):
        a.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def dedup_case(name, float_name, eps):
    v, f = R.mesh(name)
    v = v.astype(float_name)
    return v, f, R.dedup_mesh(v, f, eps)


@functools.lru_cache(maxsize=None)
def orient_case(name, seed):
    _, f = R.mesh(name)
    g = R.reverse_some(f, seed) if seed else f
    return g, R.orient(g)


def cast(arrays, float_dtype, int_dtype):
    return tuple(a.astype(float_dtype if a.dtype.kind == "f" else int_dtype) for a in arrays)


# ---------------------------------------------------------------------------------------------------- each call equals the contract
@pytest.mark.parametrize("kind", SIGNED)
@pytest.mark.parametrize("dtype", FLOATS)
@pytest.mark.parametrize("name", R.MESH_NAMES)
def test_remove_mesh_vertices_equals_the_contract(pcu, name, dtype, kind):
    c = case(name)
    v, f, mask = c["v"].astype(dtype), c["f"].astype(kind), c["mask"].copy()
    want = cast(c["masked"], dtype, kind)
    all_same(pcu.remove_mesh_vertices(v, f, mask), want)
    stats_are(pcu, len(f), len(f) - len(want[1]))
    all_same(pcu.remove_mesh_vertices(v, f, mask.reshape(-1, 1)), want)
    all_same(pcu.remove_mesh_vertices(to_torch(v), to_torch(f), to_torch(mask)), want, on_device=True)
    stats_are(pcu, len(f), len(f) - len(want[1]))


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("dtype", FLOATS)
@pytest.mark.parametrize("name", R.MESH_NAMES)
def test_remove_unreferenced_equals_the_contract(pcu, name, dtype, kind):
    c = case(name)
    v, f = c["v"].astype(dtype), c["f"].astype(kind)
    want = cast(c["unref"], dtype, kind)
    assert (want[3] == np.array(-1).astype(kind)).sum() >= 6
    got = pcu.remove_unreferenced_mesh_vertices(v, f)
    all_same(got, want)
    stats_are(pcu, len(f), 0)
    assert got[0][got[1].astype(np.int64)].tobytes() == v[f.astype(np.int64)].tobytes()
    if np.dtype(kind).kind == "i":
        all_same(pcu.remove_unreferenced_mesh_vertices(to_torch(v), to_torch(f)), want, on_device=True)


@pytest.mark.parametrize("kind", SIGNED)
@pytest.mark.parametrize("dtype", FLOATS)
@pytest.mark.parametrize("name", R.MESH_NAMES)
def test_deduplicate_mesh_vertices_equals_the_contract(pcu, name, dtype, kind):
    """epsilon = 0 on the meshes as they are (`defective` and `cube_twist` may hold equal rows; the others come back re-ordered), and what
    deduplicate_point_cloud returns for the same vertices."""
    v, f, want = dedup_case(name, np.dtype(dtype).name, 0.0)
    f = f.astype(kind)
    want = (want[0], want[1].astype(kind), want[2], want[3])
    got = pcu.deduplicate_mesh_vertices(v, f, 0.0)
    all_same(got, want)
    stats_are(pcu, len(f), len(f) - len(want[1]))
    all_same((got[0], got[2], got[3]), pcu.deduplicate_point_cloud(v, 0.0))
    all_same(pcu.deduplicate_mesh_vertices(v, f, 0.0, return_index=False), want[:2])
    all_same(pcu.deduplicate_mesh_vertices(to_torch(v), to_torch(f), 0.0), want, on_device=True)
    all_same(pcu.deduplicate_mesh_vertices(to_torch(v), to_torch(f), 0.0, return_index=False), want[:2], on_device=True)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("name", R.MESH_NAMES)
def test_orient_mesh_faces_equals_the_contract(pcu, name, kind):
    for seed in (0, 4):
        g, (o, p, tw) = orient_case(name, seed)
        f = g.astype(kind)
        want = (o.astype(kind), p.astype(kind))
        all_same(pcu.orient_mesh_faces(f), want)
        stats_are(pcu, len(f), tw)
        all_same(pcu.orient_mesh_faces(f, weighting_type="angle"), want)
        if np.dtype(kind).kind == "i":
            all_same(pcu.orient_mesh_faces(to_torch(f)), want, on_device=True)
            stats_are(pcu, len(f), tw)


# ---------------------------------------------------------------------------------------------------- empty results
@pytest.mark.parametrize("torch_in", [False, True])
def test_masks_that_leave_nothing(pcu, torch_in):
    v, f = R.mesh("tetrahedron")
    v, f = v.astype(np.float32), f.astype(np.int32)
    give = to_torch if torch_in else (lambda a: a)
    vo, fo = pcu.remove_mesh_vertices(give(v), give(f), give(np.zeros(4, dtype=bool)))
    same(vo, np.zeros((0, 3), dtype=np.float32), torch_in)
    same(fo, np.zeros((0, 3), dtype=np.int32), torch_in)
    stats_are(pcu, 4, 4)
    keep = np.array([True, False, False, True])             # two vertices stay, no whole face does
    vo, fo = pcu.remove_mesh_vertices(give(v), give(f), give(keep))
    same(vo, v[[0, 3]], torch_in)
    same(fo, np.zeros((0, 3), dtype=np.int32), torch_in)
    vo, fo = pcu.remove_mesh_vertices(give(v), give(f), give(np.ones(4, dtype=bool)))
    same(vo, v, torch_in)
    same(fo, f, torch_in)
    stats_are(pcu, 4, 0)


def test_dedup_that_drops_every_face(pcu):
    v = np.zeros((5, 3))
    f = np.array([[0, 1, 2], [2, 3, 4]])
    vo, fo, svi, svj = pcu.deduplicate_mesh_vertices(v, f, 0.0)
    same(vo, np.zeros((1, 3)))
    same(fo, np.zeros((0, 3), dtype=np.int64))
    same(svi, np.zeros(1, dtype=np.int32))
    same(svj, np.zeros(5, dtype=np.int32))
    stats_are(pcu, 2, 2)


# ---------------------------------------------------------------------------------------------------- orient: the hand-worked cases
HAND = [
    ([[0, 1, 2], [1, 0, 3]], [[0, 1, 2], [1, 0, 3]], [0, 0], 0),
    ([[0, 1, 2], [0, 1, 3]], [[0, 1, 2], [3, 1, 0]], [0, 0], 0),
    ([[0, 1, 3], [0, 1, 2]], [[0, 1, 3], [2, 1, 0]], [0, 0], 0),
    ([[0, 1, 2], [0, 1, 3], [0, 1, 4]], [[0, 1, 2], [0, 1, 3], [0, 1, 4]], [0, 1, 2], 0),
    ([[0, 0, 1], [0, 1, 2], [0, 1, 3], [3, 3, 3]], [[0, 0, 1], [0, 1, 2], [3, 1, 0], [3, 3, 3]], [0, 1, 1, 2], 0),
    ([[0, 3, 1], [3, 4, 1], [1, 4, 2], [4, 5, 2], [2, 5, 3], [5, 0, 3]], [[0, 3, 1], [3, 4, 1], [1, 4, 2], [4, 5, 2], [2, 5, 3], [5, 0, 3]], [0] * 6, 1),
    ([[5, 5, 5]], [[5, 5, 5]], [0], 0),
]


@pytest.mark.parametrize("f, oriented, patches, twisted", HAND)
def test_orient_by_hand(pcu, f, oriented, patches, twisted):
    for kind in KINDS:
        o, p = pcu.orient_mesh_faces(np.array(f, dtype=kind))
        same(o, np.array(oriented, dtype=kind))
        same(p, np.array(patches, dtype=kind))
        stats_are(pcu, len(f), twisted)


def test_orient_a_tetrahedron_with_one_face_reversed(pcu):
    _, f = R.mesh("tetrahedron")
    for k in (1, 2, 3):
        g = f.copy()
        g[k] = g[k, ::-1]
        o, p = pcu.orient_mesh_faces(g)
        same(o, f)
        same(p, np.zeros(4, dtype=np.int64))
    g = f.copy()
    g[0] = g[0, ::-1]
    same(pcu.orient_mesh_faces(g)[0], np.ascontiguousarray(f[:, ::-1]))


def test_orient_a_moebius_band_beside_a_sphere(pcu):
    """The band comes back unchanged and is counted; the sphere in the same call is oriented."""
    _, sphere = R.S.mesh("sphere258")
    band = R.reverse_some(R.moebius(40), 6)
    f = np.concatenate([band, R.reverse_some(sphere, 7) + int(band.max()) + 1])
    want_o, want_p, tw = R.orient(f)
    assert tw == 1 and np.array_equal(want_o[:80], band) and not np.array_equal(want_o[80:], f[80:])
    assert want_p[:80].tolist() == [0] * 80 and want_p[80:].tolist() == [1] * len(sphere)
    o, p = pcu.orient_mesh_faces(f)
    same(o, want_o)
    same(p, want_p)
    stats_are(pcu, len(f), 1)
    assert R.check_orientation(f, o, p) == 1
    o, p = pcu.orient_mesh_faces(to_torch(f))
    same(o, want_o, True)
    stats_are(pcu, len(f), 1)


def test_orient_the_closed_book(pcu):
    f = R.reverse_some(R.closed_book(40), 8)
    want_o, want_p, tw = R.orient(f)
    assert tw == 0 and want_p.max() == 39
    all_same(pcu.orient_mesh_faces(f), (want_o, want_p))
    stats_are(pcu, len(f), 0)


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_orient_the_bunny_with_half_of_its_faces_reversed(pcu, seed):
    g, (want_o, want_p, tw) = orient_case("bunny", seed)
    first = pcu.orient_mesh_faces(g)
    all_same(first, (want_o, want_p))
    again = pcu.orient_mesh_faces(g)
    assert all(a.tobytes() == b.tobytes() for a, b in zip(first, again))
    assert R.check_orientation(g, first[0], first[1]) == tw


# ---------------------------------------------------------------------------------------------------- wave and block edges
@pytest.mark.parametrize("nf", EDGES + [258])
def test_orient_a_strip_of_triangles(pcu, nf):
    """One patch of nf faces whose every second face must turn: the scan of one root flag, the run heads where a wave or a block ends, the last
    partial block. At 257 faces the 771 sorted corners have runs of two across the boundaries of the blocks of 256."""
    f = R.strip(nf)
    want = (np.ascontiguousarray(np.where((np.arange(nf) % 2 == 1)[:, None], f[:, ::-1], f)), np.zeros(nf, dtype=np.int64))
    all_same(pcu.orient_mesh_faces(f), want)
    stats_are(pcu, nf, 0)
    g = R.reverse_some(f, nf)                              # whichever way its first face runs decides for all
    turned = np.ascontiguousarray(want[0][:, ::-1])
    all_same(pcu.orient_mesh_faces(g.astype(np.int32)), ((want[0] if (g[0] == f[0]).all() else turned).astype(np.int32), want[1].astype(np.int32)))


def small_mesh(nv):
    if nv < 3:
        return np.arange(3.0 * nv).reshape(nv, 3), np.zeros((1, 3), dtype=np.int64) + (nv - 1)
    return R.strip_mesh(nv)


@pytest.mark.parametrize("nv", EDGES + [2, 258, 259])
def test_vertex_calls_at_wave_and_block_edges(pcu, nv):
    """#v at the edges, and #f = #v - 2 with it: 257, 258 and 259 vertices give 255, 256 and 257 faces."""
    v, f = small_mesh(nv)
    for seed in (0, 1):
        mask = np.random.default_rng(100 * nv + seed).random(nv) < (0.8 if seed else 0.5)
        mask[-1] = seed == 0                               # the last vertex kept and dropped
        all_same(pcu.remove_mesh_vertices(v, f, mask), R.remove_mesh_vertices(v, f, mask))
    for drop in (slice(0, 0), slice(0, 1), slice(-1, None), slice(1, None, 3)):
        g = np.delete(f, drop, axis=0) if len(f) > 1 else f
        if len(g):
            all_same(pcu.remove_unreferenced_mesh_vertices(v, g), R.remove_unreferenced(v, g))
    w = np.concatenate([v, v[::-1]])                       # every vertex twice: the second half welds onto the first
    g = np.concatenate([f, 2 * nv - 1 - f])
    all_same(pcu.deduplicate_mesh_vertices(w, g, 0.0), R.dedup_mesh(w, g, 0.0))


# ---------------------------------------------------------------------------------------------------- deduplication
@pytest.mark.parametrize("dtype", FLOATS)
@pytest.mark.parametrize("name", ["sphere258", "bunny"])
def test_dedup_welds_a_soup_back(pcu, name, dtype):
    v, f = R.S.mesh(name)
    v = v.astype(dtype)
    assert len(np.unique(v, axis=0)) == len(v)
    sv, sf = R.soup(v, f)
    vo, fo, svi, svj = pcu.deduplicate_mesh_vertices(sv, sf, 0.0)
    order = np.lexsort((v[:, 2], v[:, 1], v[:, 0]))
    rank = np.empty(len(v), dtype=np.int64)
    rank[order] = np.arange(len(v))
    same(vo, v[order])
    same(fo, rank[f])
    assert vo[fo].tobytes() == v[f].tobytes()
    all_same((vo, fo, svi, svj), R.dedup_mesh(sv, sf, 0.0))
    stats_are(pcu, len(f), 0)
    all_same(pcu.deduplicate_mesh_vertices(to_torch(sv), to_torch(sf), 0.0), (vo, fo, svi, svj), on_device=True)


@pytest.mark.parametrize("dtype", FLOATS)
def test_dedup_groups_a_jittered_soup_by_epsilon(pcu, dtype):
    """Vertices on a lattice of spacing 1/8 (exact in both dtypes), every corner of the soup moved by less than a twentieth of epsilon = 1/16:
    round(x / epsilon) of a corner is that of its lattice point."""
    rng = np.random.default_rng(13)
    _, f = R.S.mesh("sphere258")
    v = rng.permutation(np.stack(np.meshgrid(np.arange(7), np.arange(7), np.arange(7), indexing="ij"), axis=-1).reshape(-1, 3))[:258] / 8.0
    sv, sf = R.soup(v, f)
    sv = (sv + rng.uniform(-1, 1, sv.shape) / 320.0).astype(dtype)
    want = R.dedup_mesh(sv, sf, 1.0 / 16)
    assert len(want[0]) == 258 and len(want[1]) == len(f) and len(np.unique(sv, axis=0)) == len(sv)
    assert np.array_equal(np.unique(want[1]), np.arange(258))
    all_same(pcu.deduplicate_mesh_vertices(sv, sf, 1.0 / 16), want)
    coarse = R.dedup_mesh(sv, sf, 0.5)                      # a few lattice points to a group: faces fold up and are dropped
    assert 0 < len(coarse[1]) < len(f)
    all_same(pcu.deduplicate_mesh_vertices(sv, sf, 0.5), coarse)
    stats_are(pcu, len(f), len(f) - len(coarse[1]))
    all_same(pcu.deduplicate_mesh_vertices(to_torch(sv), to_torch(sf.astype(np.int32)), 0.5), (coarse[0], coarse[1].astype(np.int32)) + coarse[2:], on_device=True)
    all_same(pcu.deduplicate_mesh_vertices(sv, sf, 0.0), R.dedup_mesh(sv, sf, 0.0))


# ---------------------------------------------------------------------------------------------------- rows are copied, not computed with
@pytest.mark.parametrize("dtype", FLOATS)
def test_non_finite_coordinates_pass_through(pcu, dtype):
    c = case("defective")
    v, f, mask = c["v"].astype(dtype), c["f"].copy(), c["mask"].copy()
    quiet = np.array([0x7FC00123 if dtype is np.float32 else 0x7FF8000000000123], dtype=np.uint32 if dtype is np.float32 else np.uint64).view(dtype)[0]
    used = int(f[0, 0])
    v[used] = [quiet, -0.0, np.inf]
    v[int(f[1, 1])] = [-np.inf, -0.0, 1e-40]               # (a subnormal in float32)
    mask[used] = True
    vo, fo = pcu.remove_mesh_vertices(v, f, mask)
    all_same((vo, fo), R.remove_mesh_vertices(v, f, mask))
    assert vo[int(mask[:used].sum())].tobytes() == v[used].tobytes()
    got = pcu.remove_unreferenced_mesh_vertices(v, f)
    all_same(got, R.remove_unreferenced(v, f))
    assert got[0][got[1]].tobytes() == v[f].tobytes()
    tv = pcu.remove_unreferenced_mesh_vertices(to_torch(v), to_torch(f))[0]
    assert tv.cpu().numpy().tobytes() == got[0].tobytes()


# ---------------------------------------------------------------------------------------------------- refusals found on the device
def test_an_index_outside_v_is_refused_on_the_device(pcu):
    v, f = R.mesh("tetrahedron")
    bad = f.copy()
    bad[2, 1] = 4
    neg = f.copy()
    neg[3, 0] = -1
    tv = to_torch(v)
    for g in (bad, neg):
        tf = to_torch(g)
        for call in (lambda: pcu.remove_mesh_vertices(tv, tf, to_torch(np.ones(4, dtype=bool))), lambda: pcu.remove_unreferenced_mesh_vertices(tv, tf),
                     lambda: pcu.deduplicate_mesh_vertices(tv, tf, 0.0)):
            with pytest.raises(ValueError, match=r"f must hold row indices of v: found a face index outside \[0, 4\)"):
                call()
    with pytest.raises(ValueError, match=r"f must hold row indices of v: found a face index outside \[0, 4\)"):
        pcu.orient_mesh_faces(to_torch(neg))
    all_same(pcu.orient_mesh_faces(to_torch(f)), R.orient(f)[:2], on_device=True)       # the context works on
    with pytest.raises(ValueError, match="torch inputs must all be CUDA/HIP tensors on the same device"):
        pcu.remove_mesh_vertices(tv, to_torch(f), np.ones(4, dtype=bool))


# ---------------------------------------------------------------------------------------------------- the whole chip on one parent array
@functools.lru_cache(maxsize=1)
def race_case():
    """A 512 x 512 grid mesh (522,242 faces) and a dozen disjoint 24 x 24 grids (1,058 faces each) behind it in vertex order, half of all
    faces reversed, the faces of all thirteen shuffled into one order."""
    rng = np.random.default_rng(31)
    parts, at = [R.grid_faces(512)], 512 * 512
    for _ in range(12):
        parts.append(R.grid_faces(24, at))
        at += 24 * 24
    f = np.concatenate(parts)
    f = R.reverse_some(f[rng.permutation(len(f))], 32)
    f.setflags(write=False)
    return f, R.patches_by_scipy(f)


def test_half_a_million_faces_racing_on_the_double_cover(pcu):
    """About 6,300 workgroups of 256 in the union launch, on one parent array of 1.07 million elements: every CU several times over. Checked
    by the property (every manifold edge run in opposite directions, the first face of each patch kept) and against scipy's labelling."""
    f, patches = race_case()
    assert len(f) == 522_242 + 12 * 1_058 and patches.max() == 12
    o, p = pcu.orient_mesh_faces(f)
    assert o.dtype == np.int64 and p.dtype == np.int64 and o.shape == f.shape
    assert np.array_equal(p, patches)
    assert R.check_orientation(f, o, p) == 0
    stats_are(pcu, len(f), 0)
    o2, p2 = pcu.orient_mesh_faces(f)
    assert o2.tobytes() == o.tobytes() and p2.tobytes() == p.tobytes()
    to, tp = pcu.orient_mesh_faces(to_torch(f.astype(np.int32)))
    assert np.array_equal(to.cpu().numpy(), o) and np.array_equal(tp.cpu().numpy(), p)
