"""closest_points_on_mesh on the GPU (-m gpu): every row bit-equal to the contract restated in tests/mesh_contract.py -- d bits, fi, bc bits --
whatever the index prunes; MeshIndex; a million queries; run-to-run equality; cancellation."""
import ctypes
import gc
import threading
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

import mesh_contract as mc
import ray_contract as rc

pytestmark = pytest.mark.gpu
DTYPES = [np.float32, np.float64]
B = mc.B


@pytest.fixture(scope="module")
def pcu():
    import point_cloud_utils_amd as m
    from point_cloud_utils_amd import _lib
    assert _lib.device_count() > 0, "no GPU visible: the gfx950 path has no CPU fallback"
    return m


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32 if a.dtype == np.float32 else np.uint64)


def _to_numpy(x):
    return x.detach().cpu().numpy() if hasattr(x, "detach") else np.asarray(x)


def _assert_same(got, want, what):
    """Every row: the distance's bits, the face, the barycentric coordinates' bits."""
    d, fi, bc = (_to_numpy(x) for x in got)
    d0, fi0, bc0 = want
    assert d.dtype == d0.dtype and bc.dtype == bc0.dtype and d.shape == d0.shape and bc.shape == bc0.shape, what
    bad = np.flatnonzero((fi.astype(np.int64) != fi0) | (_bits(d) != _bits(d0)) | (_bits(bc) != _bits(bc0)).any(axis=1))
    assert bad.size == 0, (what, f"{bad.size} of {len(d0)} rows differ", bad[:5], d[bad[:5]], d0[bad[:5]], fi[bad[:5]], fi0[bad[:5]])


def _brute(p, v, f, faces=None, workers=8):
    """mesh_contract.closest_brute over slices of p on a few threads (numpy releases the GIL inside its loops)."""
    cuts = np.linspace(0, len(p), min(workers, max(1, len(p) // 16)) + 1).astype(int)
    def part(k):
        a, b = cuts[k], cuts[k + 1]
        return mc.closest_brute(p[a:b], v, f, None if faces is None else faces[a:b])
    with ThreadPoolExecutor(workers) as ex:
        parts = list(ex.map(part, range(len(cuts) - 1)))
    return tuple(np.concatenate([x[i] for x in parts]) for i in range(3))


def _torch(*arrays):
    import torch
    return tuple(torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in arrays)


def _candidates(p, v, f):
    """A sound float64 filter: a face can only win if the distance from the query to the face's bounding box is at most the distance to the
    nearest referenced vertex (that vertex belongs to a face, so the mesh is no farther), with a slack far above rounding: 1e-3 relative
    plus 1e-3 of the scale. Returns per query the ascending face list."""
    from scipy.spatial import cKDTree
    p64, v64 = p.astype(np.float64), v.astype(np.float64)
    scale = max(float(np.abs(v64).max()), float(np.abs(p64).max()))
    tri = v64[f]
    lo, hi = tri.min(axis=1), tri.max(axis=1)
    mid, half = (lo + hi) / 2, np.linalg.norm((hi - lo) / 2, axis=1)
    dv, _ = cKDTree(v64[np.unique(f)]).query(p64)
    r = dv * (1 + 1e-3) + 1e-3 * scale
    near = cKDTree(mid).query_ball_point(p64, r + half.max())
    out = []
    for i, cand in enumerate(near):
        cand = np.sort(np.asarray(cand, dtype=np.int64))
        gap = np.maximum(np.maximum(lo[cand] - p64[i], p64[i] - hi[cand]), 0.0)
        out.append(cand[np.linalg.norm(gap, axis=1) <= r[i]])
    return out


# ---------------------------------------------------------------------------------------------------- 1. bit-equality with the restatement
@pytest.mark.parametrize("T", DTYPES)
def test_bunny_every_input_kind_and_face_dtype(pcu, T):
    import torch
    v, f = mc.bunny(T)
    q = np.concatenate(list(mc.query_sets(v, f, 300, T).values()))
    want = _brute(q, v, f)
    for fdt in (np.int32, np.int64, np.uint32, np.uint64):
        got = pcu.closest_points_on_mesh(q, v, f.astype(fdt))
        assert got[1].dtype == fdt and got[0].shape == (len(q),) and got[2].shape == (len(q), 3)
        _assert_same(got, want, ("numpy", fdt))
    got = pcu.closest_points_on_mesh(np.asfortranarray(q), np.asfortranarray(v), np.asfortranarray(f))
    _assert_same(got, want, "F-ordered numpy")
    for fdt, tdt in ((np.int32, torch.int32), (np.int64, torch.int64)):
        tq, tv, tf = _torch(q, v, f.astype(fdt))
        got = pcu.closest_points_on_mesh(tq, tv, tf)
        assert all(isinstance(x, torch.Tensor) and x.is_cuda for x in got) and got[1].dtype == tdt and got[0].dtype == tq.dtype
        _assert_same(got, want, ("torch", fdt))


@pytest.mark.parametrize("T", DTYPES)
@pytest.mark.parametrize("nf", [1, 4, 5])
def test_meshes_of_one_leaf_and_of_two(pcu, nf, T):
    """1 face, 4 faces (one full leaf: the root is the leaf and the stack is never used), 5 faces (two leaves, one of them mostly padding)."""
    rng = np.random.default_rng(nf)
    v = rng.random((3 * nf, 3)).astype(T)
    f = rng.permutation(3 * nf).reshape(nf, 3).astype(np.int64)
    q = np.concatenate([mc.surface_samples(v, f, 200, 3), rng.random((400, 3)) * 3 - 1]).astype(T)
    want = _brute(q, v, f)
    assert len(np.unique(want[1])) == nf                                  # (every face is some query's closest)
    _assert_same(pcu.closest_points_on_mesh(q, v, f), want, (nf, "numpy"))
    got = pcu.closest_points_on_mesh(*_torch(q, v, f))
    assert all(x.is_cuda for x in got)
    _assert_same(got, want, (nf, "torch"))


@pytest.fixture(scope="module")
def big_sphere():
    return {T: mc.sphere(160, T) for T in DTYPES}            # 204,800 faces


@pytest.mark.parametrize("T", DTYPES)
def test_sphere_of_200k_faces(pcu, big_sphere, T):
    v, f = big_sphere[T]
    assert len(f) >= 200_000
    sets = mc.query_sets(v, f, 8125, T, seed=21)
    sizes = {"box": 8125, "surface": 6125, "vertex": 5125, "far": 1125}     # (a far query keeps a sixth of the faces as candidates)
    q = np.concatenate([sets[k][:n] for k, n in sizes.items()])            # 20,500 rows; the first 125 of every kind are brute-forced against all faces
    first = np.concatenate([np.arange(125) + off for off in np.cumsum([0] + list(sizes.values())[:-1])])
    rest = np.setdiff1d(np.arange(len(q)), first)
    assert len(first) == 500 and len(rest) == 20_000
    cand = _candidates(q, v, f)
    want_first = _brute(q[first], v, f)
    for row, fi in zip(first, want_first[1]):
        assert fi in cand[row], ("the filter dropped the winner", row, fi)
    want_rest = _brute(q[rest], v, f, [cand[i] for i in rest])
    want = tuple(np.empty((len(q),) + w.shape[1:], w.dtype) for w in want_first)
    for w, a, b in zip(want, want_first, want_rest):
        w[first] = a; w[rest] = b
    _assert_same(pcu.closest_points_on_mesh(q, v, f.astype(np.int32)), want, "numpy")
    _assert_same(pcu.closest_points_on_mesh(*_torch(q, v, f)), want, "torch")


@pytest.mark.parametrize("T", DTYPES)
def test_integer_lattice_every_minimum_is_a_tie(pcu, T):
    n = 40
    x, y = np.meshgrid(np.arange(n), np.arange(n), indexing="ij")
    v = np.stack([x.ravel(), y.ravel(), np.zeros(n * n)], 1).astype(T)
    i, j = np.meshgrid(np.arange(n - 1), np.arange(n - 1), indexing="ij")
    a = (i * n + j).ravel()
    f = np.concatenate([np.stack([a, a + n, a + 1], 1), np.stack([a + n, a + n + 1, a + 1], 1)]).astype(np.int64)
    f = f[np.random.default_rng(2).permutation(len(f))]
    g = np.arange(-3, n + 3) + 0.5
    qx, qy, qz = np.meshgrid(g[::2], g[::2], np.array([0.0, 0.5, 1.5, -2.5]), indexing="ij")
    q = np.stack([qx.ravel(), qy.ravel(), qz.ravel()], 1).astype(T)
    q = np.concatenate([q, np.stack([x.ravel(), y.ravel(), np.full(n * n, 2.0)], 1).astype(T)[::3]])      # above the vertices: up to six-way ties
    want = _brute(q, v, f)
    _assert_same(pcu.closest_points_on_mesh(q, v, f), want, "numpy")
    _assert_same(pcu.closest_points_on_mesh(*_torch(q, v, f)), want, "torch")


@pytest.mark.parametrize("T", DTYPES)
def test_one_face_spanning_the_box_beside_50k_tiny_ones(pcu, T):
    rng = np.random.default_rng(6)
    c = rng.random((50_000, 3))
    tiny = (c[:, None, :] + rng.normal(size=(50_000, 3, 3)) * 1e-3).reshape(-1, 3)
    v = np.concatenate([tiny, [[-0.5, -0.5, 0.3], [2.5, -0.5, 0.6], [0.5, 2.5, 0.4]]]).astype(T)
    f = np.arange(150_003, dtype=np.int64).reshape(-1, 3)
    f = np.concatenate([f[:20_000], f[-1:], f[20_000:-1]])                 # (the large face somewhere in the middle)
    q = np.concatenate([rng.random((200, 3)), rng.random((60, 3)) * 3 - 1]).astype(T)
    want = _brute(q, v, f)
    assert (want[1] == 20_000).sum() > 20                                  # the large face wins for a good share of the queries
    _assert_same(pcu.closest_points_on_mesh(q, v, f), want, "numpy")
    _assert_same(pcu.closest_points_on_mesh(*_torch(q, v, f)), want, "torch")


@pytest.mark.parametrize("T", DTYPES)
def test_10k_faces_sharing_one_morton_code(pcu, T):
    rng = np.random.default_rng(8)
    a, b = rng.normal(size=(10_000, 3)) * 0.25, rng.normal(size=(10_000, 3)) * 0.25
    centre = np.array([0.5, 0.25, 0.125])
    tri = np.stack([a, b, -a - b], 1) + centre                             # coincident centroids
    v = tri.reshape(-1, 3).astype(T)
    f = np.arange(30_000, dtype=np.int64).reshape(-1, 3)
    q = np.concatenate([rng.normal(size=(300, 3)) * 0.5 + centre, rng.normal(size=(50, 3)) * 20]).astype(T)
    want = _brute(q, v, f)
    _assert_same(pcu.closest_points_on_mesh(q, v, f), want, "numpy")
    _assert_same(pcu.closest_points_on_mesh(*_torch(q, v, f)), want, "torch")


@pytest.mark.parametrize("T", DTYPES)
@pytest.mark.parametrize("shift,scale", [(1e3, 1.0), (0.0, 2.0 ** -20), (0.0, 2.0 ** 20)])
def test_bunny_shifted_and_scaled(pcu, T, shift, scale):
    v0, f = mc.bunny(np.float64)
    v = ((v0 + shift) * scale).astype(T)
    q = np.concatenate([a for a in mc.query_sets(v, f, 100, T, seed=31).values()])
    want = _brute(q, v, f)
    _assert_same(pcu.closest_points_on_mesh(q, v, f), want, "numpy")
    _assert_same(pcu.closest_points_on_mesh(*_torch(q, v, f.astype(np.int32))), want, "torch")


@pytest.mark.parametrize("T", DTYPES)
def test_unreferenced_vertices_are_ignored(pcu, T):
    v, f = mc.bunny(T)
    q = mc.query_sets(v, f, 200, T, seed=41)["box"]
    v2 = np.concatenate([q[:100], v, q[100:]])                             # every query IS an unreferenced vertex
    f2 = f + 100
    want = _brute(q, v2, f2)
    assert want[0].min() > 0
    _assert_same(pcu.closest_points_on_mesh(q, v2, f2), want, "numpy")
    _assert_same(pcu.closest_points_on_mesh(*_torch(q, v2, f2)), want, "torch")


@pytest.mark.parametrize("T", DTYPES)
def test_degenerate_faces_mixed_in(pcu, T):
    v, f = mc.bunny(T)
    rng = np.random.default_rng(9)
    v = np.concatenate([v, np.array([[0.0625, 0.125, 0.03125], [0.125, 0.1875, 0.0625], [0.1875, 0.25, 0.09375],
                                     [0.25, 0.5, 0.125], [0.5, 0.75, 0.25], [1.0, 1.25, 0.5]], dtype=T)])      # collinear: ratio 2, ratio 3
    n = len(v)
    extra = [np.array([[n - 6, n - 5, n - 4], [n - 4, n - 6, n - 5], [n - 3, n - 2, n - 1], [n - 1, n - 3, n - 2]], dtype=np.int64)]
    for _ in range(40):
        i, j = rng.choice(len(v), 2, replace=False)
        extra.append(mc.degenerate_faces(int(i), int(j)))
    f2 = np.concatenate([f] + extra)
    f2 = f2[rng.permutation(len(f2))]
    q = np.concatenate([a for a in mc.query_sets(v, f2, 150, T, seed=51).values()])
    want = _brute(q, v, f2)
    assert not np.isnan(want[0]).any()
    _assert_same(pcu.closest_points_on_mesh(q, v, f2), want, "numpy")
    _assert_same(pcu.closest_points_on_mesh(*_torch(q, v, f2)), want, "torch")


def test_zero_rows_one_row_and_device_side_checks(pcu):
    import torch
    v, f = mc.bunny(np.float32)
    for T in DTYPES:
        d, fi, bc = pcu.closest_points_on_mesh(np.zeros((0, 3), T), v.astype(T), f.astype(np.uint32))
        assert d.shape == (0,) and fi.shape == (0,) and bc.shape == (0, 3) and d.dtype == T and bc.dtype == T and fi.dtype == np.uint32
        d, fi, bc = pcu.closest_points_on_mesh(*_torch(np.zeros((0, 3), T), v.astype(T), f))
        assert d.shape == (0,) and fi.shape == (0,) and bc.shape == (0, 3) and fi.dtype == torch.int64 and d.is_cuda
    q = mc.query_sets(v, f, 4, np.float32)["box"]
    want = _brute(q, v, f)
    d, fi, bc = pcu.closest_points_on_mesh(q[:1], v, f)                    # one row: singleton dimensions are squeezed
    assert d.shape == () and fi.shape == () and bc.shape == (3,)
    assert _bits(d.reshape(1))[0] == _bits(want[0])[0] and int(fi) == want[1][0] and np.array_equal(_bits(bc), _bits(want[2][0]))
    tq, tv, tf = _torch(q, v, f)
    for bad in (float("nan"), float("inf")):
        tb = tq.clone(); tb[2, 0] = bad
        with pytest.raises(ValueError, match="p must not contain NaN or infinite coordinates"):
            pcu.closest_points_on_mesh(tb, tv, tf)
        tb = tv.clone(); tb[5, 1] = bad
        with pytest.raises(ValueError, match="v must not contain NaN or infinite coordinates"):
            pcu.closest_points_on_mesh(tq, tb, tf)
        with pytest.raises(ValueError, match="v must not contain NaN or infinite coordinates"):
            pcu.MeshIndex(tb, tf)
    for val in (len(v), -1):
        tb = tf.clone(); tb[7, 2] = val
        with pytest.raises(ValueError, match=rf"found a face index outside \[0, {len(v)}\)"):
            pcu.closest_points_on_mesh(tq, tv, tb)
        with pytest.raises(ValueError, match=rf"found a face index outside \[0, {len(v)}\)"):
            pcu.closest_points_on_mesh(tq, tv, tb.to(torch.int32))
    with pytest.raises(ValueError, match="same device"):
        pcu.closest_points_on_mesh(tq, tv, f)                              # numpy faces beside tensors
    _assert_same(pcu.closest_points_on_mesh(tq, tv, tf), want, "after the refused calls")


# ---------------------------------------------------------------------------------------------------- 2. MeshIndex
@pytest.mark.parametrize("T", DTYPES)
def test_mesh_index_same_rows_as_the_one_shot_call(pcu, T):
    v, f = mc.bunny(T)
    sets = mc.query_sets(v, f, 2000, T, seed=61)
    q1, q2 = np.concatenate([sets["box"], sets["far"]]), np.concatenate([sets["surface"], sets["vertex"]])[:3000]
    one1, one2 = pcu.closest_points_on_mesh(q1, v, f), pcu.closest_points_on_mesh(q2, v, f)
    with pcu.MeshIndex(v, f.astype(np.int32)) as mesh:
        assert mesh.num_faces == len(f)
        a, b = mesh.closest_points(q1), mesh.closest_points(q2)
        assert a[1].dtype == np.int32
        _assert_same(a, one1, "first query set"); _assert_same(b, one2, "second query set")
        _assert_same(mesh.closest_points(q1), one1, "first query set again")
        _assert_same(mesh.closest_points(_torch(q2)[0]), one2, "tensor queries")
        with pytest.raises(ValueError, match="Invalid scalar type"):
            mesh.closest_points(q1.astype(np.float64 if T == np.float32 else np.float32))
        mesh._device += 1                                                 # (an index of another GPU)
        with pytest.raises(ValueError, match="different devices"):
            mesh.closest_points(q1)
        mesh._device -= 1
    with pytest.raises(ValueError, match="closed"):
        mesh.closest_points(q1)
    tv, tf = _torch(v, f)
    mesh = pcu.MeshIndex(tv, tf)
    del tv, tf                                                            # (the mesh was copied)
    _assert_same(mesh.closest_points(_torch(q1)[0]), one1, "index built from tensors")
    mesh.close(); mesh.close()


def _assert_bits(got, want, what):
    """Three arrays of either operator, row for row: same shapes, dtypes and bits."""
    for k, (a, b) in enumerate(zip(got, want)):
        a, b = _to_numpy(a), _to_numpy(b)
        assert a.dtype == b.dtype and a.shape == b.shape, (what, k)
        same = a == b if a.dtype.kind in "iu" else _bits(a) == _bits(b)
        assert same.all(), (what, k, f"{int((~same).sum())} of {same.size} values differ")


@pytest.mark.parametrize("T", DTYPES)
def test_points_rays_points_on_one_mesh_index(pcu, T):
    """Both operators interleaved on one index (and one context): every call gives the rows of its one-shot call, the third those of the first."""
    v, f = mc.bunny(T)
    q = mc.query_sets(v, f, 2000, T, seed=67)["box"]
    o, d = rc.rays_box_to_surface(v, f, 2000, T, 68)                      # (test_gpu_rays' family "box")
    for kind, conv in (("host arrays", lambda *a: a), ("device tensors", _torch)):
        cv, cf, cq, co, cd = conv(v, f, q, o, d)
        one_p, one_r = pcu.closest_points_on_mesh(cq, cv, cf), pcu.ray_mesh_intersection(cv, cf, co, cd)
        assert (_to_numpy(one_r[0]) >= 0).sum() >= 1000
        with pcu.MeshIndex(cv, cf) as mesh:
            first, rays, third = mesh.closest_points(cq), mesh.intersect_rays(co, cd), mesh.closest_points(cq)
        _assert_bits(first, one_p, (kind, "points")); _assert_bits(rays, one_r, (kind, "rays")); _assert_bits(third, one_p, (kind, "points again"))
        _assert_bits(third, first, (kind, "third against first"))


# ---------------------------------------------------------------------------------------------------- 3. size
@pytest.mark.parametrize("T", DTYPES)
@pytest.mark.parametrize("mesh", ["bunny", "sphere"])
def test_a_million_surface_samples_and_a_million_box_queries(pcu, big_sphere, mesh, T):
    import torch
    v, f = mc.bunny(T) if mesh == "bunny" else big_sphere[T]
    rng = np.random.default_rng(77)
    v64 = v.astype(np.float64)
    lo, hi = v64.min(0), v64.max(0)
    box = ((lo + hi) / 2 + (rng.random((1_000_000, 3)) - 0.5) * 2 * (hi - lo)).astype(T)
    surf = mc.surface_samples(v, f, 1_000_000, seed=78).astype(T)
    eps = np.finfo(T).eps
    ref_v = np.ascontiguousarray(v[np.unique(f)])
    tv, tf = _torch(v, f)
    for name, q in (("surface", surf), ("box", box)):
        scale = max(float(np.abs(v).max()), float(np.abs(q).max()))
        d, fi, bc = (_to_numpy(x) for x in pcu.closest_points_on_mesh(_torch(q)[0], tv, tf))
        assert not np.isnan(d).any() and fi.min() >= 0 and fi.max() < len(f)
        sub = np.sort(rng.choice(len(q), 20_000, replace=False))
        want = _brute(q[sub], v, f, None if mesh == "bunny" else _candidates(q[sub], v, f))
        _assert_same((d[sub], fi[sub], bc[sub]), want, (mesh, name, "subsample"))
        d_vertex, _ = pcu.k_nearest_neighbors(q, ref_v, 1)
        over = float(np.max(d.astype(np.float64) - d_vertex.astype(np.float64)) / (eps * scale))
        rep = float(np.max(np.abs(mc.reproduce64(q, v, f, fi, bc) - d.astype(np.float64))) / (eps * scale))
        print(f"{mesh} {np.dtype(T).name} {name}: d - d_vertex at most {over:.3f} eps*scale, d reproduced from (fi, bc) within {rep:.3f} eps*scale; "
              f"{pcu.last_stats()}")
        assert over <= B and rep <= B, (mesh, name, over, rep)
        assert np.abs(bc.astype(np.float64).sum(1) - 1).max() <= 2 * eps and bc.min() >= -eps


# ---------------------------------------------------------------------------------------------------- 4. run to run
def test_same_call_twice_and_after_an_unrelated_call(pcu):
    v, f = mc.bunny(np.float32)
    q = np.concatenate(list(mc.query_sets(v, f, 50_000, np.float32, seed=91).values()))
    first = pcu.closest_points_on_mesh(q, v, f)
    _assert_same(pcu.closest_points_on_mesh(q, v, f), first, "second call")
    pcu.chamfer_distance(q[:70_000], v)
    pcu.k_nearest_neighbors(q, v, 3)
    _assert_same(pcu.closest_points_on_mesh(q, v, f), first, "after unrelated calls")
    _assert_same(pcu.closest_points_on_mesh(*_torch(q, v, f)), first, "device-resident")


# ---------------------------------------------------------------------------------------------------- 5. cancellation
def _cancel_until(pcu, done, started):
    started.wait()
    for _ in range(2000):
        time.sleep(0.003)
        pcu.cancel()
        if done.is_set():
            break


def test_cancel_ends_a_large_call_and_the_next_one_is_correct(pcu, big_sphere):
    v, f = big_sphere[np.float32]
    q = (np.random.default_rng(5).random((4_000_000, 3), dtype=np.float32) - 0.5) * 4
    started, done = threading.Event(), threading.Event()
    th = threading.Thread(target=_cancel_until, args=(pcu, done, started)); th.start()
    t0 = time.perf_counter()
    try:
        with pytest.raises(KeyboardInterrupt):
            started.set()
            for _ in range(400):
                pcu.closest_points_on_mesh(q, v, f)
    finally:
        done.set(); th.join()
    assert time.perf_counter() - t0 < 60.0
    bv, bf = mc.bunny(np.float32)
    bq = mc.query_sets(bv, bf, 500, np.float32, seed=95)["box"]
    _assert_same(pcu.closest_points_on_mesh(bq, bv, bf), _brute(bq, bv, bf), "after the abandoned call")


def test_cancelled_mesh_index_build_leaves_no_device_memory(pcu, big_sphere):
    import torch
    from point_cloud_utils_amd import _lib
    v, f = big_sphere[np.float64]
    tv, tf = _torch(v, f)
    L, ctx = _lib.lib(), _lib.ctx(tv.device.index or 0)
    pcu.MeshIndex(tv, tf).close()                                          # (the context's workspace has its size now)
    torch.cuda.synchronize(); gc.collect()
    free0, ws0 = torch.cuda.mem_get_info()[0], int(L.pcu_hip_ctx_workspace_bytes(ctx))
    started, done = threading.Event(), threading.Event()
    th = threading.Thread(target=_cancel_until, args=(pcu, done, started)); th.start()
    cancelled = 0
    try:
        started.set()
        for _ in range(300):
            try:
                pcu.MeshIndex(tv, tf).close()
            except KeyboardInterrupt:
                cancelled += 1
                if cancelled >= 5:
                    break
    finally:
        done.set(); th.join()
    assert cancelled >= 1, "no build was cancelled"
    torch.cuda.synchronize(); gc.collect()
    free1, ws1 = torch.cuda.mem_get_info()[0], int(L.pcu_hip_ctx_workspace_bytes(ctx))
    index_bytes = len(f) * 9 * 8                                           # the corners alone: a leaked index is larger than this
    print(f"cancelled builds: {cancelled}; free memory {free0} -> {free1}, workspace {ws0} -> {ws1}")
    assert free0 - free1 <= max(ws1 - ws0, 0) + (4 << 20) and index_bytes > (8 << 20)
    bq = mc.query_sets(v, f, 300, np.float64, seed=96)["box"]
    with pcu.MeshIndex(tv, tf) as mesh:
        _assert_same(mesh.closest_points(bq), _brute(bq, v, f, _candidates(bq, v, f)), "index built after the cancelled ones")
