"""The four objects that own an index on the GPU -- DatasetIndex, MeshIndex, PointCloudWindingIndex, RaySurfelIntersector -- held to their
one-shot calls and to their common life cycle (-m gpu). The sizes are the smallest at which the frame of an index can go wrong: one element,
one full leaf, one element more (the leaf table goes from 1 to 2 entries), two leaves and one, and 257 (more than one block of 256). The
leaves are 4 faces, 8 points and 1 surfel; the dataset index has no leaves: 1, 2 and 257 points."""
import ctypes

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
DTYPES = [np.float32, np.float64]
SIZES = {"dataset": (1, 2, 257), "mesh": (1, 4, 5, 9, 257), "cloud": (1, 8, 9, 17, 257), "surfel": (1, 2, 3, 257)}
KINDS = list(SIZES)
NQ = 37


@pytest.fixture(scope="module")
def pcu():
    import point_cloud_utils_amd as m
    from point_cloud_utils_amd import _lib
    assert _lib.device_count() > 0, "no GPU visible: the gfx950 path has no CPU fallback"
    return m


def _np(x):
    return x.detach().cpu().numpy() if hasattr(x, "detach") else np.asarray(x)


def _same(a, b):
    """Equal bytes, dtypes and shapes, result by result."""
    a, b = (a if isinstance(a, tuple) else (a,)), (b if isinstance(b, tuple) else (b,))
    assert len(a) == len(b)
    for x, y in zip(a, b):
        x, y = np.ascontiguousarray(_np(x)), np.ascontiguousarray(_np(y))
        assert x.dtype == y.dtype and x.shape == y.shape and x.tobytes() == y.tobytes()


def _torch(*arrays):
    import torch
    return tuple(torch.from_numpy(np.ascontiguousarray(a)).cuda() if isinstance(a, np.ndarray) else a for a in arrays)


def _has_array(args):
    return any(isinstance(a, np.ndarray) for a in args)


class Kind:
    """One handle kind at one size and dtype: what it is built from, its queries, the one-shot twin of each query method."""

    def __init__(self, pcu, kind, n, dtype):
        rng = np.random.default_rng(1000 * n + len(kind))
        self.kind, self.n = kind, n
        q = (rng.random((NQ, 3)) * 1.5 - 0.25).astype(dtype)
        d = rng.standard_normal((NQ, 3)).astype(dtype)
        pts = rng.random((n, 3)).astype(dtype)
        nrm = rng.standard_normal((n, 3)).astype(dtype)
        if kind == "dataset":
            self.built, self.make = (pts,), pcu.DatasetIndex
            self.calls = [("k_nearest_neighbors", (q, 1), lambda b, a: pcu.k_nearest_neighbors(a[0], b[0], 1)),
                          ("k_nearest_neighbors", (q, 3), lambda b, a: pcu.k_nearest_neighbors(a[0], b[0], 3)),
                          ("radius_search", (q, 0.5), lambda b, a: pcu.radius_search(a[0], b[0], 0.5)),
                          ("radius_search", (q, 0.5, True, True), lambda b, a: pcu.radius_search(a[0], b[0], 0.5, squared_distances=True, sort_results=True)),
                          ("radius_count", (q, 0.5), lambda b, a: pcu.radius_count(a[0], b[0], 0.5)),
                          ("farthest_point_sample", (min(n, 64), 0, True),      # no array argument: the result is of the kind the index was built from
                           lambda b, a: pcu.downsample_point_cloud_farthest_point(b[0], min(n, 64), 0, return_distances=True))]
        elif kind == "mesh":
            v = rng.random((n + 2, 3)).astype(dtype)
            f = np.stack([np.arange(n), np.arange(n) + 1, np.arange(n) + 2], axis=1).astype(np.int32)       # a strip of n faces
            self.built, self.make = (v, f), lambda v, f: pcu.MeshIndex(v, f, winding_numbers=True)
            self.calls = [("closest_points", (q,), lambda b, a: pcu.closest_points_on_mesh(a[0], *b)),
                          ("intersect_rays", (q, d), lambda b, a: pcu.ray_mesh_intersection(*b, *a)),
                          ("intersect_rays", (q[0], d), lambda b, a: pcu.ray_mesh_intersection(*b, *a)),
                          ("winding_number", (q,), lambda b, a: pcu.triangle_soup_fast_winding_number(*b, a[0])),
                          ("signed_distance", (q,), lambda b, a: pcu.signed_distance_to_mesh(a[0], *b))]
        elif kind == "cloud":
            self.built, self.make = (pts, nrm, rng.random(n).astype(dtype)), pcu.PointCloudWindingIndex
            self.calls = [("winding_number", (q,), lambda b, a: pcu.point_cloud_fast_winding_number(*b, a[0]))]
        else:
            r = (0.2 + 0.3 * rng.random(n)).astype(dtype)
            self.built, self.make = (pts, nrm, r), lambda p, n_, r_: pcu.RaySurfelIntersector(p, n_, r_, 5)
            self.calls = [("intersect_rays", (q, d), lambda b, a: pcu.ray_surfel_intersection(b[0], b[1], a[0], a[1], b[2], 5))]


CASES = [(k, n) for k in KINDS for n in SIZES[k]]


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "f64"])
@pytest.mark.parametrize("kind,n", CASES, ids=[f"{k}-{n}" for k, n in CASES])
def test_a_handle_answers_as_the_one_shot_call_does(pcu, kind, n, dtype):
    """Byte for byte, for numpy and for tensors, and with the handle built from the one and asked with the other. The C ABI agrees with the
    count where it has a size function."""
    from point_cloud_utils_amd import _lib
    c = Kind(pcu, kind, n, dtype)
    t_built = _torch(*c.built)
    with c.make(*c.built) as from_numpy, c.make(*t_built) as from_torch:
        for method, args, one_shot in c.calls:
            want = one_shot(c.built, args)
            t_args = _torch(*args)
            _same(one_shot(t_built, t_args), want)
            for h in (from_numpy, from_torch):
                _same(getattr(h, method)(*args), want)
                got = getattr(h, method)(*t_args)
                tensors_out = _has_array(args) or h is from_torch               # tensors in, tensors out; without an array: what the handle was built from
                assert all(hasattr(x, "detach") == tensors_out for x in (got if isinstance(got, tuple) else (got,)))
                _same(got, want)
        size = {"dataset": "pcu_hip_index_size", "mesh": "pcu_hip_mesh_index_size", "surfel": "pcu_hip_surfel_index_size"}.get(kind)
        if size:
            assert getattr(_lib.lib(), size)(from_numpy._h) == n and getattr(_lib.lib(), size)(from_torch._h) == n


NOUN = {"dataset": "index", "mesh": "mesh index", "cloud": "point cloud winding index", "surfel": "surfel index"}


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "f64"])
@pytest.mark.parametrize("kind", KINDS)
def test_life_cycle_and_closed_use(pcu, kind, dtype):
    """`with`, then close() twice, then __del__; every query method of a closed handle refuses with its text, and so does the handle's own
    device check when the handle says it lives elsewhere."""
    c = Kind(pcu, kind, 9, dtype)
    with c.make(*c.built) as h:
        assert h._h is not None
        first = [getattr(h, m)(*a) for m, a, _ in c.calls]
        if kind != "dataset":                                                   # (the dataset index compares devices for tensors only)
            real, h._device = h._device, h._device + 1
            for method, args, _ in c.calls:
                with pytest.raises(ValueError) as e:
                    getattr(h, method)(*args)
                assert str(e.value) == f"{'rays' if method == 'intersect_rays' else 'query points'} and {NOUN[kind]} live on different devices"
            h._device = real
        real, h._device = h._device, h._device + 1
        for method, args, _ in c.calls:
            if not _has_array(args):                                            # (no tensor comes with the call: nothing to compare)
                continue
            with pytest.raises(ValueError) as e:
                getattr(h, method)(*_torch(*args))
            what = "query tensor" if kind == "dataset" else "rays" if method == "intersect_rays" else "query points"
            assert str(e.value) == f"{what} and {NOUN[kind]} live on different devices"
        h._device = real
        for (m, a, _), want in zip(c.calls, first):
            _same(getattr(h, m)(*a), want)
    assert h._h is None
    h.close()
    h.close()
    for method, args, _ in c.calls:
        for given in (args, _torch(*args)):
            with pytest.raises(ValueError) as e:
                getattr(h, method)(*given)
            assert str(e.value) == f"the {NOUN[kind]} has been closed"
    h.__del__()
    assert h._h is None


def _abi_queries(L, kind, suf, ctx, handle, n=3):
    """The query entry points of a family for the scalar suffix `suf`, as calls through the C ABI on `n` rows of zeros."""
    T = np.float32 if suf == "f32" else np.float64
    arrays = np.zeros((n, 3), T), np.zeros(n, T), np.zeros((n, 3), T), np.zeros(n + 1, np.int64), np.zeros(1, np.int64)
    q, val, bc, idx, total = (a.ctypes.data for a in arrays)

    def fn(name, *args):
        return lambda keep=arrays: getattr(L, f"pcu_hip_{name}_{suf}")(ctx, handle, *args, 0, None, None)
    if kind == "dataset":
        return [fn("index_knn", q, n, 1, 10, val, idx), fn("index_radius_search", q, n, 0.5, 1, idx, total), fn("index_radius_count", q, n, 0.5, idx),
                fn("index_fps", 1, 0, idx, val, None)]
    if kind == "mesh":
        return [fn("mesh_index_closest", q, n, val, idx, bc), fn("mesh_index_rays", q, n, q, n, 0.0, 1.0, idx, bc, val),
                fn("mesh_index_winding", q, n, 2.0, val), fn("mesh_index_signed_distance", q, n, -1.0, 1.0, 2.0, val, idx, bc)]
    if kind == "cloud":
        return [fn("pc_winding_index_query", q, n, 2.0, val)]
    return [fn("surfel_index_rays", q, n, q, n, 0.0, 1.0, idx, val)]


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "f64"])
@pytest.mark.parametrize("kind", KINDS)
def test_the_c_abi_refuses_the_other_scalar_type_and_a_null_handle(pcu, kind, dtype):
    from point_cloud_utils_amd import _lib
    L = _lib.lib()
    other = "f64" if dtype == np.float32 else "f32"
    c = Kind(pcu, kind, 9, dtype)
    with c.make(*c.built) as h:
        first = [getattr(h, m)(*a) for m, a, _ in c.calls]
        want = "the index was built for the other floating-point type" if kind == "dataset" else f"the {NOUN[kind]} was built for the other scalar type"
        for call in _abi_queries(L, kind, other, _lib.ctx(), h._h):
            assert call() == _lib.ERR_INVALID and _lib.last_error() == want
        for (m, a, _), w in zip(c.calls, first):                                # the refusals left the handle and the context as they were
            _same(getattr(h, m)(*a), w)
    null = "null index" if kind == "dataset" else f"null context / {NOUN[kind]}"
    for suf in ("f32", "f64"):
        for call in _abi_queries(L, kind, suf, _lib.ctx(), None):
            assert call() == _lib.ERR_INVALID and _lib.last_error() == null
    for name in ("pcu_hip_index_destroy", "pcu_hip_mesh_index_destroy", "pcu_hip_pc_winding_index_destroy", "pcu_hip_surfel_index_destroy"):
        assert getattr(L, name)(None) is None
    for name in ("pcu_hip_index_size", "pcu_hip_mesh_index_size", "pcu_hip_surfel_index_size"):
        assert getattr(L, name)(None) == 0


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "f64"])
def test_a_refused_create_leaves_no_handle_and_the_next_one_works(pcu, dtype):
    """Refused on the device (tensors: a coordinate that is not finite, a face index out of range) and on the host (subdivs = 3): the handle
    pointer of the C ABI stays null, the Python object has no handle, and a create on the same context afterwards answers as the one-shot
    call does."""
    from point_cloud_utils_amd import _lib
    L, ctx = _lib.lib(), _lib.ctx()
    suf = "f32" if dtype == np.float32 else "f64"
    mesh, cloud, surfel, data = (Kind(pcu, k, 9, dtype) for k in ("mesh", "cloud", "surfel", "dataset"))
    on_dev = _lib.PTRS_ON_DEVICE

    def refused(name, text, *args):
        h = ctypes.c_void_p(0xdead)                                             # (the create clears it before it looks at anything else)
        assert getattr(L, f"pcu_hip_{name}_create_{suf}")(ctx, *args, ctypes.byref(h)) == _lib.ERR_INVALID
        assert _lib.last_error() == text and h.value is None

    bad_p = data.built[0].copy()
    bad_p[4, 1] = np.nan
    tp, = _torch(bad_p)
    h = ctypes.c_void_p(0xdead)
    assert getattr(L, "pcu_hip_index_create_" + suf)(ctx, tp.data_ptr(), 9, 1, on_dev, None, ctypes.byref(h)) == _lib.ERR_INVALID and h.value is None
    with pytest.raises(ValueError):
        pcu.DatasetIndex(tp)

    v, f = mesh.built
    bad_v = v.copy()
    bad_v[3, 0] = np.inf
    bad_f = f.copy()
    bad_f[5, 2] = len(v)
    tv, tf, tbv, tbf = _torch(v, f, bad_v, bad_f)
    refused("mesh_index", "v must not contain NaN or infinite coordinates", tbv.data_ptr(), len(v), tf.data_ptr(), 9, 0, on_dev, None)
    refused("mesh_index", f"f must hold row indices of v: found a face index outside [0, {len(v)})", tv.data_ptr(), len(v), tbf.data_ptr(), 9, 0, on_dev, None)
    for args, text in (((tbv, tf), "v must not contain NaN or infinite coordinates"),
                       ((tv, tbf), f"f must hold row indices of v: found a face index outside [0, {len(v)})")):
        with pytest.raises(ValueError) as e:
            pcu.MeshIndex(*args)
        assert str(e.value) == text

    p, n, a = cloud.built
    bad_n = n.copy()
    bad_n[8, 2] = -np.inf
    tcp, tbn, ta = _torch(p, bad_n, a)
    refused("pc_winding_index", "n must not contain NaN or infinite coordinates", tcp.data_ptr(), tbn.data_ptr(), ta.data_ptr(), 9, on_dev, None)
    with pytest.raises(ValueError) as e:
        pcu.PointCloudWindingIndex(tcp, tbn, ta)
    assert str(e.value) == "n must not contain NaN or infinite coordinates"

    p, n, r = surfel.built
    tsp, tsn, tr = _torch(p, n, r)
    refused("surfel_index", "Invalid geometry_subdivisions_1 is less than or equal to 4.", tsp.data_ptr(), tsn.data_ptr(), tr.data_ptr(), 9, 3, on_dev, None)
    with pytest.raises(ValueError) as e:
        pcu.RaySurfelIntersector(p, n, r, 3)
    assert str(e.value) == "Invalid geometry_subdivisions_1 is less than or equal to 4."

    for c in (data, mesh, cloud, surfel):                                       # the same context, after the refusals
        with c.make(*_torch(*c.built)) as h:
            for method, args, one_shot in c.calls:
                _same(getattr(h, method)(*args), one_shot(c.built, args))
