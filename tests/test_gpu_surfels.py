"""ray_surfel_intersection, RaySurfelIntersector and pointcloud_surfel_geometry on the GPU (-m gpu): every row bit-equal to the contract
restated in tests/surfel_contract.py -- pid, the bits of t, the bits of v, f -- in both dtypes, from numpy arrays and from device-resident
tensors; the fan walk against ray_mesh_intersection on the materialised geometry where brute force is too slow; the build-once class against
the one-shot call (the reference's own test body); every refusal of the contract."""
import os
import re

import numpy as np
import pytest

import ray_contract as rc
import surfel_contract as sc

pytestmark = pytest.mark.gpu
DTYPES = [np.float32, np.float64]
SUBDIVS = [4, 7, 11]
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LEAF = int(re.search(r"constexpr int kSurfelLeaf = (\d+);", open(os.path.join(ROOT, "point_cloud_utils_amd", "csrc", "surfel.h")).read()).group(1))


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


def _torch(*arrays):
    import torch
    return tuple(torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in arrays)


def _assert_rows(got, want, what):
    """Every row: pid (int32) and the bits of t."""
    pid, t = (_to_numpy(x) for x in got)
    pid0, t0 = want
    assert pid.dtype == np.int32 and t.dtype == t0.dtype, (what, pid.dtype, t.dtype)
    if len(t0) == 1:
        assert pid.shape == () and t.shape == (), what                      # (one ray: squeezed, as ray_mesh_intersection's rows are)
    pid, t = pid.reshape(-1), t.reshape(-1)
    assert pid.shape == pid0.shape and t.shape == t0.shape, what
    bad = np.flatnonzero((pid != pid0) | (_bits(t) != _bits(t0)))
    assert bad.size == 0, (what, f"{bad.size} of {len(t0)} rows differ", bad[:5], t[bad[:5]], t0[bad[:5]], pid[bad[:5]], pid0[bad[:5]])


def _cloud(N, T, seed):
    """N points on the unit sphere with outward normals of any length and radii of 1.5 spacings (neighbouring surfels overlap), and among
    them, where there is room: a zero normal, +-y and near-+-y normals, a zero and a negative radius, and three copies of one point."""
    rng = np.random.default_rng(seed)
    u = rng.normal(size=(N, 3)); u /= np.linalg.norm(u, axis=1, keepdims=True)
    p = u.copy()
    n = u * rng.uniform(0.05, 30.0, size=(N, 1))
    r = np.full(N, min(0.6, 1.5 * np.sqrt(4 * np.pi / N))) * rng.uniform(0.8, 1.2, size=N)
    if N >= 16:
        n[3] = 0.0
        p[4], n[4] = [0, 1, 0], [0, 2, 0]
        p[5], n[5] = [0, -1, 0], [0, -0.5, 0]
        p[6], n[6] = p[4], [2e-3, 1, -1e-3]                                  # within 1e-5 of +y: the branch
        p[7], n[7] = p[5], [6e-3, -1, 2e-3]                                  # just outside it
        r[8] = 0.0
        r[9] = -r[9]
        p[2] *= 1.25                                                         # (above the sphere: nothing hides it from outside)
        p[10] = p[11] = p[2]; n[10] = n[11] = n[2]; r[10] = r[11] = r[2]    # duplicates: the lowest pid wins
    return np.ascontiguousarray(p.astype(T)), np.ascontiguousarray(n.astype(T)), np.ascontiguousarray(r.astype(T))


def _origins(rng, k, lo=2.0, hi=4.0):
    u = rng.normal(size=(k, 3)); u /= np.linalg.norm(u, axis=1, keepdims=True)
    return u * rng.uniform(lo, hi, size=(k, 1))


def _families(p, n, r, subdivs, T, seed, sizes):
    """The ray families of one cloud: name -> (o, d, near, far). `sizes` = (small, odd, large) ray counts."""
    rng = np.random.default_rng(seed)
    N = len(p)
    small, odd, large = sizes
    v, _ = sc.geometry(p, n, r, subdivs)
    v64 = v.astype(np.float64).reshape(N, subdivs + 1, 3)
    rim, ctr = v64[:, :subdivs], v64[:, subdivs]
    fams = {}

    def aimed(x, near=0.0, far=np.inf):
        # origins on the side the point faces (the far side of the sphere would hide it), a little off its axis
        k = len(x)
        o = x * rng.uniform(2.0, 4.0, size=(k, 1)) + 0.3 * rng.normal(size=(k, 3)) if N > 2 else _origins(rng, k)
        o = o.astype(T)
        return np.ascontiguousarray(o), np.ascontiguousarray((x - o.astype(np.float64)).astype(T)), near, far

    i = rng.integers(0, N, small)
    if N >= 16 and small >= 30:
        i[:30] = np.tile([2, 10, 11], 10)                                   # the three copies of one point
    fams["centres"] = aimed(ctr[i])
    i, j = rng.integers(0, N, odd), rng.integers(0, subdivs, odd)
    fams["rim vertices"] = aimed(rim[i, j])
    i, j, s = rng.integers(0, N, large), rng.integers(0, subdivs, large), rng.random(large)[:, None]
    half = large // 2
    spokes = ctr[i[:half]] + s[:half] * (rim[i[:half], j[:half]] - ctr[i[:half]])
    edges = rim[i[half:], j[half:]] + s[half:] * (rim[i[half:], (j[half:] + 1) % subdivs] - rim[i[half:], j[half:]])
    fams["spokes and rim edges"] = aimed(np.concatenate([spokes, edges]))
    i = rng.integers(0, N, large)
    fams["near surfels"] = aimed(ctr[i] + np.abs(r.astype(np.float64))[i, None] * 1.2 * rng.normal(size=(large, 3)))
    one = np.array([0.9, -2.7, 1.3]).astype(T)
    fams["one origin"] = (one, np.ascontiguousarray((ctr[rng.integers(0, N, odd)] - one.astype(np.float64)).astype(T)), 0.0, np.inf)
    fams["inside"] = (np.ascontiguousarray((0.5 * (rng.random((small, 3)) - 0.5)).astype(T)), np.ascontiguousarray(rng.normal(size=(small, 3)).astype(T)), 0.0, np.inf)
    skew = rng.normal(size=(small, 3)); skew /= np.linalg.norm(skew, axis=1, keepdims=True)
    fams["off the box"] = (np.ascontiguousarray((6.0 * skew).astype(T)), np.ascontiguousarray(np.cross(skew, rng.normal(size=(small, 3))).astype(T)), 0.0, np.inf)
    # windows: origins outside along directions through the cloud; d has length ~1, the first surfel is met at t ~ |o| - 1, the far side at ~ |o| + 1
    o = _origins(rng, large, 2.5, 3.0)
    d = -o / np.linalg.norm(o, axis=1, keepdims=True) + 0.15 * rng.normal(size=(large, 3))
    fams["near window"] = (np.ascontiguousarray(o.astype(T)), np.ascontiguousarray(d.astype(T)), 2.6, np.inf)
    fams["far window"] = (fams["near window"][0], fams["near window"][1], 0.5, 2.1)
    return fams


@pytest.fixture(scope="module")
def sphere_cases():
    """Per dtype: the 300-point cloud, subdivs 7, its families and the contract's answers (computed once)."""
    out = {}
    for T in DTYPES:
        p, n, r = _cloud(300, T, seed=41)
        fams = _families(p, n, r, 7, T, seed=42, sizes=(255, 257, 2000))
        fams["no window"] = fams["near window"][:2] + (0.0, np.inf)
        out[T] = (p, n, r, {k: (a, sc.hit(p, n, r, 7, *a)) for k, a in fams.items()})
    return out


# ---------------------------------------------------------------------------------------------------- 1. geometry
@pytest.mark.parametrize("T", DTYPES)
@pytest.mark.parametrize("N", [1, 2, 257])
def test_geometry_equals_the_contract(pcu, N, T):
    other = np.float64 if T == np.float32 else np.float32
    p, n, r = _cloud(N, T, seed=N)
    if N == 2:
        n[0] = 0.0; r[1] = -r[1]
    forms = {"array": r, "list": [float(x) for x in r], "column": r.reshape(N, 1), "other dtype": r.astype(other), "scalar": 0.25, "zero": 0.0, "negative": -0.5}
    for subdivs in SUBDIVS:
        for name, rr in forms.items():
            if name not in ("array", "scalar") and subdivs != 7:
                continue
            v0, f0 = sc.geometry(p, n, sc.radii(rr, N, T), subdivs)
            v, f = pcu.pointcloud_surfel_geometry(p, n, rr, subdivs)
            assert v.dtype == T and f.dtype == np.int32 and v.shape == v0.shape and f.shape == f0.shape, (name, subdivs)
            assert np.array_equal(_bits(v), _bits(v0)) and np.array_equal(f, f0), (name, subdivs, np.flatnonzero((_bits(v) != _bits(v0)).any(axis=1))[:5])
            tr = rr if name in ("scalar", "zero", "negative", "list") else _torch(np.asarray(rr))[0]
            tv, tf = pcu.pointcloud_surfel_geometry(*_torch(p, n), tr, subdivs)
            assert tv.is_cuda and tf.is_cuda
            assert np.array_equal(_bits(_to_numpy(tv)), _bits(v0)) and np.array_equal(_to_numpy(tf), f0) and _to_numpy(tf).dtype == np.int32, (name, subdivs, "torch")
    assert np.array_equal(_bits(pcu.pointcloud_surfel_geometry(p, n)[0]), _bits(sc.geometry(p, n, sc.radii(0.1, N, T), 7)[0])), "the defaults: r = 0.1, subdivs = 7"


# ---------------------------------------------------------------------------------------------------- 2. rays against the contract
@pytest.mark.parametrize("T", DTYPES)
@pytest.mark.parametrize("N", sorted({1, 2, max(LEAF - 1, 1), LEAF + 1}))
@pytest.mark.parametrize("subdivs", SUBDIVS)
def test_small_clouds(pcu, subdivs, N, T):
    """One leaf, and two leaves under one level: with padding leaves where the count is no power of two."""
    p, n, r = _cloud(N, T, seed=7 * N)
    p = (0.3 * p).astype(T)
    r = np.full(N, 0.5, dtype=T)
    fams = _families(p, n, r, subdivs, T, seed=N + subdivs, sizes=(1, 255, 400))
    hits = 0
    for name, a in fams.items():
        want = sc.hit(p, n, r, subdivs, *a)
        hits += int((want[0] >= 0).sum())
        if N == 1 and name in ("centres", "spokes and rim edges"):              # (the first half of that family: the spokes)
            assert (want[0][:200] == 0).all(), (name, "a ray through the centre or a spoke of one surfel cannot slip between its triangles")
        _assert_rows(pcu.ray_surfel_intersection(p, n, a[0], a[1], r, subdivs, a[2], a[3]), want, (name, "numpy"))
        got = pcu.ray_surfel_intersection(*_torch(p, n, a[0], a[1], r), subdivs, a[2], a[3])
        assert all(x.is_cuda for x in got)
        _assert_rows(got, want, (name, "torch"))
    assert hits >= 300


@pytest.mark.parametrize("T", DTYPES)
@pytest.mark.parametrize("how", ["numpy", "torch"])
def test_sphere_of_overlapping_surfels(pcu, sphere_cases, how, T):
    """300 points (several levels), every family: the nearest of several overlapping surfels, the lowest pid of duplicates."""
    p, n, r, fams = sphere_cases[T]
    for name, (a, want) in fams.items():
        pid0 = want[0]
        if name in ("centres", "rim vertices", "spokes and rim edges", "near surfels", "near window", "far window"):
            assert (pid0 >= 0).mean() > 0.5, (name, (pid0 >= 0).mean())
        if name == "off the box":
            assert (pid0 == -1).all()
        if name == "centres":
            assert (pid0[:30] == 2).sum() >= 25, "rays at the three copies of one point name the first"
        assert not np.isin(pid0, [3, 8, 10, 11]).any(), (name, "the zero normal, the zero radius and the later copies of a point are never returned")
        if how == "numpy":
            got = pcu.ray_surfel_intersection(p, n, a[0], a[1], r, 7, a[2], a[3])
        else:
            got = pcu.ray_surfel_intersection(*_torch(p, n, a[0], a[1], r), 7, a[2], a[3])
            assert all(x.is_cuda for x in got)
        _assert_rows(got, want, (name, how))
    full, near_w, far_w = (fams[k][1][1] for k in ("no window", "near window", "far window"))
    cut = full < 2.6                                                        # the near window cuts off the first surfel of these rays
    assert cut.sum() > 1000 and (near_w[cut] >= T(2.6)).all() and np.isfinite(near_w[cut]).sum() > 500, "a later surfel is returned instead"
    assert ((far_w >= T(0.5)) & (far_w <= T(2.1)) | np.isposinf(far_w)).all() and (np.isposinf(far_w) & np.isfinite(full)).sum() > 100


@pytest.mark.parametrize("T", DTYPES)
@pytest.mark.parametrize("subdivs", [4, 11])
def test_sphere_other_subdivisions(pcu, sphere_cases, subdivs, T):
    p, n, r, _ = sphere_cases[T]
    a = _families(p, n, r, subdivs, T, seed=50 + subdivs, sizes=(16, 16, 2000))["spokes and rim edges"]
    want = sc.hit(p, n, r, subdivs, *a)
    assert (want[0] >= 0).mean() > 0.9
    _assert_rows(pcu.ray_surfel_intersection(p, n, a[0], a[1], r, subdivs), want, "numpy")
    _assert_rows(pcu.ray_surfel_intersection(*_torch(p, n, a[0], a[1], r), subdivs), want, "torch")


# ---------------------------------------------------------------------------------------------------- 3. against the materialised mesh
@pytest.mark.parametrize("T", DTYPES)
def test_large_cloud_equals_the_mesh_path_on_its_geometry(pcu, T):
    """20,000 points, subdivs 7, 20,000 rays: ray_mesh_intersection (pinned to the ray contract by tests/test_gpu_rays.py) on the geometry
    pointcloud_surfel_geometry returns (pinned to the contract above), mapped by // subdivs."""
    N, subdivs = 20000, 7
    p, n, r = _cloud(N, T, seed=77)
    rng = np.random.default_rng(78)
    o = (3.0 * (rng.random((N, 3)) - 0.5) * 2.0).astype(T)
    d = (p[rng.permutation(N)].astype(np.float64) - o.astype(np.float64)).astype(T)
    tp, tn, tr, to, td = _torch(p, n, r, o, d)
    tv, tf = pcu.pointcloud_surfel_geometry(tp, tn, tr, subdivs)
    fid, _, t0 = pcu.ray_mesh_intersection(tv, tf, to, td)
    fid, t0 = _to_numpy(fid).astype(np.int64), _to_numpy(t0)
    want = (np.where(fid >= 0, fid // subdivs, -1).astype(np.int32), t0)
    assert (want[0] >= 0).mean() > 0.9 and len(np.unique(want[0])) > 5000
    _assert_rows(pcu.ray_surfel_intersection(tp, tn, to, td, tr, subdivs), want, "torch")
    _assert_rows(pcu.ray_surfel_intersection(p, n, o, d, r, subdivs), want, "numpy")


# ---------------------------------------------------------------------------------------------------- 4. the class
@pytest.mark.parametrize("T", DTYPES)
def test_intersector_equals_the_function_reference_test_body(pcu, T):
    """The reference's test_ray_surfel_intersection (tests/test_examples.py:610-628): a cube_twist cloud, r = 0.5, subdivs = 11, a 128 x 128
    grid of rays from one point, function against class -- here on bits, and the class queried twice with different windows."""
    v, f = rc.cube_twist(T)
    fi, bc = pcu.sample_mesh_random(v, f, 5000, random_seed=3)
    p = np.ascontiguousarray((v[f[fi]] * bc[:, :, None]).sum(1).astype(T))
    n = np.ascontiguousarray(pcu.estimate_mesh_face_normals(v, f)[fi])
    uv = np.stack([a.ravel() for a in np.mgrid[-1:1:128j, -1.:1.:128j]], axis=-1)
    d = np.concatenate([uv, np.ones([uv.shape[0], 1])], axis=-1)
    d = np.ascontiguousarray((d / np.linalg.norm(d, axis=-1, keepdims=True)).astype(T))
    o = np.ascontiguousarray(np.array([[2, 0, -7.0] for _ in range(d.shape[0])]).astype(T))
    pid1, t1 = pcu.ray_surfel_intersection(p, n, o, d, r=0.5, subdivs=11)
    assert pid1.dtype == np.int32 and t1.dtype == T and 0.02 < (pid1 >= 0).mean() < 0.9
    with pcu.RaySurfelIntersector(p, n, r=0.5, subdivs=11) as isector:
        assert isector.num_subdivs == 11 and isector.num_points == 5000
        _assert_rows(isector.intersect_rays(o, d), (pid1, t1), "class, first query")
        cut = float(np.median(t1[np.isfinite(t1)]))
        want = pcu.ray_surfel_intersection(p, n, o, d, 0.5, 11, cut, cut + 1.0)
        assert 0 < (want[0] >= 0).sum() and not np.array_equal(want[0], pid1)
        _assert_rows(isector.intersect_rays(o, d, ray_near=cut, ray_far=cut + 1.0), want, "class, second query with a window")
        _assert_rows(isector.intersect_rays(o[0], d), (pid1, t1), "class, one origin of shape (3,)")
        to, td = _torch(o, d)
        got = isector.intersect_rays(to, td)
        assert all(x.is_cuda for x in got)
        _assert_rows(got, (pid1, t1), "class built from numpy, queried with tensors")
    with pytest.raises(ValueError, match="the surfel index has been closed"):
        isector.intersect_rays(o, d)
    with pcu.RaySurfelIntersector(*_torch(p, n)) as dflt:                     # the defaults: r = 0.1, subdivs = 7
        _assert_rows(dflt.intersect_rays(o, d), pcu.ray_surfel_intersection(p, n, o, d, 0.1, 7), "defaults of the class")
    _assert_rows(pcu.ray_surfel_intersection(p, n, o, d), pcu.ray_surfel_intersection(p, n, o, d, 0.1, 4), "defaults of the function")


# ---------------------------------------------------------------------------------------------------- 5. refusals and empty inputs
@pytest.mark.parametrize("T", DTYPES)
@pytest.mark.parametrize("how", ["numpy", "torch"])
def test_refusals(pcu, how, T):
    other = np.float64 if T == np.float32 else np.float32
    big = np.finfo(T).max
    p, n, r = _cloud(20, T, seed=5)
    o = np.full((6, 3), 3.0, dtype=T); d = -np.ones((6, 3), dtype=T)
    dev = (lambda *a: _torch(*a)) if how == "torch" else (lambda *a: a)

    def calls(pp, nn, rr, oo=o, dd=d, near=0.0, far=np.inf, subdivs=7, rays_only=False):
        """The three entry points on the same cloud (the class is built and, where it builds, queried)."""
        tp, tn, to, td = dev(pp, nn, oo, dd)
        tr = dev(rr)[0] if isinstance(rr, np.ndarray) else rr
        out = [lambda: pcu.ray_surfel_intersection(tp, tn, to, td, tr, subdivs, near, far)]
        if not rays_only:
            out.append(lambda: pcu.pointcloud_surfel_geometry(tp, tn, tr, subdivs))
            out.append(lambda: pcu.RaySurfelIntersector(tp, tn, tr, subdivs))
        return out

    def bad(x, i, val):
        y = x.copy(); y.reshape(-1)[i] = val
        return y

    for val in (np.nan, np.inf, -np.inf):
        for fn in calls(bad(p, 7, val), n, r):
            with pytest.raises(ValueError, match="p must not contain NaN or infinite coordinates"):
                fn()
        for fn in calls(p, bad(n, 8, val), r):
            with pytest.raises(ValueError, match="n must not contain NaN or infinite coordinates"):
                fn()
        for fn in calls(p, n, bad(r, 3, val)):
            with pytest.raises(ValueError, match="r must not contain NaN or infinite values"):
                fn()
        for fn in calls(p, n, r, oo=bad(o, 4, val), rays_only=True):
            with pytest.raises(ValueError, match="ray_o must not contain NaN or infinite coordinates"):
                fn()
        for fn in calls(p, n, r, dd=bad(d, 4, val), rays_only=True):
            with pytest.raises(ValueError, match="ray_d must not contain NaN or infinite coordinates"):
                fn()
    for fn in calls(p, bad(bad(n, 0, big), 1, big), r):                      # a finite normal whose length is not
        with pytest.raises(ValueError, match="the length of a normal overflows the scalar type of p"):
            fn()
    for fn in calls(bad(p, 0, big), n, bad(r, 0, big)):                      # finite p and r, a vertex that is not
        with pytest.raises(ValueError, match="surfel vertices overflow the scalar type of p"):
            fn()
    for fn in calls(p, n, r, near=np.nan, rays_only=True) + calls(p, n, r, far=np.nan, rays_only=True):
        with pytest.raises(ValueError, match="ray_near and ray_far must not be NaN"):
            fn()
    for fn in calls(p, n, r, subdivs=3):
        with pytest.raises(ValueError, match="Invalid geometry_subdivisions_1 is less than or equal to 4."):
            fn()
    for fn in calls(p, n.astype(other), r):
        with pytest.raises(ValueError, match="Invalid scalar type .* for argument 'n'"):
            fn()
    for fn in calls(p, n, r, oo=o.astype(other), rays_only=True):
        with pytest.raises(ValueError, match="Invalid scalar type .* for argument 'ray_o'"):
            fn()
    for fn in calls(p, n, r, dd=d.astype(other), rays_only=True):
        with pytest.raises(ValueError, match="Invalid scalar type .* for argument 'ray_d'"):
            fn()
    for fn in calls(p, n, r[:19]) + calls(p, n, [0.1] * 21):
        with pytest.raises(ValueError, match="Argument r have the same number of rows as p"):
            fn()
    for fn in calls(p, n, np.ones((20, 2), dtype=T)):
        with pytest.raises(ValueError, match=r"Invalid shape for argument r, must have shape \(N,\) or \(N, 1\)"):
            fn()
    for fn in calls(p, n, {"r": 0.1}):
        with pytest.raises(ValueError, match="Argument r must be a scalar or numpy array with the same number of rows as p"):
            fn()
    for fn in calls(p, n, r, oo=o[:5], rays_only=True):
        with pytest.raises(ValueError, match="ray_o and ray_d must have the same number of rows"):
            fn()
    with pcu.RaySurfelIntersector(*dev(p, n), 0.3, 5) as cloud:
        to, td = dev(o.astype(other), d.astype(other))
        with pytest.raises(ValueError, match="Invalid scalar type .* for argument 'ray_o'"):
            cloud.intersect_rays(to, td)
        with pytest.raises(ValueError, match="ray_d must not contain NaN or infinite coordinates"):
            cloud.intersect_rays(*dev(o, bad(d, 2, np.nan)))
        with pytest.raises(ValueError, match="ray_near and ray_far must not be NaN"):
            cloud.intersect_rays(*dev(o, d), ray_near=np.nan)
    cloud.close()
    with pytest.raises(ValueError, match="the surfel index has been closed"):
        cloud.intersect_rays(*dev(o, d))


def test_row_limits_are_refused_before_anything_is_allocated(pcu):
    """More than 2^27 - 16 points or rays, and a geometry beyond int32: shapes alone decide (arrays of that shape that own no memory)."""
    big = np.lib.stride_tricks.as_strided(np.zeros(3, np.float32), shape=(2 ** 27 - 15, 3), strides=(0, 4))
    small = np.ones((4, 3), np.float32)
    with pytest.raises(ValueError, match=r"more than 2\^27-16 rows are not supported"):
        pcu.ray_surfel_intersection(big, big, small, small)
    with pytest.raises(ValueError, match=r"more than 2\^27-16 rows are not supported"):
        pcu.ray_surfel_intersection(small, small, big, big)
    with pytest.raises(ValueError, match=r"more than 2\^27-16 rows are not supported"):
        pcu.pointcloud_surfel_geometry(big, big)
    many = np.lib.stride_tricks.as_strided(np.zeros(3, np.float32), shape=(2 ** 27 - 16, 3), strides=(0, 4))
    with pytest.raises(ValueError, match=r"more than 2\^31-1 vertices"):
        pcu.pointcloud_surfel_geometry(many, many, 0.1, 16)


@pytest.mark.parametrize("T", DTYPES)
@pytest.mark.parametrize("how", ["numpy", "torch"])
def test_zero_points_and_zero_rays(pcu, how, T):
    dev = (lambda *a: _torch(*a)) if how == "torch" else (lambda *a: a)
    e = np.zeros((0, 3), dtype=T)
    o = np.full((5, 3), 2.0, dtype=T); d = -np.ones((5, 3), dtype=T)
    pid, t = pcu.ray_surfel_intersection(*dev(e, e, o, d))
    assert np.array_equal(_to_numpy(pid), np.full(5, -1, np.int32)) and _to_numpy(pid).dtype == np.int32
    assert np.isposinf(_to_numpy(t)).all() and _to_numpy(t).dtype == T and _to_numpy(t).shape == (5,)
    v, f = pcu.pointcloud_surfel_geometry(*dev(e, e))
    assert tuple(v.shape) == (0, 3) and tuple(f.shape) == (0, 3) and _to_numpy(v).dtype == T and _to_numpy(f).dtype == np.int32
    with pcu.RaySurfelIntersector(*dev(e, e)) as cloud:
        pid, t = cloud.intersect_rays(*dev(o, d))
        assert (_to_numpy(pid) == -1).all() and np.isposinf(_to_numpy(t)).all()
        with pytest.raises(ValueError, match="ray_d must not contain NaN or infinite coordinates"):
            cloud.intersect_rays(*dev(o, np.full((5, 3), np.nan, dtype=T)))
    p, n, r = _cloud(20, T, seed=9)
    pid, t = pcu.ray_surfel_intersection(*dev(p, n, e, e, r), 5)
    assert tuple(pid.shape) == (0,) and tuple(t.shape) == (0,) and _to_numpy(pid).dtype == np.int32 and _to_numpy(t).dtype == T
