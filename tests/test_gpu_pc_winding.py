"""point_cloud_fast_winding_number, PointCloudWindingIndex and estimate_mesh_face_normals on the GPU (-m gpu), against
tests/pc_winding_contract.py: the yardstick is the exact dipole sum W in float64 (a plain numpy sum over all points); the tolerance per query is
pc_winding_contract.tolerance: twice what the float64 model of the contract leaves on the same cloud and queries, plus the rounding of the sum
in the kernel's type, 8 eps terms(q) max(1, mag(q)); at beta = +inf rounding alone, 8 eps #p max(1, mag(q)). Every cloud and query here has
float32-representable values, so one W and one model serve both dtypes."""
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

import mesh_contract as mc
import pc_winding_contract as pw
import ray_contract as rc
import winding_contract as wc

pytestmark = pytest.mark.gpu
DTYPES = [np.float32, np.float64]
INF = float("inf")
N_CLOUD = 20000
ZERO_ROWS = "Invalid input point cloud with zero points: points must have shape (n, 3) (n > 0). Got points.shape =(0, 3)."
ROW_LIMIT = "meshes and point clouds with more than 2^27-16 rows are not supported"


@pytest.fixture(scope="module")
def pcu():
    import point_cloud_utils_amd as m
    from point_cloud_utils_amd import _lib
    assert _lib.device_count() > 0, "no GPU visible: the gfx950 path has no CPU fallback"
    return m


def _np(x):
    return x.detach().cpu().numpy() if hasattr(x, "detach") else np.asarray(x)


def _bits(a):
    a = np.ascontiguousarray(_np(a))
    return a.view(np.uint32 if a.dtype == np.float32 else np.uint64)


def _torch(*arrays):
    import torch
    return tuple(torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in arrays)


def _exact(q, p, n, a, workers=8):
    """pc_winding_contract.exact over slices of q on a few threads (numpy releases the GIL inside its loops)."""
    cuts = np.linspace(0, len(q), min(workers, max(1, len(q) // 16)) + 1).astype(int)
    with ThreadPoolExecutor(workers) as ex:
        return np.concatenate(list(ex.map(lambda k: pw.exact(q[cuts[k]:cuts[k + 1]], p, n, a), range(len(cuts) - 1))))


class Case:
    """A cloud, its queries, W and the model's tolerances, computed once and left unchanged."""

    def __init__(self, p, n, a, q, betas=(2.0,), inf=True):
        self.p, self.n, self.a, self.q = pw.f32_grid(p), pw.f32_grid(n), pw.f32_grid(a).reshape(-1), pw.f32_grid(q)
        self.W = _exact(self.q, self.p, self.n, self.a)
        self.tree = pw.build_tree(self.p, self.n, self.a)
        self.tol = {}
        for b in tuple(betas) + ((INF,) if inf else ()):
            walk = pw.walk_stats(self.tree, self.q, self.W, b)
            self.tol.update({(b, T): pw.tolerance(self.tree, self.q, self.W, b, T, walk) for T in DTYPES})

    def arrays(self, T):
        return self.p.astype(T), self.n.astype(T), self.a.astype(T), self.q.astype(T)

    def rounding(self, beta, T):
        tol, err, _ = self.tol[(beta, T)]
        return tol - 2.0 * err

    def check(self, w, beta, T, what):
        w = _np(w)
        assert w.dtype == T and w.shape == (len(self.q),) and np.isfinite(w).all(), what
        tol, model, terms = self.tol[(beta, T)]
        err = np.abs(w.astype(np.float64) - self.W)
        worst = int(np.argmax(err / tol))
        print(f"\n{what} beta={beta} {np.dtype(T).name}: max |w - W| = {err.max():.3e}; worst against its tolerance {err[worst]:.3e} / {tol[worst]:.3e} "
              f"(model {model:.3e}, most terms {terms})")
        assert (err <= tol).all(), (what, beta, T, float(err[worst]), float(tol[worst]))
        return float(err.max())


def _far_queries(p, count, seed):
    rng = np.random.default_rng(seed)
    d = rng.normal(size=(count, 3))
    ext = max(float(np.ptp(p, axis=0).max()), 1.0)
    return p.mean(0) + d / np.linalg.norm(d, axis=1, keepdims=True) * rng.uniform(2, 12, (count, 1)) * ext


@pytest.fixture(scope="module")
def clouds():
    out = {}
    for name, make in (("cube_twist", rc.cube_twist), ("bunny", mc.bunny)):
        v, f = make(np.float32)
        p, n, a, h = pw.mesh_cloud(v, f, N_CLOUD)
        case = Case(p, n, a, wc.box_queries(v, 2000, seed=31), betas=(2.0, 4.0))
        case.v, case.f, case.h = v, f, h
        out[name] = case
    return out


# ---------------------------------------------------------------------------------------------------- 1. small clouds
@pytest.mark.parametrize("count", [1, 8, 9, 17, 100])
def test_small_clouds(pcu, count):
    """1 point (the root is the one leaf), 8 (a full leaf), 9 (two leaves), 17 (three leaves and one padding leaf), 100; queries in the enlarged
    box, 2 to 12 extents away (the whole root is far) and on the points themselves (TERM = 0 on a point)."""
    rng = np.random.default_rng(count)
    p, n, a = rng.random((count, 3)), rng.normal(size=(count, 3)), rng.uniform(0.5, 1.5, count) / count
    case = Case(p, n, a, np.concatenate([wc.box_queries(p, 300, seed=3), _far_queries(p, 200, 7), p]))
    for T in DTYPES:
        pT, nT, aT, qT = case.arrays(T)
        for beta in (2.0, INF):
            w = pcu.point_cloud_fast_winding_number(pT, nT, aT, qT, beta=beta)
            case.check(w, beta, T, f"{count} points")
            flipped = pcu.point_cloud_fast_winding_number(pT, -nT, aT, qT, beta=beta)
            # both are within the rounding of their sums of what exact arithmetic gives, and those two are each other's negatives
            assert (np.abs(_np(flipped).astype(np.float64) + _np(w)) <= 2.0 * case.rounding(beta, T)).all(), (count, T, beta)
        assert np.array_equal(_bits(pcu.point_cloud_fast_winding_number(pT, nT, aT, qT)), _bits(pcu.point_cloud_fast_winding_number(pT, nT, aT, qT, beta=2.0)))


# ---------------------------------------------------------------------------------------------------- 2. the fixture clouds
@pytest.mark.parametrize("T", DTYPES)
@pytest.mark.parametrize("name", ["cube_twist", "bunny"])
def test_fixture_clouds(pcu, clouds, name, T):
    case = clouds[name]
    p, n, a, q = case.arrays(T)
    w = pcu.point_cloud_fast_winding_number(p, n, a, q)
    case.check(w, 2.0, T, name)
    case.check(pcu.point_cloud_fast_winding_number(p, n, a, q, beta=4.0), 4.0, T, name)
    if T == np.float64:
        case.check(pcu.point_cloud_fast_winding_number(p, n, a, q, beta=INF), INF, T, name)
    # the cloud against the mesh it was sampled from: away from the samples the two fields classify alike (tests/test_pc_winding_contract.py
    # holds |W_cloud - W_mesh| < 0.25 there)
    keep = pw.held(case.q, case.p, case.h)
    W_mesh = wc.exact_winding(case.q, case.v, case.f)
    assert keep.mean() >= 0.9
    assert np.array_equal(_np(w)[keep] > 0.5, W_mesh[keep] > 0.5), "every held query, none left out"


@pytest.mark.parametrize("T", DTYPES)
def test_device_chain_from_mesh_to_winding_number(pcu, T):
    """sample_mesh_random -> interpolate_barycentric_coords -> estimate_mesh_face_normals -> mesh_face_areas -> the winding number, all on
    torch tensors; held to the exact sum of what came back."""
    import torch
    v, f = mc.bunny(T)
    q = pw.f32_grid(wc.box_queries(v, 1000, seed=35)).astype(T)
    tv, tf, tq = _torch(v, f, q)
    fi, bc = pcu.sample_mesh_random(tv, tf, N_CLOUD, 11)
    p = pcu.interpolate_barycentric_coords(tf, fi, bc, tv)
    n = pcu.estimate_mesh_face_normals(tv, tf)[fi.long()]
    a = (pcu.mesh_face_areas(tv, tf).sum() / N_CLOUD).expand(N_CLOUD).contiguous()
    assert p.is_cuda and n.is_cuda and a.is_cuda and p.dtype == n.dtype == a.dtype == tq.dtype
    w = pcu.point_cloud_fast_winding_number(p, n, a, tq)
    assert w.is_cuda and w.shape == (len(q),) and w.dtype == p.dtype
    p64, n64, a64, q64 = (_np(x).astype(np.float64) for x in (p, n, a, tq))
    W = _exact(q64, p64, n64, a64)
    tol, model, terms = pw.tolerance(pw.build_tree(p64, n64, a64), q64, W, 2.0, T)
    err = np.abs(_np(w).astype(np.float64) - W)
    print(f"\nchain {np.dtype(T).name}: max |w - W| = {err.max():.3e} (model {model:.3e}, most terms {terms})")
    assert (err <= tol).all()
    assert torch.cuda.is_available()


# ---------------------------------------------------------------------------------------------------- 3. hard clouds
def _run(pcu, case, what, types=DTYPES, betas=(2.0, INF)):
    for T in types:
        p, n, a, q = case.arrays(T)
        for beta in betas:
            case.check(pcu.point_cloud_fast_winding_number(p, n, a, q, beta=beta), beta, T, what)


def test_thousand_coincident_points(pcu):
    """Every box is a point and every radius 0: any query off the point takes the root's expansion, a query on it opens everything and adds 0."""
    rng = np.random.default_rng(5)
    at = np.array([0.3, 0.2, 0.1])
    p, n, a = np.tile(at, (1000, 1)), rng.normal(size=(1000, 3)), rng.uniform(0.5, 1.5, 1000) * 1e-3
    q = np.concatenate([at + rng.normal(size=(300, 3)), np.tile(at, (5, 1))])
    case = Case(p, n, a, q)
    assert np.array_equal(case.W[-5:], np.zeros(5)) and np.abs(case.W[:300]).max() > 1e-3
    _run(pcu, case, "coincident")


def test_ten_thousand_points_of_one_morton_code(pcu):
    """The cloud of a tetrahedron of size 1 (its corners are in it with a = 0, so the bounding box is the unit cube) and, inside it, 9,600 points
    on a sphere of radius 2^-23 about the middle of a Morton cell (of 2^-21): all leaves of the tree but a few hold nothing else."""
    tv, tf = wc.tetrahedron(np.float64)
    tp, tn, ta, _ = pw.mesh_cloud(tv, tf, 400)
    c = (np.floor(np.array([0.3, 0.2, 0.1]) * 2 ** 21) + 0.5) * 2.0 ** -21
    sp, sn, sa = pw.fibonacci_sphere(9600, radius=2.0 ** -23)
    sp = pw.f32_grid(c + sp)
    assert np.array_equal(np.floor(sp.min(0) * 2 ** 21), np.floor(sp.max(0) * 2 ** 21))
    p = np.concatenate([tv, tp, sp])
    n = np.concatenate([np.ones((4, 3)), tn, sn])
    a = np.concatenate([np.zeros(4), ta, sa])
    assert len(p) == 10004 and np.array_equal(p.min(0), np.zeros(3)) and np.array_equal(p.max(0), np.ones(3))
    rng = np.random.default_rng(9)
    _run(pcu, Case(p, n, a, wc.box_queries(tv, 500, seed=33)), "one cell, queries outside")
    inside = Case(p, n, a, c + (rng.random((100, 3)) - 0.5) * 2.0 ** -25)
    assert np.abs(inside.W).max() > 0.5                          # (inside the small sphere: about 1 more than outside it)
    _run(pcu, inside, "one cell, queries inside", types=[np.float64])


def test_flat_cloud(pcu):
    """z = 0: a zero-extent axis of the frame."""
    rng = np.random.default_rng(6)
    p = np.concatenate([rng.random((500, 2)), np.zeros((500, 1))], axis=1)
    n = np.array([0.0, 0.0, 1.0]) + 0.1 * rng.normal(size=(500, 3))
    a = np.full(500, 1.0 / 500)
    q = np.concatenate([rng.random((300, 2)) * 1.5 - 0.25, rng.uniform(-0.5, 0.5, (300, 1))], axis=1)
    q_plane = np.concatenate([rng.random((100, 2)), np.zeros((100, 1))], axis=1)
    _run(pcu, Case(p, n, a, np.concatenate([q, q_plane, _far_queries(p, 100, 8), p[:50]])), "flat")


def test_rows_without_weight_and_negative_areas(pcu):
    """A third of the rows have a = 0 or n = 0, two whole leaves of the tree among them (weight 0: the centre is the box's); then areas of
    either sign."""
    rng = np.random.default_rng(12)
    p, n, a = rng.random((600, 3)), rng.normal(size=(600, 3)), rng.uniform(0.5, 1.5, 600) / 600
    order = pw.point_order(pw.f32_grid(p))
    dead = np.union1d(order[16:32], rng.choice(600, 190, replace=False))
    a[dead[::2]] = 0.0
    n[dead[1::2]] = 0.0
    q = np.concatenate([wc.box_queries(p, 400, seed=13), _far_queries(p, 100, 14), p[dead[:40]]])
    case = Case(p, n, a, q)
    leaf_nodes = case.tree["P"] - 1 + np.array([2, 3])
    assert (case.tree["weight"][leaf_nodes] == 0).all() and (case.tree["r"][leaf_nodes] > 0).all()
    assert np.array_equal(case.tree["ctr"][leaf_nodes], 0.5 * case.tree["lo"][leaf_nodes] + 0.5 * case.tree["hi"][leaf_nodes])
    _run(pcu, case, "a third without weight")
    signed = Case(p, rng.normal(size=(600, 3)), rng.normal(size=600) / 600, q)
    assert (signed.a < 0).sum() > 200
    _run(pcu, signed, "negative areas")


@pytest.mark.parametrize("T", DTYPES)
@pytest.mark.parametrize("power", [20, -20])
def test_scaled_by_powers_of_two(pcu, clouds, power, T):
    """W does not depend on the scale (a scales with its square) and scaling by 2^k is exact, so the tolerance is the unscaled one."""
    case = clouds["bunny"]
    p, n, a, q = case.arrays(T)
    s = T(2.0 ** power)
    case.check(pcu.point_cloud_fast_winding_number(p * s, n, a * s * s, q * s), 2.0, T, f"bunny cloud * 2^{power}")


# ---------------------------------------------------------------------------------------------------- 4. index and determinism
@pytest.mark.parametrize("T", DTYPES)
def test_index_one_shot_torch_and_shuffled_rows_give_the_same_bits(pcu, clouds, T):
    case = clouds["bunny"]
    p, n, a, q = case.arrays(T)
    w = pcu.point_cloud_fast_winding_number(p, n, a, q)
    perm = np.random.default_rng(1).permutation(len(q))
    tp, tn, ta, tq = _torch(p, n, a, q)
    with pcu.PointCloudWindingIndex(p, n, a) as cloud, pcu.PointCloudWindingIndex(tp, tn, ta) as tcloud:
        assert cloud.num_points == len(p)
        for got in (pcu.point_cloud_fast_winding_number(p, n, a, q), pcu.point_cloud_fast_winding_number(tp, tn, ta, tq), cloud.winding_number(q),
                    cloud.winding_number(q), cloud.winding_number(tq), tcloud.winding_number(q), tcloud.winding_number(tq),
                    cloud.winding_number(q[perm])[np.argsort(perm)]):
            assert np.array_equal(_bits(got), _bits(w))
        assert cloud.winding_number(tq).is_cuda and isinstance(tcloud.winding_number(q), np.ndarray)
        assert np.array_equal(_bits(cloud.winding_number(q, beta=4.0)), _bits(pcu.point_cloud_fast_winding_number(p, n, a, q, beta=4.0)))
        one = cloud.winding_number(q[:1])
        assert one.shape == () and _bits(one.reshape(1))[0] == _bits(w)[0]
        assert pcu.point_cloud_fast_winding_number(p, n, a, q[:1]).shape == ()
        assert pcu.last_stats()["n_queries"] == 1


# ---------------------------------------------------------------------------------------------------- 5. face normals
@pytest.mark.parametrize("T", DTYPES)
@pytest.mark.parametrize("name", ["cube_twist", "bunny"])
def test_face_normals_bit_for_bit(pcu, name, T):
    v, f = (rc.cube_twist if name == "cube_twist" else mc.bunny)(T)
    want = pw.face_normals(v, f)
    for fdt in (np.int32, np.int64, np.uint32, np.uint64):
        got = pcu.estimate_mesh_face_normals(v, f.astype(fdt))
        assert got.dtype == T and got.shape == (len(f), 3) and np.array_equal(_bits(got), _bits(want)), fdt
    tv, tf = _torch(v, f)
    got = pcu.estimate_mesh_face_normals(tv, tf)
    assert got.is_cuda and np.array_equal(_bits(got), _bits(want))
    assert np.array_equal(_bits(pcu.estimate_mesh_face_normals(tv, tf.int())), _bits(want))
    deg = np.concatenate([f[:5], mc.degenerate_faces(10, 20)])
    got = pcu.estimate_mesh_face_normals(v, deg)
    assert np.array_equal(_bits(got), _bits(pw.face_normals(v, deg))) and np.array_equal(got[5:], np.zeros((4, 3), T))
    assert pcu.estimate_mesh_face_normals(v, f[:1]).shape == (1, 3)


def test_face_normals_error_paths(pcu):
    import torch
    v, f = mc.bunny(np.float32)
    with pytest.raises(ValueError, match="face normals overflow the scalar type of v"):
        pcu.estimate_mesh_face_normals(v * np.float32(1e30), f)
    assert np.isfinite(pcu.estimate_mesh_face_normals(v.astype(np.float64) * 1e30, f)).all()
    bad = v.copy()
    bad[3, 1] = np.inf
    for vv, ff in ((bad, f), _torch(bad, f)):
        with pytest.raises(ValueError, match="v must not contain NaN or infinite coordinates"):
            pcu.estimate_mesh_face_normals(vv, ff)
    out = f.copy()
    out[7, 2] = len(v)
    for vv, ff in ((v, out), _torch(v, out)):
        with pytest.raises(ValueError, match="f must hold row indices of v: found a face index outside"):
            pcu.estimate_mesh_face_normals(vv, ff)
    with pytest.raises(ValueError, match="Invalid input mesh with zero elements"):
        pcu.estimate_mesh_face_normals(v, f[:0])
    with pytest.raises(ValueError, match="Invalid scalar type \\(int32\\) for argument 'v'"):
        pcu.estimate_mesh_face_normals(v.astype(np.int32), f)
    with pytest.raises(ValueError, match="Invalid scalar type \\(float32\\) for argument 'f'"):
        pcu.estimate_mesh_face_normals(v, f.astype(np.float32))
    assert torch.cuda.is_available()


# ---------------------------------------------------------------------------------------------------- 6. error paths
def test_error_paths(pcu, clouds):
    import torch
    from point_cloud_utils_amd import _lib
    case = clouds["bunny"]
    p, n, a, q = (x[:500] for x in case.arrays(np.float32))
    w = pcu.point_cloud_fast_winding_number(p, n, a, q)
    for shaped in (a.reshape(-1, 1), a.reshape(1, -1)):
        assert np.array_equal(_bits(pcu.point_cloud_fast_winding_number(p, n, shaped, q)), _bits(w))
    tp, tn, ta, tq = _torch(p, n, a, q)
    assert np.array_equal(_bits(pcu.point_cloud_fast_winding_number(tp, tn, ta.reshape(1, -1), tq)), _bits(w))

    def text(call):
        with pytest.raises(ValueError) as e:
            call()
        return str(e.value)

    f = pcu.point_cloud_fast_winding_number
    assert text(lambda: f(p[:0], n[:0], a[:0], q)) == ZERO_ROWS
    assert text(lambda: f(p, n, a, q[:0])) == ZERO_ROWS
    assert text(lambda: f(p[:, :2], n, a, q)) == "Only 3D inputs are supported: v must have shape (n, 3) (n > 0). Got points.shape =(500, 2)."
    assert text(lambda: f(p, n, a, q[:, :2])) == "Only 3D inputs are supported: v must have shape (n, 3) (n > 0). Got points.shape =(500, 2)."
    assert text(lambda: f(p, n[:, :2], a, q)) == "Invalid shape for normals: must have shape (n, 3) (n > 0). Got normals.shape =(500, 2)."
    assert text(lambda: f(p, n[:400], a, q)) == ("Invalid input point cloud. Number of normals must match number of points. "
                                                 "Got points.shape =(500, 3) and normals.shape = 400, 3")
    assert "a must have one element per point (500)" in text(lambda: f(p, n, a[:499], q))
    assert "a must have one element per point (500)" in text(lambda: f(p, n, np.stack([a, a]), q))
    assert text(lambda: f(p.astype(np.int32), n, a, q)) == "Invalid scalar type (int32) for argument 'p'. Expected one of ['float32', 'float64']."
    for name, args in (("n", (p, n.astype(np.float64), a, q)), ("a", (p, n, a.astype(np.float64), q)), ("q", (p, n, a, q.astype(np.float64)))):
        assert text(lambda: f(*args)) == f"Invalid scalar type (float64) for argument '{name}'. Expected it to match argument 'p' which is of type float32."
    for beta in (0.0, -1.0, float("nan")):
        assert text(lambda: f(p, n, a, q, beta=beta)).startswith("beta must be greater than 0")
    with pytest.raises(TypeError):
        f(p, n, a, q, 2.0)                                                  # beta is keyword-only
    # a non-finite value anywhere, found on the host for numpy and on the device for torch
    for i, (name, kind) in enumerate((("p", "coordinates"), ("n", "coordinates"), ("a", "values"), ("q", "coordinates"))):
        for value in (np.nan, np.inf):
            args = [p.copy(), n.copy(), a.copy(), q.copy()]
            args[i].reshape(-1)[17] = value
            for given in (args, _torch(*args)):
                assert text(lambda: f(*given)) == f"{name} must not contain NaN or infinite {kind}"
            if name != "q":
                for given in (args[:3], _torch(*args[:3])):
                    assert text(lambda: pcu.PointCloudWindingIndex(*given)) == f"{name} must not contain NaN or infinite {kind}"
    big_a, big_n = a.copy(), n.copy()
    big_a[3], big_n[3] = np.float32(1e30), np.float32(1e30)
    for given in ((p, big_n, big_a, q), _torch(p, big_n, big_a, q)):
        assert text(lambda: f(*given)) == "a * n overflows the scalar type of p"
    # the row limit, by the C ABI (nothing is read before the counts are checked)
    out = np.empty(1, np.float32)
    L = _lib.lib()
    assert L.pcu_hip_point_cloud_fast_winding_number_f32(_lib.ctx(), p.ctypes.data, n.ctypes.data, a.ctypes.data, 2 ** 27 - 15, q.ctypes.data, 1, 2.0,
                                                         out.ctypes.data, 0, None, None) == _lib.ERR_INVALID and _lib.last_error() == ROW_LIMIT
    assert L.pcu_hip_point_cloud_fast_winding_number_f32(_lib.ctx(), p.ctypes.data, n.ctypes.data, a.ctypes.data, 500, q.ctypes.data, 2 ** 27 - 15, 2.0,
                                                         out.ctypes.data, 0, None, None) == _lib.ERR_INVALID and _lib.last_error() == ROW_LIMIT
    assert L.pcu_hip_point_cloud_fast_winding_number_f32(_lib.ctx(), p.ctypes.data, n.ctypes.data, a.ctypes.data, 0, q.ctypes.data, 1, 2.0,
                                                         out.ctypes.data, 0, None, None) == _lib.ERR_INVALID and _lib.last_error() == ZERO_ROWS
    # the index: the other dtype, another kind of device array, closed
    with pcu.PointCloudWindingIndex(p, n, a) as cloud:
        assert text(lambda: cloud.winding_number(q.astype(np.float64))) == ("Invalid scalar type (float64) for argument 'q'. Expected it to match the "
                                                                            "indexed point cloud which is of type float32.")
        assert text(lambda: cloud.winding_number(q[:0])) == ZERO_ROWS
        assert text(lambda: cloud.winding_number(q, beta=0.0)).startswith("beta must be greater than 0")
        with pytest.raises(TypeError):
            cloud.winding_number(q, 2.0)
        with pytest.raises(ValueError, match="CUDA/HIP tensors"):
            cloud.winding_number(tq.cpu())
        rc_ = L.pcu_hip_pc_winding_index_query_f64(_lib.ctx(), cloud._h, q.ctypes.data, 1, 2.0, out.ctypes.data, 0, None, None)
        assert rc_ == _lib.ERR_INVALID and "other scalar type" in _lib.last_error()
    assert text(lambda: cloud.winding_number(q)) == "the point cloud winding index has been closed"
    cloud.close()                                                           # (a second close is harmless)
    with pytest.raises(ValueError, match="CUDA/HIP tensors"):
        f(tp, tn, ta, q)
    with pytest.raises(ValueError, match="CUDA/HIP tensors"):
        f(tp, tn, a, tq)
    assert torch.cuda.is_available()
