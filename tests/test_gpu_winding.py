"""triangle_soup_fast_winding_number and signed_distance_to_mesh on the GPU (-m gpu), against tests/winding_contract.py: the yardstick is the exact
winding number W in float64 (a plain numpy sum over all faces); the tolerance at a finite beta is twice what the float64 model of the contract
leaves on the same mesh and queries, plus the rounding of the sum (winding_contract.tolerance); at beta = +inf it is rounding alone,
8 nf eps(T). Every mesh and query here has float32-representable coordinates, so one W and one model serve both dtypes."""
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

import mesh_contract as mc
import ray_contract as rc
import winding_contract as wc

pytestmark = pytest.mark.gpu
DTYPES = [np.float32, np.float64]
INF = float("inf")
ZERO_ROWS = "Invalid input point cloud with zero points: points must have shape (n, 3) (n > 0). Got points.shape =(0, 3)."


@pytest.fixture(scope="module")
def pcu():
    import point_cloud_utils_amd as m
    from point_cloud_utils_amd import _lib
    assert _lib.device_count() > 0, "no GPU visible: the gfx950 path has no CPU fallback"
    return m


def _bits(a):
    a = np.ascontiguousarray(_np(a))
    return a.view(np.uint32 if a.dtype == np.float32 else np.uint64)


def _np(x):
    return x.detach().cpu().numpy() if hasattr(x, "detach") else np.asarray(x)


def _torch(*arrays):
    import torch
    return tuple(torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in arrays)


def _exact(q, v, f, workers=8):
    """winding_contract.exact_winding over slices of q on a few threads (numpy releases the GIL inside its loops)."""
    cuts = np.linspace(0, len(q), min(workers, max(1, len(q) // 16)) + 1).astype(int)
    with ThreadPoolExecutor(workers) as ex:
        return np.concatenate(list(ex.map(lambda k: wc.exact_winding(q[cuts[k]:cuts[k + 1]], v, f), range(len(cuts) - 1))))


def _f32_grid(a):
    return np.ascontiguousarray(np.asarray(a).astype(np.float32).astype(np.float64))


class Case:
    """A mesh, its queries, W and the model's errors, computed once and left unchanged."""

    def __init__(self, v, f, q, W=None, betas=(2.0,), two_terms=False):
        self.v, self.f, self.q = _f32_grid(v), np.ascontiguousarray(np.asarray(f).astype(np.int64)), _f32_grid(q)
        self.W = _exact(self.q, self.v, self.f) if W is None else W
        self.tree = wc.build_tree(self.v, self.f)
        self.tol = {(b, T): wc.tolerance(self.tree, self.q, self.W, b, T) for b in betas for T in DTYPES}
        self.err2 = {b: float(np.abs(wc.fast_winding(self.tree, self.q, b, terms=2) - self.W).max()) for b in betas} if two_terms else None

    def arrays(self, T):
        return self.v.astype(T), self.f, self.q.astype(T)

    def check(self, w, beta, T, what, scale=1.0):
        w = _np(w)
        assert w.dtype == T and w.shape == (len(self.q),) and np.isfinite(w).all(), what
        err = float(np.abs(w.astype(np.float64) - self.W).max())
        if np.isfinite(beta):
            tol, model, terms = self.tol[(beta, T)]
        else:
            tol, model, terms = 8.0 * len(self.f) * np.finfo(T).eps, 0.0, len(self.f)
        print(f"\n{what} beta={beta} {np.dtype(T).name}: max |w - W| = {err:.3e}, tolerance {tol * scale:.3e} (model {model:.3e}, {terms} terms)")
        assert err <= tol * scale, (what, beta, T, err, tol * scale)
        return err


@pytest.fixture(scope="module")
def closed():
    out = {}
    for name, make in (("cube_twist", rc.cube_twist), ("bunny", mc.bunny)):
        v, f = make(np.float32)
        out[name] = Case(v, f, wc.box_queries(v, 2000, seed=31), betas=(2.0, 4.0), two_terms=True)
    return out


# ---------------------------------------------------------------------------------------------------- 1. small meshes
def _small(kind):
    if kind == "tetrahedron":
        return wc.tetrahedron(np.float64)
    if kind == "octahedron":
        return rc.octahedron(np.float64)
    rng = np.random.default_rng(kind)
    return rng.random((3 * kind, 3)), rng.permutation(3 * kind).reshape(kind, 3)


@pytest.mark.parametrize("kind", [1, 4, 5, "tetrahedron", "octahedron"])
def test_small_meshes(pcu, kind):
    """1 face (the root is the one leaf), 4 (a full leaf), 5 (two leaves), two closed solids; queries in the enlarged box and 2 to 12 extents
    away, where whole nodes (and the root) are far."""
    v, f = _small(kind)
    rng = np.random.default_rng(7)
    d = rng.normal(size=(200, 3))
    far = v.mean(0) + d / np.linalg.norm(d, axis=1, keepdims=True) * rng.uniform(2, 12, (200, 1)) * np.ptp(v, axis=0).max()
    case = Case(v, f, np.concatenate([wc.box_queries(v, 300, seed=3), far]))
    if isinstance(kind, str):
        assert set(np.round(case.W[:300]).astype(int)) == {0, 1}
    for T in DTYPES:
        vT, fT, qT = case.arrays(T)
        for beta in (2.0, INF):
            w = pcu.triangle_soup_fast_winding_number(vT, fT, qT, beta=beta)
            case.check(w, beta, T, kind)
            flipped = pcu.triangle_soup_fast_winding_number(vT, np.ascontiguousarray(fT[:, ::-1]), qT, beta=beta)
            # both are within the rounding of their sums of what exact arithmetic gives, and those two are each other's negatives
            terms = case.tol[(2.0, T)][2] if np.isfinite(beta) else len(fT)
            assert np.abs(_np(flipped) + _np(w)).max() <= 2 * 8.0 * terms * np.finfo(T).eps, (kind, T, beta)
        assert np.array_equal(_bits(pcu.triangle_soup_fast_winding_number(vT, fT, qT)), _bits(pcu.triangle_soup_fast_winding_number(vT, fT, qT, beta=2.0)))


# ---------------------------------------------------------------------------------------------------- 2. the fixtures
@pytest.mark.parametrize("T", DTYPES)
@pytest.mark.parametrize("name", ["cube_twist", "bunny"])
def test_closed_fixtures(pcu, closed, name, T):
    case = closed[name]
    v, f, q = case.arrays(T)
    e2 = case.check(pcu.triangle_soup_fast_winding_number(v, f, q), 2.0, T, name)
    e4 = case.check(pcu.triangle_soup_fast_winding_number(v, f, q, beta=4.0), 4.0, T, name)
    assert case.tol[(2.0, T)][0] < case.err2[2.0], "the tolerance must refuse an evaluation without M2"
    m3, m2 = case.tol[(4.0, T)][1] / case.tol[(2.0, T)][1], case.err2[4.0] / case.err2[2.0]
    threshold = float(np.sqrt(m3 * m2))
    print(f"decay err(4)/err(2): {e4 / e2:.4f}; model: three terms {m3:.4f}, two terms {m2:.4f}, threshold {threshold:.4f}")
    assert e4 / e2 <= threshold
    if T == np.float64:
        case.check(pcu.triangle_soup_fast_winding_number(v, f, q, beta=INF), INF, T, name)


@pytest.fixture(scope="module")
def open_soup():
    v, f = mc.bunny(np.float32)
    return Case(v, f[::2], wc.box_queries(v, 2000, seed=32))


@pytest.mark.parametrize("T", DTYPES)
def test_open_soup_every_second_face(pcu, open_soup, T):
    case = open_soup
    assert np.abs(case.W - np.round(case.W)).max() > 0.2, "an open soup: fractional W"
    v, f, q = case.arrays(T)
    case.check(pcu.triangle_soup_fast_winding_number(v, f, q), 2.0, T, "bunny[::2]")


def test_ten_thousand_faces_of_one_morton_code(pcu):
    """A tetrahedron of size 1 and, inside it, 1250 copies of one octahedron of radius 2^-23: 10,000 faces in one Morton cell (of 2^-21), so all
    leaves of the tree but one or two hold nothing else. W = W(tetrahedron) + 1250 W(octahedron). Inside the octahedra (float64: the
    partial sums there are 1251 times larger than the terms the rounding allowance is made for, so it is scaled by |W|)."""
    tv, tf = wc.tetrahedron(np.float64)
    ov, of = rc.octahedron(np.float64)
    c = (np.floor(np.array([0.3, 0.2, 0.1]) * 2 ** 21) + 0.5) * 2.0 ** -21      # the middle of a cell: the corners are a quarter of a cell from it
    ov = c + ov * 2.0 ** -23
    assert np.array_equal(ov, _f32_grid(ov)) and np.array_equal(np.floor(ov.min(0) * 2 ** 21), np.floor(ov.max(0) * 2 ** 21))
    v = np.concatenate([tv, ov])
    f = np.concatenate([tf, np.tile(of + len(tv), (1250, 1))])
    assert len(f) == 10004
    rng = np.random.default_rng(9)
    q_out = wc.box_queries(tv, 500, seed=33)
    q_in = _f32_grid(c + (rng.random((100, 3)) - 0.5) * 2.0 ** -25)
    for q, types, scale in ((q_out, DTYPES, 1.0), (q_in, [np.float64], 1251.0)):
        q = _f32_grid(q)
        W = wc.exact_winding(q, tv, tf) + 1250 * wc.exact_winding(q, ov, of)
        case = Case(v, f, q, W=W)
        assert np.abs(W).max() >= scale
        for T in types:
            vT, fT, qT = case.arrays(T)
            for beta in (2.0, INF):
                case.check(pcu.triangle_soup_fast_winding_number(vT, fT, qT, beta=beta), beta, T, "one cell", scale=scale)


@pytest.mark.parametrize("T", DTYPES)
def test_degenerate_faces_and_unreferenced_vertices(pcu, closed, T):
    """Faces without area have no solid angle and unreferenced vertices (far outside: they must not widen the box) no part: W is the bunny's
    (plus what the one sliver adds whose middle corner, rounded to float32, is not exactly on the line of the other two: below 1e-7)."""
    base = closed["bunny"]
    rng = np.random.default_rng(4)
    extra_v = np.concatenate([base.v.mean(0) + 100.0 * rng.normal(size=(50, 3)), 0.5 * (base.v[10] + base.v[20])[None]])
    v = np.concatenate([base.v, extra_v])
    mid = len(v) - 1
    degenerate = np.concatenate([mc.degenerate_faces(i, j) for i, j in ((10, 20), (300, 1500), (77, 78))] + [np.array([[10, mid, 20]])])
    f = np.concatenate([base.f, degenerate])[rng.permutation(len(base.f) + len(degenerate))]
    sliver = wc.exact_winding(base.q, _f32_grid(v), degenerate)
    assert np.abs(sliver).max() < 1e-7
    case = Case(v, f, base.q, W=base.W + sliver)
    vT, fT, qT = case.arrays(T)
    case.check(pcu.triangle_soup_fast_winding_number(vT, fT, qT), 2.0, T, "bunny with degenerate faces")
    if T == np.float64:
        case.check(pcu.triangle_soup_fast_winding_number(vT, fT, qT, beta=INF), INF, T, "bunny with degenerate faces")


@pytest.mark.parametrize("T", DTYPES)
@pytest.mark.parametrize("power", [20, -20])
def test_scaled_by_powers_of_two(pcu, closed, power, T):
    """W does not depend on the scale and scaling by 2^k is exact, so the tolerance is the unscaled one."""
    case = closed["bunny"]
    v, f, q = case.arrays(T)
    s = T(2.0 ** power)
    case.check(pcu.triangle_soup_fast_winding_number(v * s, f, q * s), 2.0, T, f"bunny * 2^{power}")
    s_, fi, bc = pcu.signed_distance_to_mesh(q * s, v * s, f)
    assert np.isfinite(s_).all() and np.array_equal(s_ < 0, case.W > 0.5)


# ---------------------------------------------------------------------------------------------------- 3. signed distance
@pytest.mark.parametrize("T", DTYPES)
@pytest.mark.parametrize("name", ["cube_twist", "bunny"])
def test_signed_distance(pcu, closed, name, T):
    case = closed[name]
    v, f, q = case.arrays(T)
    d, fi0, bc0 = pcu.closest_points_on_mesh(q, v, f)
    s, fi, bc = pcu.signed_distance_to_mesh(q, v, f)
    assert s.dtype == T and bc.dtype == T and fi.dtype == np.int32 and s.shape == (len(q),) and bc.shape == (len(q), 3)
    assert np.array_equal(_bits(np.abs(s)), _bits(d)) and np.array_equal(fi, fi0.astype(np.int32)) and np.array_equal(_bits(bc), _bits(bc0))
    assert np.array_equal(np.sign(s), np.where(case.W < 0.5, 1.0, -1.0)), "every query, none left out"
    assert (s < 0).any() and (s > 0).any()
    ext = float(np.ptp(case.v, axis=0).max())
    lo, hi = -0.01 * ext, 0.1 * ext
    assert float(np.float32(lo)) != lo and float(np.float32(hi)) != hi      # (the bounds are rounded to float32 first)
    sc, fic, bcc = pcu.signed_distance_to_mesh(q, v, f, lo, hi)
    want = np.clip(s, T(np.float32(lo)), T(np.float32(hi)))
    assert (s < want).any() and (s > want).any()
    assert np.array_equal(_bits(sc), _bits(want)) and np.array_equal(fic, fi) and np.array_equal(_bits(bcc), _bits(bc))
    assert np.array_equal(_bits(pcu.signed_distance_to_mesh(q, v, f, lower_bound=-INF, upper_bound=INF)[0]), _bits(s))
    for fdt in (np.int32, np.uint64):
        assert pcu.signed_distance_to_mesh(q[:10], v, f.astype(fdt))[1].dtype == np.int32
    import torch
    ts, tfi, tbc = pcu.signed_distance_to_mesh(*_torch(q, v, f))
    assert ts.is_cuda and tfi.dtype == torch.int32
    assert np.array_equal(_bits(ts), _bits(s)) and np.array_equal(_np(tfi), fi) and np.array_equal(_bits(tbc), _bits(bc))
    for bad in ((float("nan"), 1.0), (0.0, float("nan")), (1.0, 0.5)):
        with pytest.raises(ValueError, match="lower_bound"):
            pcu.signed_distance_to_mesh(q, v, f, *bad)


# ---------------------------------------------------------------------------------------------------- 4. index and determinism
@pytest.mark.parametrize("T", DTYPES)
def test_index_one_shot_torch_and_shuffled_rows_give_the_same_bits(pcu, closed, T):
    case = closed["bunny"]
    v, f, q = case.arrays(T)
    w = pcu.triangle_soup_fast_winding_number(v, f, q)
    s, fi, bc = pcu.signed_distance_to_mesh(q, v, f)
    perm = np.random.default_rng(1).permutation(len(q))
    tq, tv, tf = _torch(q, v, f)
    with pcu.MeshIndex(v, f, winding_numbers=True) as mesh, pcu.MeshIndex(tv, tf, winding_numbers=True) as tmesh:
        for got in (pcu.triangle_soup_fast_winding_number(v, f, q), pcu.triangle_soup_fast_winding_number(tv, tf, tq), mesh.winding_number(q),
                    mesh.winding_number(q), mesh.winding_number(tq), tmesh.winding_number(q), mesh.winding_number(q[perm])[np.argsort(perm)]):
            assert np.array_equal(_bits(got), _bits(w))
        assert np.array_equal(_bits(mesh.winding_number(q, beta=4.0)), _bits(pcu.triangle_soup_fast_winding_number(v, f, q, beta=4.0)))
        for got in (pcu.signed_distance_to_mesh(q, v, f), mesh.signed_distance(q), tmesh.signed_distance(tq),
                    tuple(x[np.argsort(perm)] for x in mesh.signed_distance(q[perm]))):
            assert np.array_equal(_bits(got[0]), _bits(s)) and np.array_equal(_np(got[1]), fi) and np.array_equal(_bits(got[2]), _bits(bc))
            assert _np(got[1]).dtype == np.int32
        assert np.array_equal(_bits(mesh.signed_distance(q, -0.001, 0.01)[0]), _bits(pcu.signed_distance_to_mesh(q, v, f, -0.001, 0.01)[0]))
        d, fi0, bc0 = mesh.closest_points(q)                               # the index with moments answers the other queries as before
        assert np.array_equal(_bits(d), _bits(np.abs(s))) and np.array_equal(_bits(bc0), _bits(bc))
        one = mesh.winding_number(q[:1])
        assert one.shape == () and _bits(one.reshape(1))[0] == _bits(w)[0]
        assert mesh.signed_distance(q[:1])[2].shape == (3,)


def test_index_without_moments_refuses_and_still_answers(pcu, closed):
    case = closed["bunny"]
    v, f, q = case.arrays(np.float32)
    with pcu.MeshIndex(v, f) as mesh:
        with pytest.raises(ValueError, match="winding_number needs an index built with winding_numbers=True"):
            mesh.winding_number(q)
        with pytest.raises(ValueError, match="signed_distance needs an index built with winding_numbers=True"):
            mesh.signed_distance(q)
        for got, want in zip(mesh.closest_points(q), pcu.closest_points_on_mesh(q, v, f)):
            assert np.array_equal(got, want)
        o, d = q[:500], np.random.default_rng(2).normal(size=(500, 3)).astype(np.float32)
        for got, want in zip(mesh.intersect_rays(o, d), pcu.ray_mesh_intersection(v, f, o, d)):
            assert np.array_equal(got, want)
        from point_cloud_utils_amd import _lib                              # the C ABI's own refusal, under the Python check
        out = np.empty(len(q), np.float32)
        rc_ = _lib.lib().pcu_hip_mesh_index_winding_f32(_lib.ctx(), mesh._h, q.ctypes.data, len(q), 2.0, out.ctypes.data, 0, None, None)
        assert rc_ == _lib.ERR_INVALID and "PCU_HIP_MESH_MOMENTS" in _lib.last_error()


# ---------------------------------------------------------------------------------------------------- 5. error paths
def test_error_paths(pcu, closed):
    import torch
    case = closed["bunny"]
    v, f, q = case.arrays(np.float32)
    w = pcu.triangle_soup_fast_winding_number(v, f, q[:200])
    for fdt in (np.int32, np.int64, np.uint32, np.uint64):
        assert np.array_equal(_bits(pcu.triangle_soup_fast_winding_number(v, f.astype(fdt), q[:200])), _bits(w))
    with pytest.raises(ValueError) as e:
        pcu.triangle_soup_fast_winding_number(v, f, q[:0])
    assert str(e.value) == ZERO_ROWS
    with pytest.raises(ValueError) as e:
        pcu.signed_distance_to_mesh(q[:0], v, f)
    assert str(e.value) == ZERO_ROWS
    with pcu.MeshIndex(v, f, winding_numbers=True) as mesh:
        with pytest.raises(ValueError) as e:
            mesh.winding_number(q[:0])
        assert str(e.value) == ZERO_ROWS
        with pytest.raises(ValueError, match="match the indexed mesh which is of type float32"):
            mesh.signed_distance(q.astype(np.float64))
    with pytest.raises(ValueError) as e:
        pcu.triangle_soup_fast_winding_number(v, f, q.astype(np.float64))
    assert str(e.value) == "Invalid scalar type (float64) for argument 'p'. Expected it to match argument 'v' which is of type float32."
    with pytest.raises(ValueError) as e:
        pcu.signed_distance_to_mesh(q, v.astype(np.float64), f)
    assert str(e.value) == "Invalid scalar type (float64) for argument 'v'. Expected it to match argument 'p' which is of type float32."
    with pytest.raises(ValueError, match="Invalid scalar type \\(int32\\) for argument 'v'"):
        pcu.triangle_soup_fast_winding_number(v.astype(np.int32), f, q)
    with pytest.raises(ValueError, match="Invalid scalar type \\(float32\\) for argument 'f'"):
        pcu.triangle_soup_fast_winding_number(v, f.astype(np.float32), q)
    with pytest.raises(ValueError, match="Invalid input mesh with zero elements"):
        pcu.triangle_soup_fast_winding_number(v, f[:0], q[:0])              # (the mesh is validated before the points)
    with pytest.raises(ValueError, match="Only 3D inputs are supported: v must have shape"):
        pcu.signed_distance_to_mesh(q[:, :2], v, f)
    for beta in (0.0, -1.0, float("nan")):
        with pytest.raises(ValueError, match="beta must be greater than 0"):
            pcu.triangle_soup_fast_winding_number(v, f, q, beta=beta)
    with pytest.raises(TypeError):
        pcu.triangle_soup_fast_winding_number(v, f, q, 2.0)                 # beta is keyword-only
    bad = q.copy()
    bad[17, 1] = np.nan
    tq, tv, tf = _torch(bad, v, f)
    for call in (lambda: pcu.triangle_soup_fast_winding_number(tv, tf, tq), lambda: pcu.signed_distance_to_mesh(tq, tv, tf),
                 lambda: pcu.triangle_soup_fast_winding_number(v, f, bad)):
        with pytest.raises(ValueError, match="p must not contain NaN or infinite coordinates"):
            call()
    assert torch.cuda.is_available()
