"""orient_point_cloud_normals on the GPU (-m gpu) against tests/orient_contract.py, which is fed the library's own k_nearest_neighbors(P, P, m):
dtype, shape and bytes of the normals and of the flipped mask, no tolerance, float32 and float64, numpy arrays and device tensors, equal calls
with equal bytes. The shapes are the smallest that reach each path of csrc/orient.h: m = n, one wave and its edges, hook chains thousands of
rows deep, a lattice on which every choice is made by (lo, hi) and every mutual pair must be seen, several trees, coincident copies,
non-finite normals. Then a million rows with the whole chip racing, checked by what is known without the contract. There is no cancel test
(DESIGN.md, f23), and this file sorts behind tests/test_gpu_mesh_sampling.py (Tests)."""
import os

import numpy as np
import pytest

import orient_contract as oc

pytestmark = pytest.mark.gpu

DTYPES = [np.float32, np.float64]
HERE = os.path.dirname(os.path.abspath(__file__))


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
        assert g.tobytes() == w.tobytes(), (np.nonzero((g != w).reshape(len(g), -1).any(axis=1))[0][:8], g[:4], w[:4])


def contract(pcu, p, nrm, k, leaf=10):
    n = len(p)
    _, nbr = pcu.k_nearest_neighbors(p, p, min(k + 1, n), max_points_per_leaf=leaf)
    return oc.neighbours(nbr, n), oc.orient(p, nrm, oc.neighbours(nbr, n))


def check(pcu, p, nrm, k, tensors=True, leaf=10):
    """(normals, flipped) twice and the normals alone -- numpy, then tensors -- against the contract. Returns (the contract's, trees in the stats)."""
    nbr, want = contract(pcu, p, nrm, k, leaf)
    assert want[0].dtype == p.dtype and want[1].dtype == np.bool_
    kinds = [(p, nrm)]
    if tensors:
        import torch
        kinds.append((torch.from_numpy(p).cuda(), torch.from_numpy(nrm).cuda()))
    trees = None
    for a, b in kinds:
        got = pcu.orient_point_cloud_normals(a, b, k, return_flipped=True, max_points_per_leaf=leaf)
        st = pcu.last_stats()
        assert type(got) is tuple and all(type(g) is type(a) for g in got)
        if hasattr(a, "device"):
            assert all(g.device == a.device for g in got)
        same(got, want)
        same(pcu.orient_point_cloud_normals(a, b, k, return_flipped=True, max_points_per_leaf=leaf), want)      # equal calls, equal bytes
        alone = pcu.orient_point_cloud_normals(a, b, k=k, max_points_per_leaf=leaf)
        assert type(alone) is type(a)
        same([alone], want[:1])
        trees = oc.num_trees(p, nrm, nbr) if trees is None else trees
        assert st["n_escalated"] == trees and st["n_queries"] == len(p)
        assert st["n_passes"] <= max(1, int(np.ceil(np.log2(max(len(p), 2)))))
    return want, trees


def unit(rng, n, dtype):
    v = rng.standard_normal((n, 3))
    return (v / np.linalg.norm(v, axis=1, keepdims=True)).astype(dtype)


@pytest.mark.parametrize("dtype", DTYPES)
def test_small_sizes_around_a_wave(pcu, dtype):
    rng = np.random.default_rng(1)
    for n in (1, 2, 3, 63, 64, 65, 257):
        p = rng.random((n, 3)).astype(dtype)
        nrm = rng.standard_normal((n, 3)).astype(dtype)
        for k in (1, 3, 10, 70):
            (_, flipped), trees = check(pcu, p, nrm, k, tensors=(n, k) in ((1, 1), (65, 3), (257, 10), (64, 70)))
            if k >= n - 1:
                assert trees == 1
            if n == 1:
                assert flipped[0] == (nrm[0, 2] < 0)


@pytest.mark.parametrize("dtype", DTYPES)
def test_a_shuffled_helix_of_five_thousand_points(pcu, dtype):
    """k = 1, 2 along a curve in shuffled rows: hook chains as deep as runs of the curve are long, many trees at k = 1."""
    rng = np.random.default_rng(2)
    t = np.linspace(0.0, 40.0 * np.pi, 5000)
    p = np.stack([np.cos(t), np.sin(t), 0.01 * t], axis=1)[rng.permutation(5000)].astype(dtype)
    nrm = unit(rng, 5000, dtype)
    _, trees = check(pcu, p, nrm, 1)
    assert trees >= 100
    _, trees = check(pcu, p, nrm, 2, tensors=False)
    assert trees <= 10


@pytest.mark.parametrize("dtype", DTYPES)
def test_an_exact_lattice_where_every_weight_is_zero(pcu, dtype):
    """64 x 64 points with normals exactly +-(0, 0, 1): d = +-1, w = 0 on every edge, so (lo, hi) alone makes every choice."""
    rng = np.random.default_rng(3)
    i = np.arange(64)
    p = np.zeros((4096, 3), dtype)
    p[:, :2] = np.stack(np.meshgrid(i, i, indexing="ij"), axis=-1).reshape(-1, 2)[rng.permutation(4096)] * 0.25
    nrm = np.zeros((4096, 3), dtype)
    nrm[:, 2] = rng.choice([-1.0, 1.0], size=4096)
    for k in (4, 8):
        (out, flipped), trees = check(pcu, p, nrm, k, tensors=k == 4)
        assert trees == 1 and (out[:, 2] == 1.0).all() and np.array_equal(flipped, nrm[:, 2] < 0)


def sphere(rng, n, centre=(0.0, 0.0, 0.0), radius=1.0):
    true = rng.standard_normal((n, 3))
    true /= np.linalg.norm(true, axis=1, keepdims=True)
    return true * radius + np.asarray(centre), true


@pytest.mark.parametrize("dtype", DTYPES)
def test_several_trees_each_with_its_own_reference_row(pcu, dtype):
    """Two spheres, a clump and a handful of isolated points far from all of them: at k = 6 each group of at least seven rows lists only its
    own rows, so each is a tree with a reference row of its own (a sphere's topmost row looks up: outward). The tree count comes back in
    the stats."""
    rng = np.random.default_rng(4)
    pa, ta = sphere(rng, 700)
    pb, tb = sphere(rng, 500, centre=(50.0, 0.0, -20.0), radius=2.0)
    pc, tc = sphere(rng, 9, centre=(-80.0, 30.0, 5.0), radius=0.01)
    lone = rng.random((7, 3)) * 1000.0 + 1.0e5
    p = np.concatenate([pa, pb, pc, lone])
    true = np.concatenate([ta, tb, tc, unit(rng, 7, np.float64)])
    order = rng.permutation(len(p))
    p, true = p[order].astype(dtype), true[order]
    nrm = (true * rng.choice([-1.0, 1.0], size=(len(p), 1))).astype(dtype)
    (out, _), trees = check(pcu, p, nrm, 6)
    assert trees == 4
    on_spheres = order < 1200
    assert ((out.astype(np.float64) * true).sum(axis=1) > 0)[on_spheres].all()


@pytest.mark.parametrize("dtype", DTYPES)
def test_a_cloud_concatenated_with_itself(pcu, dtype):
    """Coincident copies push a row out of its own neighbour row: then all m entries are edges."""
    rng = np.random.default_rng(5)
    p = rng.random((300, 3)).astype(dtype)
    nrm = unit(rng, 300, dtype)
    for k in (1, 2, 5):
        check(pcu, np.concatenate([p, p]), np.concatenate([nrm, -nrm]), k, tensors=k == 2)
    check(pcu, np.concatenate([p, p, p, p]), np.concatenate([nrm, -nrm, nrm, nrm]), 2, tensors=False)


@pytest.mark.parametrize("dtype", DTYPES)
def test_non_finite_and_zero_normals(pcu, dtype):
    """A row with a NaN or infinite normal is a tree of its own and keeps its bytes (its normal_z is not < 0 here); zero rows take part."""
    rng = np.random.default_rng(6)
    p = rng.random((400, 3)).astype(dtype)
    nrm = unit(rng, 400, dtype)
    nrm[3] = [np.nan, 1.0, 1.0]
    nrm[70] = [np.inf, 0.0, 0.0]
    nrm[71] = [0.0, -np.inf, np.nan]
    nrm[200] = np.nan
    nrm[[9, 64, 399]] = 0.0
    (out, flipped), trees = check(pcu, p, nrm, 8)
    assert trees >= 5
    for r in (3, 70, 71, 200):
        assert not flipped[r] and out[r].tobytes() == nrm[r].tobytes()
    nrm[3, 2] = -1.0                                                        # (rule 4 holds for a lone row too)
    (out, flipped), _ = check(pcu, p, nrm, 8, tensors=False)
    assert flipped[3]


def test_the_clouds_non_finite_rule(pcu):
    import torch
    rng = np.random.default_rng(7)
    p = rng.random((257, 3)).astype(np.float32)
    nrm = unit(rng, 257, np.float32)
    want, _ = check(pcu, p, nrm, 5)
    p2 = np.insert(p, 10, np.asarray([np.inf, 0.5, 0.5], np.float32), axis=0)       # single-signed: the search's to handle
    n2 = np.insert(nrm, 10, nrm[0], axis=0)
    check(pcu, p2, n2, 5)
    for bad in ((5, 0, np.nan, None), (5, 1, np.inf, -np.inf)):
        p3 = p.copy()
        p3[bad[0], bad[1]] = bad[2]
        if bad[3] is not None:
            p3[200, bad[1]] = bad[3]
        for a, b in ((p3, nrm), (torch.from_numpy(p3).cuda(), torch.from_numpy(nrm).cuda())):
            with pytest.raises(ValueError, match="dataset_points contains NaN coordinates, or both"):
                pcu.orient_point_cloud_normals(a, b, 5)
    same(pcu.orient_point_cloud_normals(p, nrm, 5, return_flipped=True), want)      # the context answers as before


def torus(rng, n):
    u, v = rng.random(n) * 2.0 * np.pi, rng.random(n) * 2.0 * np.pi
    true = np.stack([np.cos(v) * np.cos(u), np.cos(v) * np.sin(u), np.sin(v)], axis=1)
    return np.stack([np.cos(u), np.sin(u), np.zeros(n)], axis=1) + 0.35 * true, true


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("shape", ["sphere", "torus"])
def test_surfaces_with_randomly_flipped_true_normals(pcu, dtype, shape):
    rng = np.random.default_rng(8)
    p, true = sphere(rng, 20000) if shape == "sphere" else torus(rng, 20000)
    sign = rng.choice([-1.0, 1.0], size=(20000, 1))
    (out, flipped), trees = check(pcu, p.astype(dtype), (true * sign).astype(dtype), 10)
    if shape == "sphere":
        assert trees == 1 and ((out.astype(np.float64) * true).sum(axis=1) > 0).all() and np.array_equal(flipped, sign[:, 0] < 0)


def test_bunny_normals_do_not_depend_on_the_input_signs(pcu):
    v = np.load(os.path.join(HERE, "golden", "bunny_v.npy"))
    idx, nrm = pcu.estimate_point_cloud_normals_knn(v, 12)
    assert len(idx) == len(v)
    (out, _), _ = check(pcu, v, nrm, 10, tensors=False)
    rng = np.random.default_rng(9)
    for _ in range(3):
        sign = rng.choice(np.array([-1.0, 1.0], v.dtype), size=(len(v), 1))
        same([pcu.orient_point_cloud_normals(v, nrm * sign, 10)], [out])


@pytest.mark.parametrize("dtype", DTYPES)
def test_a_million_shuffled_sphere_rows(pcu, dtype):
    """2^20 rows, device-resident: every compute unit offers, hooks and flattens at once. Too large for the Python contract: all normals
    point outward, a flipped input gives the same bytes, and the call run twice gives the same bytes."""
    import torch
    n = 1 << 20
    rng = np.random.default_rng(10)
    true = rng.standard_normal((n, 3)).astype(np.float32)
    true /= np.linalg.norm(true, axis=1, keepdims=True)
    sign = rng.choice(np.array([-1.0, 1.0], np.float32), size=(n, 1))
    p = torch.from_numpy(true.astype(dtype)).cuda()
    t = torch.from_numpy(true.astype(dtype)).cuda()
    a = torch.from_numpy((true * sign).astype(dtype)).cuda()
    out, flipped = pcu.orient_point_cloud_normals(p, a, 10, return_flipped=True)
    st = pcu.last_stats()
    assert st["n_escalated"] == 1 and 1 <= st["n_passes"] <= 20
    assert bool(((out * t).sum(dim=1) > 0).all())
    assert bool((flipped == torch.from_numpy(sign[:, 0] < 0).cuda()).all())
    assert bool((out == t).all())
    again = pcu.orient_point_cloud_normals(p, a, 10)
    assert torch.equal(again.view(torch.uint8), out.view(torch.uint8))
    other = pcu.orient_point_cloud_normals(p, -a, 10)
    assert torch.equal(other.view(torch.uint8), out.view(torch.uint8))


def test_kinds_flags_and_the_c_entry_point(pcu):
    """numpy in and tensor in give the same bytes; return_flipped agrees with the signs; what the C side answers and refuses."""
    import ctypes
    import torch
    from point_cloud_utils_amd import _lib
    rng = np.random.default_rng(11)
    p = rng.random((3000, 3)).astype(np.float32)
    nrm = unit(rng, 3000, np.float32)
    out, flipped = pcu.orient_point_cloud_normals(p, nrm, return_flipped=True)
    assert type(out) is np.ndarray and out.dtype == np.float32 and flipped.dtype == np.bool_
    t_out, t_flipped = pcu.orient_point_cloud_normals(torch.from_numpy(p).cuda(), torch.from_numpy(nrm).cuda(), return_flipped=True)
    assert t_out.is_cuda and t_flipped.dtype == torch.bool
    same([t_out, t_flipped], [out, flipped])
    assert out.tobytes() == np.where(flipped[:, None], -nrm, nrm).tobytes()
    assert np.array_equal(np.signbit(out) != np.signbit(nrm), np.repeat(flipped[:, None], 3, axis=1))
    _, want = contract(pcu, p, nrm, 10)
    same([out, flipped], want)
    L, ctx, st = _lib.lib(), _lib.ctx(), _lib.Stats()
    c_out, c_flip = np.full((3000, 3), -7, np.float32), np.full(3000, 9, np.uint8)
    rc = L.pcu_hip_orient_normals_f32(ctx, p.ctypes.data, nrm.ctypes.data, 3000, 10, 10, c_out.ctypes.data, c_flip.ctypes.data, 0, None, ctypes.addressof(st))
    assert rc == 0 and c_out.tobytes() == out.tobytes() and np.array_equal(c_flip, flipped.astype(np.uint8))
    assert st.n_queries == 3000 and st.n_escalated == 1 and 1 <= st.n_passes <= 12 and st.n_grid_builds >= 1
    c_out[:] = -7
    rc = L.pcu_hip_orient_normals_f32(ctx, p.ctypes.data, nrm.ctypes.data, 3000, 2 ** 40, 10, c_out.ctypes.data, None, 0, None, ctypes.addressof(st))     # no mask; k beyond the cloud
    assert rc == 0 and st.n_escalated == 1
    same([c_out], [pcu.orient_point_cloud_normals(p, nrm, 2999)])
    for args, text in (((p.ctypes.data, nrm.ctypes.data, 3000, 0), "Invalid number of neighbors"), ((p.ctypes.data, nrm.ctypes.data, 0, 10), "zero elements"),
                       ((None, nrm.ctypes.data, 3000, 10), "null points"), ((p.ctypes.data, None, 3000, 10), "null points")):
        rc = L.pcu_hip_orient_normals_f32(ctx, *args, 10, c_out.ctypes.data, None, 0, None, ctypes.addressof(st))
        assert rc == _lib.ERR_INVALID
        with pytest.raises(ValueError, match=text):
            _lib.check(rc)
