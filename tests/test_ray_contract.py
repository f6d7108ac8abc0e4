"""ray_mesh_intersection on the CPU: the contract (tests/ray_contract.py) is watertight, exact where the arithmetic is exact, unchanged by its
box clip and accurate against an independent float64 formulation; validation happens before any device work; the ray kernels of the shipped
binary use no scratch memory.

The bound B_RAY. |o + t d - x64| and |bc . tri - x64| <= B_RAY * eps(T) * max(S, |o|), x64 the crossing the float64 formulation finds. It is four
times the largest figure test_accuracy_against_independent_float64 prints (the factor 4 is row f6's convention); the figures are recorded in
ray_contract.py and DESIGN.md row f7. Both figures of a ray are nearly equal: t is interpolated from the same edge functions as bc, so o + t d
and bc . tri are the same point up to a few eps, and the error is that of the edge functions, eps |a - o|^2 over the face's projected size."""
import numpy as np
import pytest

import mesh_contract as mc
import ray_contract as rc

DTYPES = [np.float32, np.float64]
ORIGINS = [(0.0, 0.0, 0.0), (0.3, -0.2, 0.5), (0.0, 0.0, 0.9)]


# ---------------------------------------------------------------------------------------------------- the restatement
@pytest.mark.parametrize("T", DTYPES)
def test_restatement_is_watertight_on_a_closed_sphere(T):
    v, f = mc.sphere(16, T)
    for k, origin in enumerate(ORIGINS):
        o, d = rc.rays_at_edges_and_vertices(v, f, origin, 4000, T, seed=5 + k)
        fid, bc, t = rc.hit_brute(o, d, 0.0, np.inf, v, f)
        print(f"{np.dtype(T).name} origin {origin}: {int((fid < 0).sum())} misses of {len(d)}")
        assert (fid >= 0).all() and np.isfinite(t).all() and (t > 0).all()


@pytest.mark.parametrize("T", DTYPES)
def test_exact_zeros_of_the_edge_functions_on_the_octahedron(T):
    """Rays from the centre exactly at the 6 vertices and the 12 edge midpoints: every ray hits, and the face is the lowest index among the
    faces that share the target."""
    v, f = rc.octahedron(T)
    v64 = v.astype(np.float64)
    targets, want = [], []
    for i in range(6):
        targets.append(v64[i]); want.append(min(k for k in range(8) if i in f[k]))
    for i in range(6):
        for j in range(i + 1, 6):
            if np.abs(v64[i] + v64[j]).sum() > 0:                         # (not opposite corners: an edge)
                targets.append((v64[i] + v64[j]) / 2); want.append(min(k for k in range(8) if i in f[k] and j in f[k]))
    assert len(targets) == 18
    d = np.array(targets).astype(T)
    fid, bc, t = rc.hit_brute(np.zeros(3, T), d, 0.0, np.inf, v, f)
    assert fid.tolist() == want and np.array_equal(t, np.ones(18, T))
    x = np.einsum("ij,ijk->ik", bc.astype(np.float64), v64[f[fid]])
    assert np.array_equal(x, np.array(targets))                            # (bc is exact too)


@pytest.mark.parametrize("T", DTYPES)
@pytest.mark.parametrize("mesh", ["bunny", "sphere"])
def test_box_clip_never_changes_the_first_face(mesh, T):
    """Step 3 exists so that the traversal may prune by boxes; it must not bite a hit that step 1 accepts."""
    v, f = mc.bunny(T) if mesh == "bunny" else mc.sphere(24, T)
    n = 400
    edges, verts = rc.edge_and_vertex_targets(v, f, n, seed=17)
    targets = np.concatenate([edges, verts])
    for kind, (o, _) in (("near", rc.rays_box_to_surface(v, f, 2 * n, np.float64, 18)), ("far", rc.rays_far_to_surface(v, f, 2 * n, np.float64, 19))):
        o, d = o.astype(T), (targets - o).astype(T)
        with_clip = rc.hit_brute(o, d, 0.0, np.inf, v, f)
        without = rc.hit_brute(o, d, 0.0, np.inf, v, f, clip=False)
        print(f"{mesh} {np.dtype(T).name} {kind}: {int((with_clip[0] >= 0).sum())} of {len(d)} rays hit; first face differs on "
              f"{int((with_clip[0] != without[0]).sum())}")
        assert np.array_equal(with_clip[0], without[0]) and (without[0] >= 0).sum() > 0.9 * len(d)


@pytest.mark.parametrize("T", DTYPES)
@pytest.mark.parametrize("mesh", ["bunny", "sphere", "cube_twist"])
def test_accuracy_against_independent_float64(mesh, T):
    v, f = {"bunny": mc.bunny, "sphere": lambda t: mc.sphere(32, t), "cube_twist": rc.cube_twist}[mesh](T)
    o, d = rc.rays_box_to_surface(v, f, 1500, T, seed=7)
    got = rc.hit_brute(o, d, 0.0, np.inf, v, f)
    e_ray, e_bc, left_out, compared = rc.excess(o, d, v, f, got, T)
    print(f"{mesh} {np.dtype(T).name}: |o + t d - x64| <= {e_ray:.1f}, |bc . tri - x64| <= {e_bc:.1f} eps*max(S,|o|) over {compared} rays; "
          f"left out {100 * left_out:.2f} %")
    assert left_out <= 0.005 and compared >= 0.99 * len(d)
    assert e_ray <= rc.B_RAY and e_bc <= rc.B_RAY
    eps = np.finfo(T).eps
    hit = got[0] >= 0
    assert np.abs(got[1][hit].astype(np.float64).sum(1) - 1).max() <= 2 * eps and not np.isnan(got[1]).any()


@pytest.mark.parametrize("mesh", ["bunny", "sphere"])
def test_float32_and_float64_evaluations_agree_on_the_face(mesh):
    v, f = mc.bunny(np.float32) if mesh == "bunny" else mc.sphere(32, np.float32)
    o, d = rc.rays_box_to_surface(v, f, 800, np.float32, seed=27)
    f32 = rc.hit_brute(o, d, 0.0, np.inf, v, f)
    f64 = rc.hit_brute(o.astype(np.float64), d.astype(np.float64), 0.0, np.inf, v.astype(np.float64), f)
    differ = int((f32[0] != f64[0]).sum())
    print(f"{mesh}: the face differs between the float32 and the float64 evaluation on {differ} of {len(d)} rays")
    assert differ <= 0.005 * len(d)


def test_window_misses_and_zero_direction():
    v, f = rc.octahedron(np.float64)
    o = np.array([[0.1, 0.05, -3.0]] * 6)
    d = np.array([[0.0, 0.0, 1.0]] * 5 + [[0.0, 0.0, 0.0]])
    want_near, want_far = 3.0 - (1 - 0.15), 3.0 + (1 - 0.15)               # the two crossings of the line x = .1, y = .05
    for k, (near, far, t_want) in enumerate([(0.0, np.inf, want_near), (2.5, np.inf, want_far), (0.0, 2.0, np.inf), (4.0, 1.0, np.inf),
                                             (-10.0, np.inf, want_near)]):
        fid, bc, t = rc.hit_brute(o[k:k + 1], d[k:k + 1], near, far, v, f)
        assert (t[0] == np.inf and fid[0] == -1 and not bc.any()) if t_want == np.inf else abs(t[0] - t_want) < 1e-12, (near, far, t, fid)
    fid, bc, t = rc.hit_brute(o[5:], d[5:], 0.0, np.inf, v, f)
    assert fid[0] == -1 and t[0] == np.inf and not bc.any()                # a zero direction: everything NaN, a miss
    fid, bc, t = rc.hit_brute(o[:1], -d[:1], -10.0, np.inf, v, f)          # behind the origin, allowed by a negative near: the smallest t
    assert fid[0] >= 0 and abs(t[0] + want_far) < 1e-12


def test_candidate_lists_give_the_rows_of_the_full_loop():
    v, f = mc.bunny(np.float32)
    o, d = rc.rays_box_to_surface(v, f, 300, np.float32, seed=37)
    full = rc.hit_brute(o, d, 0.0, np.inf, v, f)
    cand = rc.box_candidates(o, d, v, f)
    part = rc.hit_brute(o, d, 0.0, np.inf, v, f, faces=cand)
    assert all(np.array_equal(a, b) for a, b in zip(full, part)) and np.mean([len(c) for c in cand]) < 0.02 * len(f)


def test_reference_test_body_on_the_restatement():
    """tests/test_examples.py:570-608 of the reference, with hit_brute in place of the binding."""
    import point_cloud_utils_amd as pcu
    v, f = rc.cube_twist(np.float64)
    assert v.shape == (6146, 3) and f.shape == (12288, 3)
    d = np.concatenate([np.stack([a.ravel() for a in np.mgrid[-0.1:0.1:64j, -0.1:0.1:64j]], axis=-1), 0.1 * np.ones([64 ** 2, 1])], axis=-1)
    d /= np.linalg.norm(d, axis=-1, keepdims=True)
    o1 = np.array([0., 0., -2.])
    fid1, bc1, t1 = rc.hit_brute(o1, d, 0.0, np.inf, v, f)
    mask1 = np.isfinite(t1)
    assert mask1.sum() > 0
    p11 = pcu.interpolate_barycentric_coords(f, fid1[mask1], bc1[mask1], v)
    p12 = o1 + t1[mask1, np.newaxis] * d[mask1]
    assert np.allclose(p11, p12, atol=1e-5)
    o2 = np.stack([o1] * d.shape[0])
    fid2, bc2, t2 = rc.hit_brute(o2, d, 0.0, np.inf, v, f)
    mask2 = np.isfinite(t2)
    p21 = pcu.interpolate_barycentric_coords(f, fid2[mask2], bc2[mask2], v)
    p22 = o2[mask2] + t2[mask2, np.newaxis] * d[mask2]
    assert np.allclose(p21, p22, atol=1e-5)
    assert np.all(mask1 == mask2) and np.all(fid2 == fid1) and np.allclose(bc2, bc1) and np.allclose(t1, t2)
    assert 0.5 * len(d) < mask1.sum() < len(d)                             # (the fan is wider than the twisted cube: a third of it misses)


# ---------------------------------------------------------------------------------------------------- validation (numpy input: no device work)
def _case():
    v = np.random.default_rng(0).random((8, 3)).astype(np.float32)
    f = np.array([[0, 1, 2], [2, 3, 4], [5, 6, 7]], dtype=np.int64)
    o = np.random.default_rng(1).random((5, 3)).astype(np.float32)
    d = np.random.default_rng(2).random((5, 3)).astype(np.float32)
    return v, f, o, d


ROWS = r"ray_o and ray_d must have the same number of rows \(one ray origin per ray direction\)\. \(Note: ray_o can have one row to use the same origin for all directions\)"


def test_validation_errors_are_raised_before_the_gpu_is_touched():
    import point_cloud_utils_amd as pcu
    v, f, o, d = _case()
    with pytest.raises(ValueError, match=r"Invalid scalar type \(int32\) for argument 'v'"):
        pcu.ray_mesh_intersection(v.astype(np.int32), f, o, d)
    with pytest.raises(ValueError, match=r"Invalid scalar type \(int16\) for argument 'f'"):
        pcu.ray_mesh_intersection(v, f.astype(np.int16), o, d)
    with pytest.raises(ValueError, match=r"Invalid scalar type \(float64\) for argument 'ray_o'. Expected it to match argument 'v' which is of type float32"):
        pcu.ray_mesh_intersection(v, f, o.astype(np.float64), d)
    with pytest.raises(ValueError, match=r"Invalid scalar type \(float64\) for argument 'ray_d'. Expected it to match argument 'v' which is of type float32"):
        pcu.ray_mesh_intersection(v, f, o, d.astype(np.float64))
    # the reference's order: rows, then ray_o's columns, then ray_d's columns, then the mesh
    with pytest.raises(ValueError, match=ROWS):
        pcu.ray_mesh_intersection(v[:0], f, o[:4, :2], d[:, :2])
    with pytest.raises(ValueError, match=r"Invalid shape for ray_o must have shape \(N, 3\) but got \(5, 2\)\."):
        pcu.ray_mesh_intersection(v[:0], f, o[:, :2], d[:, :2])
    with pytest.raises(ValueError, match=r"Invalid shape for ray_d must have shape \(N, 3\) but got \(5, 2\)\."):
        pcu.ray_mesh_intersection(v[:0], f, o, d[:, :2])
    with pytest.raises(ValueError, match=r"Invalid shape for ray_d must have shape \(N, 3\) but got \(5, 2\)\."):
        pcu.ray_mesh_intersection(v[:0], f, o[0], d[:, :2])               # (three elements: one origin, whatever its shape)
    with pytest.raises(ValueError, match=r"Invalid input mesh with zero elements: v and f must have shape \(n, 3\) and \(m, 3\) \(n, m > 0\)\. Got v\.shape =\(0, 3\), f\.shape = \(3, 3\)\."):
        pcu.ray_mesh_intersection(v[:0], f, o, d)
    with pytest.raises(ValueError, match=r"Only 3D inputs are supported: v and f.*f\.shape = \(3, 2\)"):
        pcu.ray_mesh_intersection(v, f[:, :2], o[:1], d)
    for bad in (np.nan, np.inf, -np.inf):
        for name, k in (("v", 0), ("ray_o", 2), ("ray_d", 3)):
            args = [v.copy(), f, o.copy(), d.copy()]
            args[k][3, 1] = bad
            with pytest.raises(ValueError, match=f"{name} must not contain NaN or infinite coordinates"):
                pcu.ray_mesh_intersection(*args)
        ob = o[0].copy(); ob[2] = bad
        with pytest.raises(ValueError, match="ray_o must not contain NaN or infinite coordinates"):
            pcu.ray_mesh_intersection(v, f, ob, d)
    for kw in ({"ray_near": np.nan}, {"ray_far": np.nan}):
        with pytest.raises(ValueError, match="ray_near and ray_far must not be NaN"):
            pcu.ray_mesh_intersection(v, f, o, d, **kw)
    for dt, badval in ((np.int64, 8), (np.int32, -1), (np.uint32, 8)):
        fb = f.astype(dt); fb[1, 2] = badval
        with pytest.raises(ValueError, match=r"found a face index outside \[0, 8\)"):
            pcu.ray_mesh_intersection(v, fb, o, d)
    big = np.lib.stride_tricks.as_strided(np.zeros(3, dtype=np.float32), shape=(2 ** 27 - 15, 3), strides=(0, 4))
    with pytest.raises(ValueError, match=r"more than 2\^27-16 rows"):
        pcu.ray_mesh_intersection(v, f, o[0], big)
    with pytest.raises(ValueError, match=r"more than 2\^27-16 rows"):
        pcu.ray_mesh_intersection(big, f, o, d)
    for name in ("ray_mesh_intersection", "RayMeshIntersector", "interpolate_barycentric_coords", "MeshIndex"):
        assert name in pcu.__all__ and hasattr(pcu, name)
    assert hasattr(pcu.MeshIndex, "intersect_rays")


def test_interpolate_barycentric_coords_is_the_reference_expression():
    import point_cloud_utils_amd as pcu
    rng = np.random.default_rng(3)
    f = rng.integers(0, 20, (30, 3)); fi = rng.integers(0, 30, 50); bc = rng.random((50, 3)); attr = rng.random((20, 4))
    want = (attr[f[fi]] * bc[:, :, np.newaxis]).sum(1)
    assert np.array_equal(pcu.interpolate_barycentric_coords(f, fi, bc, attr), want)
    import torch
    got = pcu.interpolate_barycentric_coords(*(torch.from_numpy(x) for x in (f.astype(np.int32), fi, bc, attr)))
    assert isinstance(got, torch.Tensor) and np.allclose(got.numpy(), want, rtol=0, atol=1e-15)


def test_no_cpu_fallback_without_gpu():
    import point_cloud_utils_amd as pcu
    from point_cloud_utils_amd import _lib
    if _lib.device_count() > 0:
        pytest.skip("GPU present")
    v, f, o, d = _case()
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        pcu.ray_mesh_intersection(v, f, o, d)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        pcu.RayMeshIntersector(v, f)


def test_new_entry_points_are_cancellable():
    from point_cloud_utils_amd import _lib
    L = _lib.lib()
    for suf in ("f32", "f64"):
        for op in ("ray_mesh_intersection", "mesh_index_rays"):
            name = f"pcu_hip_{op}_{suf}"
            assert name in _lib._COMPUTE_ENTRY_POINTS and getattr(L, name).errcheck is _lib._after_call


# ---------------------------------------------------------------------------------------------------- the shipped code object
def test_ray_kernels_use_no_scratch(tmp_path):
    from test_kernel_resources import _kernel_resources
    res = _kernel_resources(tmp_path)                                      # (skips without the llvm tools or the library)
    rays = {n: r for n, r in res.items() if "k_mesh_rays" in n or "k_mesh_rkeys" in n}
    print(rays)
    assert sum("k_mesh_raysIf" in n for n in rays) == 1 and sum("k_mesh_raysId" in n for n in rays) == 1, sorted(rays)
    assert len(rays) == 4
    for name, r in rays.items():
        assert r["scratch"] == 0 and r["vgpr_spill"] == 0, (name, r)
