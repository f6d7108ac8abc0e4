"""mesh_vertex_adjacency, adjacency_list and laplacian_smooth_mesh on the GPU (-m gpu) against tests/mesh_smooth_contract.py (DESIGN.md, row
f15): the adjacency equals the loop over Python sets exactly; the smoothing is measured against the float64 direct solve of the same system
(numpy's dense solve up to 1,089 vertices, scipy's sparse one above) and may err at most four times as much as the numpy restatement of the
contract run in the input dtype does against that same solve, relative to the largest coordinate.

The restatement's own errors, measured on the CPU (3 iterations; uniform / cotangent): float32 bunny 1.5e-4 / 8.3e-5, sphere4098
5.1e-6 / 3.3e-5, cube_twist 1.7e-5 / 1.9e-5, grid33 3.4e-5 / 1.1e-4, fan700 6.0e-6 / 4.4e-5, book300 1.8e-6 / 1.2e-4; float64 bunny
2.6e-13 / 1.4e-13, the others 1e-15 to 7e-14. Its solves took 1-37 iterations in float32 and 3-144 in float64 (bunny: 17-18 / 23-37 and
78 / 102-144), from x0 = u. Every test prints its own pair of figures."""
import numpy as np
import pytest

import mesh_smooth_contract as C

pytestmark = pytest.mark.gpu

FLOATS = [np.float32, np.float64]
SPARSE_FROM = 1500                    # vertices from which the direct solve is scipy's sparse one


@pytest.fixture(scope="module")
def pcu():
    import point_cloud_utils_amd as m
    from point_cloud_utils_amd import _lib
    assert _lib.device_count() > 0, "no GPU visible: the gfx950 path has no CPU fallback"
    return m


def to_torch(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


# ---------------------------------------------------------------------------------------------------- adjacency
_SETS = {}


def sets_of(name):
    if name not in _SETS:
        v, f = C.mesh(name)
        _SETS[name] = C.adjacency_sets(f, len(v))
    return _SETS[name]


@pytest.mark.parametrize("kind", [np.int32, np.int64])
@pytest.mark.parametrize("name", C.MESH_NAMES)
def test_adjacency_equals_the_set_loop(pcu, name, kind):
    v, f = C.mesh(name)
    want_off, want_nb = sets_of(name)
    off, nb = pcu.mesh_vertex_adjacency(f.astype(kind), num_vertices=len(v))
    assert off.dtype == np.int64 and nb.dtype == np.dtype(kind)
    assert np.array_equal(off, want_off) and np.array_equal(nb, want_nb)
    st = pcu.last_stats()
    assert st["n_queries"] == len(f) and st["n_escalated"] == len(want_nb)
    toff, tnb = pcu.mesh_vertex_adjacency(to_torch(f.astype(kind)), num_vertices=len(v))
    assert toff.is_cuda and tnb.is_cuda and np.array_equal(toff.cpu().numpy(), off) and tnb.cpu().numpy().tobytes() == nb.tobytes()


@pytest.mark.parametrize("name", ["tetrahedron", "defective", "fan700", "bunny"])
def test_adjacency_list_equals_the_set_loop_as_lists(pcu, name):
    v, f = C.mesh(name)
    top = int(f.max()) + 1
    off, nb = C.adjacency_sets(f, top)
    want = [nb[off[i]:off[i + 1]].tolist() for i in range(top)]
    got = pcu.adjacency_list(f.astype(np.int32))
    assert isinstance(got, list) and len(got) == top and all(isinstance(r, list) for r in got)
    assert got == want
    assert pcu.adjacency_list(to_torch(f)) == want


def test_adjacency_rows_of_repeated_and_missing_vertices(pcu):
    f = np.array([[0, 1, 1], [3, 3, 3], [5, 0, 1], [5, 0, 1]])
    off, nb = pcu.mesh_vertex_adjacency(f, num_vertices=7)
    assert off.tolist() == [0, 2, 4, 4, 4, 4, 6, 6] and nb.tolist() == [1, 5, 0, 5, 0, 1]
    assert pcu.adjacency_list(f) == [[1, 5], [0, 5], [], [], [], [0, 1]]
    off, nb = pcu.mesh_vertex_adjacency(np.array([[0, 0, 0]]))
    assert off.tolist() == [0, 0] and nb.shape == (0,)
    with pytest.raises(ValueError, match=r"found a face index outside \[0, 5\)"):
        pcu.mesh_vertex_adjacency(to_torch(f), num_vertices=5)


# ---------------------------------------------------------------------------------------------------- smoothing
_REF = {}


def references(name, T, cotan, iters):
    """(the float64 direct solve, the restatement in T, its solves' iteration counts) for the mesh rounded to T."""
    key = (name, np.dtype(T).name, cotan, iters)
    if key not in _REF:
        v, f = C.mesh(name)
        vt = v.astype(T)
        sparse = len(v) >= SPARSE_FROM
        if sparse:
            pytest.importorskip("scipy.sparse.linalg")
        direct = C.smooth_direct(vt, f, iters, 0.1, cotan, sparse=sparse)
        model, counts = C.smooth(vt, f, iters, 0.1, cotan)
        _REF[key] = (direct, model, counts)
    return _REF[key]


@pytest.mark.parametrize("iters", [1, 3])
@pytest.mark.parametrize("cotan", [False, True])
@pytest.mark.parametrize("T", FLOATS)
@pytest.mark.parametrize("name", C.MESH_NAMES)
def test_smoothing_is_within_four_times_the_restatements_own_error(pcu, name, T, cotan, iters):
    v, f = C.mesh(name)
    direct, model, counts = references(name, T, cotan, iters)
    scale = float(np.abs(direct).max())
    model_err = float(np.abs(model.astype(np.float64) - direct).max()) / scale
    u = pcu.laplacian_smooth_mesh(v.astype(T), f, iters, 0.1, cotan)
    st = pcu.last_stats()
    gpu_err = float(np.abs(u.astype(np.float64) - direct).max()) / scale
    print(f"smooth {name} {np.dtype(T).name} cotan={cotan} iters={iters}: restatement {model_err:.3e} ({counts}) gpu {gpu_err:.3e} ({st['n_passes']})")
    assert u.dtype == np.dtype(T) and u.shape == v.shape and np.isfinite(u).all()
    assert st["n_passes"] > 0 and st["n_queries"] == len(v)
    assert gpu_err <= 4 * model_err
    if cotan:
        assert abs(C.surface_area(u, f) - 1.0) <= 1000 * np.finfo(T).eps


@pytest.mark.parametrize("T", FLOATS)
@pytest.mark.parametrize("name", ["defective", "sphere4098", "fan700"])
def test_exact_properties(pcu, name, T):
    v, f = C.mesh(name)
    v = v.astype(T)
    assert pcu.laplacian_smooth_mesh(v, f, 0).tobytes() == v.tobytes()
    assert pcu.laplacian_smooth_mesh(v, f, 0, use_cotan_weights=True).tobytes() == v.tobytes()
    assert pcu.laplacian_smooth_mesh(v, f, 2, step_size=0.0).tobytes() == v.tobytes()     # from x0 = u the first residual is exactly zero
    for cotan in (False, True):
        a = pcu.laplacian_smooth_mesh(v, f, 2, 0.1, cotan)
        n_passes = pcu.last_stats()["n_passes"]
        assert n_passes > 0 and a.tobytes() != v.tobytes()
        assert pcu.laplacian_smooth_mesh(v, f, 2, 0.1, cotan).tobytes() == a.tobytes()
        for kind in (np.int32, np.int64):
            t = pcu.laplacian_smooth_mesh(to_torch(v), to_torch(f.astype(kind)), 2, 0.1, cotan)
            assert t.is_cuda and t.cpu().numpy().tobytes() == a.tobytes()
            assert pcu.last_stats()["n_passes"] == n_passes


@pytest.mark.parametrize("T", FLOATS)
def test_vertices_without_mass_keep_their_bytes(pcu, T):
    v, f, loose = C.defective_sphere()
    v = v.astype(T)
    for cotan in (False, True):
        u = pcu.laplacian_smooth_mesh(v, f, 3, 0.1, cotan)
        assert u[loose].tobytes() == v[loose].tobytes()
        assert np.isfinite(u).all()


def test_value_errors(pcu):
    v, f = C.mesh("sphere258")
    bad_v = v.copy(); bad_v[7, 1] = np.nan
    bad_f = f.copy(); bad_f[100, 2] = len(v)
    with pytest.raises(ValueError, match="Invalid value for argument num_iters in smooth_mesh_laplacian. Must be a positive integer or 0."):
        pcu.laplacian_smooth_mesh(to_torch(v), to_torch(f), -2)
    with pytest.raises(ValueError, match="step_size must be finite and not negative"):
        pcu.laplacian_smooth_mesh(to_torch(v), to_torch(f), 1, step_size=-1.0)
    with pytest.raises(ValueError, match="v must not contain NaN or infinite coordinates"):
        pcu.laplacian_smooth_mesh(bad_v, f, 1)
    with pytest.raises(ValueError, match=r"found a face index outside \[0, 258\)"):
        pcu.laplacian_smooth_mesh(v, bad_f, 1)
    # for tensors both are found on the device
    with pytest.raises(ValueError, match="v must not contain NaN or infinite coordinates"):
        pcu.laplacian_smooth_mesh(to_torch(bad_v), to_torch(f), 1)
    with pytest.raises(ValueError, match=r"found a face index outside \[0, 258\)"):
        pcu.laplacian_smooth_mesh(to_torch(v), to_torch(bad_f), 1, use_cotan_weights=True)
    with pytest.raises(ValueError, match=r"Invalid scalar type \(uint32\) for argument 'f'"):
        pcu.laplacian_smooth_mesh(v, f.astype(np.uint32), 1)
    with pytest.raises(ValueError, match=r"Invalid scalar type \(float32\) for argument 'f'"):
        pcu.mesh_vertex_adjacency(f.astype(np.float32))
    # the library is usable after a refusal
    assert np.isfinite(pcu.laplacian_smooth_mesh(v, f, 1)).all()
