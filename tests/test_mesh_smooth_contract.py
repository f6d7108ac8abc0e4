"""CPU tests of the f15 contract: the numpy restatement of tests/mesh_smooth_contract.py is checked against independent formulations
-- the adjacency against a loop over Python sets, the assembled M - h L against a dense float64 build face by face, the conjugate-gradient
smoothing against numpy's direct solve -- and the package's validation errors are raised before the GPU is touched."""
import numpy as np
import pytest

import mesh_smooth_contract as C


@pytest.fixture(scope="module", autouse=True)
def pcu():
    import point_cloud_utils_amd as m
    for name in ("adjacency_list", "mesh_vertex_adjacency", "estimate_mesh_vertex_normals", "laplacian_smooth_mesh"):
        assert callable(getattr(m, name)) and name in m.__all__
    return m


@pytest.mark.parametrize("name", C.MESH_NAMES)
def test_adjacency_restatement_equals_the_set_loop(name):
    v, f = C.mesh(name)
    want_off, want_nb = C.adjacency_sets(f, len(v))
    off, nb = C.adjacency(f, len(v))
    assert np.array_equal(off, want_off) and np.array_equal(nb, want_nb)


def test_adjacency_edge_cases():
    f = np.array([[0, 1, 1], [3, 3, 3], [5, 0, 1], [5, 0, 1]])           # a vertex twice, three times, a duplicated face; 2, 4 and 6 in no face
    off, nb = C.adjacency(f, 7)
    assert off.tolist() == [0, 2, 4, 4, 4, 4, 6, 6] and nb.tolist() == [1, 5, 0, 5, 0, 1]
    pos, ids = C.incidence(f, 7)
    assert ids[pos[1]:pos[2]].tolist() == [1, 2, 8, 11] and pos[2] == pos[3] and pos[7] == 12


def test_assembled_system_equals_a_dense_build_face_by_face():
    v, f = C.mesh("sphere258")
    off, col, val, diag = C.cot_matrix(v, f)
    for h, M in ((0.1, np.ones(len(v))), (1e-4, C.mass(v, f))):
        A = C.system_matrix(off, col, val, diag, M, h)
        want = C.dense_system_by_faces(v, f, h, M)
        assert np.abs(A - want).max() <= 1e-13 * np.abs(want).max()
        assert np.array_equal(A, A.T)                                    # both directions of a pair add the same corners in the same order
        assert np.linalg.eigvalsh(A).min() > 0
    # the barycentric mass is a third of the area of the faces round a vertex
    area = 0.5 * np.linalg.norm(np.cross(v[f[:, 1]] - v[f[:, 0]], v[f[:, 2]] - v[f[:, 0]]), axis=1)
    want_m = np.zeros(len(v))
    np.add.at(want_m, f.reshape(-1), np.repeat(area / 3, 3))
    assert np.abs(C.mass(v, f) - want_m).max() <= 1e-15


@pytest.mark.parametrize("cotan", [False, True])
def test_float64_contract_smoothing_equals_the_direct_solve(cotan):
    v, f = C.mesh("sphere258")
    h = 0.1
    u, counts = C.smooth(v, f, 2, h, cotan)
    assert all(0 < c < 100 for c in counts)
    w = v.copy()
    for _ in range(2):
        M = C.mass(w, f) if cotan else None
        A = C.dense_system_by_faces(v, f, h * 1e-3 if cotan else h, M)
        w = np.linalg.solve(A, w if M is None else M[:, None] * w)
        if cotan:
            tri = w[f]
            n = np.cross(tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0])
            a = 0.5 * np.linalg.norm(n, axis=1)
            c = (a[:, None] * tri.mean(axis=1)).sum(axis=0) / a.sum()
            w = (w - c) / np.sqrt(a.sum()) + c
    assert np.abs(u - w).max() <= 1e-12 * np.abs(w).max()
    assert np.abs(C.smooth_direct(v, f, 2, h, cotan) - w).max() <= 1e-12 * np.abs(w).max()
    if cotan:
        assert abs(C.surface_area(u, f) - 1.0) <= 1e-12


def test_vertices_without_mass_keep_their_position():
    v, f, loose = C.defective_sphere()
    for cotan in (False, True):
        u, _ = C.smooth(v, f, 2, 0.1, cotan)
        assert np.array_equal(u[loose], v[loose])
        assert np.isfinite(u).all()
        assert np.abs(u - C.smooth_direct(v, f, 2, 0.1, cotan)).max() <= 1e-12 * np.abs(v).max()


def test_normals_restatement_on_a_tetrahedron():
    v, f = C.tetrahedron()
    for w in ("uniform", "area", "angle"):
        n = C.vertex_normals(v, f, w)
        assert np.allclose(np.linalg.norm(n, axis=1), 1.0)
        assert np.allclose(n[0], -np.ones(3) / np.sqrt(3))               # the corner at the origin: three unit faces meet symmetrically
    v2 = np.concatenate([v, [[2.0, 2.0, 2.0]]])
    assert np.array_equal(C.vertex_normals(v2, f, "angle")[4], np.zeros(3))


def test_validation_errors_come_before_the_device(pcu):
    v, f = C.tetrahedron()
    f32 = f.astype(np.int32)
    with pytest.raises(ValueError, match=r"Invalid weighting_type must be one of 'uniform', 'angle', or 'area', but got 'cot'"):
        pcu.estimate_mesh_vertex_normals(v, f, "cot")
    with pytest.raises(ValueError, match="Invalid value for argument num_iters in smooth_mesh_laplacian. Must be a positive integer or 0."):
        pcu.laplacian_smooth_mesh(v, f, -1)
    for bad in (-0.1, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="step_size must be finite and not negative"):
            pcu.laplacian_smooth_mesh(v, f, 1, step_size=bad)
    for call in (lambda vv, ff: pcu.estimate_mesh_vertex_normals(vv, ff), lambda vv, ff: pcu.laplacian_smooth_mesh(vv, ff, 1)):
        with pytest.raises(ValueError, match=r"Invalid scalar type \(int64\) for argument 'v'"):
            call(v.astype(np.int64), f)
        with pytest.raises(ValueError, match=r"Invalid scalar type \(float64\) for argument 'f'"):
            call(v, f.astype(np.float64))
        with pytest.raises(ValueError, match="Invalid input mesh with zero elements"):
            call(v, f[:0])
        with pytest.raises(ValueError, match="Only 3D inputs are supported"):
            call(v[:, :2], f)
        with pytest.raises(ValueError, match="v must not contain NaN or infinite coordinates"):
            call(np.where(np.arange(12).reshape(4, 3) == 5, np.nan, v), f)
        with pytest.raises(ValueError, match=r"found a face index outside \[0, 4\)"):
            call(v, f + 1)
        with pytest.raises(ValueError, match=r"found a face index outside \[0, 4\)"):
            call(v, f32 - 1)
    with pytest.raises(ValueError, match=r"Invalid scalar type \(uint32\) for argument 'f'. Expected one of \['int32', 'int64'\]"):
        pcu.laplacian_smooth_mesh(v, f.astype(np.uint32), 1)
    for call in (pcu.adjacency_list, pcu.mesh_vertex_adjacency):
        with pytest.raises(ValueError, match=r"Invalid scalar type \(uint64\) for argument 'f'"):
            call(f.astype(np.uint64))
        with pytest.raises(ValueError, match="Invalid input faces with zero elements"):
            call(f[:0])
        with pytest.raises(ValueError, match="Only triangle inputs are supported"):
            call(np.zeros((3, 4), dtype=np.int64))
        with pytest.raises(ValueError, match=r"found a face index outside \[0, "):
            call(f - 1)
    with pytest.raises(ValueError, match=r"found a face index outside \[0, 3\)"):
        pcu.mesh_vertex_adjacency(f, num_vertices=3)
    with pytest.raises(ValueError, match="num_vertices must be positive"):
        pcu.mesh_vertex_adjacency(f, num_vertices=0)
