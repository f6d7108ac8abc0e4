"""estimate_mesh_vertex_normals on the GPU (-m gpu) against the serial restatement of tests/mesh_smooth_contract.py:
'uniform' and 'area' bit for bit in the dtype; 'angle' within four times the restatement's own error, because atan2 is correctly rounded
on neither side.

The model for 'angle' is the restatement one precision up: float64 for float32 input, and the platform's long double for float64 input (the
float64 restatement is the thing measured there, so it cannot be its own model). Errors are absolute: the rows are unit vectors. The
restatement's errors against its model, measured on the CPU (largest component of any row): float32 3.6e-8 (tetrahedron), 1.1e-7 to
1.4e-7 (the spheres, the grid, cube_twist), 1.6e-6 (bunny), 1.9e-6 (book300), 2.7e-6 (fan700: a sum of 700 terms); float64 1.7e-16 to
2.2e-16, 6.2e-16 (bunny), 5.5e-15 (book300), 5.8e-15 (fan700). Every test prints its own pair of figures."""
import numpy as np
import pytest

import mesh_smooth_contract as C

pytestmark = pytest.mark.gpu

FLOATS = [np.float32, np.float64]


@pytest.fixture(scope="module")
def pcu():
    import point_cloud_utils_amd as m
    from point_cloud_utils_amd import _lib
    assert _lib.device_count() > 0, "no GPU visible: the gfx950 path has no CPU fallback"
    return m


def to_torch(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


_WANT = {}


def want(name, T, weighting):
    key = (name, np.dtype(T).name, weighting)
    if key not in _WANT:
        v, f = C.mesh(name)
        _WANT[key] = C.vertex_normals(v.astype(T), f, weighting)
    return _WANT[key]


@pytest.mark.parametrize("T", FLOATS)
@pytest.mark.parametrize("name", C.MESH_NAMES)
def test_uniform_and_area_equal_the_restatement_bit_for_bit(pcu, name, T):
    v, f = C.mesh(name)
    v = v.astype(T)
    for weighting in ("uniform", "area"):
        n = pcu.estimate_mesh_vertex_normals(v, f, weighting)
        w = want(name, T, weighting)
        assert n.dtype == np.dtype(T) and n.shape == v.shape
        assert n.tobytes() == w.tobytes(), (name, weighting, int((n != w).any(axis=1).sum()), float(np.abs(n - w).max()))
    assert pcu.last_stats()["n_queries"] == len(v)


@pytest.mark.parametrize("T", FLOATS)
@pytest.mark.parametrize("name", C.MESH_NAMES)
def test_angle_is_within_four_times_the_restatements_own_error(pcu, name, T):
    v, f = C.mesh(name)
    v = v.astype(T)
    up = np.float64 if T is np.float32 else np.longdouble
    model = C.vertex_normals(v.astype(up), f, "angle")
    model_err = float(np.abs(want(name, T, "angle").astype(up) - model).max())
    n = pcu.estimate_mesh_vertex_normals(v, f, "angle")
    gpu_err = float(np.abs(n.astype(up) - model).max())
    print(f"angle {name} {np.dtype(T).name}: restatement {model_err:.3e} gpu {gpu_err:.3e}")
    assert n.dtype == np.dtype(T) and np.isfinite(n).all()
    assert gpu_err <= 4 * model_err


@pytest.mark.parametrize("kind", [np.int32, np.int64, np.uint32, np.uint64])
def test_every_face_dtype_gives_the_same_bytes(pcu, kind):
    v, f = C.mesh("defective")
    v = v.astype(np.float32)
    for weighting in ("uniform", "area", "angle"):
        a = pcu.estimate_mesh_vertex_normals(v, f.astype(kind), weighting)
        b = pcu.estimate_mesh_vertex_normals(v, f, weighting)
        assert a.tobytes() == b.tobytes()


@pytest.mark.parametrize("T", FLOATS)
@pytest.mark.parametrize("kind", [np.int32, np.int64])
def test_tensors_give_the_bytes_of_numpy_and_stay_on_the_device(pcu, T, kind):
    v, f = C.mesh("sphere4098")
    v, f = v.astype(T), f.astype(kind)
    for weighting in ("uniform", "area", "angle"):
        a = pcu.estimate_mesh_vertex_normals(v, f, weighting)
        t = pcu.estimate_mesh_vertex_normals(to_torch(v), to_torch(f), weighting)
        assert t.is_cuda and t.cpu().numpy().tobytes() == a.tobytes()
        assert pcu.estimate_mesh_vertex_normals(v, f, weighting).tobytes() == a.tobytes()


def test_vertices_without_a_face_or_an_area_get_zero_rows(pcu):
    v, f, loose = C.defective_sphere()
    mid = loose[0] - 3
    for T in FLOATS:
        for weighting in ("uniform", "area", "angle"):
            n = pcu.estimate_mesh_vertex_normals(v.astype(T), f, weighting)
            assert np.array_equal(n[loose], np.zeros((3, 3))) and np.array_equal(n[mid:mid + 3], np.zeros((3, 3)))
            rest = np.delete(np.arange(len(v)), np.concatenate([loose, [mid, mid + 1, mid + 2]]))
            assert np.abs(np.linalg.norm(n[rest].astype(np.float64), axis=1) - 1).max() < 1e-6


def test_value_errors(pcu):
    v, f = C.mesh("sphere258")
    with pytest.raises(ValueError, match=r"Invalid weighting_type must be one of 'uniform', 'angle', or 'area', but got 'Area'"):
        pcu.estimate_mesh_vertex_normals(v, f, "Area")
    bad_v = v.copy(); bad_v[7, 1] = np.inf
    bad_f = f.copy(); bad_f[100, 2] = len(v)
    with pytest.raises(ValueError, match="v must not contain NaN or infinite coordinates"):
        pcu.estimate_mesh_vertex_normals(bad_v, f)
    with pytest.raises(ValueError, match=r"found a face index outside \[0, 258\)"):
        pcu.estimate_mesh_vertex_normals(v, bad_f)
    # for tensors both are found on the device
    with pytest.raises(ValueError, match="v must not contain NaN or infinite coordinates"):
        pcu.estimate_mesh_vertex_normals(to_torch(bad_v), to_torch(f))
    with pytest.raises(ValueError, match=r"found a face index outside \[0, 258\)"):
        pcu.estimate_mesh_vertex_normals(to_torch(v), to_torch(bad_f), "angle")
    with pytest.raises(ValueError, match=r"found a face index outside \[0, 258\)"):
        pcu.estimate_mesh_vertex_normals(to_torch(v), to_torch(np.where(bad_f == len(v), -1, bad_f)))
    with pytest.raises(ValueError, match="vertex normals overflow the scalar type of v"):
        pcu.estimate_mesh_vertex_normals((v * 1e30).astype(np.float32), f, "area")
    with pytest.raises(ValueError, match=r"Invalid scalar type \(float16\) for argument 'v'"):
        pcu.estimate_mesh_vertex_normals(v.astype(np.float16), f)
