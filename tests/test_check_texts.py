"""The texts, order and exception types of the shared argument checks (point_cloud_utils_amd/_checks.py) and of the closed / other-device
refusals of the four handle classes (_call._Handle), each compared in full with a literal. The literals were written from the package as it
was before the checks were gathered into one module, and this file passed against that package first, with the helpers imported from where
they lived then. No GPU: nothing here reaches the device."""
import numpy as np
import pytest

from point_cloud_utils_amd import _checks as K

F32, F64 = np.float32, np.float64
P = np.zeros((4, 3), F32)
FLOAT = "Expected one of ['float32', 'float64']."
ROWS = "meshes and point clouds with more than 2^27-16 rows are not supported"
ALL_SAME = "torch inputs must all be CUDA/HIP tensors on the same device"
ZERO = "Invalid input point cloud with zero points: points must have shape (n, 3) (n > 0). Got points.shape =(0, 3)."
NOT3D = "Only 3D inputs are supported: v must have shape (n, 3) (n > 0). Got points.shape =(4, 2)."
RAY_ROWS = ("ray_o and ray_d must have the same number of rows (one ray origin per ray direction). "
            "(Note: ray_o can have one row to use the same origin for all directions)")


def Big(rows, dtype=F32):
    """An array of many rows that holds one: the row limit is checked before anything reads it."""
    return np.broadcast_to(np.zeros((1, 3), dtype), (rows, 3))


def refuses(text, fn, *args, **kw):
    with pytest.raises(ValueError) as e:
        fn(*args, **kw)
    assert str(e.value) == text


def test_scalar_types_and_counts():
    refuses(f"Invalid scalar type (int32) for argument 'dataset_points'. {FLOAT}", K._check_float, np.zeros((1, 3), np.int32), "dataset_points")
    assert K._check_float(P, "p") == "float32" and K._check_float(P.astype(F64), "v") == "float64"
    refuses("Invalid scalar type (float64) for argument 'n'. Expected it to match argument 'p' which is of type float32.",
            K._match, P.astype(F64), "n", "float32", "argument 'p'")
    assert K._match(P, "q", "float32", "the indexed point cloud") is None
    refuses(ROWS, K._check_rows, 3, 2 ** 27 - 15)
    assert K._check_rows(2 ** 27 - 16, 0) is None


def test_points():
    refuses(f"Invalid scalar type (float16) for argument 'p'. {FLOAT}", K._check_points_dtype, P.astype(np.float16))
    refuses("Invalid scalar type (float32) for argument 'p'. Expected it to match the indexed mesh which is of type float64.",
            K._check_points_dtype, P, "float64")
    assert K._check_points_dtype(P) == ("float32", (4, 3))
    refuses(f"Invalid scalar type (int64) for argument 'p'. {FLOAT}", K._check_points, np.zeros((4, 3), np.int64))
    refuses(NOT3D, K._check_points, P[:, :2])
    refuses(ROWS, K._check_points, Big(2 ** 27))
    assert K._check_points(P[:0]) == ("float32", 0)
    refuses(ZERO, K._check_points_nonzero, P[:0])
    refuses(NOT3D, K._check_points_nonzero, P[:, :2])
    refuses(ROWS, K._check_points_nonzero, Big(2 ** 27))
    assert K._check_points_nonzero(P) == 4
    refuses("Invalid number of dimensions (3): expected a matrix of shape (n, 3).", K._check_points, np.zeros((1, 2, 3), F32))


def test_normals():
    n64 = P.astype(F64)
    refuses(f"Invalid scalar type (int32) for argument 'p'. {FLOAT}", K._check_normals, P.astype(np.int32), P, True)
    refuses("Invalid scalar type (float64) for argument 'n'. Expected it to match argument 'p' which is of type float32.", K._check_normals, P, n64, True)
    refuses("Invalid scalar type (float64) for argument 'a'. Expected it to match argument 'p' which is of type float32.",
            K._check_normals, P[:0], P[:0], False, a=np.zeros(0))                                  # (a's type ahead of the zero rows)
    refuses(ZERO, K._check_normals, P[:0], P[:0], False, a=P[:0, 0])
    assert K._check_normals(P[:0], P[:0], True) == ("float32", 0)
    refuses(NOT3D, K._check_normals, P[:, :2], P, True)
    refuses("Invalid shape for normals: must have shape (n, 3) (n > 0). Got normals.shape =(4, 2).", K._check_normals, P, P[:, :2], True)
    refuses("Invalid input point cloud. Number of normals must match number of points. Got points.shape =(4, 3) and normals.shape = 3, 3",
            K._check_normals, P, P[:3], False, a=P[:, 0])
    assert K._check_normals(P, P, False, a=P[:, 0]) == ("float32", 4)


def test_parameters():
    refuses("beta must be greater than 0 (finite, or +inf for the plain sum over all faces)", K._check_beta, 0.0, "faces")
    refuses("beta must be greater than 0 (finite, or +inf for the plain sum over all points)", K._check_beta, float("nan"), "points")
    assert K._check_beta(np.float32(2), "faces") == 2.0 and K._check_beta(float("inf"), "points") == float("inf")
    refuses("lower_bound and upper_bound must not be NaN", K._check_bounds, float("nan"), 1.0)
    refuses("lower_bound must not be greater than upper_bound", K._check_bounds, 1.0, 0.5)
    assert K._check_bounds(-np.inf, 1) == (-np.inf, 1.0)


def test_rays():
    mesh = "argument 'v'"
    refuses("Invalid scalar type (float64) for argument 'ray_o'. Expected it to match argument 'v' which is of type float32.",
            K._check_rays, P.astype(F64), P.astype(F64), "float32", mesh)
    refuses("Invalid scalar type (float64) for argument 'ray_d'. Expected it to match the indexed mesh which is of type float32.",
            K._check_rays, P, P.astype(F64), "float32", "the indexed mesh")
    refuses(RAY_ROWS, K._check_rays, P[:2], P, "float32", mesh)
    refuses("Invalid shape for ray_o must have shape (N, 3) but got (4, 2).", K._check_rays, P[:, :2], P, "float32", mesh)
    refuses("Invalid shape for ray_d must have shape (N, 3) but got (4, 2).", K._check_rays, P, P[:, :2], "float32", mesh)
    assert K._check_rays(P, P, "float32", mesh) == (4, False)
    assert K._check_rays(P[0], P, "float32", mesh) == (4, True) and K._check_rays(P[:1], P, "float32", mesh) == (4, True)
    refuses(ROWS, K._check_ray_limits, 2 ** 27, 0.0, 1.0)
    refuses("ray_near and ray_far must not be NaN", K._check_ray_limits, 4, 0.0, float("nan"))
    assert K._check_ray_limits(4, 0, np.inf) == (0.0, np.inf)


class HostCall:
    """What _beside, _origins_for and _mesh_args read of the resolved arrays of a call, for host arrays."""
    torch, tdev, pa = False, None, 1234


class FakeTensor:
    """Enough of a tensor to be taken for one (the checks go by the type's module)."""
    is_cuda, device = False, "cpu"

    def data_ptr(self):
        return 0


FakeTensor.__module__ = "torch"


def test_beside_and_origins():
    d = HostCall()
    x = np.arange(12, dtype=F32).reshape(4, 3)[:, ::-1]
    y = K._beside(d, x)
    assert y.flags.c_contiguous and np.array_equal(x, y)
    refuses(ALL_SAME, K._beside, d, FakeTensor())
    t = HostCall()
    t.torch, t.tdev = True, "cuda:0"
    refuses(ALL_SAME, K._beside, t, x)
    refuses(ALL_SAME, K._beside, t, FakeTensor())                     # (a tensor that is not on the GPU)
    oo, rows = K._origins_for(d, P[0], True)
    assert oo.shape == (1, 3) and rows == 1
    oo, rows = K._origins_for(d, P, False)
    assert oo.shape == (4, 3) and rows == 4
    refuses(ALL_SAME, K._origins_for, d, FakeTensor(), True)


def test_host_checks():
    bad = P.copy()
    bad[1, 2] = np.inf
    refuses("p must not contain NaN or infinite coordinates", K._host_finite, p=bad)
    refuses("a must not contain NaN or infinite values", K._host_finite, p=P, a=bad[:, 2])
    refuses("q must not contain NaN or infinite coordinates", K._host_finite, q=np.full((2, 3), np.nan))
    refuses("ray_o must not contain NaN or infinite coordinates", K._host_ray_checks, bad, bad)
    refuses("ray_d must not contain NaN or infinite coordinates", K._host_ray_checks, P, bad)
    f = np.array([[0, 1, 2], [1, 2, 3]], np.int32)
    refuses("v must not contain NaN or infinite coordinates", K._host_mesh_checks, bad, f)
    refuses("f must hold row indices of v: found a face index outside [0, 4)", K._host_mesh_checks, P, f + 1)
    refuses("f must hold row indices of v: found a face index outside [0, 4)", K._host_mesh_checks, P, f - 1)
    refuses("f must hold row indices of v: found a face index outside [0, 4)", K._host_mesh_checks, P, (f + 1).astype(np.uint64))
    assert K._host_mesh_checks(P, f) is None and K._host_finite(p=P, n=P) is None


def test_meshes():
    f = np.array([[0, 1, 2], [1, 2, 3]], np.int64)
    assert K._face_dtype_name(f) == "int64" and K._face_dtype_name(f.astype(np.uint32)) == "uint32"
    refuses("Invalid scalar type (int16) for argument 'f'. Expected one of ['int32', 'int64', 'uint32', 'uint64'].", K._check_face_dtype, f.astype(np.int16))
    refuses(f"Invalid scalar type (int32) for argument 'v'. {FLOAT}", K._check_mesh, P.astype(np.int32), f)
    refuses("Invalid scalar type (float32) for argument 'v'. Expected it to match argument 'p' which is of type float64.", K._check_mesh, P, f, "float64")
    refuses("Invalid scalar type (float32) for argument 'f'. Expected one of ['int32', 'int64', 'uint32', 'uint64'].", K._check_mesh, P, P)
    refuses("Invalid input mesh with zero elements: v and f must have shape (n, 3) and (m, 3) (n, m > 0). Got v.shape =(4, 3), f.shape = (0, 3).",
            K._check_mesh, P, f[:0])
    refuses("Only 3D inputs are supported: v and f must have shape (n, 3) and (m, 3) (n, m > 0). Got v.shape =(4, 2), f.shape = (2, 3).",
            K._check_mesh, P[:, :2], f)
    refuses(ROWS, K._check_mesh, P, Big(2 ** 27, np.int32))
    assert K._check_mesh(P, f) == ("float32", 4, 2) and K._check_mesh(P, f, "float32") == ("float32", 4, 2)
    refuses("f must hold row indices of v: found a face index outside [0, 4)", K._resolve, P, f + 2)     # (ahead of any device work)
    d = HostCall()
    ff = np.ascontiguousarray(f.astype(np.uint32))
    assert K._mesh_args(d, ff, 4, 2) == (1234, 4, ff.ctypes.data, 2, 2)


def test_results():
    w = np.arange(3, dtype=F32)
    assert K._scalar_rows(w, 3) is w and K._scalar_rows(w[:1], 1).shape == ()
    fi, bc = np.array([5, -1], np.int64), np.zeros((2, 3), F32)
    a, b = K._face_rows(fi, bc, np.empty(0, np.uint32), 2)
    assert a.dtype == np.uint32 and a.tolist() == [5, 2 ** 32 - 1] and b is bc
    a, b = K._face_rows(fi[:1], bc[:1], np.empty(0, np.int32), 1)
    assert a.dtype == np.int32 and a.shape == () and int(a) == 5 and b.shape == (3,)


# ---------------------------------------------------------------------------------------------------- the four handles
@pytest.fixture
def no_device(monkeypatch):
    """A context is a token and the default device is 0: a query gets as far as comparing devices; reaching the library fails the test."""
    from point_cloud_utils_amd import _lib

    def _touched(*a, **k):
        raise AssertionError("the library was reached")
    monkeypatch.setattr(_lib, "ctx", lambda device=None: "ctx")
    monkeypatch.setattr(_lib, "default_device", lambda: 0)
    monkeypatch.setattr(_lib, "lib", _touched)


def stub(cls, h, **fields):
    """An instance without the create call: `h` stands for its handle, on device 7."""
    x = object.__new__(cls)
    x._h, x._device, x._dtype_name, x._suffix = h, 7, "float32", "f32"
    for k, v in fields.items():
        setattr(x, k, v)
    return x


def handle_queries(pcu):
    """(class, noun, [(query, what lives elsewhere)]) with arguments that pass every check ahead of the device's."""
    return [
        (pcu.MeshIndex, "mesh index", [(lambda m: m.closest_points(P), "query points"), (lambda m: m.winding_number(P), "query points"),
                                       (lambda m: m.signed_distance(P), "query points"), (lambda m: m.intersect_rays(P[0], P), "rays")]),
        (pcu.PointCloudWindingIndex, "point cloud winding index", [(lambda c: c.winding_number(P), "query points")]),
        (pcu.RaySurfelIntersector, "surfel index", [(lambda c: c.intersect_rays(P, P), "rays")]),
    ]


def test_closed_handles_refuse_every_query(no_device):
    import point_cloud_utils_amd as pcu
    for cls, noun, queries in handle_queries(pcu):
        for query, _ in queries:
            refuses(f"the {noun} has been closed", query, stub(cls, None, _winding=True))
    refuses("the index has been closed", stub(pcu.DatasetIndex, None, num_points=4).k_nearest_neighbors, P, 1)


def test_handles_refuse_another_device(no_device, monkeypatch):
    import point_cloud_utils_amd as pcu
    for cls, noun, queries in handle_queries(pcu):
        for query, what in queries:
            x = stub(cls, "handle", _winding=True)
            refuses(f"{what} and {noun} live on different devices", query, x)
            x._h = None                                                     # (nothing to destroy when the stub goes)
    # the dataset index compares devices for tensors only: a numpy query passes that line and goes on to the library
    x = stub(pcu.DatasetIndex, "handle", num_points=4)
    monkeypatch.setattr("point_cloud_utils_amd._call._fn", lambda op, suffix: pytest.fail("reached " + op, pytrace=False))
    with pytest.raises(pytest.fail.Exception, match="reached index_knn"):
        x.k_nearest_neighbors(P, 1)
    x._h = None


def test_closing_is_idempotent_and_safe_without_a_handle(no_device):
    import point_cloud_utils_amd as pcu
    for cls in (pcu.DatasetIndex, pcu.MeshIndex, pcu.PointCloudWindingIndex, pcu.RaySurfelIntersector):
        x = stub(cls, None)
        x.close()
        x.close()
        with x as y:
            assert y is x
        x.__del__()
        object.__new__(cls).__del__()                                       # an object whose __init__ raised before the create call
        x = stub(cls, "handle")                                             # not a handle the create call made: dropped, the library is not reached
        x.close()
        assert x._h is None
