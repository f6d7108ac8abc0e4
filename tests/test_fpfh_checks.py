"""The refusals of compute_point_cloud_fpfh, every text in full, raised before anything touches the device: the library is replaced by an object
that fails the test when it is asked for anything. The scalar-type, shape and row-count refusals are orient_point_cloud_normals'
(_check_normals), the radius rule and text are radius_search's, the cloud's non-finite rule and its text are the k-NN calls'. No GPU."""
import inspect

import numpy as np
import pytest

import point_cloud_utils_amd as pcu
from point_cloud_utils_amd import _checks, _lib

NONFINITE = ("Invalid input: dataset_points contains NaN coordinates, or both +inf and -inf along one axis. The reference builds its kd-tree over "
             "NaN bounds for such data and returns rows that depend on the traversal; not supported (non-finite query points and single-signed "
             "infinities in the dataset are handled as the reference handles them).")


@pytest.fixture(autouse=True)
def no_device(monkeypatch):
    def refuse(*a, **k):
        raise AssertionError("the call reached the library")
    monkeypatch.setattr(_lib, "lib", refuse)
    monkeypatch.setattr(_lib, "ctx", refuse)


def raises(text, *args, **kw):
    with pytest.raises(ValueError) as e:
        pcu.compute_point_cloud_fpfh(*args, **kw)
    assert str(e.value) == text


P = np.random.default_rng(1).random((10, 3))
N = np.random.default_rng(2).standard_normal((10, 3))


def test_scalar_types_and_shapes():
    raises("Invalid scalar type (int64) for argument 'p'. Expected one of ['float32', 'float64'].", np.zeros((10, 3), np.int64), N, 0.1)
    raises("Invalid scalar type (float32) for argument 'n'. Expected it to match argument 'p' which is of type float64.", P, N.astype(np.float32), 0.1)
    raises("Invalid scalar type (float64) for argument 'n'. Expected it to match argument 'p' which is of type float32.", P.astype(np.float32), N, 0.1)
    raises("Invalid input point cloud with zero points: points must have shape (n, 3) (n > 0). Got points.shape =(0, 3).", P[:0], N[:0], 0.1)
    raises("Only 3D inputs are supported: v must have shape (n, 3) (n > 0). Got points.shape =(10, 2).", P[:, :2], N, 0.1)
    raises("Invalid shape for normals: must have shape (n, 3) (n > 0). Got normals.shape =(10, 2).", P, N[:, :2], 0.1)
    raises("Invalid input point cloud. Number of normals must match number of points. Got points.shape =(10, 3) and normals.shape = 9, 3", P, N[:9], 0.1)
    big = np.broadcast_to(np.zeros((1, 3), np.float32), (2 ** 27 - 15, 3))
    raises("meshes and point clouds with more than 2^27-16 rows are not supported", big, big, 0.1)


@pytest.mark.parametrize("radius", [-1.0, -1e-300, float("nan"), float("inf"), -float("inf")])
def test_radius(radius):
    raises(f"Invalid radius ({float(radius)}): must be finite and not negative.", P, N, radius)
    raises(f"Invalid radius ({float(radius)}): must be finite and not negative.", P.astype(np.float32), N.astype(np.float32), radius=radius, return_spfh=True)


def test_the_clouds_non_finite_rule_is_the_k_nn_calls():
    assert _checks._KNN_NONFINITE == NONFINITE
    Q = P.copy()
    Q[7, 1] = np.nan
    raises(NONFINITE, Q, N, 0.1)
    Q = P.copy()
    Q[2, 0], Q[8, 0] = np.inf, -np.inf
    raises(NONFINITE, Q, N, 0.1)
    raises(NONFINITE, Q.astype(np.float32), N.astype(np.float32), 0.0, True)


def test_the_order_of_the_checks():
    """The arrays, then the row limit, then the radius, then the cloud's values."""
    Q = P.copy()
    Q[0, 0] = np.nan
    raises("Invalid shape for normals: must have shape (n, 3) (n > 0). Got normals.shape =(10, 2).", Q, N[:, :2], -1.0)
    raises("Invalid radius (-1.0): must be finite and not negative.", Q, N, -1.0)
    raises(NONFINITE, Q, N, 1.0)


def test_accepted_edges():
    assert _checks._check_radius(0) == 0.0 and _checks._check_radius(np.float32(0.5)) == 0.5
    assert "compute_point_cloud_fpfh" in pcu.__all__ and callable(pcu.compute_point_cloud_fpfh)
    assert str(inspect.signature(pcu.compute_point_cloud_fpfh)) == "(points, normals, radius, return_spfh=False)"
    # non-finite and zero NORMALS are allowed: such rows are invalid, not refused (the call goes on to the library, which this test has replaced)
    bad = N.copy()
    bad[3] = np.nan
    bad[4] = 0.0
    with pytest.raises(AssertionError, match="the call reached the library"):
        pcu.compute_point_cloud_fpfh(P, bad, 0.1)
