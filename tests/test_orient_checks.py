"""The refusals of orient_point_cloud_normals, every text in full, raised before anything touches the device: the library is replaced by an
object that fails the test when it is asked for anything. The scalar-type and shape refusals are point_cloud_fast_winding_number's
(_check_normals), k's is estimate_point_cloud_normals_knn's, the cloud's non-finite rule and its text are the k-NN calls'. No GPU."""
import numpy as np
import pytest

import point_cloud_utils_amd as pcu
from point_cloud_utils_amd import _checks, _lib, _orient

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
        pcu.orient_point_cloud_normals(*args, **kw)
    assert str(e.value) == text


P = np.random.default_rng(1).random((10, 3))
N = np.random.default_rng(2).standard_normal((10, 3))


def test_scalar_types_and_shapes():
    raises("Invalid scalar type (int64) for argument 'p'. Expected one of ['float32', 'float64'].", np.zeros((10, 3), np.int64), N)
    raises("Invalid scalar type (float32) for argument 'n'. Expected it to match argument 'p' which is of type float64.", P, N.astype(np.float32))
    raises("Invalid scalar type (float64) for argument 'n'. Expected it to match argument 'p' which is of type float32.", P.astype(np.float32), N)
    raises("Invalid input point cloud with zero points: points must have shape (n, 3) (n > 0). Got points.shape =(0, 3).", P[:0], N[:0])
    raises("Only 3D inputs are supported: v must have shape (n, 3) (n > 0). Got points.shape =(10, 2).", P[:, :2], N)
    raises("Invalid shape for normals: must have shape (n, 3) (n > 0). Got normals.shape =(10, 2).", P, N[:, :2])
    raises("Invalid input point cloud. Number of normals must match number of points. Got points.shape =(10, 3) and normals.shape = 9, 3", P, N[:9])
    big = np.broadcast_to(np.zeros((1, 3), np.float32), (2 ** 27 - 15, 3))
    raises("meshes and point clouds with more than 2^27-16 rows are not supported", big, big)


@pytest.mark.parametrize("k", [0, -1, -2 ** 40, 1.5, "7", None])
def test_k(k):
    raises(f"Invalid number of neighbors ({k}) must be greater than 0.", P, N, k)
    raises(f"Invalid number of neighbors ({k}) must be greater than 0.", P, N, k=k, return_flipped=True)


def test_the_clouds_non_finite_rule_is_the_k_nn_calls():
    assert _checks._KNN_NONFINITE == NONFINITE
    Q = P.copy()
    Q[7, 1] = np.nan
    raises(NONFINITE, Q, N)
    Q = P.copy()
    Q[2, 0], Q[8, 0] = np.inf, -np.inf
    raises(NONFINITE, Q, N)
    raises(NONFINITE, Q.astype(np.float32), N.astype(np.float32), 3, True)
    # single-signed infinities, and +inf and -inf on different axes, are the search's to handle; non-finite NORMALS are allowed (rule 2)
    for rows in (((2, 0, np.inf), (8, 0, np.inf)), ((2, 0, np.inf), (8, 1, -np.inf))):
        Q = P.copy()
        for i, a, v in rows:
            Q[i, a] = v
        _checks._host_searched_cloud(Q)
    _checks._host_searched_cloud(P)


def test_the_order_of_the_checks():
    """The arrays, then the row limit, then k, then the cloud's values."""
    Q = P.copy()
    Q[0, 0] = np.nan
    raises("Invalid shape for normals: must have shape (n, 3) (n > 0). Got normals.shape =(10, 2).", Q, N[:, :2], 0)
    raises("Invalid number of neighbors (0) must be greater than 0.", Q, N, 0)
    raises(NONFINITE, Q, N, 1)


def test_accepted_edges():
    assert _orient._check_k(1) == 1 and _orient._check_k(np.int64(70)) == 70 and _orient._check_k(2 ** 40) == 2 ** 27 - 16
    assert "orient_point_cloud_normals" in pcu.__all__
    import inspect
    assert str(inspect.signature(pcu.orient_point_cloud_normals)) == "(points, normals, k=10, return_flipped=False, max_points_per_leaf=10)"
