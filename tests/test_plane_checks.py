"""The refusals of segment_point_cloud_plane, every new text in full, raised before anything touches the device: the library is replaced by
an object that fails the test when it is asked for anything. The dtype, shape, row-limit and non-finite refusals are those of
downsample_point_cloud_farthest_point, with its texts. No GPU."""
import numpy as np
import pytest

import point_cloud_utils_amd as pcu
from point_cloud_utils_amd import _checks, _fps, _lib, _plane


@pytest.fixture(autouse=True)
def no_device(monkeypatch):
    def refuse(*a, **k):
        raise AssertionError("the call reached the library")
    monkeypatch.setattr(_lib, "lib", refuse)
    monkeypatch.setattr(_lib, "ctx", refuse)


def raises(text, *args, **kw):
    with pytest.raises(ValueError) as e:
        pcu.segment_point_cloud_plane(*args, **kw)
    assert str(e.value) == text


P = np.random.default_rng(1).random((10, 3))


@pytest.mark.parametrize("n", [1, 2])
def test_fewer_than_three_points(n):
    raises(f"Invalid number of points ({n}): a plane needs at least 3.", P[:n], 0.1)
    raises(f"Invalid number of points ({n}): a plane needs at least 3.", P[:n].astype(np.float32), 0.1)


@pytest.mark.parametrize("thr", [-1.0, -1e-300, float("nan"), float("inf"), float("-inf")])
def test_distance_threshold(thr):
    raises(f"Invalid distance_threshold ({float(thr)}): must be finite and not negative.", P, thr)


@pytest.mark.parametrize("it", [0, -1, 2 ** 20 + 1, 2 ** 40, 1.5, "7", None])
def test_num_iterations(it):
    raises(f"Invalid num_iterations ({it}): must be an integer in [1, 2**20].", P, 0.1, it)


@pytest.mark.parametrize("seed", [-1, 2 ** 32])
def test_random_seed(seed):
    raises(f"random_seed must be an unsigned 32-bit integer, got {seed}", P, 0.1, 10, seed)


def test_the_cloud_checks_are_the_farthest_point_calls():
    assert _fps._check_cloud is _checks._check_finite_cloud
    raises("Invalid scalar type (int64) for argument 'points'. Expected one of ['float32', 'float64'].", np.zeros((10, 3), np.int64), 0.1)
    raises("Only 3D inputs are supported: v must have shape (n, 3) (n > 0). Got points.shape =(10, 2).", P[:, :2], 0.1)
    raises("Invalid input point cloud with zero points: points must have shape (n, 3) (n > 0). Got points.shape =(0, 3).", P[:0], 0.1)
    for bad in (np.nan, np.inf, -np.inf):
        Q = P.copy()
        Q[7, 1] = bad
        raises("points must not contain NaN or infinite coordinates", Q, 0.1)
    for call in (lambda x: pcu.segment_point_cloud_plane(x, 0.1), lambda x: pcu.downsample_point_cloud_farthest_point(x, 1)):
        with pytest.raises(ValueError) as e:
            call(np.broadcast_to(np.zeros((1, 3), np.float32), (2 ** 27 - 15, 3)))
        assert str(e.value) == "meshes and point clouds with more than 2^27-16 rows are not supported"


def test_the_order_of_the_checks():
    """The cloud, then the threshold, then the iteration count, then the seed."""
    raises("Invalid number of points (2): a plane needs at least 3.", P[:2], -1.0, 0, -1)
    raises("Invalid distance_threshold (-1.0): must be finite and not negative.", P, -1.0, 0, -1)
    raises("Invalid num_iterations (0): must be an integer in [1, 2**20].", P, 0.1, 0, -1)


def test_accepted_edges():
    assert _checks._check_distance_threshold(0) == 0.0 and _checks._check_num_iterations(1) == 1
    assert _checks._check_num_iterations(np.int64(2 ** 20)) == 2 ** 20
    assert _checks._check_seed(2 ** 32 - 1) == 2 ** 32 - 1 and 1 <= _checks._check_seed(0) <= 2 ** 32 - 1
    assert _plane.PlaneResult._fields == ("plane", "inliers", "best_iteration", "status", "random_seed")
    assert "segment_point_cloud_plane" in pcu.__all__ and "PlaneResult" in pcu.__all__
