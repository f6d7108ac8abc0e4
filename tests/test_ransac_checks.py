"""The refusals of register_point_clouds_ransac that Python makes, every text in full, raised before anything touches the device: the library
is replaced by an object that fails the test when it is asked for anything. The dtype, shape, zero-row, row-limit and non-finite refusals of
either cloud are those of segment_point_cloud_plane, with its texts. (An entry of correspondences outside its cloud is the library's to find,
on the device: tests/test_gpu_point_cloud_ransac.py.) No GPU."""
import numpy as np
import pytest

import point_cloud_utils_amd as pcu
from point_cloud_utils_amd import _checks, _lib, _ransac


@pytest.fixture(autouse=True)
def no_device(monkeypatch):
    def refuse(*a, **k):
        raise AssertionError("the call reached the library")
    monkeypatch.setattr(_lib, "lib", refuse)
    monkeypatch.setattr(_lib, "ctx", refuse)


def raises(text, *args, **kw):
    with pytest.raises(ValueError) as e:
        pcu.register_point_clouds_ransac(*args, **kw)
    assert str(e.value) == text


rng = np.random.default_rng(1)
S, T = rng.random((10, 3)), rng.random((12, 3))
C = np.stack([np.arange(8), np.arange(8) + 2], axis=1).astype(np.int64)


def test_the_cloud_checks_are_the_plane_calls_for_either_cloud():
    for put in (lambda x: (x, T), lambda x: (S, x)):
        raises("Invalid scalar type (int64) for argument 'points'. Expected one of ['float32', 'float64'].", *put(np.zeros((10, 3), np.int64)), C, 0.1)
        raises("Only 3D inputs are supported: v must have shape (n, 3) (n > 0). Got points.shape =(10, 2).", *put(S[:, :2]), C, 0.1)
        raises("Invalid input point cloud with zero points: points must have shape (n, 3) (n > 0). Got points.shape =(0, 3).", *put(S[:0]), C, 0.1)
        for bad in (np.nan, np.inf, -np.inf):
            Q = S.copy()
            Q[7, 1] = bad
            raises("points must not contain NaN or infinite coordinates", *put(Q), C, 0.1)
        raises("meshes and point clouds with more than 2^27-16 rows are not supported",
               *put(np.broadcast_to(np.zeros((1, 3)), (2 ** 27 - 15, 3))), C, 0.1)


def test_one_dtype_for_both_clouds():
    raises("Invalid scalar type (float32) for argument 'target_points'. Expected it to match argument 'source_points' which is of type float64.",
           S, T.astype(np.float32), C, 0.1)
    raises("Invalid scalar type (float64) for argument 'target_points'. Expected it to match argument 'source_points' which is of type float32.",
           S.astype(np.float32), T, C, 0.1)


@pytest.mark.parametrize("dtype", [np.int32, np.uint64, np.float64, np.bool_])
def test_correspondences_dtype(dtype):
    raises(f"Invalid scalar type ({np.dtype(dtype).name}) for argument 'correspondences'. Expected one of ['int64'].", S, T, C.astype(dtype), 0.1)


@pytest.mark.parametrize("shape", [(8,), (8, 3), (8, 1), (2, 2, 2), (0, 3)])
def test_correspondences_shape(shape):
    raises("Invalid shape for correspondences: must have shape (c, 2), one [source row, target row] per row. "
           f"Got correspondences.shape = {shape}.", S, T, np.zeros(shape, np.int64), 0.1)


@pytest.mark.parametrize("c", [0, 1, 2])
def test_fewer_than_three_correspondences(c):
    raises(f"Invalid number of correspondences ({c}): a rigid transform needs at least 3.", S, T, C[:c], 0.1)


def test_too_many_correspondences():
    raises("correspondences with more than 2^27-16 rows are not supported", S, T, np.broadcast_to(np.zeros((1, 2), np.int64), (2 ** 27 - 15, 2)), 0.1)


@pytest.mark.parametrize("thr", [-1.0, -1e-300, float("nan"), float("inf"), float("-inf")])
def test_max_correspondence_distance(thr):
    raises(f"Invalid max_correspondence_distance ({float(thr)}): must be finite and not negative.", S, T, C, thr)


@pytest.mark.parametrize("it", [0, -1, 2 ** 20 + 1, 2 ** 40, 1.5, "7", None])
def test_num_iterations(it):
    raises(f"Invalid num_iterations ({it}): must be an integer in [1, 2**20].", S, T, C, 0.1, it)


@pytest.mark.parametrize("seed", [-1, 2 ** 32])
def test_random_seed(seed):
    raises(f"random_seed must be an unsigned 32-bit integer, got {seed}", S, T, C, 0.1, 10, seed)


@pytest.mark.parametrize("ratio", [-0.1, 1.0000001, 2, float("nan"), float("inf"), float("-inf")])
def test_edge_length_ratio(ratio):
    raises(f"Invalid edge_length_ratio ({float(ratio)}): must be in [0, 1].", S, T, C, 0.1, 10, 1, ratio)


def test_the_order_of_the_checks():
    """The source, the target, their dtypes, the correspondences, then the scalars in the order of the arguments."""
    bad_c = C[:2]
    raises("Only 3D inputs are supported: v must have shape (n, 3) (n > 0). Got points.shape =(10, 2).", S[:, :2], T[:0], bad_c, -1.0, 0, -1, 2.0)
    raises("Invalid input point cloud with zero points: points must have shape (n, 3) (n > 0). Got points.shape =(0, 3).", S, T[:0], bad_c, -1.0, 0, -1, 2.0)
    raises("Invalid scalar type (float32) for argument 'target_points'. Expected it to match argument 'source_points' which is of type float64.",
           S, T.astype(np.float32), bad_c, -1.0, 0, -1, 2.0)
    raises("Invalid number of correspondences (2): a rigid transform needs at least 3.", S, T, bad_c, -1.0, 0, -1, 2.0)
    raises("Invalid max_correspondence_distance (-1.0): must be finite and not negative.", S, T, C, -1.0, 0, -1, 2.0)
    raises("Invalid num_iterations (0): must be an integer in [1, 2**20].", S, T, C, 0.1, 0, -1, 2.0)
    raises("random_seed must be an unsigned 32-bit integer, got -1", S, T, C, 0.1, 10, -1, 2.0)
    raises("Invalid edge_length_ratio (2.0): must be in [0, 1].", S, T, C, 0.1, 10, 1, 2.0)


def test_accepted_edges():
    assert _checks._check_tolerance(0, "max_correspondence_distance") == 0.0
    assert _checks._check_edge_length_ratio(0) == 0.0 and _checks._check_edge_length_ratio(1) == 1.0 and _checks._check_edge_length_ratio(np.float32(0.5)) == 0.5
    assert _checks._check_correspondences(C[:3]) == 3 and _checks._check_ransac_clouds(S[:1], T[:1]) == (1, 1)
    assert _ransac.RansacRegistrationResult._fields == ("transform", "inliers", "fitness", "inlier_rmse", "best_iteration", "status", "random_seed")
    assert "register_point_clouds_ransac" in pcu.__all__ and "RansacRegistrationResult" in pcu.__all__ and callable(pcu.register_point_clouds_ransac)
    import inspect
    sig = inspect.signature(pcu.register_point_clouds_ransac)
    assert [(k, v.default) for k, v in sig.parameters.items()][3:] == [("max_correspondence_distance", inspect.Parameter.empty), ("num_iterations", 100000),
                                                                          ("random_seed", 0), ("edge_length_ratio", 0.9), ("refit", True)]
    doc = pcu.register_point_clouds_ransac.__doc__
    assert "match_point_features(source_features, target_features, mutual=True)" in doc and "np.stack([np.flatnonzero(is_mutual), nearest[is_mutual]], axis=1)" in doc
