"""Every refusal of cluster_point_cloud_dbscan (and of DatasetIndex.cluster_dbscan) that is decided before the device is touched, with its
text and order: the dtype, zero-row, shape and row-limit checks are k_nearest_neighbors' on the cloud as both of its clouds, eps has the
radius' check, min_points its own. No GPU: a check that let its input through would fail here on the missing device with a RuntimeError, not
a ValueError. In the style of tests/test_radius_checks.py."""
import re

import numpy as np
import pytest

import point_cloud_utils_amd as pcu

P = np.ones((5, 3), np.float32)
CALLS = [lambda p, eps, m: pcu.cluster_point_cloud_dbscan(p, eps, m), lambda p, eps, m: pcu.cluster_point_cloud_dbscan(p, eps, m, return_core=True)]


def refuses(text, fn, *args):
    with pytest.raises(ValueError, match=re.escape(text)):
        fn(*args)


def many_rows(dtype):
    return np.broadcast_to(np.zeros((1, 3), dtype), (2 ** 27 - 15, 3))       # one row more than the limit, without its memory


@pytest.mark.parametrize("call", CALLS)
def test_the_knn_checks_with_their_texts(call):
    refuses("Invalid scalar type (int32) for argument 'query_points'. Expected one of ['float32', 'float64'].", call, P.astype(np.int32), 1.0, 4)
    refuses("Invalid scalar type (float16) for argument 'query_points'. Expected one of ['float32', 'float64'].", call, P.astype(np.float16), 1.0, 4)
    refuses("Invalid input set with zero elements: query_points and dataset_points must have shape (n, 3) and (m, 3). "
            "Got query_points.shape = (0, 3), dataset_points.shape = (0, 3).", call, P[:0], 1.0, 4)
    refuses("Only 3D inputs are supported: query_points and dataset_points must have shape (n, 3) and (m, 3). "
            "Got query_points.shape = (5, 2), dataset_points.shape = (5, 2).", call, P[:, :2], 1.0, 4)
    refuses("Got query_points.shape = (5, 4), dataset_points.shape = (5, 4).", call, np.ones((5, 4), np.float64), 1.0, 4)
    refuses("point clouds with more than 2^27-16 rows are not supported", call, many_rows(np.float32), 1.0, 4)
    refuses("point clouds with more than 2^27-16 rows are not supported", call, many_rows(np.float64), 1.0, 4)


@pytest.mark.parametrize("call", CALLS)
@pytest.mark.parametrize("eps, shown", [(float("nan"), "nan"), (-1.0, "-1.0"), (-0.5, "-0.5"), (float("inf"), "inf"), (float("-inf"), "-inf"),
                                        (np.float32("nan"), "nan")])
def test_eps_must_be_finite_and_not_negative(call, eps, shown):
    refuses(f"Invalid radius ({shown}): must be finite and not negative.", call, P, eps, 4)


@pytest.mark.parametrize("call", CALLS)
@pytest.mark.parametrize("min_points, shown", [(0, "0"), (-3, "-3"), (2.0, "2.0"), (2.5, "2.5"), (float("nan"), "nan"), (None, "None"), ("4", "4"),
                                               (np.int64(0), "0"), (np.float32(3), "3.0")])
def test_min_points_must_be_an_integer_of_at_least_one(call, min_points, shown):
    refuses(f"Invalid min_points ({shown}): must be an integer of at least 1.", call, P, 1.0, min_points)


def test_the_checks_come_in_order():
    """dtype, then zero rows, then the shape, then the row limit, then eps, then min_points."""
    call = pcu.cluster_point_cloud_dbscan
    refuses("Invalid scalar type (int64)", call, np.zeros((0, 2), np.int64), -1.0, 0)
    refuses("Invalid input set with zero elements", call, P[:0, :2], -1.0, 0)
    refuses("Only 3D inputs are supported", call, P[:, :2], -1.0, 0)
    refuses("point clouds with more than 2^27-16 rows", call, many_rows(np.float32), -1.0, 0)
    refuses("Invalid radius (-1.0)", call, P, -1.0, 0)
    refuses("Invalid min_points (0)", call, P, 0.0, 0)


def stub(num_points, suffix="f32", handle="handle"):
    """A DatasetIndex that was never built (no device): what its methods check before they use the handle."""
    x = object.__new__(pcu.DatasetIndex)
    x._h, x._suffix, x._np_dtype, x._torch, x._device, x.num_points = handle, suffix, np.float32, False, 0, num_points
    x.close = lambda: None
    return x


def test_dataset_index_method_checks_before_the_device():
    refuses("the index has been closed", stub(5, handle=None).cluster_dbscan, 1.0, 4)
    refuses("the index has been closed", stub(5, handle=None).cluster_dbscan, -1.0, 0)        # (first of all)
    call = stub(5).cluster_dbscan
    for eps, shown in ((float("nan"), "nan"), (-2.0, "-2.0"), (float("inf"), "inf")):
        refuses(f"Invalid radius ({shown}): must be finite and not negative.", call, eps, 0)
    for min_points, shown in ((0, "0"), (-1, "-1"), (1.5, "1.5")):
        refuses(f"Invalid min_points ({shown}): must be an integer of at least 1.", call, 0.5, min_points)


def test_exported():
    assert "cluster_point_cloud_dbscan" in pcu.__all__ and callable(pcu.cluster_point_cloud_dbscan)
    assert callable(pcu.DatasetIndex.cluster_dbscan)
