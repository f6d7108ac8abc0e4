"""Every refusal of radius_search / radius_count (and of DatasetIndex.radius_*) that is decided before the device is touched, with its text:
the dtype, zero-row, shape and row-limit checks are k_nearest_neighbors', the radius checks are this call's own. No GPU: a check that let its
input through would fail here on the missing device with a RuntimeError, not a ValueError."""
import re

import numpy as np
import pytest

import point_cloud_utils_amd as pcu

Q = np.zeros((4, 3), np.float32)
P = np.ones((5, 3), np.float32)
CALLS = [lambda q, p, r: pcu.radius_search(q, p, r), lambda q, p, r: pcu.radius_count(q, p, r),
         lambda q, p, r: pcu.radius_search(q, p, r, squared_distances=True, sort_results=False)]


def refuses(text, fn, *args):
    with pytest.raises(ValueError, match=re.escape(text)):
        fn(*args)


def many_rows(dtype):
    return np.broadcast_to(np.zeros((1, 3), dtype), (2 ** 27 - 15, 3))       # one row more than the limit, without its memory


@pytest.mark.parametrize("call", CALLS)
def test_the_knn_checks_with_their_texts(call):
    refuses("Invalid scalar type (int32) for argument 'query_points'. Expected one of ['float32', 'float64'].", call, Q.astype(np.int32), P, 1.0)
    refuses("Invalid scalar type (float16) for argument 'query_points'. Expected one of ['float32', 'float64'].", call, Q.astype(np.float16), P, 1.0)
    refuses("Invalid scalar type (float64) for argument 'dataset_points'. Expected it to match argument 'query_points' which is of type float32.",
            call, Q, P.astype(np.float64), 1.0)
    refuses("Invalid input set with zero elements: query_points and dataset_points must have shape (n, 3) and (m, 3). "
            "Got query_points.shape = (0, 3), dataset_points.shape = (5, 3).", call, Q[:0], P, 1.0)
    refuses("Got query_points.shape = (4, 3), dataset_points.shape = (0, 3).", call, Q, P[:0], 1.0)
    refuses("Only 3D inputs are supported: query_points and dataset_points must have shape (n, 3) and (m, 3). "
            "Got query_points.shape = (4, 2), dataset_points.shape = (5, 3).", call, Q[:, :2], P, 1.0)
    refuses("Got query_points.shape = (4, 3), dataset_points.shape = (5, 4).", call, Q, np.ones((5, 4), np.float32), 1.0)
    refuses("point clouds with more than 2^27-16 rows are not supported", call, many_rows(np.float32), P, 1.0)
    refuses("point clouds with more than 2^27-16 rows are not supported", call, Q.astype(np.float64), many_rows(np.float64), 1.0)


@pytest.mark.parametrize("call", CALLS)
@pytest.mark.parametrize("radius, shown", [(float("nan"), "nan"), (-1.0, "-1.0"), (-0.5, "-0.5"), (float("inf"), "inf"), (float("-inf"), "-inf"),
                                           (np.float32("nan"), "nan")])
def test_radius_must_be_finite_and_not_negative(call, radius, shown):
    refuses(f"Invalid radius ({shown}): must be finite and not negative.", call, Q, P, radius)


def test_the_checks_come_in_the_knn_order():
    """dtype, then zero rows, then the shape, then the row limit, then the radius."""
    refuses("Invalid scalar type (int64)", pcu.radius_search, np.zeros((0, 2), np.int64), P, -1.0)
    refuses("Invalid input set with zero elements", pcu.radius_search, Q[:0, :2], P, -1.0)
    refuses("Only 3D inputs are supported", pcu.radius_count, Q[:, :2], P, -1.0)
    refuses("point clouds with more than 2^27-16 rows", pcu.radius_count, many_rows(np.float32), P, -1.0)


def stub(num_points, suffix="f32", handle="handle"):
    """A DatasetIndex that was never built (no device): what its methods check before they use the handle."""
    x = object.__new__(pcu.DatasetIndex)
    x._h, x._suffix, x._np_dtype, x._torch, x._device, x.num_points = handle, suffix, np.float32, False, 0, num_points
    x.close = lambda: None
    return x


@pytest.mark.parametrize("method", ["radius_search", "radius_count", "k_nearest_neighbors"])
def test_dataset_index_methods_check_before_the_device(method):
    """The three query methods share one check of the query (1.0: the radius, or k = 1); each then refuses its own parameter."""
    refuses("the index has been closed", getattr(stub(5, handle=None), method), Q, 1.0)
    call = getattr(stub(5), method)
    refuses("Invalid scalar type (int32) for argument 'query_points'. Expected one of ['float32', 'float64'].", call, Q.astype(np.int32), 1.0)
    refuses("Invalid scalar type (float64) for argument 'query_points'. Expected it to match the indexed dataset which is of type float32.",
            call, Q.astype(np.float64), 1.0)
    refuses("Got query_points.shape = (0, 3), dataset_points.shape = (5, 3).", call, Q[:0], 1.0)
    refuses("Only 3D inputs are supported: query_points and dataset_points must have shape (n, 3) and (m, 3). "
            "Got query_points.shape = (4, 2), dataset_points.shape = (5, 3).", call, Q[:, :2], 1.0)
    refuses("point clouds with more than 2^27-16 rows are not supported", call, many_rows(np.float32), 1.0)
    if method == "k_nearest_neighbors":
        refuses("Invalid value for k (0) must be greater than 0.", call, Q, 0)
        return
    for radius, shown in ((float("nan"), "nan"), (-2.0, "-2.0"), (float("inf"), "inf")):
        refuses(f"Invalid radius ({shown}): must be finite and not negative.", call, Q, radius)


def test_exported():
    assert "radius_search" in pcu.__all__ and "radius_count" in pcu.__all__
    assert callable(pcu.DatasetIndex.radius_search) and callable(pcu.DatasetIndex.radius_count)
