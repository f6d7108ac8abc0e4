"""Every refusal of downsample_point_cloud_farthest_point (and of DatasetIndex.farthest_point_sample) that is decided before the device is
touched, with its text. No GPU: a check that let its input through would fail here on the missing device with a RuntimeError, not a
ValueError."""
import re

import numpy as np
import pytest

import point_cloud_utils_amd as pcu

P = np.arange(15, dtype=np.float32).reshape(5, 3)
CALLS = [lambda p, m=2, s=0: pcu.downsample_point_cloud_farthest_point(p, m, s),
         lambda p, m=2, s=0: pcu.downsample_point_cloud_farthest_point(p, m, start_index=s, return_distances=True, squared_distances=True)]


def refuses(text, fn, *args):
    with pytest.raises(ValueError, match=re.escape(text)):
        fn(*args)


@pytest.mark.parametrize("call", CALLS)
def test_the_cloud(call):
    refuses("Invalid scalar type (int32) for argument 'points'. Expected one of ['float32', 'float64'].", call, P.astype(np.int32))
    refuses("Invalid scalar type (float16) for argument 'points'. Expected one of ['float32', 'float64'].", call, P.astype(np.float16))
    refuses("Only 3D inputs are supported: v must have shape (n, 3) (n > 0). Got points.shape =(5, 2).", call, P[:, :2])
    refuses("Only 3D inputs are supported: v must have shape (n, 3) (n > 0). Got points.shape =(15, 1).", call, P.reshape(-1))
    refuses("Invalid number of dimensions (3): expected a matrix of shape (n, 3).", call, P.reshape(5, 3, 1))
    refuses("Invalid input point cloud with zero points: points must have shape (n, 3) (n > 0). Got points.shape =(0, 3).", call, P[:0])
    many = np.broadcast_to(np.zeros((1, 3), np.float32), (2 ** 27 - 15, 3))          # one row more than the limit, without its memory
    refuses("meshes and point clouds with more than 2^27-16 rows are not supported", call, many)
    for bad in (np.nan, np.inf, -np.inf):
        for dtype in (np.float32, np.float64):
            q = P.astype(dtype); q[3, 1] = bad
            refuses("points must not contain NaN or infinite coordinates", call, q)


@pytest.mark.parametrize("call", CALLS)
def test_the_counts_name_the_offending_values(call):
    refuses("Invalid num_samples (0): must be at least 1 and at most the number of points (5).", call, P, 0)
    refuses("Invalid num_samples (-3): must be at least 1 and at most the number of points (5).", call, P, -3)
    refuses("Invalid num_samples (6): must be at least 1 and at most the number of points (5).", call, P, 6)
    refuses("Invalid start_index (5): must be a row of points, in [0, 5).", call, P, 2, 5)
    refuses("Invalid start_index (-1): must be a row of points, in [0, 5).", call, P, 2, -1)


def test_the_order_of_the_checks():
    """dtype, shape, zero rows, the row limit, the coordinates, num_samples, start_index."""
    f = pcu.downsample_point_cloud_farthest_point
    refuses("Invalid scalar type (int64)", f, np.zeros((0, 2), np.int64), 0, -1)
    refuses("Only 3D inputs are supported", f, np.zeros((0, 2), np.float32), 0, -1)
    refuses("Invalid input point cloud with zero points", f, P[:0], 0, -1)
    q = P.copy(); q[0, 0] = np.nan
    refuses("points must not contain NaN", f, q, 0, -1)
    refuses("Invalid num_samples (0)", f, P, 0, -1)
    refuses("Invalid start_index (-1)", f, P, 1, -1)


def test_inputs_that_pass_reach_the_device():
    from point_cloud_utils_amd import _lib
    if _lib.device_count() > 0:
        pytest.skip("GPU present")
    big = (P + 1) * np.float32(1e20)                       # d2 overflows: allowed
    for args in ((P, 5, 4), (big, 1, 0), (P.astype(np.float64), 3, 2)):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            pcu.downsample_point_cloud_farthest_point(*args)


def stub(num_points, suffix="f32", handle="handle"):
    """A DatasetIndex that was never built (no device): what its method checks before it uses the handle."""
    x = object.__new__(pcu.DatasetIndex)
    x._h, x._suffix, x._np_dtype, x._torch, x._device, x.num_points = handle, suffix, np.float32, False, 0, num_points
    x.close = lambda: None
    return x


def test_the_dataset_index_method_checks_before_the_device():
    refuses("the index has been closed", stub(5, handle=None).farthest_point_sample, 2)
    call = stub(5).farthest_point_sample
    refuses("Invalid num_samples (0): must be at least 1 and at most the number of points (5).", call, 0)
    refuses("Invalid num_samples (6): must be at least 1 and at most the number of points (5).", call, 6)
    refuses("Invalid start_index (5): must be a row of points, in [0, 5).", call, 2, 5)
    refuses("Invalid start_index (-2): must be a row of points, in [0, 5).", call, 2, -2)


def test_exported():
    assert "downsample_point_cloud_farthest_point" in pcu.__all__
    assert callable(pcu.DatasetIndex.farthest_point_sample)
    assert "farthest_point_sample" in pcu.DatasetIndex.__doc__
