"""Every refusal of register_point_clouds_icp (and of DatasetIndex.register_icp) that is decided before the device is touched, with its text
and order: the dtype, zero-row, shape and row-limit checks are k_nearest_neighbors' with the source as query and the target as dataset; the
normals, the initial transform, the distance, the iteration count and the two tolerances have their own. And the fields of IcpResult. No GPU: a
check that let its input through would fail here on the missing device with a RuntimeError, not a ValueError. In the style of
tests/test_dbscan_checks.py."""
import math
import re

import numpy as np
import pytest

import point_cloud_utils_amd as pcu

S = np.ones((5, 3), np.float32)
T = np.ones((7, 3), np.float32)
N = np.ones((7, 3), np.float32)
INIT_TEXT = "Invalid init_transform: must be a finite (4, 4) matrix with last row [0, 0, 0, 1]."
icp = pcu.register_point_clouds_icp


def refuses(text, fn, *args, **kw):
    with pytest.raises(ValueError, match=re.escape(text)):
        fn(*args, **kw)


def many_rows(dtype):
    return np.broadcast_to(np.zeros((1, 3), dtype), (2 ** 27 - 15, 3))       # one row more than the limit, without its memory


def test_the_knn_checks_with_their_texts():
    refuses("Invalid scalar type (int32) for argument 'query_points'. Expected one of ['float32', 'float64'].", icp, S.astype(np.int32), T)
    refuses("Invalid scalar type (float64) for argument 'dataset_points'. Expected it to match argument 'query_points' which is of type float32.",
            icp, S, T.astype(np.float64))
    refuses("Invalid input set with zero elements: query_points and dataset_points must have shape (n, 3) and (m, 3). "
            "Got query_points.shape = (0, 3), dataset_points.shape = (7, 3).", icp, S[:0], T)
    refuses("Got query_points.shape = (5, 3), dataset_points.shape = (0, 3).", icp, S, T[:0])
    refuses("Only 3D inputs are supported: query_points and dataset_points must have shape (n, 3) and (m, 3). "
            "Got query_points.shape = (5, 2), dataset_points.shape = (7, 3).", icp, S[:, :2], T)
    refuses("Got query_points.shape = (5, 3), dataset_points.shape = (7, 4).", icp, S, np.ones((7, 4), np.float32))
    refuses("point clouds with more than 2^27-16 rows are not supported", icp, many_rows(np.float32), T)
    refuses("point clouds with more than 2^27-16 rows are not supported", icp, S.astype(np.float64), many_rows(np.float64))


def test_target_normals_match_the_target():
    refuses("Invalid scalar type (float64) for argument 'target_normals'. Expected it to match argument 'target_points' which is of type float32.",
            icp, S, T, N.astype(np.float64))
    refuses("Invalid scalar type (int64) for argument 'target_normals'.", icp, S, T, N.astype(np.int64))
    for bad in (N[:5], N[:, :2], N.reshape(-1), np.ones((7, 3, 1), np.float32)):
        refuses(f"Invalid shape for target_normals: must have shape (7, 3), one normal per target point. Got target_normals.shape = {tuple(bad.shape)}.",
                icp, S, T, bad)


@pytest.mark.parametrize("init", [np.eye(3), np.zeros(16), np.eye(4)[None], "abc", [[1, 0], [0]], np.full((4, 4), np.nan),
                                  np.diag([1.0, 1.0, 1.0, 2.0]), np.eye(4) + np.eye(4)[::-1] * np.array([0, 0, 0, 1.0])[:, None],
                                  np.array([[1, 0, 0, np.inf], [0, 1, 0, 0], [0, 0, 1, 0], [0, 0, 0, 1]])])
def test_init_transform_is_a_finite_4_by_4_with_a_unit_last_row(init):
    refuses(INIT_TEXT, icp, S, T, init_transform=init)


@pytest.mark.parametrize("value, shown", [(float("nan"), "nan"), (-1.0, "-1.0"), (float("-inf"), "-inf"), (np.float32(-0.5), "-0.5")])
def test_max_correspondence_distance_is_not_nan_and_not_negative(value, shown):
    refuses(f"Invalid max_correspondence_distance ({shown}): must not be NaN or negative.", icp, S, T, max_correspondence_distance=value)


@pytest.mark.parametrize("value, shown", [(-1, "-1"), (2.0, "2.0"), (float("nan"), "nan"), (None, "None"), ("4", "4"), (np.int64(-2), "-2")])
def test_max_iterations_is_an_integer_of_at_least_zero(value, shown):
    refuses(f"Invalid max_iterations ({shown}): must be an integer of at least 0.", icp, S, T, max_iterations=value)


@pytest.mark.parametrize("name", ["relative_fitness", "relative_rmse"])
@pytest.mark.parametrize("value, shown", [(float("nan"), "nan"), (-1e-9, "-1e-09"), (float("inf"), "inf"), (float("-inf"), "-inf")])
def test_the_tolerances_are_finite_and_not_negative(name, value, shown):
    refuses(f"Invalid {name} ({shown}): must be finite and not negative.", icp, S, T, **{name: value})


def test_the_checks_come_in_order():
    """dtype, zero rows, shape, row limit, normals, init_transform, distance, iterations, fitness, rmse."""
    bad = dict(target_normals=N[:2], init_transform=np.zeros(3), max_correspondence_distance=-1.0, max_iterations=-1, relative_fitness=-1.0,
               relative_rmse=-1.0)
    refuses("Invalid scalar type (int64)", icp, np.zeros((0, 2), np.int64), T, **bad)
    refuses("Invalid input set with zero elements", icp, S[:0, :2], T, **bad)
    refuses("Only 3D inputs are supported", icp, S[:, :2], T, **bad)
    refuses("point clouds with more than 2^27-16 rows", icp, many_rows(np.float32), T, **bad)
    refuses("Invalid shape for target_normals", icp, S, T, **bad)
    for gone, text in (("target_normals", INIT_TEXT), ("init_transform", "Invalid max_correspondence_distance (-1.0)"),
                       ("max_correspondence_distance", "Invalid max_iterations (-1)"), ("max_iterations", "Invalid relative_fitness (-1.0)"),
                       ("relative_fitness", "Invalid relative_rmse (-1.0)")):
        del bad[gone]
        refuses(text, icp, S, T, **bad)


def stub(num_points, suffix="f32", handle="handle"):
    """A DatasetIndex that was never built (no device): what its methods check before they use the handle."""
    x = object.__new__(pcu.DatasetIndex)
    x._h, x._suffix, x._np_dtype, x._torch, x._device, x.num_points = handle, suffix, np.float32, False, 0, num_points
    x.close = lambda: None
    return x


def test_dataset_index_method_checks_before_the_device():
    refuses("the index has been closed", stub(7, handle=None).register_icp, S)
    call = stub(7).register_icp
    refuses("Invalid scalar type (float64) for argument 'query_points'. Expected it to match the indexed dataset which is of type float32.",
            call, S.astype(np.float64))
    refuses("Got query_points.shape = (0, 3), dataset_points.shape = (7, 3).", call, S[:0])
    refuses("Got query_points.shape = (5, 2), dataset_points.shape = (7, 3).", call, S[:, :2])
    refuses("point clouds with more than 2^27-16 rows are not supported", call, many_rows(np.float32))
    refuses("Invalid shape for target_normals: must have shape (7, 3)", call, S, N[:5])
    refuses("Invalid scalar type (float64) for argument 'target_normals'", call, S, N.astype(np.float64))
    refuses(INIT_TEXT, call, S, init_transform=np.eye(3))
    refuses("Invalid max_correspondence_distance (nan)", call, S, max_correspondence_distance=math.nan)
    refuses("Invalid max_iterations (-1)", call, S, max_iterations=-1)
    refuses("Invalid relative_fitness (inf)", call, S, relative_fitness=math.inf)
    refuses("Invalid relative_rmse (-2.0)", call, S, relative_rmse=-2.0)


def test_result_fields_and_exports():
    assert pcu.IcpResult._fields == ("transform", "fitness", "inlier_rmse", "iterations", "status", "correspondences")
    import icp_contract
    assert icp_contract.IcpResult._fields == pcu.IcpResult._fields
    assert "register_point_clouds_icp" in pcu.__all__ and callable(pcu.register_point_clouds_icp) and "IcpResult" in pcu.__all__
    assert callable(pcu.DatasetIndex.register_icp)
    import inspect
    free = inspect.signature(pcu.register_point_clouds_icp).parameters
    assert list(free) == ["source_points", "target_points", "target_normals", "init_transform", "max_correspondence_distance", "max_iterations",
                          "relative_fitness", "relative_rmse", "return_correspondences"]
    assert [free[k].default for k in list(free)[2:]] == [None, None, math.inf, 30, 1e-6, 1e-6, False]
    method = inspect.signature(pcu.DatasetIndex.register_icp).parameters
    assert list(method)[1:] == [k for k in free if k != "target_points"] and all(method[k].default == free[k].default for k in list(method)[1:])


def test_the_normals_docstrings_point_here():
    for fn in (pcu.estimate_point_cloud_normals_knn, pcu.estimate_point_cloud_normals_ball):
        assert "target_normals" in fn.__doc__ and "register_point_clouds_icp" in fn.__doc__
