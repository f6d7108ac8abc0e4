"""register_point_clouds_icp: rigid ICP alignment of a source cloud onto a target over the HIP kernels of csrc/icp.h and the host loop of
csrc/icp_host.h. Not in the reference's API; the values follow this library's stated contract (in numpy:
tests/icp_contract.py). DatasetIndex.register_icp ends here too."""
import collections
import ctypes
import math
import operator

import numpy as np

from ._call import _Dev, _call, _shape2
from ._checks import (_KNN_DIM, _KNN_ROW_LIMIT, _KNN_ZERO, _beside, _check_init_transform, _check_max_correspondence_distance, _check_pair,
                      _check_rows, _check_target_normals, _check_tolerance)

IcpResult = collections.namedtuple("IcpResult", "transform fitness inlier_rmse iterations status correspondences")

_STATUS = ("converged", "max_iterations", "no_correspondences", "degenerate")      # PCU_HIP_ICP_*
_MAX_ITERATIONS_TOP = 2 ** 31 - 2          # (the evaluations are counted in 32 bits)


class _Result(ctypes.Structure):           # pcu_hip_icp_result
    _fields_ = [("transform", ctypes.c_double * 16), ("fitness", ctypes.c_double), ("inlier_rmse", ctypes.c_double),
                ("iterations", ctypes.c_int64), ("status", ctypes.c_int32), ("n_evaluations", ctypes.c_int32)]


def _check_max_iterations(max_iterations):
    try:
        m = operator.index(max_iterations)
    except TypeError:
        m = -1
    if m < 0:
        raise ValueError(f"Invalid max_iterations ({max_iterations}): must be an integer of at least 0.")
    return min(m, _MAX_ITERATIONS_TOP)


def _check_params(init_transform, max_correspondence_distance, max_iterations, relative_fitness, relative_rmse):
    return (_check_init_transform(init_transform), _check_max_correspondence_distance(max_correspondence_distance),
            _check_max_iterations(max_iterations), _check_tolerance(relative_fitness, "relative_fitness"),
            _check_tolerance(relative_rmse, "relative_rmse"))


def _register(name, d, head, n, normals, params, return_correspondences):
    init, distance, max_iterations, tol_fitness, tol_rmse = params
    nrm = None if normals is None else _beside(d, normals)
    corr = d.empty((n,), "i64") if return_correspondences else None
    res = _Result()
    _call(name, d, *head, _Dev.ptr(nrm), init.ctypes.data, distance, max_iterations, tol_fitness, tol_rmse, ctypes.addressof(res), _Dev.ptr(corr))
    transform = np.array(res.transform, dtype=np.float64).reshape(4, 4)
    if d.torch:
        import torch
        transform = torch.from_numpy(transform).to(d.tdev)
    return IcpResult(transform, float(res.fitness), float(res.inlier_rmse), int(res.iterations), _STATUS[res.status], corr)


def register_point_clouds_icp(source_points, target_points, target_normals=None, init_transform=None, max_correspondence_distance=math.inf,
                              max_iterations=30, relative_fitness=1e-6, relative_rmse=1e-6, return_correspondences=False):
    """
    Align a source point cloud onto a target by rigid ICP (iterative closest point): point-to-point, or point-to-plane with target normals

    Args:
        source_points : n by 3 array of points (float32 or float64; numpy, or a CUDA/HIP torch tensor): the cloud that moves
        target_points : m by 3 array of the same dtype and kind: the cloud that stays
        target_normals : None (point-to-point, Horn's closed form per iteration), or an m by 3 array of the same dtype and kind, one normal per
            target point (point-to-plane, one linearised 6x6 solve per iteration), e.g. from estimate_point_cloud_normals_knn. Their sign does not matter.
        init_transform : None (identity) or a finite (4, 4) matrix with last row [0, 0, 0, 1]: where the source starts
        max_correspondence_distance : a source point farther than this from its nearest target point takes no part in an iteration. Not NaN, not
            negative; inf (the default) keeps every point.
        max_iterations : the largest number of updates of the transform; an integer >= 0
        relative_fitness, relative_rmse : stop when fitness and inlier_rmse both changed by less than these from one iteration to the next.
            Finite and >= 0. Defaults, names and meaning are Open3D's ICPConvergenceCriteria: despite the names the differences are absolute.
        return_correspondences : If True, also return the target row every source point ended up matched to. Default is False.

    Returns:
        IcpResult(transform, fitness, inlier_rmse, iterations, status, correspondences):
        transform : (4, 4) float64, maps source onto target: target ~ transform[:3, :3] @ p + transform[:3, 3]
        fitness : the share of source points with a correspondence (inliers / n), a float
        inlier_rmse : the root of the mean squared distance of the inliers to their target points, a float
        iterations : the number of updates made, an int
        status : "converged", "max_iterations", "no_correspondences" (no source point within max_correspondence_distance of the target) or
            "degenerate" (point-to-plane: the 6x6 system has a pivot that is not positive -- e.g. a planar target, which leaves three motions free)
        correspondences : None, or (n,) int64: the target row of every inlier, -1 elsewhere
        (numpy arrays in, numpy arrays out; CUDA/HIP torch tensors in, tensors on the same device out)

    Notes:
        The contract (executable in tests/icp_contract.py), reproduced byte for byte. With T the input dtype and M the current
        transform: every source row is transformed in float64, x' = ((M00*x + M01*y) + M02*z) + M03 with separate multiplies and adds, and rounded
        once to T; its correspondence is k_nearest_neighbors(p, target_points, k=1, squared_distances=True) as this library answers it, exact ties
        included; it is an inlier iff d2 < T(max_correspondence_distance)**2 (strict, as everywhere in this library). The sums over the inliers are
        float64 and taken in one fixed order, the solve runs on the host in float64: equal arguments give equal bytes.
        fitness, inlier_rmse and correspondences belong to the returned transform.
        ValueError: the dtype, shape, zero-row and row-limit checks of k_nearest_neighbors (source is the query, target the dataset), with its
        texts; target_normals of another dtype or shape; a bad init_transform, max_correspondence_distance, max_iterations or tolerance; a target
        with NaN, or with +inf and -inf on one axis (the k-NN calls' text).
    """
    dt = _check_pair(source_points, target_points, "query_points", "dataset_points", _KNN_ZERO, _KNN_DIM)
    n, m = _shape2(source_points)[0], _shape2(target_points)[0]
    _check_rows(n, m, text=_KNN_ROW_LIMIT)
    if target_normals is not None:
        _check_target_normals(target_normals, dt, m)
    params = _check_params(init_transform, max_correspondence_distance, max_iterations, relative_fitness, relative_rmse)
    d = _Dev(source_points, target_points)
    return _register("icp", d, (d.pa, n, d.pb, m), n, target_normals, params, return_correspondences)


def _index_register_icp(index, source_points, target_normals=None, init_transform=None, max_correspondence_distance=math.inf, max_iterations=30,
                        relative_fitness=1e-6, relative_rmse=1e-6, return_correspondences=False):
    index._check_query(source_points)
    if target_normals is not None:
        _check_target_normals(target_normals, "float32" if index._suffix == "f32" else "float64", index.num_points)
    params = _check_params(init_transform, max_correspondence_distance, max_iterations, relative_fitness, relative_rmse)
    d = index._resolve_query(source_points)
    n = int(d.a.shape[0])
    return _register("index_icp", d, (index._h, d.pa, n), n, target_normals, params, return_correspondences)
