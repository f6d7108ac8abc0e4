"""segment_point_cloud_plane: the dominant plane of a cloud by RANSAC over the HIP kernels of csrc/plane.h and the host solve of
csrc/plane_host.h. Not in the reference's API; the values follow this library's stated contract (in numpy:
tests/plane_contract.py). No DatasetIndex method: the call needs no spatial index, and an index object's row order is not the user's."""
import collections
import ctypes

import numpy as np

from . import _lib
from ._call import _Dev, _call
from ._checks import _check_distance_threshold, _check_finite_cloud, _check_num_iterations, _check_plane_rows, _check_seed

PlaneResult = collections.namedtuple("PlaneResult", "plane inliers best_iteration status random_seed")

_STATUS = ("ok", "no_plane")               # PCU_HIP_PLANE_*


class _Result(ctypes.Structure):           # pcu_hip_plane_result
    _fields_ = [("plane", ctypes.c_double * 4), ("num_inliers", ctypes.c_int64), ("best_iteration", ctypes.c_int64), ("score", ctypes.c_int64),
                ("status", ctypes.c_int32), ("reserved", ctypes.c_int32)]


def _geometry():
    """(rows a lane of the scoring kernel keeps in registers, (row, hypothesis) tests of one scoring launch)"""
    g = (ctypes.c_int64 * 2)()
    _lib.lib().pcu_hip_plane_geometry(g)
    return tuple(int(x) for x in g)


def _segment(points, distance_threshold, num_iterations, random_seed, refit, launch_tests):
    n = _check_plane_rows(_check_finite_cloud(points))
    distance_threshold = _check_distance_threshold(distance_threshold)
    num_iterations = _check_num_iterations(num_iterations)
    seed = _check_seed(random_seed)
    d = _Dev(points, points)
    rows = d.empty((n,), "i64")
    res = _Result()
    _call("plane", d, d.pa, n, distance_threshold, num_iterations, seed, 1 if refit else 0, launch_tests, ctypes.addressof(res), _Dev.ptr(rows))
    k = int(res.num_inliers)
    inliers = rows[:k]
    if n > 2 * k:                                          # (do not keep the cloud's room alive behind a small result)
        inliers = inliers.clone() if d.torch else inliers.copy()
    plane = np.array(res.plane, dtype=np.float64)
    if d.torch:
        import torch
        plane = torch.from_numpy(plane).to(d.tdev)
    return PlaneResult(plane, inliers, int(res.best_iteration), _STATUS[res.status], seed)


def _forced(points, distance_threshold, num_iterations=1000, random_seed=0, refit=True, launch_tests=0):
    """The call with the scoring launches cut at `launch_tests` (row, hypothesis) tests instead of _geometry()[1] (tests): same bytes."""
    return _segment(points, distance_threshold, num_iterations, random_seed, refit, int(launch_tests))


def segment_point_cloud_plane(points, distance_threshold, num_iterations=1000, random_seed=0, refit=True):
    """
    Find the dominant plane of a point cloud by RANSAC: the plane through three of its points that has the most points within a distance

    Args:
        points : n by 3 array of points, n >= 3 (float32 or float64; numpy, or a CUDA/HIP torch tensor)
        distance_threshold : a point closer to the plane than this is an inlier; finite and not negative
        num_iterations : the number of three-point hypotheses tried, an integer in [1, 2**20]. Default is 1000.
        random_seed : A random seed used to draw the hypotheses. Passing in 0 will use the current time. (0 by default).
        refit : If True (the default), fit the plane once more to all inliers of the best hypothesis (least squares) and return the inliers
            of that plane. If False, return the best three-point plane and its inliers.

    Returns:
        PlaneResult(plane, inliers, best_iteration, status, random_seed):
        plane : (4,) float64 [a, b, c, d] with a*x + b*y + c*z + d = 0 and a unit normal, the first non-zero of a, b, c positive
        inliers : (k,) int64 rows of points, ascending
        best_iteration : the index of the winning hypothesis, an int
        status : "ok", or "no_plane" when no hypothesis has an inlier (all points identical or collinear, a threshold of 0): the plane is
            all zeros then and inliers is empty
        random_seed : the seed actually used (never 0): passing it back repeats the result
        (numpy arrays in, numpy arrays out; CUDA/HIP torch tensors in, tensors on the same device out)

    Notes:
        The contract (executable in tests/plane_contract.py), reproduced byte for byte. All arithmetic is float64, every
        operation rounded on its own; coordinates are converted exactly. Hypothesis h draws three distinct rows from three 64-bit hashes of
        (random_seed, h) -- it depends on (random_seed, h, points) alone, so the hypotheses of a shorter call are the first of a longer one.
        With a = p1 - p0, b = p2 - p0, c = a x b, l2 = (c0*c0 + c1*c1) + c2*c2 and k = (c0*p0x + c1*p0y) + c2*p0z, row i is an inlier iff
        e*e < distance_threshold**2 * l2 with e = ((c0*x + c1*y) + c2*z) - k: no square root, no division, and the comparison is strict, as
        everywhere in this library. Three points without a plane (two equal, collinear) have no inliers. The winner is the lowest h of the
        largest inlier count: an integer, so the result does not depend on how the GPU was launched. The refit takes the inliers' first and
        second moments about p0 in one fixed order and the smallest eigenvector of their covariance by a cyclic Jacobi iteration.
        Equal arguments give equal bytes.
        ValueError: the dtype, a shape that is not (n, 3), n == 0, more than 2**27 - 16 rows, NaN or infinite coordinates (the checks and
        texts of downsample_point_cloud_farthest_point), n < 3, a distance_threshold that is NaN, negative or infinite, num_iterations
        outside [1, 2**20], a random_seed that is not an unsigned 32-bit integer. KeyboardInterrupt: a cancelled call.
    """
    return _segment(points, distance_threshold, num_iterations, random_seed, refit, 0)
