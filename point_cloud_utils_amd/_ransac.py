"""register_point_clouds_ransac: global rigid alignment from putative correspondences by RANSAC over the HIP kernels of csrc/ransac.h and the
host solve of csrc/icp_host.h. Not in the reference's API; the values follow this library's stated contract (in numpy:
tests/ransac_contract.py). No DatasetIndex method: the call needs no spatial index, and an index object's row order is not the user's."""
import collections
import ctypes

import numpy as np

from . import _lib
from ._call import _Dev, _call, _is_torch
from ._checks import (_beside, _check_correspondences, _check_edge_length_ratio, _check_num_iterations, _check_ransac_clouds, _check_seed,
                      _check_tolerance)

RansacRegistrationResult = collections.namedtuple("RansacRegistrationResult", "transform inliers fitness inlier_rmse best_iteration status random_seed")

_STATUS = ("ok", "no_alignment")           # PCU_HIP_RANSAC_*


class _Result(ctypes.Structure):           # pcu_hip_ransac_result
    _fields_ = [("transform", ctypes.c_double * 16), ("fitness", ctypes.c_double), ("inlier_rmse", ctypes.c_double), ("num_inliers", ctypes.c_int64),
                ("best_iteration", ctypes.c_int64), ("score", ctypes.c_int64), ("status", ctypes.c_int32), ("reserved", ctypes.c_int32)]


def _geometry():
    """(correspondences a lane of the scoring kernel keeps in registers, (correspondence, hypothesis) tests of one scoring launch)"""
    g = (ctypes.c_int64 * 2)()
    _lib.lib().pcu_hip_ransac_geometry(g)
    return tuple(int(x) for x in g)


def _register(source_points, target_points, correspondences, max_correspondence_distance, num_iterations, random_seed, edge_length_ratio, refit, launch_tests):
    n, m = _check_ransac_clouds(source_points, target_points)
    if not _is_torch(correspondences):
        correspondences = np.asarray(correspondences)
    c = _check_correspondences(correspondences)
    distance = _check_tolerance(max_correspondence_distance, "max_correspondence_distance")
    num_iterations = _check_num_iterations(num_iterations)
    seed = _check_seed(random_seed)
    ratio = _check_edge_length_ratio(edge_length_ratio)
    d = _Dev(source_points, target_points)
    corr = _beside(d, correspondences)
    rows = d.empty((c,), "i64")
    res = _Result()
    _call("ransac", d, d.pa, n, d.pb, m, _Dev.ptr(corr), c, distance, num_iterations, seed, ratio, 1 if refit else 0, launch_tests, ctypes.addressof(res),
          _Dev.ptr(rows))
    k = int(res.num_inliers)
    inliers = rows[:k]
    if c > 2 * k:                                          # (do not keep the correspondences' room alive behind a small result)
        inliers = inliers.clone() if d.torch else inliers.copy()
    transform = np.array(res.transform, dtype=np.float64).reshape(4, 4)
    if d.torch:
        import torch
        transform = torch.from_numpy(transform).to(d.tdev)
    return RansacRegistrationResult(transform, inliers, float(res.fitness), float(res.inlier_rmse), int(res.best_iteration), _STATUS[res.status], seed)


def _forced(source_points, target_points, correspondences, max_correspondence_distance, num_iterations=100000, random_seed=0, edge_length_ratio=0.9,
            refit=True, launch_tests=0):
    """The call with the scoring launches cut at `launch_tests` (correspondence, hypothesis) tests instead of _geometry()[1] (tests): same bytes."""
    return _register(source_points, target_points, correspondences, max_correspondence_distance, num_iterations, random_seed, edge_length_ratio, refit,
                     int(launch_tests))


def register_point_clouds_ransac(source_points, target_points, correspondences, max_correspondence_distance, num_iterations=100000, random_seed=0,
                                 edge_length_ratio=0.9, refit=True):
    """
    Align a source point cloud onto a target from putative correspondences by RANSAC: the rigid transform through three of them that brings
    the most of them within a distance. Global: the clouds may start far apart; the result is the start register_point_clouds_icp needs.

    Args:
        source_points : n by 3 array of points (float32 or float64; numpy, or a CUDA/HIP torch tensor): the cloud that moves
        target_points : m by 3 array of the same dtype and kind: the cloud that stays
        correspondences : c by 2 int64 array of the same kind, c >= 3: each row is [source row, target row]; a row may repeat. From features:
                nearest, _, is_mutual = match_point_features(source_features, target_features, mutual=True)
                correspondences = np.stack([np.flatnonzero(is_mutual), nearest[is_mutual]], axis=1)
            (torch.stack([torch.nonzero(is_mutual)[:, 0], nearest[is_mutual]], dim=1) for tensors)
        max_correspondence_distance : a correspondence whose moved source point is closer than this to its target point is an inlier; finite
            and not negative
        num_iterations : the number of three-correspondence hypotheses tried, an integer in [1, 2**20]. Default is 100000.
        random_seed : A random seed used to draw the hypotheses. Passing in 0 will use the current time. (0 by default).
        edge_length_ratio : a hypothesis is tried only if every edge of its source triangle is at least this times as long as the same edge of
            its target triangle, and the other way round; in [0, 1], 0 switches the check off. Default is 0.9 (Open3D's edge-length checker).
        refit : If True (the default), solve once more for the least-squares transform of all inliers of the best hypothesis (Horn's closed
            form) and return the inliers of that transform. If False, return the best three-correspondence transform and its inliers.

    Returns:
        RansacRegistrationResult(transform, inliers, fitness, inlier_rmse, best_iteration, status, random_seed):
        transform : (4, 4) float64, maps source onto target: target ~ transform[:3, :3] @ p + transform[:3, 3]; last row [0, 0, 0, 1]
        inliers : (k,) int64 rows of correspondences, ascending
        fitness : k / c, a float
        inlier_rmse : the root of the mean squared distance of the inliers' moved source points to their target points, a float
        best_iteration : the index of the winning hypothesis, an int
        status : "ok", or "no_alignment" when no hypothesis has an inlier (a distance of 0, all points collinear, no triple passes the edge
            check): the transform is the identity then, inliers is empty, fitness and inlier_rmse are 0.0
        random_seed : the seed actually used (never 0): passing it back repeats the result
        (numpy arrays in, numpy arrays out; CUDA/HIP torch tensors in, tensors on the same device out)

    Notes:
        The contract (executable in tests/ransac_contract.py), reproduced byte for byte. All arithmetic is float64, every
        operation rounded on its own; coordinates are converted exactly. Hypothesis h draws three distinct correspondences from three 64-bit
        hashes of (random_seed, h), as segment_point_cloud_plane draws rows -- it depends on (random_seed, h, c) alone, so the hypotheses of a
        shorter call are the first of a longer one. The edge check compares squared lengths, without a square root. The transform of a
        hypothesis is a decision, not a fit: an orthonormal frame on each triangle (e1 along the first edge, e3 along the normal, e2 = e3 x e1),
        R = E_target E_source^T, and the translation that maps the source triangle's centroid onto the target's; triangles without a frame (two
        equal points, collinear points) have no inliers. Correspondence i is an inlier iff |R s_i + t - t_i|^2 < max_correspondence_distance**2,
        strict, as everywhere in this library. The winner is the lowest h of the largest inlier count: an integer, so the result does not depend
        on how the GPU was launched. The refit takes the inliers' sums in register_point_clouds_icp's fixed order and its Horn solve.
        Equal arguments give equal bytes.
        ValueError: for either cloud the dtype, a shape that is not (n, 3), n == 0, more than 2**27 - 16 rows, NaN or infinite coordinates
        (the checks and texts of segment_point_cloud_plane), two dtypes that differ; correspondences that are not (c, 2) int64, c < 3 or
        c > 2**27 - 16, or hold an entry that is not a row of its cloud; a max_correspondence_distance that is NaN, negative or infinite;
        num_iterations outside [1, 2**20]; a random_seed that is not an unsigned 32-bit integer; an edge_length_ratio that is NaN or outside
        [0, 1]. KeyboardInterrupt: a cancelled call.
    """
    return _register(source_points, target_points, correspondences, max_correspondence_distance, num_iterations, random_seed, edge_length_ratio, refit, 0)
