"""downsample_point_cloud_farthest_point: farthest-point sampling over the HIP kernels of csrc/fps.h. Not in the reference's API (it samples a
cloud on a voxel grid or by Poisson disk); the values follow this library's stated contract (in numpy:
tests/fps_contract.py). DatasetIndex.farthest_point_sample ends here too."""
import ctypes

import numpy as np

from . import _lib
from ._call import _Dev, _call
from ._checks import _check_finite_cloud as _check_cloud


def _check_counts(n, num_samples, start_index):
    num_samples, start_index = int(num_samples), int(start_index)
    if num_samples < 1 or num_samples > n:
        raise ValueError(f"Invalid num_samples ({num_samples}): must be at least 1 and at most the number of points ({n}).")
    if start_index < 0 or start_index >= n:
        raise ValueError(f"Invalid start_index ({start_index}): must be a row of points, in [0, {n}).")
    return num_samples, start_index


def _sample(name, d, head, num_samples, start_index, return_distances, squared_distances, force=0, counters=None):
    idx = d.empty((num_samples,), "i64")
    dists = d.empty((num_samples,), "T") if return_distances else None
    d.flags |= force | (_lib.SQUARED if squared_distances else 0)
    _call(name, d, *head, num_samples, start_index, _Dev.ptr(idx), _Dev.ptr(dists), None if counters is None else counters.ctypes.data)
    return (idx, dists) if return_distances else idx


def _forced(points, num_samples, start_index=0, path="grid", return_distances=True, squared_distances=False):
    """The free function on one named path, 'block' or 'grid', with the grid path's counters (tests and profiles/fps_record.py).
    Returns (idx, dists, counters): counters = int64 [bucket bound tests, bucket updates], summed over the iterations."""
    n = _check_cloud(points)
    num_samples, start_index = _check_counts(n, num_samples, start_index)
    d = _Dev(points, points)
    counters = np.zeros(2, np.int64)
    out = _sample("fps", d, (d.pa, n), num_samples, start_index, return_distances, squared_distances,
                  force={"block": _lib.FPS_ONE_BLOCK, "grid": _lib.FPS_GRID, None: 0}[path], counters=counters)
    return (*out, counters) if return_distances else (out, None, counters)


def _geometry():
    """(one-block row limit in float32 rows -- float64 holds half --, records per bucket, blocks per iteration launch, iterations per replay)"""
    g = (ctypes.c_int * 4)()
    _lib.lib().pcu_hip_fps_geometry(g)
    return tuple(int(x) for x in g)


def downsample_point_cloud_farthest_point(points, num_samples, start_index=0, return_distances=False, squared_distances=False):
    """
    Downsample a point cloud by farthest-point sampling: every sample is the point farthest from the samples before it

    Args:
        points : n by 3 array of points (float32 or float64; numpy, or a CUDA/HIP torch tensor)
        num_samples : the number of samples, 1 <= num_samples <= n
        start_index : the row of the first sample. Default is 0.
        return_distances : If True, also return each sample's distance to the samples before it. Default is False.
        squared_distances : If set to True, then return squared L2 distances. Default is False.

    Returns:
        idx : (num_samples,) int64 rows of points, in the order of selection, all distinct
        dists : (if return_distances) (num_samples,) in the input dtype: dists[0] = +inf; dists[t] is the distance from sample t to the nearest
            of samples 0 .. t-1. It never increases with t, and dists[t] is the covering radius of the first t samples: every point lies
            within dists[t] of one of them.
        (numpy arrays in, numpy arrays out; CUDA/HIP torch tensors in, tensors on the same device out)

    Notes:
        The contract. With T the input dtype, d2(i, s) = ((dx*dx) + (dy*dy)) + (dz*dz) in T, separate multiplies and adds.
        mind[i] starts at +inf and idx[0] = start_index; after row s is selected, mind[i] = min(mind[i], d2(i, s)) for every row and s is out
        of all later choices; the next sample is the remaining row of largest mind, the lowest row among exactly equal values. dists[t] is
        mind[idx[t]] at that moment, as the correctly rounded sqrt, or as it is with squared_distances. The result is a function of the
        arguments alone, and duplicate points never yield a row twice (once every remaining mind is 0, rows follow in ascending order).
        Prefix property: the first j entries of the result are the result for num_samples = j -- sample once for the largest size needed.
        Coordinates so large that d2 overflows to +inf are allowed; the rule above covers them (ties at +inf go to the lowest row).
        ValueError: the dtype, a shape that is not (n, 3), n == 0, more than 2**27 - 16 rows, NaN or infinite coordinates, num_samples outside
        [1, n], start_index outside [0, n).
    """
    n = _check_cloud(points)
    num_samples, start_index = _check_counts(n, num_samples, start_index)
    d = _Dev(points, points)
    return _sample("fps", d, (d.pa, n), num_samples, start_index, return_distances, squared_distances)


def _index_farthest_point_sample(index, num_samples, start_index=0, return_distances=False, squared_distances=False):
    index._check_open()
    num_samples, start_index = _check_counts(index.num_points, num_samples, start_index)
    like = index._like_built()        # no array comes with the call: the results are of the kind the index was built from
    d = _Dev(like, like)
    return _sample("index_fps", d, (index._h,), num_samples, start_index, return_distances, squared_distances)
