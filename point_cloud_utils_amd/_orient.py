"""orient_point_cloud_normals: consistent signs for the normals of a cloud over the HIP kernels of csrc/orient.h. Not in the reference's API; the
values follow this library's stated contract (in numpy: tests/orient_contract.py)."""
import operator

import numpy as np

from ._call import _Dev, _call, _int_out, _is_torch
from ._checks import _MAX_ROWS, _check_normals, _check_rows, _host_searched_cloud


def _check_k(k):
    try:
        m = operator.index(k)
    except TypeError:
        m = 0
    if m <= 0:                  # estimate_point_cloud_normals_knn's text
        raise ValueError(f"Invalid number of neighbors ({k}) must be greater than 0.")
    return min(m, _MAX_ROWS)    # (no cloud has more other rows)


def orient_point_cloud_normals(points, normals, k=10, return_flipped=False, max_points_per_leaf=10):
    """
    Give the normals of a point cloud consistent signs: each comes back as it is or negated, outward for a closed surface

    Args:
        points : n by 3 array of points (float32 or float64; numpy, or a CUDA/HIP torch tensor)
        normals : n by 3 array of normals (the points' dtype and kind), for instance estimate_point_cloud_normals_knn's; need not have unit length
        k : the signs are propagated between a point and its k nearest neighbours; an integer >= 1. Default is 10.
        return_flipped : If True, also return which normals were negated. Default is False.
        max_points_per_leaf : as in k_nearest_neighbors: it only fixes the order of exactly tied neighbours

    Returns:
        normals_out : (n, 3) array: normals_out[i] is normals[i] or its exact negation (the three sign bits inverted); nothing is normalised
        flipped : (if return_flipped) (n,) bool: which rows were negated
        (numpy arrays in, numpy arrays out; CUDA/HIP torch tensors in, tensors on the same device out)
        These are what point_cloud_fast_winding_number, ray_surfel_intersection and pointcloud_surfel_geometry take as oriented normals.

    Notes:
        The contract. With m = min(k + 1, n) and nbr the (n, m) rows of k_nearest_neighbors(points, points, m, max_points_per_leaf=...),
        every (i, nbr[i, c]) with nbr[i, c] != i is an undirected edge {lo, hi}. Its agreement is d = (n_lo0*n_hi0 + n_lo1*n_hi1) + n_lo2*n_hi2 in
        float64, separate multiplies and adds; an edge whose d is not finite is no edge (a row with a NaN or infinite normal stays alone and keeps
        its bytes). The signs follow the minimum spanning forest of the edges under the strict total order (1 - |d|, lo, hi), which is unique:
        across a tree edge two rows get opposite flips iff d < 0 (Hoppe et al. 1992: the flattest parts of the surface are crossed first). In every
        tree the row with the largest z (the first among equal ones) ends with normal_z >= 0: the topmost point looks up. A cloud whose
        neighbour graph is not connected is oriented tree by tree, each by its own topmost row; last_stats()["n_escalated"] is the number of
        trees and ["n_passes"] the rounds the forest took. The result is a function of the arguments alone, and multiplying any input normals by
        -1 leaves it unchanged (unless an agreement or the topmost normal_z is exactly 0). Equal arguments give equal bytes.
        ValueError: the scalar-type and shape checks of point_cloud_fast_winding_number's p and n, with its texts; the row limit; a k that is
        not an integer >= 1 (estimate_point_cloud_normals_knn's text); a cloud with NaN, or with +inf and -inf on one axis (the k-NN calls' text).
    """
    _, n = _check_normals(points, normals, False)
    _check_rows(n)
    k = _check_k(k)
    if not (_is_torch(points) or _is_torch(normals)):
        _host_searched_cloud(np.asarray(points))
    d = _Dev(points, normals)
    out = d.empty((n, 3), "T")
    flipped = _int_out(d, (n,), np.bool_) if return_flipped else None
    _call("orient_normals", d, d.pa, d.pb, n, k, int(max_points_per_leaf), _Dev.ptr(out), _Dev.ptr(flipped))
    return (out, flipped) if return_flipped else out
