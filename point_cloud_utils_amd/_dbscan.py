"""cluster_point_cloud_dbscan: density-based clustering (DBSCAN) over the HIP kernels of csrc/dbscan.h. Not in the reference's API; the values
follow this library's stated contract (in numpy: tests/dbscan_contract.py). DatasetIndex.cluster_dbscan ends here too."""
import ctypes
import operator

import numpy as np

from ._call import _Dev, _call, _int_out, _shape2
from ._checks import _KNN_DIM, _KNN_ROW_LIMIT, _KNN_ZERO, _check_pair, _check_radius, _check_rows

_MIN_POINTS_TOP = 2 ** 62          # (beyond any row count: nobody is core)


def _check_min_points(min_points):
    try:
        m = operator.index(min_points)
    except TypeError:
        m = 0
    if m < 1:
        raise ValueError(f"Invalid min_points ({min_points}): must be an integer of at least 1.")
    return min(m, _MIN_POINTS_TOP)


def _check_cloud(points):
    """The cloud is query and dataset of its own radius search: k_nearest_neighbors' checks of that pair, in its order and with its texts."""
    _check_pair(points, points, "query_points", "dataset_points", _KNN_ZERO, _KNN_DIM)
    n = _shape2(points)[0]
    _check_rows(n, text=_KNN_ROW_LIMIT)
    return n


def _cluster(name, d, head, n, eps, min_points, return_core):
    labels = d.empty((n,), "i64")
    core = _int_out(d, (n,), np.bool_) if return_core else None
    count = ctypes.c_int64(0)
    _call(name, d, *head, eps, min_points, _Dev.ptr(labels), _Dev.ptr(core), ctypes.addressof(count))
    return (labels, core) if return_core else labels


def cluster_point_cloud_dbscan(points, eps, min_points, return_core=False):
    """
    Cluster a point cloud by density (DBSCAN): points with enough neighbours within eps grow clusters, sparse points are noise

    Args:
        points : n by 3 array of points (float32 or float64; numpy, or a CUDA/HIP torch tensor)
        eps : the neighbourhood radius (L2 distance); finite and not negative
        min_points : a point with at least this many points within eps of it, itself included, is a core point; an integer >= 1
        return_core : If True, also return which points are core points. Default is False.

    Returns:
        labels : (n,) int64: the cluster of every point, 0, 1, ... in the order of the clusters' smallest core rows; -1 for noise
        is_core : (if return_core) (n,) bool
        (numpy arrays in, numpy arrays out; CUDA/HIP torch tensors in, tensors on the same device out -- one small read-back crosses to the host)

    Notes:
        The contract. The neighbourhood of point i is exactly its row of radius_search(points, points, eps): with T the input
        dtype, d2 = ((dx*dx) + (dy*dy)) + (dz*dz) in T, separate multiplies and adds; r2 = T(eps) * T(eps); j is a neighbour of i iff d2 < r2.
        The comparison is strict, as everywhere in this library: eps == 0 gives all noise, and two points at exactly eps are not neighbours.
        is_core == (radius_count(points, points, eps) >= min_points). The clusters are the connected components of the core points joined
        where d2 < r2, numbered like connected_components' (and like scikit-learn's ascending loop numbers them). A point that is not core but
        has a core neighbour takes the label of its NEAREST core neighbour (smallest d2, the smaller row among equal ones): a function of the
        arguments alone, where scikit-learn gives such a point to whichever cluster reaches it first. Core mask, core labels and the noise set
        equal scikit-learn's DBSCAN(eps, min_samples=min_points) whenever no distance lies within rounding of eps.
        A row with a non-finite coordinate is noise and nobody's neighbour. Equal arguments give equal bytes.
        ValueError: the dtype, shape, zero-row and row-limit checks of k_nearest_neighbors (the cloud is both of its clouds), with its texts;
        an eps that is NaN, negative or infinite; a min_points that is not an integer >= 1; a cloud with NaN, or with +inf and -inf on one
        axis (the k-NN calls' text).
    """
    n = _check_cloud(points)
    eps = _check_radius(eps)
    min_points = _check_min_points(min_points)
    d = _Dev(points, points)
    return _cluster("dbscan", d, (d.pa, n), n, eps, min_points, return_core)


def _index_cluster_dbscan(index, eps, min_points, return_core=False):
    index._check_open()
    eps = _check_radius(eps)
    min_points = _check_min_points(min_points)
    like = index._like_built()        # no array comes with the call: the results are of the kind the index was built from
    d = _Dev(like, like)
    return _cluster("index_dbscan", d, (index._h,), int(index.num_points), eps, min_points, return_core)
