"""radius_search and radius_count: every dataset point within a radius of every query, over the HIP kernels of csrc/radius.h. Not in the
reference's exported API (its kd-tree's radiusSearch, which it uses inside estimate_point_cloud_normals_ball only); the values follow this
library's stated contract (in numpy: tests/radius_contract.py). DatasetIndex.radius_search / radius_count end here too."""
import ctypes

import numpy as np

from . import _lib
from ._call import _Dev, _call, _shape2, _take
from ._checks import _KNN_DIM, _KNN_ROW_LIMIT, _KNN_ZERO, _check_pair, _check_radius, _check_rows


def _search(name, d, head, radius, squared_distances, sort_results):
    """The two halves of a search: offsets and the total, then the parked rows. `head`: the entry point's arguments before the radius."""
    n = int(d.a.shape[0])
    offsets = d.empty((n + 1,), "i64")
    total = ctypes.c_int64(0)
    if squared_distances:
        d.flags |= _lib.SQUARED
    _call(name, d, *head, radius, int(bool(sort_results)), _Dev.ptr(offsets), ctypes.addressof(total))
    m = int(total.value)
    indices, dists = _take("radius_search", d, [((m,), np.int64), ((m,), np.dtype(d.np_dtype))], n, m)
    return offsets, indices, dists


def _count(name, d, head, radius):
    counts = d.empty((int(d.a.shape[0]),), "i64")
    _call(name, d, *head, radius, _Dev.ptr(counts))
    return counts


def _check_free(query_points, dataset_points, radius):
    _check_pair(query_points, dataset_points, "query_points", "dataset_points", _KNN_ZERO, _KNN_DIM)
    _check_rows(_shape2(query_points)[0], _shape2(dataset_points)[0], text=_KNN_ROW_LIMIT)
    return _check_radius(radius)


def radius_search(query_points, dataset_points, radius, squared_distances=False, sort_results=True):
    """
    All points of the dataset point cloud within a radius (L2 distance) of each point of the query point cloud

    Args:
        query_points : n by 3 array of representing a set of n points (each row is a point of dimension 3)
        dataset_points : m by 3 array of representing a set of m points (each row is a point of dimension 3); same dtype (float32 or float64)
        radius : the search radius; finite and not negative
        squared_distances : If set to True, then return squared L2 distances. Default is False.
        sort_results : If True (default) every row is ascending by (distance, dataset row); if False the rows hold the same neighbours in an
            order that is a function of the arguments alone (two equal calls give equal bytes) and is otherwise not promised

    Returns:
        offsets : (n + 1,) int64: the neighbours of query i are indices[offsets[i]:offsets[i + 1]], with dists alongside them
        indices : (offsets[n],) int64 rows of dataset_points
        dists : (offsets[n],) distances in the input dtype
        (numpy arrays in, numpy arrays out; CUDA/HIP torch tensors in, tensors on the same device out -- only the total crosses to the host)

    Notes:
        The contract. With T the input dtype, d2 = ((dx*dx) + (dy*dy)) + (dz*dz) in T, query minus dataset, separate multiplies
        and adds; r2 = T(radius) * T(radius); dataset row j is a neighbour of query i iff d2 < r2. The comparison is strict, as nanoflann's
        RadiusResultSet::addPoint is: radius == 0 gives empty rows even for a coincident point, and a point at exactly the radius is out.
        dists is the correctly rounded sqrt(d2) in T, or d2 itself. Ties in d2 are ordered by dataset row (nanoflann leaves them to std::sort).
        A query row with a non-finite coordinate gets an empty row; a dataset row with single-signed infinities is nobody's neighbour.
        ValueError: the dtype, shape, zero-row and row-limit checks of k_nearest_neighbors, with its texts; a radius that is NaN, negative or
        infinite; a dataset with NaN, or with +inf and -inf on one axis (the k-NN calls' text); a result of 2**31 neighbours or more (the
        text names the total; nothing is allocated for it -- radius_count has no such limit).
    """
    radius = _check_free(query_points, dataset_points, radius)
    d = _Dev(query_points, dataset_points)
    return _search("radius_search", d, (d.pa, int(d.a.shape[0]), d.pb, int(d.b.shape[0])), radius, squared_distances, sort_results)


def radius_count(query_points, dataset_points, radius):
    """
    The number of points of the dataset point cloud within a radius of each point of the query point cloud

    Returns:
        counts : (n,) int64; counts[i] == offsets[i + 1] - offsets[i] of radius_search with the same arguments. Only (n,) is allocated and
        there is no limit on the total.
    """
    radius = _check_free(query_points, dataset_points, radius)
    d = _Dev(query_points, dataset_points)
    return _count("radius_count", d, (d.pa, int(d.a.shape[0]), d.pb, int(d.b.shape[0])), radius)


def _check_index(index, query_points, radius):
    """The handle's checks of a query, then the radius' as in the free functions, then the resolved query."""
    index._check_query(query_points)
    radius = _check_radius(radius)
    return index._resolve_query(query_points), radius


def _index_radius_search(index, query_points, radius, squared_distances=False, sort_results=True):
    d, radius = _check_index(index, query_points, radius)
    return _search("index_radius_search", d, (index._h, d.pa, int(d.a.shape[0])), radius, squared_distances, sort_results)


def _index_radius_count(index, query_points, radius):
    d, radius = _check_index(index, query_points, radius)
    return _count("index_radius_count", d, (index._h, d.pa, int(d.a.shape[0])), radius)
