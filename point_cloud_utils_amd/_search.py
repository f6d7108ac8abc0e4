"""k_nearest_neighbors, one_sided_hausdorff_distance, hausdorff_distance, chamfer_distance and DatasetIndex: the reference's
``pcu.k_nearest_neighbors`` / ``pcu.one_sided_hausdorff_distance`` (``src/point_cloud_distance.cpp:123-164``, ``:186-234``) and
``pcu.hausdorff_distance`` / ``pcu.chamfer_distance`` (``point_cloud_utils/__init__.py:52-81``, ``:84-120``) over the grid search, with their
signatures, defaults, dtypes, shapes and error behaviour. DatasetIndex's radius and farthest-point methods delegate to _radius and _fps: this
is the one module that composes them ("The Python layer")."""
import ctypes
import math

import numpy as np

from . import _lib
from ._call import _Dev, _Handle, _call, _shape2
from ._checks import _HD_DIM, _HD_ZERO, _KNN_DIM, _KNN_ROW_LIMIT, _KNN_ZERO, _check_float, _check_pair, _check_rows
from ._dbscan import _index_cluster_dbscan
from ._fps import _index_farthest_point_sample
from ._icp import _index_register_icp
from ._radius import _index_radius_count, _index_radius_search


def _check_k(k):
    k = int(k)
    if k <= 0:   # src/point_cloud_distance.cpp:133-135
        raise ValueError(f"Invalid value for k ({k}) must be greater than 0.")
    return k


def _knn(name, d, head, query_points, k, squared_distances, max_points_per_leaf):
    """The k-NN call `name` for the resolved query `d` and its result as the reference's binding returns it. `head`: the entry point's
    arguments before k."""
    n = int(d.a.shape[0])
    dists = d.empty((n, k), "T")
    corrs = d.empty((n, k), "i64")
    if squared_distances:
        d.flags |= _lib.SQUARED
    _call(name, d, *head, k, int(max_points_per_leaf), _Dev.ptr(dists), _Dev.ptr(corrs))
    if k == 1 or n == 1:
        # npe::move(..., squeeze): singleton dimensions are dropped, as numpy.squeeze does -- (n,) for k == 1 (pinned by the reference's
        # tests/test_examples.py:363-368), (k,) for n == 1, 0-d for n == k == 1 (unpinned in the reference)
        shape = () if n == 1 and k == 1 else (-1,)
        return dists.reshape(shape), corrs.reshape(shape)
    if not d.torch:
        q = np.asarray(query_points)
        if q.flags.f_contiguous and not q.flags.c_contiguous:      # EigenDenseLike keeps the query's storage order
            dists = np.asfortranarray(dists)
    return dists, corrs


def k_nearest_neighbors(query_points, dataset_points, k, squared_distances=False, max_points_per_leaf=10,
                        num_threads=-1):
    """
    Compute the k nearest neighbors (L2 distance) from each point in the query point cloud to the dataset point cloud.

    Args:
        query_points : n by 3 array of representing a set of n points (each row is a point of dimension 3).
        dataset_points : m by 3 array of representing a set of m points (each row is a point of dimension 3).
        k : the number of nearest neighbors to query per point. Any k > 0 (k <= 127: grid search; larger k: the reference's
            kd-tree traversal run on the GPU, slower per query). If k exceeds the dataset size the trailing slots hold -1 / -1.0.
        squared_distances : If set to True, then return squared L2 distances. Default is False.
        max_points_per_leaf : leaf size of the reference's kd-tree. Does not change distances; it only fixes the order of exactly tied neighbours, which is reproduced.
        num_threads : OpenMP knob of the reference; accepted and ignored.

    Limit of this implementation: point clouds of more than 2**27 - 16 (134,217,712) rows are rejected with a ValueError.

    Returns:
        dists : An (n, k)-shaped array such that `dists[i,k]` contains the k^th shortest L2 distance from the point `query_points[i, :]` to `dataset_points`
        corrs : An (n, k)-shaped array such that `corrs[i,k]` contains the index into `dataset_points` of the k^th nearest point to `query_points[i, :]`
        (singleton dimensions are squeezed, as the reference's binding does: k == 1 gives (n,)-shaped results)
    """
    k = _check_k(k)
    _check_pair(query_points, dataset_points, "query_points", "dataset_points", _KNN_ZERO, _KNN_DIM)
    d = _Dev(query_points, dataset_points)
    return _knn("knn", d, (d.pa, int(d.a.shape[0]), d.pb, int(d.b.shape[0])), query_points, k, squared_distances, max_points_per_leaf)


def _hausdorff(name, a, b, squared_distances, max_points_per_leaf):
    """The Hausdorff call `name`: (distances, rows of a, rows of b), two slots each (the one-sided call fills the first)."""
    _check_pair(a, b, "source", "target", _HD_ZERO, _HD_DIM)
    d = _Dev(a, b)
    od = np.zeros(2, dtype=d.np_dtype)
    oi = np.zeros(2, dtype=np.int64)
    oj = np.zeros(2, dtype=np.int64)
    if squared_distances:
        d.flags |= _lib.SQUARED
    _call(name, d, d.pa, int(d.a.shape[0]), d.pb, int(d.b.shape[0]), int(max_points_per_leaf), od.ctypes.data, oi.ctypes.data, oj.ctypes.data)
    return od, oi, oj


def one_sided_hausdorff_distance(source, target, return_index=True, squared_distances=False, max_points_per_leaf=10):
    """
    Compute the one sided Hausdorff distance from source to target

    Args:
        source : n by 3 array of representing a set of n points (each row is a point of dimension 3)
        target : m by 3 array of representing a set of m points (each row is a point of dimension 3)
        return_index : Optionally return the index pair `(i, j)` into source and target such that `source[i, :]` and `target[j, :]` are the two points with maximum shortest distance.
        squared_distances : If set to True, then return squared L2 distances.
        max_points_per_leaf : leaf size of the reference's kd-tree. Does not change distances; it only fixes the order of exactly tied neighbours, which is reproduced.

    Returns:
        d : The largest shortest distance, `d` between each point in `source` and the points in `target`.
        i, j : (if return_index) indices such that `source[i, :]` and `target[j, :]` are the two points with maximum shortest distance.
    """
    od, oi, oj = _hausdorff("one_sided_hausdorff", source, target, squared_distances, max_points_per_leaf)
    if return_index:
        return float(od[0]), int(oi[0]), int(oj[0])
    return float(od[0])


def hausdorff_distance(x, y, return_index=False, squared_distances=False, max_points_per_leaf=10):
    """
    Compute the Hausdorff distance between x and y

    Args:
        x : n by 3 array of representing a set of n points (each row is a point of dimension 3)
        y : m by 3 array of representing a set of m points (each row is a point of dimension 3)
        return_index : Optionally return the index pair `(i, j)` into x and y such that `x[i, :]` and `y[j, :]` are the two points with maximum shortest distance.
        squared_distances : If set to True, then return squared L2 distances. Default is False.
        max_points_per_leaf : leaf size of the reference's kd-tree. Does not change distances; it only fixes the order of exactly tied neighbours, which is reproduced.

    Returns:
        The largest shortest distance, `d` between each point in `source` and the points in `target`.
        If `return_index` is set, then this function returns a tuple (d, i, j).
    """
    # one call: both clouds are indexed once and searched in both directions
    od, oi, oj = _hausdorff("hausdorff", x, y, squared_distances, max_points_per_leaf)
    # point_cloud_utils/__init__.py:69-81, on Python floats exactly as there
    hausdorff_x_to_y, idx_x1, idx_y1 = float(od[0]), int(oi[0]), int(oj[0])
    hausdorff_y_to_x, idx_y2, idx_x2 = float(od[1]), int(oi[1]), int(oj[1])
    hausdorff = max(hausdorff_x_to_y, hausdorff_y_to_x)
    if return_index and hausdorff_x_to_y > hausdorff_y_to_x:
        return hausdorff, idx_x1, idx_y1
    elif return_index and hausdorff_x_to_y <= hausdorff_y_to_x:
        return hausdorff, idx_x2, idx_y2
    return hausdorff


def chamfer_distance(x, y, return_index=False, p_norm=2, max_points_per_leaf=10):
    """
    Compute the chamfer distance between two point clouds x, and y

    Args:
        x : n by 3 array of points
        y : m by 3 array of points
        return_index: If set to True, will return a pair (corrs_x_to_y, corrs_y_to_x) where
                    corrs_x_to_y[i] stores the index into y of the closest point to x[i]
                    (i.e. y[corrs_x_to_y[i]] is the nearest neighbor to x[i] in y).
                    corrs_y_to_x is similar to corrs_x_to_y but with x and y reversed.
        max_points_per_leaf : leaf size of the reference's kd-tree. Does not change distances; it only fixes the order of exactly tied neighbours, which is reproduced.
        p_norm : Which norm to use. p_norm can be any real number, inf (for the max norm) -inf (for the min norm),
                0 (for sum(x != 0))
    Returns:
        The chamfer distance between x an dy.
        If return_index is set, then this function returns a tuple (chamfer_dist, corrs_x_to_y, corrs_y_to_x).
    """
    _check_pair(x, y, "query_points", "dataset_points", _KNN_ZERO, _KNN_DIM)
    d = _Dev(x, y)
    n, m = int(d.a.shape[0]), int(d.b.shape[0])
    cxy = d.empty((n,), "i64") if return_index else None
    cyx = d.empty((m,), "i64") if return_index else None
    means = (ctypes.c_double * 2)()
    _call("chamfer", d, d.pa, n, d.pb, m, float(p_norm), int(max_points_per_leaf), ctypes.addressof(means), _Dev.ptr(cxy), _Dev.ptr(cyx))
    # __init__.py:112-115: both means are scalars of the input dtype (np.mean of such a scalar is that scalar);
    # their sum, in that dtype, is the result
    dists_x_to_y = d.np_dtype(means[1])      # norm(x[corrs_y_to_x] - y).mean()
    dists_y_to_x = d.np_dtype(means[0])      # norm(y[corrs_x_to_y] - x).mean()
    cham_dist = dists_x_to_y + dists_y_to_x
    if return_index:
        return cham_dist, cxy, cyx
    return cham_dist


class DatasetIndex(_Handle):
    """A dataset kept on the GPU together with its search index (not in the reference API, which rebuilds its kd-tree on
    every call -- three times, src/point_cloud_distance.cpp:41-42): build once, query many times.

        index = pcu.DatasetIndex(dataset_points, k_hint=8)
        dists, corrs = index.k_nearest_neighbors(query_points, 8)       # same results as pcu.k_nearest_neighbors

    `dataset_points`: (m, 3) float32 / float64, numpy or CUDA/HIP torch tensor (copied; the caller's array can go away).
    `k_hint` sizes the grid cells for the k that will mostly be asked for; any k > 0 is answered exactly.
    Queries must have the dataset's dtype. The index lives on one GPU; call close() (or use `with`) to free it.
    radius_search / radius_count answer fixed-radius queries over the same grid; farthest_point_sample downsamples the dataset itself."""
    _noun, _destroy = "index", "pcu_hip_index_destroy"

    def __init__(self, dataset_points, k_hint=1):
        _check_float(dataset_points, "dataset_points")
        sh = _shape2(dataset_points)
        if sh[0] == 0 or sh[1] != 3:
            raise ValueError(f"dataset_points must have shape (m, 3) with m > 0. Got dataset_points.shape = ({sh[0]}, {sh[1]}).")
        d = _Dev(dataset_points, dataset_points)
        self._suffix, self._np_dtype, self._torch = d.suffix, d.np_dtype, d.torch
        self._open("index_create", d, d.pa, int(d.a.shape[0]), int(k_hint))
        self.num_points = int(d.a.shape[0])

    def _check_query(self, query_points):
        """The checks of a query against the handle that need no device, in k_nearest_neighbors' order and with its texts: open, the index's
        dtype, zero rows, the shape, the row limit. A call's check of its own parameter follows them (the radius') or comes after the first (k)."""
        self._check_open()
        dq = _check_float(query_points, "query_points")
        want = "float32" if self._suffix == "f32" else "float64"
        if dq != want:
            raise ValueError(f"Invalid scalar type ({dq}) for argument 'query_points'. Expected it to match the indexed dataset which is of type {want}.")
        sq = _shape2(query_points)
        if sq[0] == 0:
            raise ValueError(_KNN_ZERO.format(sq[0], sq[1], self.num_points, 3))
        if sq[1] != 3:
            raise ValueError(_KNN_DIM.format(sq[0], sq[1], self.num_points, 3))
        _check_rows(sq[0], text=_KNN_ROW_LIMIT)

    def _resolve_query(self, query_points):
        """The checked query, resolved: a tensor must live on the index's device (a numpy query goes to the default device's context,
        whatever the index's)."""
        d = _Dev(query_points, query_points)
        if d.torch:
            self._same_device(d, "query tensor")
        return d

    def _like_built(self):
        """An empty (0, 3) array of the kind the index was built from -- numpy, or a tensor on its device: what a call that comes without
        an array resolves, so that its results are of that kind."""
        if self._torch:
            import torch
            return torch.empty((0, 3), dtype=torch.float32 if self._suffix == "f32" else torch.float64, device=torch.device("cuda", self._device))
        return np.empty((0, 3), np.float32 if self._suffix == "f32" else np.float64)

    def k_nearest_neighbors(self, query_points, k, squared_distances=False, max_points_per_leaf=10):
        """See point_cloud_utils_amd.k_nearest_neighbors; the dataset is the indexed one."""
        self._check_open()
        k = _check_k(k)
        self._check_query(query_points)
        d = self._resolve_query(query_points)
        return _knn("index_knn", d, (self._h, d.pa, int(d.a.shape[0])), query_points, k, squared_distances, max_points_per_leaf)

    def radius_search(self, query_points, radius, squared_distances=False, sort_results=True):
        """See point_cloud_utils_amd.radius_search; the dataset is the indexed one and the bytes returned are the free function's for every
        radius (with sort_results=False the members are the same and their order follows the index's own grid). The index was laid out for
        k-NN (k_hint): when the radius is large against its cells the scan walks more cells -- it stays exact and only gets slower."""
        return _index_radius_search(self, query_points, radius, squared_distances, sort_results)

    def radius_count(self, query_points, radius):
        """See point_cloud_utils_amd.radius_count; the dataset is the indexed one (the note of radius_search on large radii holds here too)."""
        return _index_radius_count(self, query_points, radius)

    def farthest_point_sample(self, num_samples, start_index=0, return_distances=False, squared_distances=False):
        """See point_cloud_utils_amd.downsample_point_cloud_farthest_point; the cloud is the indexed dataset, nothing is rebuilt, and the bytes
        returned are the free function's (numpy arrays if the index was built from one, tensors on its device otherwise). Above the one-block
        size the sampling walks the index's own cell order: cells sized for a small k_hint make its buckets long and thin, which costs
        speed, never exactness."""
        return _index_farthest_point_sample(self, num_samples, start_index, return_distances, squared_distances)

    def cluster_dbscan(self, eps, min_points, return_core=False):
        """See point_cloud_utils_amd.cluster_point_cloud_dbscan; the cloud is the indexed dataset, nothing is rebuilt, and the bytes returned
        are the free function's (numpy arrays if the index was built from one, tensors on its device otherwise). The walks run over the
        index's own grid: when eps is large against its cells they visit more cells, which costs speed, never exactness."""
        return _index_cluster_dbscan(self, eps, min_points, return_core)

    def register_icp(self, source_points, target_normals=None, init_transform=None, max_correspondence_distance=math.inf, max_iterations=30,
                     relative_fitness=1e-6, relative_rmse=1e-6, return_correspondences=False):
        """See point_cloud_utils_amd.register_point_clouds_icp; the target is the indexed dataset, its grid is built once for all calls, and
        the bytes returned are the free function's for every k_hint. source_points and target_normals are of the dataset's dtype; results
        are of source_points' kind."""
        return _index_register_icp(self, source_points, target_normals, init_transform, max_correspondence_distance, max_iterations,
                                   relative_fitness, relative_rmse, return_correspondences)
