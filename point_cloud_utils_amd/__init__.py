"""point_cloud_utils_amd -- MI355X (gfx950) drop-in for point-cloud-utils' KNN / Chamfer / Hausdorff hot path.

The four callables below have the signatures, defaults, dtypes, shapes and error behaviour of the reference's
``pcu.k_nearest_neighbors`` / ``pcu.one_sided_hausdorff_distance`` (``src/point_cloud_distance.cpp:123-164``,
``:186-234``) and ``pcu.hausdorff_distance`` / ``pcu.chamfer_distance``
(``point_cloud_utils/__init__.py:52-81``, ``:84-120``), so

    import point_cloud_utils_amd as pcu

is a drop-in for that path. All computation happens in hand-written HIP kernels behind the C ABI of
``libpcu_hip.so`` (``include/pcu_hip.h``); there is no CPU fallback: without the library or without a GPU the
calls raise.

Inputs may be numpy arrays (host; copied to the GPU for the call, results returned as numpy / Python scalars,
exactly as the reference returns them) or, as an extension, CUDA/HIP ``torch`` tensors (device-resident: nothing
crosses PCIe, array results are returned as ``torch`` tensors on the same device).

``num_threads`` is an OpenMP knob of the reference: accepted, ignored. ``max_points_per_leaf`` is the reference's
kd-tree leaf size: it cannot change distances, but the order of *exactly tied* neighbours in the reference is the
order its kd-tree traversal meets them, so it is forwarded and that order is reproduced on the GPU.
"""
import ctypes

import numpy as np

from . import _lib
from ._lib import Stats, set_cell_occupancy, device_count  # noqa: F401
from ._call import (_DT_FAST, _ENV_FLAGS, _FN, _TIMING, _Dev, _Handle, _dtype_name, _flags, _fn, _is_torch,  # noqa: F401
                    _last_stats, _record, _shape2)
from ._checks import _check_float

__all__ = ["k_nearest_neighbors", "one_sided_hausdorff_distance", "hausdorff_distance", "chamfer_distance",
           "estimate_point_cloud_normals_knn", "estimate_point_cloud_normals_ball",
           "morton_encode", "morton_decode", "morton_add", "morton_subtract", "morton_knn",
           "downsample_point_cloud_on_voxel_grid", "deduplicate_point_cloud", "downsample_point_cloud_poisson_disk",
           "pairwise_distances", "sinkhorn", "earth_movers_distance", "closest_points_on_mesh", "MeshIndex",
           "ray_mesh_intersection", "RayMeshIntersector", "interpolate_barycentric_coords",
           "triangle_soup_fast_winding_number", "signed_distance_to_mesh",
           "mesh_face_areas", "sample_mesh_random", "sample_mesh_poisson_disk",
           "point_cloud_fast_winding_number", "PointCloudWindingIndex", "estimate_mesh_face_normals",
           "ray_surfel_intersection", "RaySurfelIntersector", "pointcloud_surfel_geometry",
           "voxelize_triangle_mesh", "sparse_voxel_grid_boundary", "voxel_grid_geometry",
           "connected_components", "flood_fill_3d",
           "marching_cubes_sparse_voxel_grid", "sparse_voxel_grid_to_hex_mesh",
           "adjacency_list", "mesh_vertex_adjacency", "estimate_mesh_vertex_normals", "laplacian_smooth_mesh",
           "remove_mesh_vertices", "remove_unreferenced_mesh_vertices", "deduplicate_mesh_vertices", "orient_mesh_faces", "decimate_triangle_mesh",
           "radius_search", "radius_count", "downsample_point_cloud_farthest_point",
           "last_stats", "set_timing", "set_cell_occupancy", "device_count", "DatasetIndex", "cancel"]

def cancel():
    """Ask the call that is in flight (any thread of this process) to stop: it returns early and raises KeyboardInterrupt in its caller, as
    Ctrl-C does -- the reference polls PyErr_CheckSignals() inside its search loops (src/point_cloud_distance.cpp:60-75, 96-98). Callable from
    another thread or a signal handler; a request made while no call is running is dropped when the next one starts."""
    _lib.lib().pcu_hip_cancel()


def set_timing(level):
    """Device-side timing written into last_stats(): 0 = none (default; counters only), 1 = the main search launches
    (ms_kernel_search / n_kernel_search), 2 = also the phases of the call (ms_index / ms_search / ms_total / ms_tie).
    Every HIP event costs a few microseconds of bubble between kernels, which is why it is opt-in. Returns the old level."""
    old = _TIMING[0]
    _TIMING[0] = int(level)
    return old


def last_stats():
    """Statistics of the most recent call (escalations, tie handling, device milliseconds)."""
    st = _last_stats[0]
    return st.as_dict() if st is not None else {}


def _check_pair(a, b, aname, bname, zero_fmt, dim_fmt):
    """dtype / shape validation in the order of src/point_cloud_distance.cpp:136-149 (and :195-208)."""
    da, db = _check_float(a, aname), _dtype_name(b)
    if db != da:
        raise ValueError(f"Invalid scalar type ({db}) for argument '{bname}'. Expected it to match argument "
                         f"'{aname}' which is of type {da}.")
    sa, sb = _shape2(a), _shape2(b)
    if sa[0] == 0 or sb[0] == 0:
        raise ValueError(zero_fmt.format(sa[0], sa[1], sb[0], sb[1]))
    if sa[1] != 3 or sb[1] != 3:
        raise ValueError(dim_fmt.format(sa[0], sa[1], sb[0], sb[1]))
    return da


_KNN_ZERO = ("Invalid input set with zero elements: query_points and dataset_points must have shape (n, 3) and (m, 3). "
             "Got query_points.shape = ({}, {}), dataset_points.shape = ({}, {}).")
_KNN_DIM = ("Only 3D inputs are supported: query_points and dataset_points must have shape (n, 3) and (m, 3). "
            "Got query_points.shape = ({}, {}), dataset_points.shape = ({}, {}).")
_HD_ZERO = ("Invalid input set with zero elements: source and targets must have shape (n, 3) and (m, 3). "
            "Got source.shape = ({}, {}), target.shape = ({}, {}).")
_HD_DIM = ("Only 3D inputs are supported: source and targets must have shape (n, 3) and (m, 3). "
           "Got source.shape = ({}, {}), target.shape = ({}, {}).")


def _squeeze(dists, corrs, n, k):
    """npe::move(..., squeeze): singleton dimensions are dropped, as numpy.squeeze does -- (n,) for k == 1 (pinned by the
    reference's tests/test_examples.py:363-368), (k,) for n == 1, 0-d for n == k == 1 (unpinned in the reference)."""
    if n == 1 and k == 1:
        return dists.reshape(()), corrs.reshape(())
    return dists.reshape(-1), corrs.reshape(-1)


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
    k = int(k)
    if k <= 0:   # src/point_cloud_distance.cpp:133-135
        raise ValueError(f"Invalid value for k ({k}) must be greater than 0.")
    _check_pair(query_points, dataset_points, "query_points", "dataset_points", _KNN_ZERO, _KNN_DIM)
    d = _Dev(query_points, dataset_points)
    n, m = int(d.a.shape[0]), int(d.b.shape[0])
    dists = d.empty((n, k), "T")
    corrs = d.empty((n, k), "i64")
    st = Stats()
    flags = d.flags | (_lib.SQUARED if squared_distances else 0)
    rc = _fn("knn", d.suffix)(d.ctx, d.pa, n, d.pb, m, k, int(max_points_per_leaf), _Dev.ptr(dists), _Dev.ptr(corrs),
                              flags, d.stream, ctypes.addressof(st))
    _lib.check(rc)
    _record(st)
    if k == 1 or n == 1:
        return _squeeze(dists, corrs, n, k)
    if not d.torch:
        q = np.asarray(query_points)
        if q.flags.f_contiguous and not q.flags.c_contiguous:      # EigenDenseLike keeps the query's storage order
            dists = np.asfortranarray(dists)
    return dists, corrs


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
    _check_pair(source, target, "source", "target", _HD_ZERO, _HD_DIM)
    d = _Dev(source, target)
    n, m = int(d.a.shape[0]), int(d.b.shape[0])
    od = np.zeros(2, dtype=d.np_dtype)
    oi = np.zeros(2, dtype=np.int64)
    oj = np.zeros(2, dtype=np.int64)
    st = Stats()
    flags = d.flags | (_lib.SQUARED if squared_distances else 0)
    rc = _fn("one_sided_hausdorff", d.suffix)(
        d.ctx, d.pa, n, d.pb, m, int(max_points_per_leaf), od.ctypes.data, oi.ctypes.data, oj.ctypes.data, flags, d.stream,
        ctypes.addressof(st))
    _lib.check(rc)
    _record(st)
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
    _check_pair(x, y, "source", "target", _HD_ZERO, _HD_DIM)
    d = _Dev(x, y)
    n, m = int(d.a.shape[0]), int(d.b.shape[0])
    od = np.zeros(2, dtype=d.np_dtype)
    oi = np.zeros(2, dtype=np.int64)
    oj = np.zeros(2, dtype=np.int64)
    st = Stats()
    flags = d.flags | (_lib.SQUARED if squared_distances else 0)
    rc = _fn("hausdorff", d.suffix)(   # one call: both clouds are indexed once and searched in both directions
        d.ctx, d.pa, n, d.pb, m, int(max_points_per_leaf), od.ctypes.data, oi.ctypes.data, oj.ctypes.data, flags, d.stream,
        ctypes.addressof(st))
    _lib.check(rc)
    _record(st)
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
    st = Stats()
    rc = _fn("chamfer", d.suffix)(
        d.ctx, d.pa, n, d.pb, m, float(p_norm), int(max_points_per_leaf), ctypes.addressof(means), _Dev.ptr(cxy), _Dev.ptr(cyx),
        d.flags, d.stream, ctypes.addressof(st))
    if rc:
        _lib.check(rc)
    _record(st)
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

    def k_nearest_neighbors(self, query_points, k, squared_distances=False, max_points_per_leaf=10):
        """See point_cloud_utils_amd.k_nearest_neighbors; the dataset is the indexed one."""
        self._check_open()
        k = int(k)
        if k <= 0:
            raise ValueError(f"Invalid value for k ({k}) must be greater than 0.")
        dq = _check_float(query_points, "query_points")
        want = "float32" if self._suffix == "f32" else "float64"
        if dq != want:
            raise ValueError(f"Invalid scalar type ({dq}) for argument 'query_points'. Expected it to match the indexed dataset which is of type {want}.")
        sq = _shape2(query_points)
        if sq[0] == 0:
            raise ValueError(_KNN_ZERO.format(sq[0], sq[1], self.num_points, 3))
        if sq[1] != 3:
            raise ValueError(_KNN_DIM.format(sq[0], sq[1], self.num_points, 3))
        d = _Dev(query_points, query_points)
        if d.torch:                                  # (a numpy query goes to the default device's context, whatever the index's)
            self._same_device(d, "query tensor")
        n = int(d.a.shape[0])
        dists = d.empty((n, k), "T")
        corrs = d.empty((n, k), "i64")
        st = Stats()
        flags = d.flags | (_lib.SQUARED if squared_distances else 0)
        rc = _fn("index_knn", d.suffix)(d.ctx, self._h, d.pa, n, k, int(max_points_per_leaf), _Dev.ptr(dists), _Dev.ptr(corrs),
                                        flags, d.stream, ctypes.addressof(st))
        if rc:
            _lib.check(rc)
        _record(st)
        if k == 1 or n == 1:
            return _squeeze(dists, corrs, n, k)
        if not d.torch:
            q = np.asarray(query_points)
            if q.flags.f_contiguous and not q.flags.c_contiguous:
                dists = np.asfortranarray(dists)
        return dists, corrs

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


from ._normals import estimate_point_cloud_normals_knn, estimate_point_cloud_normals_ball  # noqa: E402,F401
from ._voxel import (morton_encode, morton_decode, morton_add, morton_subtract, morton_knn,  # noqa: E402,F401
                     downsample_point_cloud_on_voxel_grid, deduplicate_point_cloud)
from ._sinkhorn import pairwise_distances, sinkhorn, earth_movers_distance  # noqa: E402,F401
from ._poisson import downsample_point_cloud_poisson_disk  # noqa: E402,F401
from ._mesh import (closest_points_on_mesh, MeshIndex, ray_mesh_intersection, RayMeshIntersector,  # noqa: E402,F401
                    interpolate_barycentric_coords, triangle_soup_fast_winding_number, signed_distance_to_mesh)
from ._mesh_sample import mesh_face_areas, sample_mesh_random, sample_mesh_poisson_disk  # noqa: E402,F401
from ._pc_winding import point_cloud_fast_winding_number, PointCloudWindingIndex, estimate_mesh_face_normals  # noqa: E402,F401
from ._surfel import ray_surfel_intersection, RaySurfelIntersector, pointcloud_surfel_geometry  # noqa: E402,F401
from ._voxelize import voxelize_triangle_mesh, sparse_voxel_grid_boundary, voxel_grid_geometry  # noqa: E402,F401
from ._components import connected_components, flood_fill_3d  # noqa: E402,F401
from ._marching_cubes import marching_cubes_sparse_voxel_grid, sparse_voxel_grid_to_hex_mesh  # noqa: E402,F401
from ._mesh_smooth import adjacency_list, mesh_vertex_adjacency, estimate_mesh_vertex_normals, laplacian_smooth_mesh  # noqa: E402,F401
from ._mesh_repair import remove_mesh_vertices, remove_unreferenced_mesh_vertices, deduplicate_mesh_vertices, orient_mesh_faces  # noqa: E402,F401
from ._mesh_decimate import decimate_triangle_mesh  # noqa: E402,F401
from ._radius import radius_search, radius_count, _index_radius_search, _index_radius_count  # noqa: E402,F401
from ._fps import downsample_point_cloud_farthest_point, _index_farthest_point_sample  # noqa: E402,F401
