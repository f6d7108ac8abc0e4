"""point_cloud_utils_amd -- MI355X (gfx950) drop-in for point-cloud-utils' KNN / Chamfer / Hausdorff hot path.

Its first four callables (_search.py) have the signatures, defaults, dtypes, shapes and error behaviour of the reference's
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
from . import _lib
from ._lib import Stats, set_cell_occupancy, device_count  # noqa: F401
from ._call import (_DT_FAST, _ENV_FLAGS, _FN, _TIMING, _Dev, _Handle, _dtype_name, _flags, _fn, _is_torch,  # noqa: F401
                    _last_stats, _record, _shape2)
from ._search import k_nearest_neighbors, one_sided_hausdorff_distance, hausdorff_distance, chamfer_distance, DatasetIndex  # noqa: F401
from ._normals import estimate_point_cloud_normals_knn, estimate_point_cloud_normals_ball  # noqa: F401
from ._voxel import (morton_encode, morton_decode, morton_add, morton_subtract, morton_knn,  # noqa: F401
                     downsample_point_cloud_on_voxel_grid, deduplicate_point_cloud)
from ._sinkhorn import pairwise_distances, sinkhorn, earth_movers_distance  # noqa: F401
from ._poisson import downsample_point_cloud_poisson_disk  # noqa: F401
from ._mesh import (closest_points_on_mesh, MeshIndex, ray_mesh_intersection, RayMeshIntersector,  # noqa: F401
                    interpolate_barycentric_coords, triangle_soup_fast_winding_number, signed_distance_to_mesh)
from ._mesh_sample import mesh_face_areas, sample_mesh_random, sample_mesh_poisson_disk  # noqa: F401
from ._pc_winding import point_cloud_fast_winding_number, PointCloudWindingIndex, estimate_mesh_face_normals  # noqa: F401
from ._surfel import ray_surfel_intersection, RaySurfelIntersector, pointcloud_surfel_geometry  # noqa: F401
from ._voxelize import voxelize_triangle_mesh, sparse_voxel_grid_boundary, voxel_grid_geometry  # noqa: F401
from ._components import connected_components, flood_fill_3d  # noqa: F401
from ._marching_cubes import marching_cubes_sparse_voxel_grid, sparse_voxel_grid_to_hex_mesh  # noqa: F401
from ._mesh_smooth import adjacency_list, mesh_vertex_adjacency, estimate_mesh_vertex_normals, laplacian_smooth_mesh  # noqa: F401
from ._mesh_repair import remove_mesh_vertices, remove_unreferenced_mesh_vertices, deduplicate_mesh_vertices, orient_mesh_faces  # noqa: F401
from ._mesh_decimate import decimate_triangle_mesh  # noqa: F401
from ._radius import radius_search, radius_count  # noqa: F401
from ._fps import downsample_point_cloud_farthest_point  # noqa: F401
from ._dbscan import cluster_point_cloud_dbscan  # noqa: F401
from ._icp import register_point_clouds_icp, IcpResult  # noqa: F401
from ._plane import segment_point_cloud_plane, PlaneResult  # noqa: F401
from ._orient import orient_point_cloud_normals  # noqa: F401
from ._fpfh import compute_point_cloud_fpfh  # noqa: F401
from ._feature_match import match_point_features  # noqa: F401
from ._ransac import register_point_clouds_ransac, RansacRegistrationResult  # noqa: F401

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
           "radius_search", "radius_count", "downsample_point_cloud_farthest_point", "cluster_point_cloud_dbscan",
           "register_point_clouds_icp", "IcpResult", "segment_point_cloud_plane", "PlaneResult",
           "orient_point_cloud_normals", "compute_point_cloud_fpfh", "match_point_features",
           "register_point_clouds_ransac", "RansacRegistrationResult",
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
