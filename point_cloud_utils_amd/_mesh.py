"""closest_points_on_mesh: the reference's binding (src/closest_point_on_mesh.cpp:9-50) over the HIP linear BVH of csrc/mesh.h, and MeshIndex,
the mesh-side twin of DatasetIndex. Same arguments, error texts, dtypes and return order; the rows follow this library's deterministic contract
 instead of libigl's AABB tree. ray_mesh_intersection (f7), triangle_soup_fast_winding_number and signed_distance_to_mesh
(f8, csrc/mesh_winding.h) are queries of the same index."""
import numpy as np

from . import _lib
from ._call import _FACE_KINDS, _Dev, _Handle, _call, _int_out, _is_torch
from ._checks import (_beside, _check_beta, _check_bounds, _check_face_dtype, _check_float, _check_mesh, _check_points, _check_points_dtype,
                      _check_points_nonzero, _check_ray_limits, _check_rays, _face_dtype_name, _face_rows, _host_finite, _host_mesh_checks,
                      _host_ray_checks, _match, _origins_for, _scalar_rows)

_POINT_ORDER, _RAY_ORDER = (0, 1, 2), (1, 2, 0)     # (d, f_idx, bc) and (f_id, bc, t) out of _results' (value, face, barycentrics)


def _results(d, n):
    """What both operators write per row: one value (distance / t), one int64 face, three barycentric coordinates."""
    return d.empty((n,), "T"), d.empty((n,), "i64"), d.empty((n, 3), "T")


def _finish(val, fi, bc, like, n, order):
    """The results in the operator's return order: the face and the barycentrics as _face_rows gives them, the value squeezed with them."""
    res = (_scalar_rows(val, n),) + _face_rows(fi, bc, like, n)
    return tuple(res[i] for i in order)


def closest_points_on_mesh(p, v, f):
    """
    Compute distances from a set of points p to a triangle mesh (v, f)

    Args:
      p : (#p, 3)-shaped array of query point positions (float32 or float64; numpy, or a CUDA/HIP torch tensor)
      v : (#v, 3)-shaped array of mesh vertex positions (same dtype as p)
      f : (#f, 3)-shaped array of triangle face indices (int32, int64, uint32 or uint64; int32 / int64 for torch)

    Returns:
      d : a (#p,)-shaped array of shortest distances for each query point p
      f_idx : a (#p,)-shaped array of indices into f of the face containing the closest point to each query point (f's dtype)
      bc : a (#p, 3)-shaped array of barycentric coordinates for each query point

    Notes:
      This only computes distances to given primitives, so unreferenced vertices are ignored. Degenerate primitives are handled correctly: triangle
      [1 2 2] is treated as a segment [1 2], and triangle [1 1 1] is treated as a point.
      Every face is evaluated by one closest-point function in the input dtype; among faces of exactly equal distance the lowest face index is
      returned, with that face's barycentric coordinates (u = (1 - v) - w may undershoot 0 by one rounding). Non-finite coordinates, face indices
      outside [0, #v) and arrays of more than 2**27 - 16 rows raise ValueError.
    """
    dp, n = _check_points(p)
    _, nv, nf = _check_mesh(v, f, want=dp)
    if not (_is_torch(p) or _is_torch(v) or _is_torch(f)):
        _host_mesh_checks(np.asarray(v), np.asarray(f))
        _host_finite(p=np.asarray(p))
    d = _Dev(p, v)
    ff = _beside(d, f)
    dist, fi, bc = _results(d, n)
    _call("closest_points_on_mesh", d, d.pb, nv, _Dev.ptr(ff), nf, _FACE_KINDS[_face_dtype_name(ff)], d.pa, n, _Dev.ptr(dist), _Dev.ptr(fi), _Dev.ptr(bc))
    return _finish(dist, fi, bc, ff, n, _POINT_ORDER)


def triangle_soup_fast_winding_number(v, f, p, *, beta=2.0):
    """
    Compute a consistent inside/outside field given a triangle soup and evaluate that field at a set of query points

    Args:
      v : (#v, 3)-shaped array of mesh vertex positions (float32 or float64; numpy, or a CUDA/HIP torch tensor)
      f : (#f, 3)-shaped array of mesh face indexes into v (int32, int64, uint32 or uint64; int32 / int64 for torch)
      p : (#p, 3)-shaped array of query positions at which to evaluate the winding number field (v's dtype)
      beta : accuracy of the fast evaluation (not in the reference API, which uses libigl's default 2): a tree node farther from the query
             than beta times its radius is replaced by a three-term expansion; float('inf') gives the plain sum over all faces

    Returns:
      A (#p,)-shaped array with the generalized winding number of each query point: about 1 inside a closed, outward-oriented mesh and
      about 0 outside.

    Notes:
      The fast winding number of Barill et al. (2018) with the tree, moments and evaluation order stated in DESIGN.md (f8): finite for every
      finite query, equal bits for equal arguments. Non-finite coordinates, face indices outside [0, #v) and arrays of more than 2**27 - 16
      rows raise ValueError.
    """
    dv = _check_float(v, "v")
    _check_face_dtype(f)
    _match(p, "p", dv, "argument 'v'")
    _, nv, nf = _check_mesh(v, f)
    n = _check_points_nonzero(p)
    beta = _check_beta(beta, "faces")
    if not (_is_torch(p) or _is_torch(v) or _is_torch(f)):
        _host_mesh_checks(np.asarray(v), np.asarray(f))
        _host_finite(p=np.asarray(p))
    d = _Dev(p, v)
    ff = _beside(d, f)
    w = d.empty((n,), "T")
    _call("triangle_soup_fast_winding_number", d, d.pb, nv, _Dev.ptr(ff), nf, _FACE_KINDS[_face_dtype_name(ff)], d.pa, n, beta, _Dev.ptr(w))
    return _scalar_rows(w, n)


def signed_distance_to_mesh(p, v, f, lower_bound=-np.inf, upper_bound=np.inf):
    """
    Computes signed distances of a point cloud with respect to a Mesh using Fast Winding Numbers

    Args:
      p : (#p, 3)-shaped array point cloud (one 3D point per row; float32 or float64; numpy, or a CUDA/HIP torch tensor)
      v : (#v, 3)-shaped array of mesh vertex positions (one vertex position per row; p's dtype)
      f : (#f, 3)-shaped array of mesh face indexes into v (int32, int64, uint32 or uint64; int32 / int64 for torch)
      lower_bound : The minimum distance value possible (use this to clamp SDF values). negative infinite by default
      upper_bound : The maximum distance value possible (use this to clamp SDF values). infinite by default

    Returns:
      s : a (#p,) shaped array of signed distance values for each query point in p
      fi : a (#p,) shaped int32 array of indices to the closest face for each query point in p
      bc : a (#p, 3) shaped array of barycentric coordinates for the closest point on the mesh to each query point in p

    Notes:
      |s|, fi and bc are the rows of closest_points_on_mesh(p, v, f) bit for bit; s is negative where the fast winding number (beta = 2) is
      above 1/2 in absolute value; then s is clamped to [lower_bound, upper_bound] (both rounded to float32 first, as the reference's
      arguments are). A NaN bound or lower_bound > upper_bound raises ValueError.
    """
    dp, _ = _check_points_dtype(p)
    _, nv, nf = _check_mesh(v, f, want=dp)
    n = _check_points_nonzero(p)
    lower_bound, upper_bound = _check_bounds(lower_bound, upper_bound)
    if not (_is_torch(p) or _is_torch(v) or _is_torch(f)):
        _host_mesh_checks(np.asarray(v), np.asarray(f))
        _host_finite(p=np.asarray(p))
    d = _Dev(p, v)
    ff = _beside(d, f)
    s, fi, bc = _results(d, n)
    _call("signed_distance_to_mesh", d, d.pb, nv, _Dev.ptr(ff), nf, _FACE_KINDS[_face_dtype_name(ff)], d.pa, n, lower_bound, upper_bound, 2.0,
          _Dev.ptr(s), _Dev.ptr(fi), _Dev.ptr(bc))
    return _finish(s, fi, bc, _int_out(d, (0,), np.int32), n, _POINT_ORDER)


def ray_mesh_intersection(v, f, ray_o, ray_d, ray_near=0.0, ray_far=np.inf):
    """
    Compute intersection between a set of rays and a triangle mesh

    Args:
      v : (#v, 3)-shaped array of mesh vertex positions (float32 or float64; numpy, or a CUDA/HIP torch tensor)
      f : (#f, 3)-shaped array of triangle face indices (int32, int64, uint32 or uint64; int32 / int64 for torch)
      ray_o : array of shape (#rays, 3) of ray origins (one per row) or an array of three elements, (3,) or (1, 3), used for all rays (v's dtype)
      ray_d : array of shape (#rays, 3) of ray directions (one per row; v's dtype; not normalised: t is in units of the direction's length)
      ray_near : an optional floating point value indicating the distance along each ray to start searching (default 0.0)
      ray_far : an optional floating point value indicating the maximum distance along each ray to search (default inf)

    Returns:
      f_id : an array of shape (#rays,) representing the face id hit by each ray (f's dtype; -1 for a miss)
      bc : an array of shape (#rays, 3) where each row is the barycentric coordinates within each face of the ray intersection (0 for a miss)
      t : the distance along each ray to the intersection (inf for a miss)

    Notes:
      Every face is tested by one watertight ray / triangle test (Woop, Benthin, Wald 2013) in the input dtype: a ray through an edge or a vertex
      shared by faces hits one of them. The nearest crossing with ray_near <= t <= ray_far is returned, among faces of exactly equal t the
      lowest face index. A zero direction, a face of no area and a face seen exactly edge-on are misses; ray_near > ray_far gives all misses.
      Non-finite coordinates, NaN ray_near / ray_far, face indices outside [0, #v) and arrays of more than 2**27 - 16 rows raise ValueError.
    """
    dv = _check_float(v, "v")
    _check_face_dtype(f)
    n, single = _check_rays(ray_o, ray_d, dv, "argument 'v'")
    _, nv, nf = _check_mesh(v, f)
    ray_near, ray_far = _check_ray_limits(n, ray_near, ray_far)
    if not (_is_torch(v) or _is_torch(f) or _is_torch(ray_o) or _is_torch(ray_d)):
        _host_mesh_checks(np.asarray(v), np.asarray(f))
        _host_ray_checks(np.asarray(ray_o), np.asarray(ray_d))
    d = _Dev(ray_d, v)
    ff = _beside(d, f)
    oo, o_rows = _origins_for(d, ray_o, single)
    t, fi, bc = _results(d, n)
    _call("ray_mesh_intersection", d, d.pb, nv, _Dev.ptr(ff), nf, _FACE_KINDS[_face_dtype_name(ff)], _Dev.ptr(oo), o_rows, d.pa, n, ray_near, ray_far,
          _Dev.ptr(fi), _Dev.ptr(bc), _Dev.ptr(t))
    return _finish(t, fi, bc, ff, n, _RAY_ORDER)


def interpolate_barycentric_coords(f, fi, bc, attribute):
    """
    Interpolate an attribute stored at each vertex of a mesh across the faces of a triangle mesh using barycentric coordinates

    Args:
      f : a (#faces, 3)-shaped array of mesh faces (indexing into some vertex array)
      fi : a (#attribs,)-shaped array of indexes into f indicating which face each attribute lies within
      bc : a (#attribs, 3)-shaped array of barycentric coordinates for each attribute
      attribute : a (#vertices, dim)-shaped array of attributes at each of the mesh vertices

    Returns:
      A (#attribs, dim)-shaped array of interpolated attributes (numpy arrays or torch tensors, as given).
    """
    if _is_torch(attribute):
        return (attribute[f.long()[fi.long()]] * bc[:, :, None]).sum(1)
    return (attribute[f[fi]] * bc[:, :, np.newaxis]).sum(1)


class MeshIndex(_Handle):
    """A triangle mesh kept on the GPU as its search index (not in the reference API, which rebuilds libigl's AABB tree on every call): build
    once, query many times.

        with pcu.MeshIndex(v, f) as mesh:
            d, fi, bc = mesh.closest_points(p)          # same rows as pcu.closest_points_on_mesh(p, v, f)
        with pcu.MeshIndex(v, f, winding_numbers=True) as mesh:
            w = mesh.winding_number(p)                  # same rows as pcu.triangle_soup_fast_winding_number(v, f, p)
            s, fi, bc = mesh.signed_distance(p)         # same rows as pcu.signed_distance_to_mesh(p, v, f)

    `v`: (#v, 3) float32 / float64, `f`: (#f, 3) integer faces; numpy or CUDA/HIP torch tensors (copied; the caller's arrays can go away).
    Queries must have the mesh's dtype. `winding_numbers=True` also builds what winding_number() and signed_distance() need (about 17 more
    scalars per face). The index lives on one GPU; call close() (or use `with`) to free it."""
    _noun, _destroy = "mesh index", "pcu_hip_mesh_index_destroy"

    def __init__(self, v, f, winding_numbers=False):
        dv, nv, nf = _check_mesh(v, f)
        if not (_is_torch(v) or _is_torch(f)):
            _host_mesh_checks(np.asarray(v), np.asarray(f))
        d = _Dev(v, v)
        ff = _beside(d, f)
        self._suffix, self._dtype_name = d.suffix, dv
        self._face_like = ff[:0]                    # carries f's dtype (and kind of array) for the result
        self._winding = bool(winding_numbers)
        self._open("mesh_index_create", d, d.pa, nv, _Dev.ptr(ff), nf, _FACE_KINDS[_face_dtype_name(ff)],
                   flags=d.flags | (_lib.MESH_MOMENTS if self._winding else 0))
        self.num_faces = nf

    def closest_points(self, p):
        """See point_cloud_utils_amd.closest_points_on_mesh; the mesh is the indexed one."""
        self._check_open()
        _, n = _check_points(p, want=self._dtype_name)
        if not _is_torch(p):
            _host_finite(p=np.asarray(p))
        d = _Dev(p, p)
        self._same_device(d, "query points")
        dist, fi, bc = _results(d, n)
        _call("mesh_index_closest", d, self._h, d.pa, n, _Dev.ptr(dist), _Dev.ptr(fi), _Dev.ptr(bc))
        return _finish(dist, fi, bc, self._like_for(d), n, _POINT_ORDER)

    def _points(self, p, what):
        """The checks and resolved arrays of a winding_number / signed_distance call."""
        self._check_open()
        if not self._winding:
            raise ValueError(f"{what} needs an index built with winding_numbers=True")
        _check_points_dtype(p, want=self._dtype_name)
        n = _check_points_nonzero(p)
        if not _is_torch(p):
            _host_finite(p=np.asarray(p))
        d = _Dev(p, p)
        self._same_device(d, "query points")
        return d, n

    def winding_number(self, p, *, beta=2.0):
        """See point_cloud_utils_amd.triangle_soup_fast_winding_number; the mesh is the indexed one."""
        beta = _check_beta(beta, "faces")
        d, n = self._points(p, "winding_number")
        w = d.empty((n,), "T")
        _call("mesh_index_winding", d, self._h, d.pa, n, beta, _Dev.ptr(w))
        return _scalar_rows(w, n)

    def signed_distance(self, p, lower_bound=-np.inf, upper_bound=np.inf):
        """See point_cloud_utils_amd.signed_distance_to_mesh; the mesh is the indexed one."""
        lower_bound, upper_bound = _check_bounds(lower_bound, upper_bound)
        d, n = self._points(p, "signed_distance")
        s, fi, bc = _results(d, n)
        _call("mesh_index_signed_distance", d, self._h, d.pa, n, lower_bound, upper_bound, 2.0, _Dev.ptr(s), _Dev.ptr(fi), _Dev.ptr(bc))
        return _finish(s, fi, bc, _int_out(d, (0,), np.int32), n, _POINT_ORDER)

    def _like_for(self, d):
        """An empty array of f's dtype and of the kind (numpy / torch) of the call's results."""
        like = self._face_like
        if _is_torch(like) and not d.torch:          # index built from tensors, numpy queries: numpy results
            like = np.empty((0,), dtype=str(like.dtype).replace("torch.", ""))
        elif d.torch and not _is_torch(like):
            import torch
            like = torch.empty((0,), dtype=getattr(torch, like.dtype.name if like.dtype.kind == "i" else "int64"))
        return like

    def intersect_rays(self, ray_o, ray_d, ray_near=0.0, ray_far=np.inf):
        """See point_cloud_utils_amd.ray_mesh_intersection; the mesh is the indexed one and the rays must have its dtype."""
        self._check_open()
        n, single = _check_rays(ray_o, ray_d, self._dtype_name, "the indexed mesh")
        ray_near, ray_far = _check_ray_limits(n, ray_near, ray_far)
        if not (_is_torch(ray_o) or _is_torch(ray_d)):
            _host_ray_checks(np.asarray(ray_o), np.asarray(ray_d))
        d = _Dev(ray_d, ray_d)
        self._same_device(d, "rays")
        oo, o_rows = _origins_for(d, ray_o, single)
        t, fi, bc = _results(d, n)
        _call("mesh_index_rays", d, self._h, _Dev.ptr(oo), o_rows, d.pa, n, ray_near, ray_far, _Dev.ptr(fi), _Dev.ptr(bc), _Dev.ptr(t))
        return _finish(t, fi, bc, self._like_for(d), n, _RAY_ORDER)


class RayMeshIntersector:
    """
    Class used to find the intersection between rays and a triangle mesh (the reference's point_cloud_utils.RayMeshIntersector): the mesh is
    indexed once (a MeshIndex) and queried many times. f_id comes back as int32 and bc, t in ray_o's dtype, as in the reference; rays of the
    other float dtype are converted to the mesh's. close() (or `with`) frees the index.
    """
    def __init__(self, mesh_v, mesh_f):
        """
        Create a RayMeshIntersector object which can be used to do ray/mesh queries with a triangle mesh.

        Args:
          mesh_v : #v by 3 array of vertex positions (each row is a vertex)
          mesh_f : #f by 3 Matrix of face (triangle) indices
        """
        self.v = mesh_v
        self.f = mesh_f
        self._index = MeshIndex(mesh_v, mesh_f)

    def intersect_rays(self, ray_o, ray_d, ray_near=0.0, ray_far=np.inf):
        """
        Compute intersection between a set of rays and the triangle mesh enclosed in this class

        Args:
          ray_o : array of shape (#rays, 3) of ray origins (one per row) or a single array of shape (3,) to use
          ray_d : array of shape (#rays, 3) of ray directions (one per row)
          ray_near : an optional floating point value indicating the distance along each ray to start searching (default 0.0)
          ray_far : an optional floating point value indicating the maximum distance along each ray to search (default inf)

        Returns:
          f_id : an array of shape (#rays,) representing the face id hit by each ray
          bc : an array of shape (#rays, 3) where each row is the barycentric coordinates within each face of the ray intersection
          t : the distance along each ray to the intersection
        """
        do = _check_float(ray_o, "ray_o")
        _match(ray_d, "ray_d", do, "argument 'ray_o'")
        want = self._index._dtype_name
        if do != want:
            conv = (lambda a: a.to(getattr(__import__("torch"), want))) if _is_torch(ray_o) else (lambda a: np.asarray(a).astype(want))
            fi, bc, t = self._index.intersect_rays(conv(ray_o), conv(ray_d), ray_near, ray_far)
            back = (lambda a: a.to(ray_o.dtype)) if _is_torch(ray_o) else (lambda a: a.astype(do))
            bc, t = back(bc), back(t)
        else:
            fi, bc, t = self._index.intersect_rays(ray_o, ray_d, ray_near, ray_far)
        if _is_torch(fi):
            import torch
            return fi.to(torch.int32), bc, t
        return fi.astype(np.int32), bc, t

    def close(self):
        self._index.close()

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()
        return False
