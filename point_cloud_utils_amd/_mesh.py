"""closest_points_on_mesh: the reference's binding (src/closest_point_on_mesh.cpp:9-50) over the HIP linear BVH of csrc/mesh.h, and MeshIndex,
the mesh-side twin of DatasetIndex. Same arguments, error texts, dtypes and return order; the rows follow this library's deterministic contract
 instead of libigl's AABB tree. ray_mesh_intersection (f7), triangle_soup_fast_winding_number and signed_distance_to_mesh
(f8, csrc/mesh_winding.h) are queries of the same index."""
import ctypes

import numpy as np

from ._call import _FACE_KINDS, _call

_MAX_ROWS = 2 ** 27 - 16


def _face_dtype_name(f):
    from . import _is_torch
    if _is_torch(f):
        return str(f.dtype).replace("torch.", "")
    return np.asarray(f).dtype.name


def _check_scalar_v(v):
    from . import _dtype_name
    dv = _dtype_name(v)
    if dv not in ("float32", "float64"):
        raise ValueError(f"Invalid scalar type ({dv}) for argument 'v'. Expected one of ['float32', 'float64'].")
    return dv


def _check_face_dtype(f):
    from . import _is_torch
    df = _face_dtype_name(f)
    kinds = ["int32", "int64"] if _is_torch(f) else list(_FACE_KINDS)
    if df not in kinds:
        raise ValueError(f"Invalid scalar type ({df}) for argument 'f'. Expected one of {kinds}.")


def _check_rows(*counts):
    if max(counts) > _MAX_ROWS:
        raise ValueError("meshes and point clouds with more than 2^27-16 rows are not supported")


def _check_mesh(v, f, want=None):
    """Scalar types, then validate_mesh (src/common/common.h:133-147), then this package's row limit. Returns (dtype name, #v, #f)."""
    from . import _dtype_name, _shape2
    dv = _check_scalar_v(v) if want is None else _dtype_name(v)
    if want is not None and dv != want:
        raise ValueError(f"Invalid scalar type ({dv}) for argument 'v'. Expected it to match argument 'p' which is of type {want}.")
    _check_face_dtype(f)
    sv, sf = _shape2(v), _shape2(f)
    got = f"Got v.shape =({sv[0]}, {sv[1]}), f.shape = ({sf[0]}, {sf[1]})."
    if sv[0] == 0 or sf[0] == 0:
        raise ValueError("Invalid input mesh with zero elements: v and f must have shape (n, 3) and (m, 3) (n, m > 0). " + got)
    if sv[1] != 3 or sf[1] != 3:
        raise ValueError("Only 3D inputs are supported: v and f must have shape (n, 3) and (m, 3) (n, m > 0). " + got)
    _check_rows(sv[0], sf[0])
    return dv, sv[0], sf[0]


def _check_points_dtype(p, want=None):
    from . import _dtype_name, _shape2
    dp = _dtype_name(p)
    if dp not in ("float32", "float64"):
        raise ValueError(f"Invalid scalar type ({dp}) for argument 'p'. Expected one of ['float32', 'float64'].")
    if want is not None and dp != want:
        raise ValueError(f"Invalid scalar type ({dp}) for argument 'p'. Expected it to match the indexed mesh which is of type {want}.")
    return dp, _shape2(p)


def _check_points(p, want=None):
    """Scalar type, then validate_point_cloud (src/common/common.h:58-74; zero rows are allowed), then the row limit. Returns (dtype name, #p)."""
    dp, sp = _check_points_dtype(p, want)
    if sp[1] != 3:
        raise ValueError(f"Only 3D inputs are supported: v must have shape (n, 3) (n > 0). Got points.shape =({sp[0]}, {sp[1]}).")
    _check_rows(sp[0])
    return dp, sp[0]


def _host_mesh_checks(v, f):
    """What the library checks on the device for device-resident input, found on the host for host arrays (before any device work)."""
    if not bool(np.isfinite(v).all()):
        raise ValueError("v must not contain NaN or infinite coordinates")
    nv = int(v.shape[0])
    if (f.dtype.kind == "i" and int(f.min()) < 0) or int(f.max()) >= nv:
        raise ValueError(f"f must hold row indices of v: found a face index outside [0, {nv})")


def _host_point_checks(p):
    if not bool(np.isfinite(p).all()):
        raise ValueError("p must not contain NaN or infinite coordinates")


def _faces_for(d, f):
    """The face array next to the resolved point arrays of a call: same kind (torch on that device / numpy), contiguous."""
    from . import _is_torch
    if d.torch:
        if not _is_torch(f) or not f.is_cuda or f.device != d.tdev:
            raise ValueError("torch inputs must all be CUDA/HIP tensors on the same device")
        return f.contiguous()
    if _is_torch(f):
        raise ValueError("torch inputs must all be CUDA/HIP tensors on the same device")
    return np.ascontiguousarray(f)


_POINT_ORDER, _RAY_ORDER = (0, 1, 2), (1, 2, 0)     # (d, f_idx, bc) and (f_id, bc, t) out of _results' (value, face, barycentrics)


def _results(d, n):
    """What both operators write per row: one value (distance / t), one int64 face, three barycentric coordinates."""
    return d.empty((n,), "T"), d.empty((n,), "i64"), d.empty((n, 3), "T")


def _finish(val, fi, bc, like, n, order):
    """The results in the operator's return order. The face in the dtype of `like`, f's (-1 wraps for an unsigned one, as the reference's
    assignment does); singleton dimensions squeezed as the package's other calls do (numpyeigen's squeeze)."""
    from . import _is_torch
    fi = fi.to(like.dtype) if _is_torch(fi) else fi.astype(like.dtype, copy=False)
    if n == 1:
        val, fi, bc = val.reshape(()), fi.reshape(()), bc.reshape(3)
    res = (val, fi, bc)
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
    from . import _Dev, _is_torch
    dp, n = _check_points(p)
    _, nv, nf = _check_mesh(v, f, want=dp)
    if not (_is_torch(p) or _is_torch(v) or _is_torch(f)):
        _host_mesh_checks(np.asarray(v), np.asarray(f))
        _host_point_checks(np.asarray(p))
    d = _Dev(p, v)
    ff = _faces_for(d, f)
    dist, fi, bc = _results(d, n)
    _call("closest_points_on_mesh", d, d.pb, nv, _Dev.ptr(ff), nf, _FACE_KINDS[_face_dtype_name(ff)], d.pa, n, _Dev.ptr(dist), _Dev.ptr(fi), _Dev.ptr(bc))
    return _finish(dist, fi, bc, ff, n, _POINT_ORDER)


def _check_points_nonzero(p):
    """validate_point_cloud(p, allow_0=false) (src/common/common.h:58-74), then the row limit. Returns #p."""
    from . import _shape2
    sp = _shape2(p)
    if sp[0] == 0:
        raise ValueError(f"Invalid input point cloud with zero points: points must have shape (n, 3) (n > 0). Got points.shape =({sp[0]}, {sp[1]}).")
    if sp[1] != 3:
        raise ValueError(f"Only 3D inputs are supported: v must have shape (n, 3) (n > 0). Got points.shape =({sp[0]}, {sp[1]}).")
    _check_rows(sp[0])
    return sp[0]


def _check_beta(beta):
    beta = float(beta)
    if not beta > 0.0:
        raise ValueError("beta must be greater than 0 (finite, or +inf for the plain sum over all faces)")
    return beta


def _check_bounds(lower_bound, upper_bound):
    lower_bound, upper_bound = float(lower_bound), float(upper_bound)
    if lower_bound != lower_bound or upper_bound != upper_bound:
        raise ValueError("lower_bound and upper_bound must not be NaN")
    if lower_bound > upper_bound:
        raise ValueError("lower_bound must not be greater than upper_bound")
    return lower_bound, upper_bound


def _int32_like(d):
    """An empty int32 array of the kind of the call's results: signed_distance_to_mesh returns int32 faces (the reference's EigenDense<int>)."""
    if d.torch:
        import torch
        return torch.empty((0,), dtype=torch.int32)
    return np.empty((0,), dtype=np.int32)


def _scalar_rows(w, n):
    return w.reshape(()) if n == 1 else w


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
    from . import _Dev, _dtype_name, _is_torch
    dv = _check_scalar_v(v)
    _check_face_dtype(f)
    dp = _dtype_name(p)
    if dp != dv:
        raise ValueError(f"Invalid scalar type ({dp}) for argument 'p'. Expected it to match argument 'v' which is of type {dv}.")
    _, nv, nf = _check_mesh(v, f)
    n = _check_points_nonzero(p)
    beta = _check_beta(beta)
    if not (_is_torch(p) or _is_torch(v) or _is_torch(f)):
        _host_mesh_checks(np.asarray(v), np.asarray(f))
        _host_point_checks(np.asarray(p))
    d = _Dev(p, v)
    ff = _faces_for(d, f)
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
    from . import _Dev, _is_torch
    dp, _ = _check_points_dtype(p)
    _, nv, nf = _check_mesh(v, f, want=dp)
    n = _check_points_nonzero(p)
    lower_bound, upper_bound = _check_bounds(lower_bound, upper_bound)
    if not (_is_torch(p) or _is_torch(v) or _is_torch(f)):
        _host_mesh_checks(np.asarray(v), np.asarray(f))
        _host_point_checks(np.asarray(p))
    d = _Dev(p, v)
    ff = _faces_for(d, f)
    s, fi, bc = _results(d, n)
    _call("signed_distance_to_mesh", d, d.pb, nv, _Dev.ptr(ff), nf, _FACE_KINDS[_face_dtype_name(ff)], d.pa, n, lower_bound, upper_bound, 2.0,
          _Dev.ptr(s), _Dev.ptr(fi), _Dev.ptr(bc))
    return _finish(s, fi, bc, _int32_like(d), n, _POINT_ORDER)


_RAY_ROWS = ("ray_o and ray_d must have the same number of rows (one ray origin per ray direction). "
             "(Note: ray_o can have one row to use the same origin for all directions)")


def _size(a):
    n = 1
    for x in a.shape:
        n *= int(x)
    return n


def _check_rays(ray_o, ray_d, want, match):
    """Scalar types (both must be `want`; `match` names what that is), then the reference's shape checks in its order
    (src/ray_mesh_intersection.cpp:117-134). Returns (#rays, single origin?)."""
    from . import _dtype_name, _shape2
    for name, a in (("ray_o", ray_o), ("ray_d", ray_d)):
        dt = _dtype_name(a)
        if dt != want:
            raise ValueError(f"Invalid scalar type ({dt}) for argument '{name}'. Expected it to match {match} which is of type {want}.")
    so, sd = _shape2(ray_o), _shape2(ray_d)
    single = _size(ray_o) == 3
    if not single and so[0] != sd[0]:
        raise ValueError(_RAY_ROWS)
    if so[1] != 3 and not single:
        raise ValueError(f"Invalid shape for ray_o must have shape (N, 3) but got ({so[0]}, {so[1]}).")
    if sd[1] != 3:
        raise ValueError(f"Invalid shape for ray_d must have shape (N, 3) but got ({sd[0]}, {sd[1]}).")
    return sd[0], single


def _check_ray_limits(n, ray_near, ray_far):
    _check_rows(n)
    ray_near, ray_far = float(ray_near), float(ray_far)
    if ray_near != ray_near or ray_far != ray_far:
        raise ValueError("ray_near and ray_far must not be NaN")
    return ray_near, ray_far


def _host_ray_checks(ray_o, ray_d):
    if not bool(np.isfinite(ray_o).all()):
        raise ValueError("ray_o must not contain NaN or infinite coordinates")
    if not bool(np.isfinite(ray_d).all()):
        raise ValueError("ray_d must not contain NaN or infinite coordinates")


def _origins_for(d, ray_o, single):
    """ray_o next to the resolved arrays of a call (_faces_for), as (1, 3) or (n, 3). Returns (array, rows)."""
    oo = _faces_for(d, ray_o)
    if single:
        oo = oo.reshape(1, 3)
    return oo, int(oo.shape[0])


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
    from . import _Dev, _is_torch
    dv = _check_scalar_v(v)
    _check_face_dtype(f)
    n, single = _check_rays(ray_o, ray_d, dv, "argument 'v'")
    _, nv, nf = _check_mesh(v, f)
    ray_near, ray_far = _check_ray_limits(n, ray_near, ray_far)
    if not (_is_torch(v) or _is_torch(f) or _is_torch(ray_o) or _is_torch(ray_d)):
        _host_mesh_checks(np.asarray(v), np.asarray(f))
        _host_ray_checks(np.asarray(ray_o), np.asarray(ray_d))
    d = _Dev(ray_d, v)
    ff = _faces_for(d, f)
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
    from . import _is_torch
    if _is_torch(attribute):
        return (attribute[f.long()[fi.long()]] * bc[:, :, None]).sum(1)
    return (attribute[f[fi]] * bc[:, :, np.newaxis]).sum(1)


class MeshIndex:
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

    def __init__(self, v, f, winding_numbers=False):
        from . import _lib, _Dev, _fn, _is_torch
        dv, nv, nf = _check_mesh(v, f)
        if not (_is_torch(v) or _is_torch(f)):
            _host_mesh_checks(np.asarray(v), np.asarray(f))
        d = _Dev(v, v)
        ff = _faces_for(d, f)
        self._suffix, self._dtype_name, self._device = d.suffix, dv, d.device
        self._face_like = ff[:0]                    # carries f's dtype (and kind of array) for the result
        self._h = None
        self._winding = bool(winding_numbers)
        h = ctypes.c_void_p()
        rc = _fn("mesh_index_create", d.suffix)(d.ctx, d.pa, nv, _Dev.ptr(ff), nf, _FACE_KINDS[_face_dtype_name(ff)],
                                                d.flags | (_lib.MESH_MOMENTS if self._winding else 0), d.stream, ctypes.byref(h))
        if rc:
            _lib.check(rc)
        self._h = h
        self.num_faces = nf

    def closest_points(self, p):
        """See point_cloud_utils_amd.closest_points_on_mesh; the mesh is the indexed one."""
        from . import _Dev, _is_torch
        self._check_open()
        _, n = _check_points(p, want=self._dtype_name)
        if not _is_torch(p):
            _host_point_checks(np.asarray(p))
        d = _Dev(p, p)
        if d.device != self._device:
            raise ValueError("query points and mesh index live on different devices")
        dist, fi, bc = _results(d, n)
        _call("mesh_index_closest", d, self._h, d.pa, n, _Dev.ptr(dist), _Dev.ptr(fi), _Dev.ptr(bc))
        return _finish(dist, fi, bc, self._like_for(d), n, _POINT_ORDER)

    def _points(self, p, what):
        """The checks and resolved arrays of a winding_number / signed_distance call."""
        from . import _Dev, _is_torch
        self._check_open()
        if not self._winding:
            raise ValueError(f"{what} needs an index built with winding_numbers=True")
        _check_points_dtype(p, want=self._dtype_name)
        n = _check_points_nonzero(p)
        if not _is_torch(p):
            _host_point_checks(np.asarray(p))
        d = _Dev(p, p)
        if d.device != self._device:
            raise ValueError("query points and mesh index live on different devices")
        return d, n

    def winding_number(self, p, *, beta=2.0):
        """See point_cloud_utils_amd.triangle_soup_fast_winding_number; the mesh is the indexed one."""
        from . import _Dev
        beta = _check_beta(beta)
        d, n = self._points(p, "winding_number")
        w = d.empty((n,), "T")
        _call("mesh_index_winding", d, self._h, d.pa, n, beta, _Dev.ptr(w))
        return _scalar_rows(w, n)

    def signed_distance(self, p, lower_bound=-np.inf, upper_bound=np.inf):
        """See point_cloud_utils_amd.signed_distance_to_mesh; the mesh is the indexed one."""
        from . import _Dev
        lower_bound, upper_bound = _check_bounds(lower_bound, upper_bound)
        d, n = self._points(p, "signed_distance")
        s, fi, bc = _results(d, n)
        _call("mesh_index_signed_distance", d, self._h, d.pa, n, lower_bound, upper_bound, 2.0, _Dev.ptr(s), _Dev.ptr(fi), _Dev.ptr(bc))
        return _finish(s, fi, bc, _int32_like(d), n, _POINT_ORDER)

    def _check_open(self):
        if self._h is None:
            raise ValueError("the mesh index has been closed")

    def _like_for(self, d):
        """An empty array of f's dtype and of the kind (numpy / torch) of the call's results."""
        from . import _is_torch
        like = self._face_like
        if _is_torch(like) and not d.torch:          # index built from tensors, numpy queries: numpy results
            like = np.empty((0,), dtype=str(like.dtype).replace("torch.", ""))
        elif d.torch and not _is_torch(like):
            import torch
            like = torch.empty((0,), dtype=getattr(torch, like.dtype.name if like.dtype.kind == "i" else "int64"))
        return like

    def intersect_rays(self, ray_o, ray_d, ray_near=0.0, ray_far=np.inf):
        """See point_cloud_utils_amd.ray_mesh_intersection; the mesh is the indexed one and the rays must have its dtype."""
        from . import _Dev, _is_torch
        self._check_open()
        n, single = _check_rays(ray_o, ray_d, self._dtype_name, "the indexed mesh")
        ray_near, ray_far = _check_ray_limits(n, ray_near, ray_far)
        if not (_is_torch(ray_o) or _is_torch(ray_d)):
            _host_ray_checks(np.asarray(ray_o), np.asarray(ray_d))
        d = _Dev(ray_d, ray_d)
        if d.device != self._device:
            raise ValueError("rays and mesh index live on different devices")
        oo, o_rows = _origins_for(d, ray_o, single)
        t, fi, bc = _results(d, n)
        _call("mesh_index_rays", d, self._h, _Dev.ptr(oo), o_rows, d.pa, n, ray_near, ray_far, _Dev.ptr(fi), _Dev.ptr(bc), _Dev.ptr(t))
        return _finish(t, fi, bc, self._like_for(d), n, _RAY_ORDER)

    def close(self):
        if getattr(self, "_h", None) is not None:
            from . import _lib
            _lib.lib().pcu_hip_mesh_index_destroy(self._h)
            self._h = None

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()
        return False

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


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
        from . import _dtype_name, _is_torch
        do = _dtype_name(ray_o)
        if do not in ("float32", "float64"):
            raise ValueError(f"Invalid scalar type ({do}) for argument 'ray_o'. Expected one of ['float32', 'float64'].")
        dd = _dtype_name(ray_d)
        if dd != do:
            raise ValueError(f"Invalid scalar type ({dd}) for argument 'ray_d'. Expected it to match argument 'ray_o' which is of type {do}.")
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
