"""ray_surfel_intersection, RaySurfelIntersector and pointcloud_surfel_geometry: the reference's callables
(point_cloud_utils/_ray_point_cloud_intersector.py, _point_cloud_geometry.py over src/ray_point_cloud_intersection.cpp) over the HIP kernels of
csrc/surfel.h. Same arguments, defaults, dtypes and result order; the values follow this library's deterministic contract (DESIGN.md, row
f11): the ray contract of ray_mesh_intersection (f7) applied to a stated fan geometry, bit for bit, instead of Embree's float32."""
import numpy as np

from ._call import _Dev, _Handle, _call, _int_out, _is_torch
from ._checks import (_SAME_DEVICE, _beside, _check_normals, _check_ray_limits, _check_rays, _check_rows, _host_finite, _host_ray_checks,
                      _origins_for, _scalar_rows)

_INT32_MAX = 2 ** 31 - 1


def _check_subdivs(subdivs):
    subdivs = int(subdivs)
    if subdivs < 4:
        raise ValueError("Invalid geometry_subdivisions_1 is less than or equal to 4.")        # (the reference's text)
    if subdivs > _INT32_MAX:
        raise ValueError("subdivs does not fit an int32")
    return subdivs


def _check_surfels(p, n):
    """Scalar types, then validate_point_cloud_normals (src/common/common.h:78-110; zero points are allowed, as in the reference) and the
    row limit. Returns (dtype name, #p)."""
    dp, np_ = _check_normals(p, n, True)
    _check_rows(np_)
    return dp, np_


def _radii(p, r, np_):
    """_validate_point_radius_internal (point_cloud_utils/_point_cloud_geometry.py:24-42) for numpy and torch: a scalar, a list or tuple, or
    an array of shape (N,) or (N, 1), in p's dtype and of p's kind (a tensor on p's device for a tensor p)."""
    if _is_torch(p):
        import torch
        if not _is_torch(r):
            if isinstance(r, np.ndarray):
                raise ValueError(_SAME_DEVICE)
            if np.isscalar(r):
                r = torch.full((np_,), float(r), dtype=p.dtype, device=p.device)
            elif isinstance(r, (list, tuple)):
                r = torch.tensor(r, dtype=p.dtype, device=p.device)
            else:
                raise ValueError("Argument r must be a scalar or numpy array with the same number of rows as p")
    elif _is_torch(r):
        raise ValueError(_SAME_DEVICE)
    elif not isinstance(r, np.ndarray):
        if np.isscalar(r):
            r = r * np.ones(np_)
        elif isinstance(r, (list, tuple)):
            r = np.array(r).astype(np.asarray(p).dtype)
        else:
            raise ValueError("Argument r must be a scalar or numpy array with the same number of rows as p")
    sh = tuple(int(x) for x in r.shape)
    if len(sh) == 0 or sh[0] != np_:
        raise ValueError("Argument r have the same number of rows as p")
    if len(sh) > 2 or (len(sh) == 2 and sh[1] != 1):
        raise ValueError("Invalid shape for argument r, must have shape (N,) or (N, 1)")
    r = r.reshape(-1)
    return r.to(p.dtype) if _is_torch(r) else r.astype(np.asarray(p).dtype, copy=False)


def _resolve_surfels(p, n, r, np_, rays=()):
    """The cloud's arrays resolved for a call (_Dev over p and n), and r next to them. What the library checks on the device for
    device-resident input is found on the host for host arrays (before any device work), the call's rays included."""
    rr = _radii(p, r, np_)
    if not any(_is_torch(x) for x in (p, n) + tuple(rays)):
        _host_finite(p=np.asarray(p), n=np.asarray(n))
        if not bool(np.isfinite(rr).all()):
            raise ValueError("r must not contain NaN or infinite values")
        if rays:
            _host_ray_checks(*(np.asarray(x) for x in rays))
    d = _Dev(p, n)
    return d, _beside(d, rr)


def _pid32(pid):
    if _is_torch(pid):
        import torch
        return pid.to(torch.int32)
    return pid.astype(np.int32)


def ray_surfel_intersection(p, n, ray_o, ray_d, r=0.1, subdivs=4, ray_near=0.0, ray_far=np.inf):
    """
    Compute intersection between a set of rays and a point cloud converted to surfels (i.e. circular patches oriented
    with the point normals)

    Args:
      p : (#p, 3)-shaped array of point positions (float32 or float64; numpy, or a CUDA/HIP torch tensor)
      n : (#p, 3)-shaped array of point normals (p's dtype; need not have unit length)
      ray_o : array of shape (#rays, 3) of ray origins (one per row) or an array of three elements, used for all rays (p's dtype)
      ray_d : array of shape (#rays, 3) of ray directions (one per row; p's dtype; not normalised: t is in units of the direction's length)
      r : Array or Scalar describing the size of each geometry element (either one radius per point, or a global size for the whole cloud)
      subdivs : Number of triangles per surfel (at least 4)
      ray_near : an optional floating point value indicating the distance along each ray to start searching (default 0.0)
      ray_far : an optional floating point value indicating the maximum distance along each ray to search (default inf)

    Returns:
      pid : a (#rays,) shaped int32 array of indices corresponding to which points were hit (-1 for a ray miss)
      t : a (#rays,) shaped array encoding the distance between the ray origin and intersection point for each ray (inf for missed rays)

    Notes:
      (pid, t) is (f_id // subdivs, t) of ray_mesh_intersection on pointcloud_surfel_geometry(p, n, r, subdivs), bit for bit, without that
      mesh being built: a surfel is a regular subdivs-gon inscribed in the disc of radius |r|. Among surfels of exactly equal t the lowest
      pid wins. A point with a zero normal or a zero radius is never hit. Non-finite values, NaN ray_near / ray_far, subdivs < 4 and arrays
      of more than 2**27 - 16 rows raise ValueError; zero points (every ray misses) and zero rays are allowed.
    """
    dp, np_ = _check_surfels(p, n)
    nr, single = _check_rays(ray_o, ray_d, dp, "argument 'p'")
    subdivs = _check_subdivs(subdivs)
    ray_near, ray_far = _check_ray_limits(nr, ray_near, ray_far)
    d, rr = _resolve_surfels(p, n, r, np_, rays=(ray_o, ray_d))
    dd = _beside(d, ray_d)
    oo, o_rows = _origins_for(d, ray_o, single)
    pid, t = d.empty((nr,), "i64"), d.empty((nr,), "T")
    _call("surfel_rays", d, d.pa, d.pb, _Dev.ptr(rr), np_, subdivs, _Dev.ptr(oo), o_rows, _Dev.ptr(dd), nr, ray_near, ray_far, _Dev.ptr(pid), _Dev.ptr(t))
    return _scalar_rows(_pid32(pid), nr), _scalar_rows(t, nr)


def pointcloud_surfel_geometry(p, n, r=0.1, subdivs=7):
    """
    Generate geometry for a point cloud encoded as surfels (i.e. circular patches centered at each point and oriented
    perpendicularly to each normal)

    Args:
      p : (#p, 3)-shaped array of point positions (float32 or float64; numpy, or a CUDA/HIP torch tensor)
      n : (#p, 3)-shaped array of point normals (p's dtype; need not have unit length)
      r : Array or Scalar describing the size of each geometry element (either one radius per point, or a global size for the whole cloud)
      subdivs : Number of triangles per surfel (at least 4)

    Returns:
      verts : an array of shape (#p * (subdivs + 1), 3), in p's dtype: per point its subdivs rim vertices, then its centre
      faces : an int32 array of shape (#p * subdivs, 3) indexing into verts: face j of a point is (centre, rim j, rim (j + 1) % subdivs)

    Notes:
      The vertices follow the contract of DESIGN.md (f11), not the reference's float32 angles: they are the geometry ray_surfel_intersection
      traces. A zero normal gives a fan collapsed onto its centre. Non-finite values, subdivs < 4, more than 2**27 - 16 points and more than
      2**31 - 1 vertices raise ValueError.
    """
    _, np_ = _check_surfels(p, n)
    subdivs = _check_subdivs(subdivs)
    if np_ * (subdivs + 1) > _INT32_MAX:
        raise ValueError("surfel geometry with more than 2^31-1 vertices does not fit the int32 faces")
    d, rr = _resolve_surfels(p, n, r, np_)
    v = d.empty((np_ * (subdivs + 1), 3), "T")
    f = _int_out(d, (np_ * subdivs, 3), np.int32)
    _call("surfel_geometry", d, d.pa, d.pb, _Dev.ptr(rr), np_, subdivs, _Dev.ptr(v), _Dev.ptr(f))
    return v, f


class RaySurfelIntersector(_Handle):
    """
    Class used to find the intersection between rays and a point cloud converted to surfels (the reference's
    point_cloud_utils.RaySurfelIntersector): the cloud is indexed once and queried many times.

        with pcu.RaySurfelIntersector(p, n, r=0.05, subdivs=7) as cloud:
            pid, t = cloud.intersect_rays(ray_o, ray_d)      # same rows as pcu.ray_surfel_intersection(p, n, ray_o, ray_d, 0.05, 7)

    The index holds 9 scalars per point (a copy: the caller's arrays can go away) and lives on one GPU; close() (or `with`) frees it.
    """
    _noun, _destroy = "surfel index", "pcu_hip_surfel_index_destroy"

    def __init__(self, p, n, r=0.1, subdivs=7):
        """
        Args:
          p : (#p, 3)-shaped array of point positions (float32 or float64; numpy, or a CUDA/HIP torch tensor)
          n : (#p, 3)-shaped array of point normals (p's dtype)
          r : Array or Scalar describing the size of each geometry element
          subdivs : Number of triangles per surfel (at least 4)
        """
        dp, np_ = _check_surfels(p, n)
        subdivs = _check_subdivs(subdivs)
        d, rr = _resolve_surfels(p, n, r, np_)
        self.p, self.n, self.r, self.num_subdivs = p, n, rr, subdivs
        self._dtype_name = dp
        self._open("surfel_index_create", d, d.pa, d.pb, _Dev.ptr(rr), np_, subdivs)
        self.num_points = np_

    def intersect_rays(self, ray_o, ray_d, ray_near=0.0, ray_far=np.inf):
        """See point_cloud_utils_amd.ray_surfel_intersection; the cloud is the indexed one and the rays must have its dtype."""
        self._check_open()
        nr, single = _check_rays(ray_o, ray_d, self._dtype_name, "the indexed point cloud")
        ray_near, ray_far = _check_ray_limits(nr, ray_near, ray_far)
        if not (_is_torch(ray_o) or _is_torch(ray_d)):
            _host_ray_checks(np.asarray(ray_o), np.asarray(ray_d))
        d = _Dev(ray_d, ray_d)
        self._same_device(d, "rays")
        oo, o_rows = _origins_for(d, ray_o, single)
        pid, t = d.empty((nr,), "i64"), d.empty((nr,), "T")
        _call("surfel_index_rays", d, self._h, _Dev.ptr(oo), o_rows, d.pa, nr, ray_near, ray_far, _Dev.ptr(pid), _Dev.ptr(t))
        return _scalar_rows(_pid32(pid), nr), _scalar_rows(t, nr)
