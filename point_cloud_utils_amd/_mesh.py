"""closest_points_on_mesh: the reference's binding (src/closest_point_on_mesh.cpp:9-50) over the HIP linear BVH of csrc/mesh.h, and MeshIndex,
the mesh-side twin of DatasetIndex. Same arguments, error texts, dtypes and return order; the rows follow this library's deterministic contract
 instead of libigl's AABB tree."""
import ctypes

import numpy as np

_MAX_ROWS = 2 ** 27 - 16
_FACE_KINDS = {"int32": 0, "int64": 1, "uint32": 2, "uint64": 3}


def _face_dtype_name(f):
    from . import _is_torch
    if _is_torch(f):
        return str(f.dtype).replace("torch.", "")
    return np.asarray(f).dtype.name


def _check_mesh(v, f, want=None):
    """Scalar types, then validate_mesh (src/common/common.h:133-147), then this package's row limit. Returns (dtype name, #v, #f)."""
    from . import _dtype_name, _is_torch, _shape2
    dv = _dtype_name(v)
    if want is None and dv not in ("float32", "float64"):
        raise ValueError(f"Invalid scalar type ({dv}) for argument 'v'. Expected one of ['float32', 'float64'].")
    if want is not None and dv != want:
        raise ValueError(f"Invalid scalar type ({dv}) for argument 'v'. Expected it to match argument 'p' which is of type {want}.")
    df = _face_dtype_name(f)
    kinds = ["int32", "int64"] if _is_torch(f) else list(_FACE_KINDS)
    if df not in kinds:
        raise ValueError(f"Invalid scalar type ({df}) for argument 'f'. Expected one of {kinds}.")
    sv, sf = _shape2(v), _shape2(f)
    got = f"Got v.shape =({sv[0]}, {sv[1]}), f.shape = ({sf[0]}, {sf[1]})."
    if sv[0] == 0 or sf[0] == 0:
        raise ValueError("Invalid input mesh with zero elements: v and f must have shape (n, 3) and (m, 3) (n, m > 0). " + got)
    if sv[1] != 3 or sf[1] != 3:
        raise ValueError("Only 3D inputs are supported: v and f must have shape (n, 3) and (m, 3) (n, m > 0). " + got)
    if sv[0] > _MAX_ROWS or sf[0] > _MAX_ROWS:
        raise ValueError("meshes and point clouds with more than 2^27-16 rows are not supported")
    return dv, sv[0], sf[0]


def _check_points(p, want=None):
    """Scalar type, then validate_point_cloud (src/common/common.h:58-74; zero rows are allowed), then the row limit. Returns (dtype name, #p)."""
    from . import _dtype_name, _shape2
    dp = _dtype_name(p)
    if dp not in ("float32", "float64"):
        raise ValueError(f"Invalid scalar type ({dp}) for argument 'p'. Expected one of ['float32', 'float64'].")
    if want is not None and dp != want:
        raise ValueError(f"Invalid scalar type ({dp}) for argument 'p'. Expected it to match the indexed mesh which is of type {want}.")
    sp = _shape2(p)
    if sp[1] != 3:
        raise ValueError(f"Only 3D inputs are supported: v must have shape (n, 3) (n > 0). Got points.shape =({sp[0]}, {sp[1]}).")
    if sp[0] > _MAX_ROWS:
        raise ValueError("meshes and point clouds with more than 2^27-16 rows are not supported")
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


def _results(d, n):
    return d.empty((n,), "T"), d.empty((n,), "i64"), d.empty((n, 3), "T")


def _finish(dist, fi, bc, f, n):
    """fi in f's dtype; singleton dimensions squeezed as the package's other calls do (numpyeigen's squeeze)."""
    from . import _is_torch
    fi = fi.to(f.dtype) if _is_torch(fi) else fi.astype(f.dtype, copy=False)
    if n == 1:
        return dist.reshape(()), fi.reshape(()), bc.reshape(3)
    return dist, fi, bc


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
    from . import _lib, _Dev, _fn, _is_torch, _record, Stats
    dp, n = _check_points(p)
    _, nv, nf = _check_mesh(v, f, want=dp)
    if not (_is_torch(p) or _is_torch(v) or _is_torch(f)):
        _host_mesh_checks(np.asarray(v), np.asarray(f))
        _host_point_checks(np.asarray(p))
    d = _Dev(p, v)
    ff = _faces_for(d, f)
    dist, fi, bc = _results(d, n)
    st = Stats()
    rc = _fn("closest_points_on_mesh", d.suffix)(d.ctx, d.pb, nv, _Dev.ptr(ff), nf, _FACE_KINDS[_face_dtype_name(ff)], d.pa, n,
                                                 _Dev.ptr(dist), _Dev.ptr(fi), _Dev.ptr(bc), d.flags, d.stream, ctypes.addressof(st))
    if rc:
        _lib.check(rc)
    _record(st)
    return _finish(dist, fi, bc, ff, n)


class MeshIndex:
    """A triangle mesh kept on the GPU as its search index (not in the reference API, which rebuilds libigl's AABB tree on every call): build
    once, query many times.

        with pcu.MeshIndex(v, f) as mesh:
            d, fi, bc = mesh.closest_points(p)          # same rows as pcu.closest_points_on_mesh(p, v, f)

    `v`: (#v, 3) float32 / float64, `f`: (#f, 3) integer faces; numpy or CUDA/HIP torch tensors (copied; the caller's arrays can go away).
    Queries must have the mesh's dtype. The index lives on one GPU; call close() (or use `with`) to free it."""

    def __init__(self, v, f):
        from . import _lib, _Dev, _fn, _is_torch
        dv, nv, nf = _check_mesh(v, f)
        if not (_is_torch(v) or _is_torch(f)):
            _host_mesh_checks(np.asarray(v), np.asarray(f))
        d = _Dev(v, v)
        ff = _faces_for(d, f)
        self._suffix, self._dtype_name, self._device = d.suffix, dv, d.device
        self._face_like = ff[:0]                    # carries f's dtype (and kind of array) for the result
        self._h = None
        h = ctypes.c_void_p()
        rc = _fn("mesh_index_create", d.suffix)(d.ctx, d.pa, nv, _Dev.ptr(ff), nf, _FACE_KINDS[_face_dtype_name(ff)], d.flags, d.stream, ctypes.byref(h))
        if rc:
            _lib.check(rc)
        self._h = h
        self.num_faces = nf

    def closest_points(self, p):
        """See point_cloud_utils_amd.closest_points_on_mesh; the mesh is the indexed one."""
        from . import _lib, _Dev, _fn, _record, _is_torch, Stats
        if self._h is None:
            raise ValueError("the mesh index has been closed")
        _, n = _check_points(p, want=self._dtype_name)
        if not _is_torch(p):
            _host_point_checks(np.asarray(p))
        d = _Dev(p, p)
        if d.device != self._device:
            raise ValueError("query points and mesh index live on different devices")
        dist, fi, bc = _results(d, n)
        st = Stats()
        rc = _fn("mesh_index_closest", d.suffix)(d.ctx, self._h, d.pa, n, _Dev.ptr(dist), _Dev.ptr(fi), _Dev.ptr(bc), d.flags, d.stream,
                                                 ctypes.addressof(st))
        if rc:
            _lib.check(rc)
        _record(st)
        like = self._face_like
        if _is_torch(like) and not d.torch:          # index built from tensors, numpy queries: numpy results
            like = np.empty((0,), dtype=str(like.dtype).replace("torch.", ""))
        elif d.torch and not _is_torch(like):
            import torch
            like = torch.empty((0,), dtype=getattr(torch, like.dtype.name if like.dtype.kind == "i" else "int64"))
        return _finish(dist, fi, bc, like, n)

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
