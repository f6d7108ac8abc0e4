"""point_cloud_fast_winding_number and estimate_mesh_face_normals: the reference's bindings (src/fast_winding_numbers.cpp:51-67,
src/mesh_normals.cpp:65-80) over the HIP kernels of csrc/pc_winding.h, and PointCloudWindingIndex, the build-once twin of the one-shot call.
Same arguments, dtypes and error texts where the reference has one; the values follow this library's deterministic contract (DESIGN.md,
row f10) instead of libigl's."""
import ctypes

import numpy as np

from ._call import _call
from ._mesh import _check_mesh, _check_rows, _scalar_rows
from ._mesh_sample import _mesh_args, _resolve

_SAME_DEVICE = "torch inputs must all be CUDA/HIP tensors on the same device"


def _check_beta(beta):
    beta = float(beta)
    if not beta > 0.0:
        raise ValueError("beta must be greater than 0 (finite, or +inf for the plain sum over all points)")
    return beta


def _match(x, name, want, what):
    from . import _dtype_name
    dx = _dtype_name(x)
    if dx != want:
        raise ValueError(f"Invalid scalar type ({dx}) for argument '{name}'. Expected it to match {what} which is of type {want}.")


def _check_cloud(p, n, a):
    """Scalar types, then validate_point_cloud_normals(p, n, allow_0=false) (src/common/common.h:78-110), the size of `a` (any shape with
    #p elements: the reference reshapes it) and the row limit. Returns (dtype name, #p)."""
    from . import _dtype_name, _shape2
    dp = _dtype_name(p)
    if dp not in ("float32", "float64"):
        raise ValueError(f"Invalid scalar type ({dp}) for argument 'p'. Expected one of ['float32', 'float64'].")
    _match(n, "n", dp, "argument 'p'")
    _match(a, "a", dp, "argument 'p'")
    sp, sn = _shape2(p), _shape2(n)
    if sp[0] == 0:
        raise ValueError(f"Invalid input point cloud with zero points: points must have shape (n, 3) (n > 0). Got points.shape =({sp[0]}, {sp[1]}).")
    if sp[1] != 3:
        raise ValueError(f"Only 3D inputs are supported: v must have shape (n, 3) (n > 0). Got points.shape =({sp[0]}, {sp[1]}).")
    if sn[1] != 3:
        raise ValueError(f"Invalid shape for normals: must have shape (n, 3) (n > 0). Got normals.shape =({sn[0]}, {sn[1]}).")
    if sn[0] != sp[0]:
        raise ValueError("Invalid input point cloud. Number of normals must match number of points. "
                         f"Got points.shape =({sp[0]}, {sp[1]}) and normals.shape = {sn[0]}, {sn[1]}")
    size = 1
    for x in a.shape:
        size *= int(x)
    if size != sp[0]:
        raise ValueError(f"Invalid shape for areas: a must have one element per point ({sp[0]}). Got a.shape = {tuple(int(x) for x in a.shape)}.")
    _check_rows(sp[0])
    return dp, sp[0]


def _check_queries(q, want, what):
    """Scalar type, then validate_point_cloud(q, allow_0=false) and the row limit. Returns #q."""
    from . import _shape2
    _match(q, "q", want, what)
    sq = _shape2(q)
    if sq[0] == 0:
        raise ValueError(f"Invalid input point cloud with zero points: points must have shape (n, 3) (n > 0). Got points.shape =({sq[0]}, {sq[1]}).")
    if sq[1] != 3:
        raise ValueError(f"Only 3D inputs are supported: v must have shape (n, 3) (n > 0). Got points.shape =({sq[0]}, {sq[1]}).")
    _check_rows(sq[0])
    return sq[0]


def _host_finite(**arrays):
    """What the library checks on the device for device-resident input, found on the host for host arrays (before any device work)."""
    for name, x in arrays.items():
        if not bool(np.isfinite(x).all()):
            raise ValueError(f"{name} must not contain NaN or infinite " + ("values" if name == "a" else "coordinates"))


def _host_cloud_checks(p, n, a):
    _host_finite(p=p, n=n, a=a)
    with np.errstate(over="ignore"):
        if not bool(np.isfinite(np.reshape(a, (-1, 1)) * n).all()):
            raise ValueError("a * n overflows the scalar type of p")


def _beside(d, x):
    """`x` next to the resolved arrays of a call: same kind (torch on that device / numpy), contiguous."""
    from . import _is_torch
    if d.torch:
        if not _is_torch(x) or not x.is_cuda or x.device != d.tdev:
            raise ValueError(_SAME_DEVICE)
        return x.contiguous()
    if _is_torch(x):
        raise ValueError(_SAME_DEVICE)
    return np.ascontiguousarray(x)


def _resolve_cloud(p, n, a):
    from . import _Dev, _is_torch
    if not (_is_torch(p) or _is_torch(n) or _is_torch(a)):
        _host_cloud_checks(np.asarray(p), np.asarray(n), np.asarray(a))
    d = _Dev(p, n)
    return d, _beside(d, a).reshape(-1)


def point_cloud_fast_winding_number(p, n, a, q, *, beta=2.0):
    """
    Compute a consistent inside/outside field given an oriented point cloud and evaluate that field at a set of query points

    Args:
      p : (#p, 3)-shaped array of point positions (float32 or float64; numpy, or a CUDA/HIP torch tensor)
      n : (#p, 3)-shaped array of point normals (p's dtype; need not have unit length)
      a : array of #p point areas in any shape (p's dtype; any finite value)
      q : (#q, 3)-shaped array of query positions at which to evaluate the winding number field (p's dtype)
      beta : accuracy of the fast evaluation (not in the reference API, which uses libigl's default 2): a tree node farther from the query
             than beta times its radius is replaced by a three-term expansion; float('inf') gives the plain sum over all points

    Returns:
      A (#q,)-shaped array with the winding number of each query point: about 1 inside a closed surface sampled with outward normals and
      areas that sum to its area, about 0 outside.

    Notes:
      Point i is the dipole a_i * n_i: W(q) = (1/4 pi) sum_i a_i n_i . (p_i - q) / |p_i - q|^3; a query on a point gets nothing from that
      point. The fast evaluation is that of Barill et al. (2018) with the tree, moments and evaluation order stated in DESIGN.md (f10):
      equal bits for equal arguments. Near a sample (closer than the sample spacing) the field of a point cloud is not that of the surface.
      Zero rows in p or q, non-finite values, a product a_i * n_i that overflows and arrays of more than 2**27 - 16 rows raise ValueError.
    """
    from . import _Dev, _is_torch
    dp, np_ = _check_cloud(p, n, a)
    nq = _check_queries(q, dp, "argument 'p'")
    beta = _check_beta(beta)
    d, aa = _resolve_cloud(p, n, a)
    qq = _beside(d, q)
    if not _is_torch(q):
        _host_finite(q=qq)
    w = d.empty((nq,), "T")
    _call("point_cloud_fast_winding_number", d, d.pa, d.pb, _Dev.ptr(aa), np_, _Dev.ptr(qq), nq, beta, _Dev.ptr(w))
    return _scalar_rows(w, nq)


class PointCloudWindingIndex:
    """An oriented point cloud kept on the GPU as the tree of its fast winding number (not in the reference API, which rebuilds libigl's
    octree on every call): build once, query many times.

        with pcu.PointCloudWindingIndex(p, n, a) as cloud:
            w = cloud.winding_number(q)                 # same rows as pcu.point_cloud_fast_winding_number(p, n, a, q)

    `p`, `n`: (#p, 3) float32 / float64, `a`: #p areas; numpy or CUDA/HIP torch tensors (copied; the caller's arrays can go away). Queries
    must have the cloud's dtype. The index lives on one GPU; call close() (or use `with`) to free it."""

    def __init__(self, p, n, a):
        from . import _lib, _Dev, _fn
        dp, np_ = _check_cloud(p, n, a)
        d, aa = _resolve_cloud(p, n, a)
        self._dtype_name, self._device = dp, d.device
        self._h = None
        h = ctypes.c_void_p()
        rc = _fn("pc_winding_index_create", d.suffix)(d.ctx, d.pa, d.pb, _Dev.ptr(aa), np_, d.flags, d.stream, ctypes.byref(h))
        if rc:
            _lib.check(rc)
        self._h = h
        self.num_points = np_

    def winding_number(self, q, *, beta=2.0):
        """See point_cloud_utils_amd.point_cloud_fast_winding_number; the cloud is the indexed one."""
        from . import _Dev, _is_torch
        if self._h is None:
            raise ValueError("the point cloud winding index has been closed")
        nq = _check_queries(q, self._dtype_name, "the indexed point cloud")
        beta = _check_beta(beta)
        if not _is_torch(q):
            _host_finite(q=np.asarray(q))
        d = _Dev(q, q)
        if d.device != self._device:
            raise ValueError("query points and point cloud winding index live on different devices")
        w = d.empty((nq,), "T")
        _call("pc_winding_index_query", d, self._h, d.pa, nq, beta, _Dev.ptr(w))
        return _scalar_rows(w, nq)

    def close(self):
        if getattr(self, "_h", None) is not None:
            from . import _lib
            _lib.lib().pcu_hip_pc_winding_index_destroy(self._h)
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


def estimate_mesh_face_normals(v, f):
    """
    Compute the normal of each face of a triangle mesh

    Args:
      v : (#v, 3)-shaped array of mesh vertex positions (float32 or float64; numpy, or a CUDA/HIP torch tensor)
      f : (#f, 3)-shaped array of mesh face indices (int32, int64, uint32 or uint64; int32 / int64 for torch)

    Returns:
      n : (#f, 3)-shaped array of unit face normals, in v's dtype ((0, 0, 0) for a face without area)

    Notes:
      Per face (a, b, c), in v's dtype, every operation rounded on its own (no FMA): N = (b - a) x (c - a), r = sqrt((N0*N0 + N1*N1) + N2*N2),
      n = N / r component by component. A face whose cross product underflows to zero gets a zero normal like a face without area; one whose
      length overflows raises ValueError("face normals overflow the scalar type of v"). Non-finite coordinates, face indices outside [0, #v)
      and arrays of more than 2**27 - 16 rows raise ValueError.
    """
    from . import _Dev
    _check_mesh(v, f)
    d, ff, nv, nf = _resolve(v, f)
    out = d.empty((nf, 3), "T")
    _call("estimate_mesh_face_normals", d, *_mesh_args(d, ff, nv, nf), _Dev.ptr(out))
    return out
