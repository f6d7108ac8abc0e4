"""point_cloud_fast_winding_number and estimate_mesh_face_normals: the reference's bindings (src/fast_winding_numbers.cpp:51-67,
src/mesh_normals.cpp:65-80) over the HIP kernels of csrc/pc_winding.h, and PointCloudWindingIndex, the build-once twin of the one-shot call.
Same arguments, dtypes and error texts where the reference has one; the values follow this library's deterministic contract (DESIGN.md,
row f10) instead of libigl's."""
import numpy as np

from ._call import _Dev, _Handle, _call, _is_torch
from ._checks import (_beside, _check_beta, _check_mesh, _check_normals, _check_points_nonzero, _check_rows, _host_finite, _match, _mesh_args,
                      _resolve, _scalar_rows, _size)


def _check_cloud(p, n, a):
    """Scalar types, then validate_point_cloud_normals(p, n, allow_0=false) (src/common/common.h:78-110), the size of `a` (any shape with
    #p elements: the reference reshapes it) and the row limit. Returns (dtype name, #p)."""
    dp, np_ = _check_normals(p, n, False, a=a)
    if _size(a) != np_:
        raise ValueError(f"Invalid shape for areas: a must have one element per point ({np_}). Got a.shape = {tuple(int(x) for x in a.shape)}.")
    _check_rows(np_)
    return dp, np_


def _check_queries(q, want, what):
    """Scalar type, then validate_point_cloud(q, allow_0=false) and the row limit. Returns #q."""
    _match(q, "q", want, what)
    return _check_points_nonzero(q)


def _host_cloud_checks(p, n, a):
    _host_finite(p=p, n=n, a=a)
    with np.errstate(over="ignore"):
        if not bool(np.isfinite(np.reshape(a, (-1, 1)) * n).all()):
            raise ValueError("a * n overflows the scalar type of p")


def _resolve_cloud(p, n, a):
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
    dp, np_ = _check_cloud(p, n, a)
    nq = _check_queries(q, dp, "argument 'p'")
    beta = _check_beta(beta, "points")
    d, aa = _resolve_cloud(p, n, a)
    qq = _beside(d, q)
    if not _is_torch(q):
        _host_finite(q=qq)
    w = d.empty((nq,), "T")
    _call("point_cloud_fast_winding_number", d, d.pa, d.pb, _Dev.ptr(aa), np_, _Dev.ptr(qq), nq, beta, _Dev.ptr(w))
    return _scalar_rows(w, nq)


class PointCloudWindingIndex(_Handle):
    """An oriented point cloud kept on the GPU as the tree of its fast winding number (not in the reference API, which rebuilds libigl's
    octree on every call): build once, query many times.

        with pcu.PointCloudWindingIndex(p, n, a) as cloud:
            w = cloud.winding_number(q)                 # same rows as pcu.point_cloud_fast_winding_number(p, n, a, q)

    `p`, `n`: (#p, 3) float32 / float64, `a`: #p areas; numpy or CUDA/HIP torch tensors (copied; the caller's arrays can go away). Queries
    must have the cloud's dtype. The index lives on one GPU; call close() (or use `with`) to free it."""
    _noun, _destroy = "point cloud winding index", "pcu_hip_pc_winding_index_destroy"

    def __init__(self, p, n, a):
        dp, np_ = _check_cloud(p, n, a)
        d, aa = _resolve_cloud(p, n, a)
        self._dtype_name = dp
        self._open("pc_winding_index_create", d, d.pa, d.pb, _Dev.ptr(aa), np_)
        self.num_points = np_

    def winding_number(self, q, *, beta=2.0):
        """See point_cloud_utils_amd.point_cloud_fast_winding_number; the cloud is the indexed one."""
        self._check_open()
        nq = _check_queries(q, self._dtype_name, "the indexed point cloud")
        beta = _check_beta(beta, "points")
        if not _is_torch(q):
            _host_finite(q=np.asarray(q))
        d = _Dev(q, q)
        self._same_device(d, "query points")
        w = d.empty((nq,), "T")
        _call("pc_winding_index_query", d, self._h, d.pa, nq, beta, _Dev.ptr(w))
        return _scalar_rows(w, nq)


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
    _check_mesh(v, f)
    d, ff, nv, nf = _resolve(v, f)
    out = d.empty((nf, 3), "T")
    _call("estimate_mesh_face_normals", d, *_mesh_args(d, ff, nv, nf), _Dev.ptr(out))
    return out
