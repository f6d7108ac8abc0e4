"""adjacency_list, estimate_mesh_vertex_normals and laplacian_smooth_mesh: the reference's bindings (src/adjacency_list.cpp,
src/mesh_normals.cpp:24-50, src/smooth.cpp:24-79) over the HIP kernels of csrc/mesh_smooth.h, and mesh_vertex_adjacency, the same structure
as CSR. Same arguments, defaults and error texts; the values follow this library's stated contract instead of libigl's
and Eigen's code, which was not at hand."""
import ctypes
import math

import numpy as np

from ._call import _Dev, _FACE_KINDS, _call, _is_torch, _shape2, _take
from ._checks import _beside, _check_mesh, _check_rows, _face_dtype_name, _mesh_args, _resolve

_WEIGHTINGS = {"uniform": 0, "area": 1, "angle": 2}


def _check_faces(f):
    """Scalar type (int32 / int64: the reference's), then validate_mesh_faces (src/common/common.h:113-127) and the row limit. Returns #f."""
    df = _face_dtype_name(f)
    if df not in ("int32", "int64"):
        raise ValueError(f"Invalid scalar type ({df}) for argument 'f'. Expected one of ['int32', 'int64'].")
    sf = _shape2(f)
    if sf[0] == 0:
        raise ValueError(f"Invalid input faces with zero elements: f must have shape (n, 3) where n > 0. Got f.shape =({sf[0]}, {sf[1]}).")
    if sf[1] != 3:
        raise ValueError(f"Only triangle inputs are supported: f must have shape (n, 3) where n > 0. Got f.shape =({sf[0]}, {sf[1]}).")
    _check_rows(sf[0])
    return sf[0]


def mesh_vertex_adjacency(f, num_vertices=None):
    """
    The vertex adjacency of a triangle mesh in compressed rows (not in the reference API: adjacency_list without leaving the device)

    Args:
        f : (#f, 3)-shaped array of face indices (int32 or int64; numpy, or a CUDA/HIP torch tensor)
        num_vertices : the number of rows nv; f.max() + 1 if None (for a tensor that reads one number back)

    Returns:
        offsets : (nv + 1,) int64: the neighbours of vertex i are neighbours[offsets[i]:offsets[i + 1]]
        neighbours : (offsets[nv],) in f's dtype
        (tensors in, tensors on the same device out)

    Notes:
        The contract: the neighbours of i are the j != i that share a face with i, each once, ascending. A face that lists
        a vertex twice adds no i -> i entry; a vertex that no face lists has an empty row. Equal arguments give equal bytes.
        ValueError: a dtype other than int32 / int64, zero rows or a second dimension other than 3 (the reference's texts), a face index
        outside [0, nv), more than 2**27 - 16 rows.
    """
    nf = _check_faces(f)
    if num_vertices is None:
        top = int(f.max())
        if top < 0:
            raise ValueError("f must hold row indices of v: found a face index outside [0, 0)")
        nv = top + 1
    else:
        nv = int(num_vertices)
        if nv <= 0:
            raise ValueError("num_vertices must be positive")
    _check_rows(nv)
    if not _is_torch(f):
        fa = np.asarray(f)
        if int(fa.min()) < 0 or int(fa.max()) >= nv:
            raise ValueError(f"f must hold row indices of v: found a face index outside [0, {nv})")
    d = _Dev(f, f)
    ff = _beside(d, f)
    name = _face_dtype_name(ff)
    count = ctypes.c_int64(0)
    _call("mesh_adjacency", d, _Dev.ptr(ff), nf, _FACE_KINDS[name], nv, ctypes.addressof(count), suffix=False)
    ne = int(count.value)
    offsets, neighbours = _take("mesh_adjacency", d, [((nv + 1,), np.int64), ((ne,), np.dtype(name))], nv, ne)
    return offsets, neighbours


def adjacency_list(f):
    """
    Compute the adjacency list given a set of mesh faces.

    Args:
        f : (#f, 3)-shaped array of face (triangle) indices (int32 or int64; numpy, or a CUDA/HIP torch tensor)

    Returns:
        adj_list : a list of f.max() + 1 lists such that adj_list[i] contains the indexes of vertices adjacent to vertex i

    Notes:
        The rows of mesh_vertex_adjacency(f) as Python lists: each neighbour once, ascending. This is libigl's sorted, unique
        igl::adjacency_list as far as its source is remembered here; it was not at hand.
    """
    offsets, neighbours = mesh_vertex_adjacency(f)
    if _is_torch(offsets):
        offsets, neighbours = offsets.cpu().numpy(), neighbours.cpu().numpy()
    nb = neighbours.tolist()
    off = offsets.tolist()
    return [nb[off[i]:off[i + 1]] for i in range(len(off) - 1)]


def estimate_mesh_vertex_normals(v, f, weighting_type="uniform"):
    """
    Compute vertex normals of a mesh from its vertices and faces

    Args:
        v : (#v, 3)-shaped array of mesh vertex 3D positions (float32 or float64; numpy, or a CUDA/HIP torch tensor)
        f : (#f, 3)-shaped array of face (triangle) indices (int32, int64, uint32 or uint64; int32 / int64 for torch)
        weighting_type : Weighting type must be one of 'uniform', 'angle', or 'area' (default is 'uniform')

    Returns:
        n : (#v, 3)-shaped array of vertex normals (i.e. n[i] is the normal at vertex v[i]), in v's dtype

    Notes:
        The contract. Per face N = (b - a) x (c - a) and the unit normal exactly as estimate_mesh_face_normals computes
        them (v's dtype, no FMA, zero for a face without area). Corner c of face t adds to its vertex the unit normal ('uniform'), N itself
        ('area'), or the unit normal times atan2(|e1 x e2|, e1 . e2) with e1, e2 the two edges that leave the corner ('angle'). A vertex's
        corners are added from zero, ascending by 3 t + c, component by component; the sum s is divided by sqrt((s0*s0 + s1*s1) + s2*s2).
        A zero sum gives a zero row where libigl gives NaN; so does a vertex in no face. Equal arguments give equal bytes.
        ValueError: the reference's text for another weighting_type; the dtype, shape and row-limit checks of the other mesh operators;
        non-finite coordinates; a face index outside [0, #v); normals whose length overflows v's dtype.
    """
    _check_mesh(v, f)
    if weighting_type not in _WEIGHTINGS:
        raise ValueError(f"Invalid weighting_type must be one of 'uniform', 'angle', or 'area', but got '{weighting_type}'")
    d, ff, nv, nf = _resolve(v, f)
    out = d.empty((nv, 3), "T")
    _call("mesh_vertex_normals", d, *_mesh_args(d, ff, nv, nf), _WEIGHTINGS[weighting_type], _Dev.ptr(out))
    return out


def laplacian_smooth_mesh(v, f, num_iters, step_size=0.1, use_cotan_weights=False):
    """
    Smooth a mesh using Laplacian smoothing

    Args:
        v : (#v, 3)-shaped array of mesh vertex 3D positions (float32 or float64; numpy, or a CUDA/HIP torch tensor)
        f : (#f, 3)-shaped array of face (triangle) indices (int32 or int64)
        num_iters : Number of smoothing iterations to perform
        step_size : Step size per iteration (default is 0.1)
        use_cotan_weights : weigh every step by the vertices' areas and rescale to unit area after it (default False)

    Returns:
        u : (#v, 3)-shaped array of smoothed vertex positions, in v's dtype

    Notes:
        The contract. L is the cotangent matrix of the input v in both modes, as in the reference: corner c of face t,
        with e1, e2 the edges that leave it and (j, k) the edge opposite, adds (0.5 * (e1 . e2)) / |e1 x e2| (0 where |e1 x e2| == 0) to
        L[j, k] and L[k, j]; L[i, i] is minus the sum of row i. Every iteration solves (M - h L) u' = M u for the three columns, with M = I
        and h = step_size, or with use_cotan_weights M_ii = (sum of |N| over the faces at i, of the current u) / 6, h = step_size * 1e-3 and
        then the reference's rescale u' <- (u' - c) / sqrt(A) + c (A the surface area, c the area-weighted centroid of u').
        The solve is Jacobi-preconditioned conjugate gradients from x0 = u; a column stops when its recurrence residual satisfies
        r.r <= (64 eps)^2 b.b. All sums have a fixed order and there are no floating-point atomics: equal arguments give equal bytes, numpy
        or tensor. last_stats()["n_passes"] is the number of conjugate-gradient iterations of the call.
        Differences from the reference. It factors with Eigen's SimplicialLLT and returns NaN for a face without area or an unreferenced
        vertex with use_cotan_weights; here a vertex with M_ii == 0 (unreferenced, or in faces without area only) keeps its position: its
        row and column leave the system and the rescale passes it by. A step_size that is negative or not finite is a ValueError.
        ValueError: num_iters < 0 (the reference's text); the dtype, shape and row-limit checks of the other mesh operators (f: int32 /
        int64); non-finite coordinates; a face index outside [0, #v). RuntimeError: a solve that has not stopped after 4096 iterations (a
        chosen cap) or that met p.Ap <= 0.
    """
    _check_mesh(v, f)
    df = _face_dtype_name(f)
    if df not in ("int32", "int64"):
        raise ValueError(f"Invalid scalar type ({df}) for argument 'f'. Expected one of ['int32', 'int64'].")
    num_iters = int(num_iters)
    if num_iters < 0:
        raise ValueError("Invalid value for argument num_iters in smooth_mesh_laplacian. Must be a positive integer or 0.")
    step = float(step_size)
    if not math.isfinite(step) or step < 0.0:
        raise ValueError("step_size must be finite and not negative")
    d, ff, nv, nf = _resolve(v, f)
    out = d.empty((nv, 3), "T")
    _call("laplacian_smooth_mesh", d, *_mesh_args(d, ff, nv, nf), num_iters, step, int(bool(use_cotan_weights)), _Dev.ptr(out))
    return out
