"""remove_mesh_vertices, remove_unreferenced_mesh_vertices, deduplicate_mesh_vertices and orient_mesh_faces: the reference's bindings
(src/remove_mesh_vertices.cpp:22-73, src/remove_unreferenced_mesh_vertices.cpp:23-37, src/remove_duplicates.cpp:37-81 and :152-176,
src/orient_mesh_faces.cpp:21-35) over the HIP kernels of csrc/mesh_repair.h. Same arguments, defaults, dtypes and return order; the values
follow this library's stated contract where the reference reaches libigl, which was not at hand."""
import ctypes

import numpy as np

from ._call import _Dev, _FACE_KINDS, _call, _int_out, _is_torch, _shape2
from ._checks import _beside, _check_face_dtype, _check_mesh, _check_rows, _face_dtype_name

_MAX_INDEX = 2 ** 31 - 16


def _check_signed_faces(f):
    df = _face_dtype_name(f)
    if df not in ("int32", "int64"):
        raise ValueError(f"Invalid scalar type ({df}) for argument 'f'. Expected one of ['int32', 'int64'].")


def _host_face_range(v, f, nv):
    """For host arrays, what the library checks on the device: before any device work."""
    if not (_is_torch(v) or _is_torch(f)):
        fa = np.asarray(f)
        if (fa.dtype.kind == "i" and int(fa.min()) < 0) or int(fa.max()) >= nv:
            raise ValueError(f"f must hold row indices of v: found a face index outside [0, {nv})")


def _head(x, m, d):
    """The first m rows of a buffer sized for the worst case (a copy where they are less than half of it: the rest is not kept alive)."""
    y = x[:m]
    if 2 * m < int(x.shape[0]):
        y = y.clone() if d.torch else y.copy()
    return y


def remove_mesh_vertices(v, f, mask):
    """
    Removes vertices specified by a mask from a triangle mesh and updates the face indices accordingly.

    Args:
        v : (#v, 3)-shaped array of mesh vertex 3D positions (float32 or float64; numpy, or a CUDA/HIP torch tensor)
        f : (#f, 3)-shaped array of face (triangle) indices (int32 or int64)
        mask : a boolean mask of shape (#v,) or (#v, 1) indicating which vertices to keep (True) or remove (False)

    Returns:
        v_out : (#kept, 3)-shaped array of the kept vertices, in input order, in v's dtype
        f_out : (#f_out, 3)-shaped array of the faces whose three corners are all kept, re-indexed, in input order, in f's dtype
        (on the side the inputs came from; (0, 3) arrays where nothing is kept)

    Notes:
        The contract is the reference's two loops. Rows of v are copied, never computed with: NaN, infinities and -0.0
        pass through. last_stats()["n_escalated"] is the number of faces dropped. Equal arguments give equal bytes.
        ValueError: the dtype, shape and row-limit checks of the other mesh operators (f: int32 / int64), a mask that is not bool, "mask
        should have the same number of rows as v", "mask should have only one column", a face index outside [0, #v).
    """
    _, nv, nf = _check_mesh(v, f)
    _check_signed_faces(f)
    dm = str(mask.dtype).replace("torch.", "") if _is_torch(mask) else np.asarray(mask).dtype.name
    if dm != "bool":
        raise ValueError(f"Invalid scalar type ({dm}) for argument 'mask'. Expected one of ['bool'].")
    sm = _shape2(mask if _is_torch(mask) else np.asarray(mask))
    if sm[0] != nv:
        raise ValueError("mask should have the same number of rows as v")
    if sm[1] != 1:
        raise ValueError("mask should have only one column")
    _host_face_range(v, f, nv)
    d = _Dev(v, v)
    ff, mm = _beside(d, f), _beside(d, mask)
    name = _face_dtype_name(ff)
    v_out, f_out = d.empty((nv, 3), "T"), _int_out(d, (nf, 3), np.dtype(name))
    kept_v, kept_f = ctypes.c_int64(0), ctypes.c_int64(0)
    _call("remove_mesh_vertices", d, d.pa, nv, _Dev.ptr(ff), nf, _FACE_KINDS[name], _Dev.ptr(mm), _Dev.ptr(v_out), _Dev.ptr(f_out),
          ctypes.addressof(kept_v), ctypes.addressof(kept_f))
    return _head(v_out, int(kept_v.value), d), _head(f_out, int(kept_f.value), d)


def remove_unreferenced_mesh_vertices(v, f):
    """
    Removes the vertices of a triangle mesh that no face lists

    Args:
        v : (#v, 3)-shaped array of mesh vertex 3D positions (float32 or float64; numpy, or a CUDA/HIP torch tensor)
        f : (#f, 3)-shaped array of face (triangle) indices (int32, int64, uint32 or uint64; int32 / int64 for torch)

    Returns:
        v_new : (#v_new, 3)-shaped array of the referenced vertices, in input order, in v's dtype
        f_new : (#f, 3)-shaped array of all the faces, indexing into v_new
        correspondences_v : (#v_new,)-shaped array of indices so that v_new = v[correspondences_v]
        correspondences_f : (#v,)-shaped array that maps an old vertex index to its new one, -1 for a vertex that no face lists (an unsigned
                            dtype wraps it, as the reference's assignment would)
        (the last three in f's dtype; all four on the side the inputs came from)

    Notes:
        The contract: a vertex stays when some face lists it, and the vertices that stay keep their order. This is
        igl::remove_unreferenced as far as its source is remembered here; it was not at hand. The names of the two maps are the reference's.
        Rows of v are copied, never computed with: v_new[f_new] equals v[f] bit for bit. last_stats()["n_escalated"] is 0: no face is dropped.
        ValueError: the dtype, shape and row-limit checks of the other mesh operators, a face index outside [0, #v).
    """
    _, nv, nf = _check_mesh(v, f)
    _host_face_range(v, f, nv)
    d = _Dev(v, v)
    ff = _beside(d, f)
    name = _face_dtype_name(ff)
    dt = np.dtype(name)
    v_new, f_new, corr_v, corr_f = d.empty((nv, 3), "T"), _int_out(d, (nf, 3), dt), _int_out(d, (nv,), dt), _int_out(d, (nv,), dt)
    kept_v = ctypes.c_int64(0)
    _call("remove_unreferenced_mesh_vertices", d, d.pa, nv, _Dev.ptr(ff), nf, _FACE_KINDS[name], _Dev.ptr(v_new), _Dev.ptr(f_new), _Dev.ptr(corr_v),
          _Dev.ptr(corr_f), ctypes.addressof(kept_v))
    m = int(kept_v.value)
    return _head(v_new, m, d), f_new, _head(corr_v, m, d), corr_f


def deduplicate_mesh_vertices(v, f, epsilon, return_index=True):
    """
    Removes duplicated vertices from a triangle mesh where two vertices are considered the same if they agree after rounding to multiples of
    epsilon (epsilon <= 0: exactly equal)

    Args:
        v : (#v, 3)-shaped array of mesh vertex 3D positions (float32 or float64; numpy, or a CUDA/HIP torch tensor)
        f : (#f, 3)-shaped array of face (triangle) indices (int32 or int64)
        epsilon : threshold below which two vertices are considered equal
        return_index : if true, return indices to map between input and output

    Returns:
        v_out : (#v_out, 3)-shaped array of mesh vertices with duplicates removed
        f_out : (#f_out, 3)-shaped array of mesh faces corresponding to the deduplicated mesh, in f's dtype
        svi : (#v_out,) int32 indices so that v_out = v[svi] (only returned if return_index is True)
        svj : (#v,) int32 indices so that v ~ v_out[svj] (only returned if return_index is True)

    Notes:
        The contract: v_out, svi and svj are exactly what deduplicate_point_cloud(v, epsilon) returns (unique rows in
        lexicographic order of the rounded coordinates, the lowest row of every group); f_out is svj[f] without the rows in which two
        corners coincide, in input order. The row order is igl::unique_rows' as far as it is remembered here; libigl was not at hand.
        last_stats()["n_escalated"] is the number of faces dropped. Equal arguments give equal bytes.
        ValueError: the dtype, shape and row-limit checks of the other mesh operators (f: int32 / int64), a face index outside [0, #v).
    """
    _, nv, nf = _check_mesh(v, f)
    _check_signed_faces(f)
    eps = float(epsilon)
    _host_face_range(v, f, nv)
    d = _Dev(v, v)
    ff = _beside(d, f)
    name = _face_dtype_name(ff)
    v_out, f_out = d.empty((nv, 3), "T"), _int_out(d, (nf, 3), np.dtype(name))
    svi, svj = _int_out(d, (nv,), np.int32), _int_out(d, (nv,), np.int32)
    kept_v, kept_f = ctypes.c_int64(0), ctypes.c_int64(0)
    _call("deduplicate_mesh_vertices", d, d.pa, nv, _Dev.ptr(ff), nf, _FACE_KINDS[name], eps, _Dev.ptr(v_out), _Dev.ptr(f_out), _Dev.ptr(svi), _Dev.ptr(svj),
          ctypes.addressof(kept_v), ctypes.addressof(kept_f))
    m = int(kept_v.value)
    v_out, f_out = _head(v_out, m, d), _head(f_out, int(kept_f.value), d)
    if return_index:
        return v_out, f_out, _head(svi, m, d), svj
    return v_out, f_out


def orient_mesh_faces(f, weighting_type="uniform"):
    """
    Consistently orient faces of a mesh within each connected component

    Args:
        f : (#f, 3)-shaped array of face (triangle) indices (int32, int64, uint32 or uint64; numpy, or an int32 / int64 CUDA/HIP torch tensor)
        weighting_type : accepted and ignored, as the reference ignores it

    Returns:
        oriented_faces : (#f, 3)-shaped array of faces which are consistently oriented
        face_components : (#f,)-shaped array of component ids (face_components[i] is the component of the face f[i])
        (both in f's dtype, on the side f came from)

    Notes:
        The contract. Face i has the directed edges (f[i,0], f[i,1]), (f[i,1], f[i,2]), (f[i,2], f[i,0]); a face that lists
        a vertex twice takes part in no edge. An undirected edge is manifold when exactly two faces list it. Two faces are in one patch when
        a chain of manifold edges joins them: boundary edges and edges of three or more faces join nothing (what igl::bfs_orient gets from
        igl::orientable_patches, as far as their sources are remembered here; libigl was not at hand). Patches are numbered from 0 in the
        order of their smallest face. Two faces across a manifold edge agree when they run along it in opposite directions. In an orientable
        patch the face with the smallest index keeps its row and every other face is kept or reversed, (a, b, c) -> (c, b, a), so that all
        agree: what a breadth-first search from the first face of each patch produces, and unique.
        One difference from the reference: where no such assignment exists (a Moebius band) its output depends on its queue order; here
        every face of that patch is returned unchanged, and last_stats()["n_escalated"] is the number of such patches (0: every patch was
        oriented). Equal arguments give equal bytes. For a tensor the call reads f.max() back first.
        ValueError: a dtype other than the four integer types, zero rows or a second dimension other than 3 (the reference's texts), more
        than 2**27 - 16 rows, a negative index, an index above 2**31 - 17.
    """
    _check_face_dtype(f)
    sf = _shape2(f if _is_torch(f) else np.asarray(f))
    if sf[0] == 0:
        raise ValueError(f"Invalid input faces with zero elements: f must have shape (n, 3) where n > 0. Got f.shape =({sf[0]}, {sf[1]}).")
    if sf[1] != 3:
        raise ValueError(f"Only triangle inputs are supported: f must have shape (n, 3) where n > 0. Got f.shape =({sf[0]}, {sf[1]}).")
    _check_rows(sf[0])
    nf = sf[0]
    if not _is_torch(f):
        fa = np.asarray(f)
        if fa.dtype.kind == "i" and int(fa.min()) < 0:
            raise ValueError(f"f must hold row indices of v: found a face index outside [0, {max(int(fa.max()), -1) + 1})")
    top = int(f.max())
    if top < 0:
        raise ValueError("f must hold row indices of v: found a face index outside [0, 0)")
    if top >= _MAX_INDEX:
        raise ValueError("face indices above 2^31-17 are not supported")
    d = _Dev(f, f)
    ff = _beside(d, f)
    name = _face_dtype_name(ff)
    dt = np.dtype(name)
    oriented, comps = _int_out(d, (nf, 3), dt), _int_out(d, (nf,), dt)
    count = ctypes.c_int64(0)
    _call("orient_mesh_faces", d, _Dev.ptr(ff), nf, _FACE_KINDS[name], top + 1, _Dev.ptr(oriented), _Dev.ptr(comps), ctypes.addressof(count), suffix=False)
    return oriented, comps
