"""decimate_triangle_mesh: the reference's binding (src/mesh_decimate.cpp:23-66) over the HIP kernels of csrc/decimate.h. Same arguments,
default, dtypes and return order; the values follow this library's stated contract where the reference reaches
igl::decimate, which was not at hand."""
import ctypes

import numpy as np

from ._call import _Dev, _FACE_KINDS, _call, _is_torch, _take
from ._checks import _beside, _check_mesh, _face_dtype_name

_NON_MANIFOLD = "decimate_triangle_mesh_doc produced an empty mesh. This can happen if the input is non-manifold."
_TWICE = "f must not hold a face that lists a vertex twice"


def _host_face_checks(fa, nv):
    """For host arrays, what the library checks on the device: before any device work."""
    if (fa.dtype.kind == "i" and int(fa.min()) < 0) or int(fa.max()) >= nv:
        raise ValueError(f"f must hold row indices of v: found a face index outside [0, {nv})")
    a, b, c = fa[:, 0], fa[:, 1], fa[:, 2]
    if bool(((a == b) | (b == c) | (a == c)).any()):
        raise ValueError(_TWICE)
    x, y = fa.reshape(-1).astype(np.uint64), fa[:, [1, 2, 0]].reshape(-1).astype(np.uint64)
    _, count = np.unique(np.minimum(x, y) * np.uint64(nv) + np.maximum(x, y), return_counts=True)
    if int(count.max()) > 2:
        raise ValueError(_NON_MANIFOLD)


def decimate_triangle_mesh(v, f, max_faces, decimation_heuristic="shortest_edge"):
    """
    Decimate a (manifold) triangle mesh by collapsing edges

    Args:
        v : (#v, 3)-shaped array of mesh vertex positions (float32 or float64; numpy, or a CUDA/HIP torch tensor)
        f : (#f, 3)-shaped array of triangle face indices (int32, int64, uint32 or uint64; int32 / int64 for torch)
        max_faces : The maximum number of faces in the decimated output mesh (must be between 0 and #f)
        decimation_heuristic : Which decimation heuristic to use. Currently only supports "shortest_edge".

    Returns:
        v_out : (#v_out, 3)-shaped array of vertex positions for the decimated mesh, in v's dtype
        f_out : (#f_out, 3)-shaped array of triangle face indices for the decimated mesh
        v_correspondences : (#v_out,)-shaped array where v_correspondences[i] is the index of the vertex in v which generated v_out[i]
        f_correspondences : (#f_out,)-shaped array where f_correspondences[i] is the index of the face in f which generated f_out[i]
        (the last three in f's dtype; all four on the side the inputs came from)

    Notes:
        The two correspondences are one-dimensional, like the maps of remove_unreferenced_mesh_vertices; the reference's docstring says
        (n, 1). v[v_correspondences] and f[f_correspondences] work with both.
        The contract (executable in tests/decimate_contract.py) is a round-synchronous shortest-edge collapse, not
        igl::decimate's sequential queue. Per round: the distinct edges (lo, hi) in lexicographic order; the cost of one is its squared
        length computed in double and rounded to float32, its key (cost, rank). An edge is valid when its cost is finite and it passes the
        link condition on the mesh closed by one virtual vertex over all boundary edges: lo and hi have exactly two common neighbours and
        no face of hi lands on an existing face. Every valid edge claims lo, hi and their neighbours by the smaller key; an edge that
        holds all its claims collapses: lo moves to the midpoint, computed in v's dtype, hi becomes lo, the one or two faces on the edge
        go. In the last round the winners are taken in key order until max_faces is met, so the result has max_faces or max_faces - 1
        faces. Where no valid edge is left (a tetrahedron, an isolated triangle) the mesh comes back with more faces, without an error, as
        igl::decimate ends when it runs out of collapsible edges. Normal flips are not tested; igl's shortest-edge heuristic does not test
        them either. Faces keep their input order and orientation; vertices that no output face lists are dropped, so max_faces == #f
        only compacts. Edges with a NaN or infinite end, or whose squared length overflows float32, never collapse.
        last_stats(): n_queries = #f, n_passes = the rounds that collapsed an edge, n_escalated = the collapses. Equal arguments give
        equal bytes.
        ValueError: the dtype, shape and row-limit checks of the other mesh operators; "max_faces must be greater than 0, got N.";
        "max_faces must be less than or equal to the number of input faces (#f), got N."; "Invalid decimation heuristic, must be
        'shortest_edge'. ..." (the reference's texts); a face index outside [0, #v); a face that lists a vertex twice; an undirected
        edge listed by more than two faces ("decimate_triangle_mesh_doc produced an empty mesh. This can happen if the input is
        non-manifold.", what the reference raises when igl::decimate returns nothing). The last three are found on the host for numpy
        input, before any device work, and on the device for tensors.
    """
    _, nv, nf = _check_mesh(v, f)
    max_faces = int(max_faces)
    if max_faces <= 0:
        raise ValueError(f"max_faces must be greater than 0, got {max_faces}.")
    if max_faces > nf:
        raise ValueError(f"max_faces must be less than or equal to the number of input faces ({nf}), got {max_faces}.")
    if decimation_heuristic != "shortest_edge":
        raise ValueError("Invalid decimation heuristic, must be 'shortest_edge'. Others will be implemented in future versions of Point Cloud Utils.")
    if not (_is_torch(v) or _is_torch(f)):
        _host_face_checks(np.asarray(f), nv)
    d = _Dev(v, v)
    ff = _beside(d, f)
    name = _face_dtype_name(ff)
    dt = np.dtype(name)
    out_nv, out_nf = ctypes.c_int64(0), ctypes.c_int64(0)
    _call("decimate_triangle_mesh", d, d.pa, nv, _Dev.ptr(ff), nf, _FACE_KINDS[name], max_faces, ctypes.addressof(out_nv), ctypes.addressof(out_nf))
    mv, mf = int(out_nv.value), int(out_nf.value)
    v_out, f_out, corr_v, corr_f = _take("decimate_triangle_mesh", d, [((mv, 3), d.np_dtype), ((mf, 3), dt), ((mv,), dt), ((mf,), dt)], mv, mf)
    return v_out, f_out, corr_v, corr_f
