"""connected_components and flood_fill_3d: the reference's callables (src/connected_components.cpp:11-110, point_cloud_utils/_voxels.py:7-30 over
src/flood_fill_3d.cpp:10-75) over the HIP union-find of csrc/components.h. Same arguments, dtypes and return order; both follow this
library's stated contract, which differs from the reference's loops where the Notes below say so."""
import ctypes
import operator

import numpy as np

from ._call import _Dev, _FACE_KINDS, _call, _int_out, _is_torch, _shape2
from ._checks import _beside, _check_mesh, _face_dtype_name

_MAX_CELLS = 2 ** 31 - 16
_GRID_KINDS = {"int32": 0, "int64": 1, "float32": 2, "float64": 3}


def connected_components(v, f):
    """
    Determine the connected components of a mesh

    Args:
        v : (#v, 3)-shaped array of mesh vertex positions (float32 or float64; numpy, or a CUDA/HIP torch tensor). Only its row count is used.
        f : (#f, 3)-shaped array of mesh face indexes into v (int32, int64, uint32 or uint64; int32 / int64 for torch)

    Returns:
        cv : a (#v,)-shaped array of integer indexes (starting from 0): cv[i] is the component of the vertex v[i]
        nv : the number of vertices in each connected component: nv[j] is the number of vertices in component j
        cf : a (#f,)-shaped array of integer indexes (starting from 0): cf[i] is the component of the face f[i]
        nf : the number of faces in each connected component: nf[j] is the number of faces in component j
        (all four 1-D, in f's dtype, on the side the inputs came from)

    Notes:
        The contract: two vertices are connected when a face lists both -- one shared vertex joins two faces, a shared edge
        is not needed. Components are numbered from 0 in the order of their smallest vertex index, which is what the reference's ascending
        outer loop with one breadth-first search per unvisited vertex produces. cf[i] = cv[f[i, 0]]. A vertex that no face lists is a
        component of its own with nf = 0. Equal arguments give equal bytes.
        One difference from the reference: it sizes its adjacency matrix with libigl's adjacency_matrix, which (as far as its source is
        remembered here; it was not at hand) has f.max() + 1 rows, so the reference's cv is shorter than v when the last vertices are not
        referenced. Here cv always has #v rows, as the reference's docstring promises; the reference's rows are a prefix of these.
        ValueError: the dtype, shape and row-limit checks of the other mesh operators (more than 2**27 - 16 rows), a face index outside
        [0, #v). v's coordinates are never read: non-finite ones are not an error here.
    """
    _check_mesh(v, f)
    nv, nf = _shape2(v)[0], _shape2(f)[0]
    if not (_is_torch(v) or _is_torch(f)):
        fa = np.asarray(f)
        if (fa.dtype.kind == "i" and int(fa.min()) < 0) or int(fa.max()) >= nv:
            raise ValueError(f"f must hold row indices of v: found a face index outside [0, {nv})")
    d = _Dev(v, v)
    ff = _beside(d, f)
    name = _face_dtype_name(ff)
    cv, cf, cnv, cnf = (_int_out(d, (n,), np.dtype(name)) for n in (nv, nf, nv, nv))
    count = ctypes.c_int64(0)
    _call("connected_components", d, _Dev.ptr(ff), nf, _FACE_KINDS[name], nv, _Dev.ptr(cv), _Dev.ptr(cf), _Dev.ptr(cnv), _Dev.ptr(cnf),
          ctypes.addressof(count), suffix=False)
    m = int(count.value)
    cnv, cnf = cnv[:m], cnf[:m]
    if nv > 2 * m:                                         # (do not keep #v rows alive behind a few counts)
        cnv, cnf = (cnv.clone(), cnf.clone()) if d.torch else (cnv.copy(), cnf.copy())
    return cv, cnv, cf, cnf


def _coord3i(coord):
    """A triple of integers, for lists, tuples, numpy arrays and tensors; "Invalid shape" as _voxelize._coord3d gives otherwise."""
    if not hasattr(coord, "__len__") or len(coord) != 3:
        raise ValueError("Invalid shape")
    out = []
    for c in coord:
        try:
            out.append(operator.index(c))
        except TypeError:
            try:
                x = float(c)
            except (TypeError, ValueError):
                raise ValueError("Invalid shape") from None
            if x != x or x in (float("inf"), float("-inf")) or x != int(x):
                raise ValueError("Invalid shape") from None
            out.append(int(x))
    return out


def flood_fill_3d(grid, start_coord, fill_value):
    """
    Flood fill a 3D grid starting from start_coord with fill_value. This will return a copy of grid where the region in the input grid which
    is connected to start_coord and shares the value of start_coord is set to fill_value.

    Args:
        grid : [w, h, d] array of scalars as input to the flood fill (int32, int64, float32 or float64; a numpy array in any memory order,
               or a CUDA/HIP torch tensor). It is never modified.
        start_coord : (i, j, k) integer coordinate to start the flood fill
        fill_value : scalar value to flood fill

    Returns:
        A flood filled copy of grid where all voxels which are connected to start_coord are set to fill_value (numpy for numpy, a tensor on
        the same device for a tensor)

    Notes:
        The contract: the cells changed are those that == the seed cell's value (C++'s ==: -0.0 matches 0.0, and a NaN seed
        matches nothing, so the copy comes back unchanged) and are joined to the seed through the six face neighbours inside the grid.
        fill_value goes through float(fill_value) to double and then to grid's dtype, as the reference's cast does (an int64 fill beyond
        2**53 rounds the same way). A numpy grid is read as np.ascontiguousarray gives it.
        Two differences from the reference's loop. It computes neighbour offsets from (x +- 1, y +- 1, z +- 1) and only checks
        0 <= offset < size, so its +z neighbour of (x, y, d-1) is (x, y+1, 0); that leak across rows is not reproduced (on [[[1, 0], [0, 1]]]
        with seed (0, 0, 1) the reference fills two cells, this contract one). And with fill_value == the seed's value the reference never
        terminates (filled cells still match and are queued again); here the unchanged copy is returned.
        The work is four kernel launches whatever the region's shape. ValueError: a start_coord that is not a triple of integers ("Invalid
        shape"), grid.ndim != 3 ("grid must have shape [w, h, d]"), an unsupported dtype, a seed outside the grid or a zero-sized axis
        ("seed point must be inside grid"), more than 2**31 - 16 cells.
    """
    seed = _coord3i(start_coord)
    if not _is_torch(grid):
        grid = np.asarray(grid)
    sizes = tuple(int(s) for s in grid.shape)
    if len(sizes) != 3:
        raise ValueError("grid must have shape [w, h, d]")
    dn = str(grid.dtype).replace("torch.", "") if _is_torch(grid) else grid.dtype.name
    if dn not in _GRID_KINDS:
        raise ValueError(f"Invalid scalar type ({dn}) for argument 'grid'. Expected one of {list(_GRID_KINDS)}.")
    if any(not 0 <= c < s for c, s in zip(seed, sizes)):
        raise ValueError("seed point must be inside grid")
    if sizes[0] * sizes[1] * sizes[2] > _MAX_CELLS:
        raise ValueError("grids with more than 2^31-16 cells are not supported")
    fill = float(fill_value)
    d = _Dev(grid, grid)                                   # (contiguous: a copy only where the input is not)
    if d.torch:
        import torch
        out = torch.empty(sizes, dtype=grid.dtype, device=d.tdev)
    else:
        out = np.empty(sizes, dtype=grid.dtype)
    seed3 = (ctypes.c_int64 * 3)(*seed)
    filled = ctypes.c_int64(0)
    _call("flood_fill_3d", d, d.pa, _Dev.ptr(out), sizes[0], sizes[1], sizes[2], ctypes.addressof(seed3), _GRID_KINDS[dn], fill, ctypes.addressof(filled),
          suffix=False)
    return out
