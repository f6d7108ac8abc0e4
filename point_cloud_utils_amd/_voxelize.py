"""voxelize_triangle_mesh, sparse_voxel_grid_boundary and voxel_grid_geometry: the reference's callables (point_cloud_utils/_voxels.py:33-54,
src/sparse_voxel_grid.cpp:473-522, point_cloud_utils/_point_cloud_geometry.py:45-63) over the HIP kernels of csrc/voxelize.h. Same arguments,
defaults, dtypes and return order; the voxelization follows this library's stated contract: the reference's overlap test
bit for bit, its candidate loop over all three axes instead of the first x column only."""
import ctypes

import numpy as np

from ._call import _Dev, _FACE_KINDS, _call, _int_out, _is_torch, _plain, _shape2, _take
from ._checks import _check_mesh, _mesh_args, _resolve

_RANGE = 2 ** 20                       # voxel coordinates live in [-2^20, 2^20): the 21 bits per axis of a 64-bit Morton code
_INT32_MAX = 2 ** 31 - 1
_OVERFLOW = "Invalid vertex leads to an overflow integer. Perhaps grid_size is too small."


def _coord3d(coord):
    """_coord3d_to_array (point_cloud_utils/_point_cloud_geometry.py:7-14) to float64, for lists, tuples, numpy arrays and tensors."""
    if not hasattr(coord, "__len__") or len(coord) != 3:
        raise ValueError("Invalid shape")
    try:
        return np.array([float(c) for c in coord], dtype=np.float64)
    except (TypeError, ValueError):
        raise ValueError("Invalid shape") from None


def _number_or_coord3d(x):
    if isinstance(x, (float, int, np.floating, np.integer)) and not isinstance(x, bool):
        return np.array([float(x)] * 3, dtype=np.float64)
    return _coord3d(x)


def _grid(voxel_size, voxel_origin, size_text):
    """(size, origin) as float64 triples, checked: the shapes first, then the sign of the size, then finiteness."""
    origin = _coord3d(voxel_origin)
    size = _number_or_coord3d(voxel_size)
    if not bool((size > 0.0).all()):
        raise ValueError(size_text)
    if not (bool(np.isfinite(size).all()) and bool(np.isfinite(origin).all())):
        raise ValueError("voxel_size and voxel_origin must be finite")
    return size, origin


def _triple(a):
    return (ctypes.c_double * 3)(*[float(x) for x in a])


def _check_ijk(ijk, name, zero_text, shape_text):
    """dtype, rows and columns of an (n, 3) integer array. Returns (kind, n)."""
    dn = str(ijk.dtype).replace("torch.", "") if _is_torch(ijk) else np.asarray(ijk).dtype.name
    kinds = ["int32", "int64"] if _is_torch(ijk) else list(_FACE_KINDS)
    if dn not in kinds:
        raise ValueError(f"Invalid scalar type ({dn}) for argument '{name}'. Expected one of {kinds}.")
    sh = _shape2(ijk)
    if sh[0] == 0:
        raise ValueError(zero_text.format(sh[0], sh[1]))
    if sh[1] != 3:
        raise ValueError(shape_text.format(sh[0], sh[1]))
    return _FACE_KINDS[dn], sh[0]


def voxelize_triangle_mesh(v, f, voxel_size, voxel_origin):
    """
    Return ijk coordinates of voxels which intersect the given mesh.
    Each voxel is assumed to have size voxel_size (scalar or triple of floats) and the (0, 0, 0) voxel has its CENTRE at voxel_origin.

    Args:
        v : [num_vertices, 3] array of triangle mesh vertices (float32 or float64; numpy, or a CUDA/HIP torch tensor)
        f : [num_faces, 3] array of face indexes into v (int32, int64, uint32 or uint64; int32 / int64 for torch)
        voxel_size: A float or triple specifying the size of each voxel
        voxel_origin: A triple specifying the position of the centre of the (0, 0, 0) voxel

    Returns:
        ijk: [num_vox, 3] int32 array of integer ijk coordinates for each voxel intersecting the mesh, ascending by 64-bit Morton code

    Notes:
        The contract: voxel ijk is the box with centre voxel_origin + ijk * voxel_size and half size voxel_size / 2 -- what
        the reference's code does, although its docstring says "bottom-back-left corner". A face's candidates are the boxes lo..hi on all
        three axes, lo = floor((min - origin) / size), hi = ceil((max - origin) / size) over its corners; one is kept iff the reference's
        triangle-box test (Akenine-Moller's separating axes, evaluated in double in the reference's operation order, touching counts) says
        so. The reference's loop visits only the first x column of every face's candidates (3,388 of the bunny's 15,277 voxels at 64 across);
        that is not reproduced: the reference's rows are a subset of these. Draw the result with
        voxel_grid_geometry(ijk, voxel_size, voxel_origin - voxel_size / 2). Equal arguments give equal bytes.
        ValueError: the mesh checks of the other mesh operators; a voxel_size or voxel_origin that is not a triple ("Invalid shape"), a size
        that is not > 0 ("Invalid voxel size") or not finite; a candidate coordinate outside [-2**20, 2**20); more than 2**32 candidates in
        all (a chosen cap, so that one huge face on a fine grid cannot hold the GPU for minutes).
    """
    origin = _coord3d(voxel_origin)
    size = _number_or_coord3d(voxel_size)
    _check_mesh(v, f)
    size, origin = _grid(size, origin, "Invalid voxel size")
    d, ff, nv, nf = _resolve(v, f)
    cs, co = _triple(size), _triple(origin)
    rows = ctypes.c_int64(0)
    _call("voxelize_triangle_mesh", d, *_mesh_args(d, ff, nv, nf), ctypes.addressof(cs), ctypes.addressof(co), ctypes.addressof(rows))
    m = int(rows.value)
    return _take("voxelize", d, [((m, 3), np.int32)], m)[0]


def sparse_voxel_grid_boundary(grid_coordinates):
    """
    Find the voxels of a sparse voxel grid that lie on its boundary: those that lack at least one of their six face neighbours.

    Args:
        grid_coordinates : An (n, 3) shaped integer array of voxel coordinates (int32, int64, uint32 or uint64; int32 / int64 for torch;
                           numpy, or a CUDA/HIP torch tensor)

    Returns:
        boundary_voxels : An (m,) shaped int64 array of ascending indices into grid_coordinates encoding which voxels lie on the boundary

    Notes:
        Duplicated rows are allowed and each is judged like the others. Coordinates live in [-2**20, 2**20) (64-bit Morton codes): a neighbour
        beyond that range is absent, a coordinate beyond it raises ValueError (the reference has undefined behaviour there). Zero rows and
        a second dimension other than 3 raise ValueError with the reference's texts.
    """
    kind, n = _check_ijk(grid_coordinates, "grid_coordinates", "Invalid grid_coordinates has zero rows!",
                         "Invalid shape for grid_coordinates must have shape (N, 3) but got ({}, {})")
    if n > _INT32_MAX - 15:
        raise ValueError("voxel grids with more than 2^31-16 rows are not supported")
    if not _is_torch(grid_coordinates):
        g = np.asarray(grid_coordinates)
        if (g.dtype.kind == "i" and int(g.min()) < -_RANGE) or int(g.max()) >= _RANGE:
            raise ValueError(_OVERFLOW)
    d = _Dev(grid_coordinates, grid_coordinates)
    idx = d.empty((n,), "i64")
    cnt = ctypes.c_int64(0)
    _plain("sparse_voxel_grid_boundary", d.ctx, d.pa, n, kind, _Dev.ptr(idx), ctypes.addressof(cnt), d.flags, d.stream)
    m = int(cnt.value)
    idx = idx[:m]
    if n > 2 * m:                                          # (do not keep the grid's room alive behind a small result)
        idx = idx.clone() if d.torch else idx.copy()
    return idx


def voxel_grid_geometry(ijk, voxel_size=np.array((1., 1., 1.)), voxel_origin=np.array((0., 0., 0.)), gap_fraction=0.0):
    """
    Generate a triangle mesh of cubes for voxel coordinates ijk. The [0, 0, 0] voxel has its CORNER at voxel_origin and each voxel has
    voxel_size.

    Args:
        ijk : [num_voxels, 3] array of integer voxel coordinates (int32, int64, uint32 or uint64; int32 / int64 for torch)
        voxel_size: Float or triple representing the size of each voxel. Defaults to (1, 1, 1).
        voxel_origin: Coordinate of the low corner of the [0, 0, 0] voxel. Defaults to (0, 0, 0).
        gap_fraction: Fraction of a voxel to leave as a gap between voxels (default 0.0)

    Returns:
        v: float32 array of shape (8 * num_voxels, 3): the vertices of the cube mesh
        f: int32 array of shape (12 * num_voxels, 3): the faces of the cube mesh

    Notes:
        vertex = ((unit * (1 - gap_fraction) + 0.5 * gap_fraction) + ijk) * voxel_size + voxel_origin in double, operation by operation,
        rounded once to float32, with the reference's eight unit corners and twelve triangles (face indices: corner + 8 * row). As in the
        reference's code (whose docstring says "center"), voxel (0, 0, 0) spans voxel_origin .. voxel_origin + voxel_size: the voxels of
        voxelize_triangle_mesh(v, f, s, o), which are centred on o + ijk * s, are drawn with voxel_origin = o - s / 2.
        ValueError: zero rows, a non-positive size ("Voxel size must be positive"), a size or origin that is not a triple ("Invalid shape"),
        more than (2**31 - 1) / 8 voxels.
    """
    origin = _coord3d(voxel_origin)
    size = _number_or_coord3d(voxel_size)
    kind, n = _check_ijk(ijk, "ijk", "Invalid input point cloud with zero points: points must have shape (n, 3) (n > 0). Got points.shape =({}, {}).",
                         "Only 3D inputs are supported: v must have shape (n, 3) (n > 0). Got points.shape =({}, {}).")
    size, origin = _grid(size, origin, "Voxel size must be positive")
    if 8 * n > _INT32_MAX:
        raise ValueError("voxel geometry with more than 2^31-1 vertices does not fit the int32 faces")
    gap = float(gap_fraction)
    d = _Dev(ijk, ijk)
    v, f = _int_out(d, (8 * n, 3), np.float32), _int_out(d, (12 * n, 3), np.int32)
    cs, co = _triple(size), _triple(origin)
    _plain("voxel_grid_geometry", d.ctx, d.pa, n, kind, ctypes.addressof(cs), ctypes.addressof(co), gap, _Dev.ptr(v), _Dev.ptr(f), d.flags, d.stream)
    return v, f
