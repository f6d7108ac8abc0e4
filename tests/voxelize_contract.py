"""The contract of voxelize_triangle_mesh, sparse_voxel_grid_boundary and voxel_grid_geometry (csrc/voxelize.h), restated
in numpy. float64 arithmetic, every operation rounded on its own, in the order the reference's triangle-box test evaluates it; the GPU tests
compare the library with these functions row for row."""
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
SLICE = 2048                  # candidate ranks per block of the library's test pass (csrc/voxelize.h: kVxSlice)
SC_TILE = 4096                # the tile of the library's inclusive scan (csrc/radix.h: kScTile)
RANGE = 2 ** 20               # voxel coordinates live in [-2^20, 2^20)
MAX_CANDIDATES = 2 ** 32      # the candidate cap of one call (csrc/voxelize.h: kVxMaxCandidates)


def golden_mesh(name, dtype):
    v = np.load(os.path.join(GOLDEN, f"{name}_v.npy")).astype(dtype)
    f = np.load(os.path.join(GOLDEN, f"{name}_f.npy")).astype(np.int64)
    return np.ascontiguousarray(v), np.ascontiguousarray(f)


# ---- Morton order (MortonCode64: 21 bits per axis, x lowest, the three sign bits inverted)
def _split21(r):
    r = r.astype(np.uint64)
    r = (r | r << np.uint64(32)) & np.uint64(0x1f00000000ffff)
    r = (r | r << np.uint64(16)) & np.uint64(0x1f0000ff0000ff)
    r = (r | r << np.uint64(8)) & np.uint64(0x100f00f00f00f00f)
    r = (r | r << np.uint64(4)) & np.uint64(0x10c30c30c30c30c3)
    r = (r | r << np.uint64(2)) & np.uint64(0x1249249249249249)
    return r


def morton(ijk):
    """64-bit codes of (n, 3) integer coordinates in [-2^20, 2^20): unsigned order of the codes follows the coordinates' interleaved bits."""
    u = (np.asarray(ijk).astype(np.int64) & 0x1fffff).astype(np.uint64)         # 21-bit two's complement
    code = _split21(u[:, 0]) | _split21(u[:, 1]) << np.uint64(1) | _split21(u[:, 2]) << np.uint64(2)
    return code ^ np.uint64(0x7000000000000000)


# ---- 1. the overlap test
def tribox(centre, half, tri):
    """centre (n, 3), half (3,) or (n, 3), tri (n, 3, 3): corner j of triangle i is tri[i, j]. Returns (n,) bool."""
    c = np.asarray(centre, dtype=np.float64)
    h = np.broadcast_to(np.asarray(half, dtype=np.float64), c.shape)
    t = np.asarray(tri, dtype=np.float64)
    v0, v1, v2 = t[:, 0] - c, t[:, 1] - c, t[:, 2] - c
    e0, e1, e2 = v1 - v0, v2 - v1, v0 - v2
    X, Y, Z = 0, 1, 2

    def apart(pa, pb, rad):
        mn, mx = np.where(pa < pb, pa, pb), np.where(pa < pb, pb, pa)
        return (mn > rad) | (mx < -rad)

    def ax(e, p, q):
        a, b = e[:, Z], e[:, Y]
        return apart(a * p[:, Y] - b * p[:, Z], a * q[:, Y] - b * q[:, Z], np.abs(e[:, Z]) * h[:, Y] + np.abs(e[:, Y]) * h[:, Z])

    def ay(e, p, q):
        a, b = e[:, Z], e[:, X]
        return apart(-a * p[:, X] + b * p[:, Z], -a * q[:, X] + b * q[:, Z], np.abs(e[:, Z]) * h[:, X] + np.abs(e[:, X]) * h[:, Z])

    def az(e, p, q):
        a, b = e[:, Y], e[:, X]
        return apart(a * p[:, X] - b * p[:, Y], a * q[:, X] - b * q[:, Y], np.abs(e[:, Y]) * h[:, X] + np.abs(e[:, X]) * h[:, Y])

    out = ax(e0, v0, v2) | ay(e0, v0, v2) | az(e0, v1, v2)
    out |= ax(e1, v0, v2) | ay(e1, v0, v2) | az(e1, v0, v1)
    out |= ax(e2, v0, v1) | ay(e2, v0, v1) | az(e2, v1, v2)
    for k in (X, Y, Z):
        mn = np.minimum(np.minimum(v0[:, k], v1[:, k]), v2[:, k])
        mx = np.maximum(np.maximum(v0[:, k], v1[:, k]), v2[:, k])
        out |= (mn > h[:, k]) | (mx < -h[:, k])
    n = np.stack([e0[:, Y] * e1[:, Z] - e0[:, Z] * e1[:, Y], e0[:, Z] * e1[:, X] - e0[:, X] * e1[:, Z], e0[:, X] * e1[:, Y] - e0[:, Y] * e1[:, X]], axis=1)
    pos = n > 0.0
    lo = np.where(pos, -h - v0, h - v0)
    hi = np.where(pos, h - v0, -h - v0)
    dlo = (n[:, 0] * lo[:, 0] + n[:, 1] * lo[:, 1]) + n[:, 2] * lo[:, 2]
    dhi = (n[:, 0] * hi[:, 0] + n[:, 1] * hi[:, 1]) + n[:, 2] * hi[:, 2]
    out |= dlo > 0.0
    out |= ~(dhi >= 0.0)
    return ~out


# ---- 2. candidates
def _grid(voxel_size, voxel_origin):
    size = np.asarray(voxel_size, dtype=np.float64) * np.ones(3)
    return size, np.asarray(voxel_origin, dtype=np.float64)


def candidates(v, f, voxel_size, voxel_origin):
    """(lo, hi): per face the integer boxes lo..hi on every axis. ValueError outside [-2^20, 2^20) or above the cap."""
    size, origin = _grid(voxel_size, voxel_origin)
    t = np.asarray(v, dtype=np.float64)[np.asarray(f).astype(np.int64)]         # (nf, 3 corners, 3 axes)
    lo = np.floor((t.min(axis=1) - origin) / size)
    hi = np.ceil((t.max(axis=1) - origin) / size)
    if not bool(((lo >= -RANGE) & (hi < RANGE)).all()):
        raise ValueError("a voxel coordinate outside [-2^20, 2^20)")
    lo, hi = lo.astype(np.int64), hi.astype(np.int64)
    counts = [int(a) * int(b) * int(c) for a, b, c in (hi - lo + 1)]
    if sum(counts) > MAX_CANDIDATES:
        raise ValueError("more than 2^32 candidate voxels")
    return lo, hi


def candidate_count(v, f, voxel_size, voxel_origin):
    lo, hi = candidates(v, f, voxel_size, voxel_origin)
    return int((hi - lo + 1).prod(axis=1).sum())


# ---- 3. the voxelization
def kept_pairs(v, f, voxel_size, voxel_origin, x_first_only=False):
    """(face, ijk, verdict) of every candidate in the library's rank order: faces in order, x outermost and z innermost within a face.
    x_first_only: the reference's loop, which visits the first x column of every face only."""
    size, origin = _grid(voxel_size, voxel_origin)
    f = np.asarray(f).astype(np.int64)
    lo, hi = candidates(v, f, voxel_size, voxel_origin)
    n = hi - lo + 1
    if x_first_only:
        n[:, 0] = 1
    cnt = n.prod(axis=1)
    C = np.cumsum(cnt)
    face = np.repeat(np.arange(len(f)), cnt)
    local = np.arange(int(C[-1])) - (C - cnt)[face]
    iz = local % n[face, 2]
    t = local // n[face, 2]
    ijk = np.stack([lo[face, 0] + t // n[face, 1], lo[face, 1] + t % n[face, 1], lo[face, 2] + iz], axis=1)
    centre = origin + ijk.astype(np.float64) * size
    tri = np.asarray(v, dtype=np.float64)[f[face]]
    return face, ijk, tribox(centre, size / 2, tri)


def voxelize(v, f, voxel_size, voxel_origin, x_first_only=False):
    """(m, 3) int32: the kept ijk, each once, ascending by Morton code."""
    _, ijk, yes = kept_pairs(v, f, voxel_size, voxel_origin, x_first_only)
    ijk = ijk[yes]
    code, first = np.unique(morton(ijk), return_index=True)
    return np.ascontiguousarray(ijk[first].astype(np.int32))


# ---- 4. the boundary of a sparse grid
def boundary(ijk):
    """Ascending rows whose voxel lacks one of its six face neighbours among the rows; a neighbour outside [-2^20, 2^20) is absent."""
    rows = [tuple(int(x) for x in r) for r in np.asarray(ijk)]
    for r in rows:
        if not all(-RANGE <= x < RANGE for x in r):
            raise ValueError("Invalid vertex leads to an overflow integer. Perhaps grid_size is too small.")
    have = set(rows)
    out = []
    for i, (x, y, z) in enumerate(rows):
        for q in ((x + 1, y, z), (x - 1, y, z), (x, y + 1, z), (x, y - 1, z), (x, y, z + 1), (x, y, z - 1)):
            if not all(-RANGE <= c < RANGE for c in q) or q not in have:
                out.append(i)
                break
    return np.array(out, dtype=np.int64)


# ---- 5. the cubes
UNIT = np.array([[0, 0, 1], [1, 0, 1], [0, 1, 1], [1, 1, 1], [0, 0, 0], [1, 0, 0], [0, 1, 0], [1, 1, 0]], dtype=np.float64)
CUBE = np.array([[2, 7, 6], [2, 3, 7], [0, 4, 5], [0, 5, 1], [0, 2, 6], [0, 6, 4], [1, 7, 3], [1, 5, 7], [0, 3, 2], [0, 1, 3], [4, 6, 7], [4, 7, 5]],
                dtype=np.int32)


def geometry(ijk, voxel_size=(1.0, 1.0, 1.0), voxel_origin=(0.0, 0.0, 0.0), gap_fraction=0.0):
    """(8n, 3) float32 vertices, (12n, 3) int32 faces."""
    size, origin = _grid(voxel_size, voxel_origin)
    gap = np.float64(gap_fraction)
    c = np.asarray(ijk).astype(np.float64)
    u = UNIT * (1.0 - gap) + 0.5 * gap
    vert = u[None, :, :] + c[:, None, :]
    vert = vert * size
    vert = vert + origin
    n = len(c)
    faces = CUBE[None, :, :] + (8 * np.arange(n, dtype=np.int32))[:, None, None]
    return np.ascontiguousarray(vert.reshape(8 * n, 3).astype(np.float32)), np.ascontiguousarray(faces.reshape(12 * n, 3).astype(np.int32))


def inside_boxes(p, ijk, voxel_size, voxel_origin):
    """Which points p (n, 3) lie in the closed box of at least one voxel of ijk (centres origin + ijk * size). Exact in the indices: a
    point is tried against the voxels around its rounded index."""
    size, origin = _grid(voxel_size, voxel_origin)
    have = set(tuple(int(x) for x in r) for r in np.asarray(ijk))
    p = np.asarray(p, dtype=np.float64)
    base = np.rint((p - origin) / size).astype(np.int64)
    out = np.zeros(len(p), dtype=bool)
    for dx in (-1, 0, 1):
        for dy in (-1, 0, 1):
            for dz in (-1, 0, 1):
                q = base + np.array([dx, dy, dz])
                centre = origin + q.astype(np.float64) * size
                hit = (np.abs(p - centre) <= size / 2).all(axis=1)
                if hit.any():
                    has = np.fromiter((tuple(r) in have for r in q[hit].tolist()), dtype=bool, count=int(hit.sum()))
                    idx = np.nonzero(hit)[0]
                    out[idx[has]] = True
    return out
