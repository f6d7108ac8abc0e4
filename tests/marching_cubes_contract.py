"""The contract of marching_cubes_sparse_voxel_grid and sparse_voxel_grid_to_hex_mesh (csrc/marching_cubes.h), restated in
numpy: the rule that generates the case table, the surface with its vertex and face order, the hex mesh as sets and dicts. Arithmetic in the
dtype of the coordinates, every operation rounded on its own; the GPU tests compare the library with these functions bit for bit."""
import collections
import importlib.util
import os

import numpy as np

import voxelize_contract as vc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "point_cloud_utils_amd", "csrc")
RANGE = vc.RANGE

# corner c of a cube, as offsets along (x, y, z); edge e joins the corners EDGES[e]; the faces as corner cycles, counter-clockwise from outside
CORNERS = np.array([[0, 0, 0], [1, 0, 0], [1, 1, 0], [0, 1, 0], [0, 0, 1], [1, 0, 1], [1, 1, 1], [0, 1, 1]], dtype=np.int64)
EDGES = np.array([[0, 1], [1, 2], [2, 3], [3, 0], [4, 5], [5, 6], [6, 7], [7, 4], [0, 4], [1, 5], [2, 6], [3, 7]], dtype=np.int64)
FACES = [[3, 0, 4, 7], [5, 1, 2, 6], [4, 0, 1, 5], [6, 2, 3, 7], [1, 0, 3, 2], [7, 4, 5, 6]]
TABLE_SHA256 = "adcb2239f3f3693051b66260acad88e37eb439a287ca3cb5fd65b810e8775999"


def generator():
    """csrc/gen_mc_table.py as a module (it is no part of the installed package's import path)."""
    spec = importlib.util.spec_from_file_location("gen_mc_table", os.path.join(CSRC, "gen_mc_table.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


# ---- 1. the table, from the rule
def _segments(mask):
    """Directed segments (from edge, to edge) on the six faces: each maximal run of inside corners along a face's cycle is cut off by one
    segment from the edge where the walk leaves the run to the edge where it enters the run."""
    edge_of = {frozenset((int(a), int(b))): e for e, (a, b) in enumerate(EDGES)}
    inside = [bool(mask >> c & 1) for c in range(8)]
    segs = []
    for cyc in FACES:
        sign = [inside[c] for c in cyc]
        if all(sign) or not any(sign):
            continue
        for start in range(4):
            if sign[start] and not sign[start - 1]:                     # a run begins at `start` ...
                end = start
                while sign[(end + 1) % 4]:
                    end += 1                                            # ... and ends at `end`
                leave = edge_of[frozenset((cyc[end % 4], cyc[(end + 1) % 4]))]
                enter = edge_of[frozenset((cyc[start - 1], cyc[start]))]
                segs.append((leave, enter))
    return segs


def case_triangles(mask):
    succ = dict(_segments(mask))
    assert len(succ) == len(_segments(mask)), "an edge with two successors"
    todo, tris = sorted(succ), []
    while todo:
        loop, e = [todo[0]], succ[todo[0]]
        while e != loop[0]:
            loop.append(e)
            e = succ[e]
        todo = [x for x in todo if x not in loop]
        tris += [(loop[0], loop[i], loop[i + 1]) for i in range(1, len(loop) - 1)]
    return tris


def build_table():
    """(256, 16) int8: edge triples, -1 padded."""
    tab = np.full((256, 16), -1, dtype=np.int8)
    for mask in range(256):
        flat = [e for t in case_triangles(mask) for e in t]
        tab[mask, :len(flat)] = flat
    return tab


TABLE = build_table()
N_TRI = (TABLE[:, 0:15:3] >= 0).sum(axis=1)


def header_table():
    """The 256 x 16 numbers of the committed csrc/mc_table.h."""
    rows = []
    for line in open(os.path.join(CSRC, "mc_table.h")):
        line = line.strip()
        if line.startswith("{") and "}" in line:
            rows.append([int(x) for x in line[1:line.index("}")].split(",")])
    return np.array(rows, dtype=np.int8)


# ---- 2. the surface
def marching_cubes(grid_scalars, grid_coordinates, cube_indices, isovalue):
    """(v, f): v in the coordinates' dtype, rows ascending by (lo, hi); f in the cubes' dtype, cubes in input order, triangles in table order."""
    P = np.ascontiguousarray(grid_coordinates)
    T = P.dtype.type
    S = np.asarray(grid_scalars).astype(T).reshape(-1)
    C = np.asarray(cube_indices)
    idx = C.astype(np.int64)
    iso = T(isovalue)
    if not (np.isfinite(P).all() and np.isfinite(S).all() and np.isfinite(iso)):
        raise ValueError("non-finite input")
    if idx.min() < 0 or idx.max() >= len(P) or (C.dtype.kind == "u" and int(C.max()) >= len(P)):
        raise ValueError("cube index out of range")
    mask = ((S[idx] > iso).astype(np.int64) << np.arange(8)).sum(axis=1)
    cnt = N_TRI[mask]
    if cnt.sum() == 0:
        raise ValueError("No level set found for isovalue %f" % float(isovalue))
    cube = np.repeat(np.arange(len(idx)), cnt)                                          # the cube of every triangle
    local = np.arange(int(cnt.sum())) - np.repeat(np.cumsum(cnt) - cnt, cnt)            # its place in the cube's row
    edges = TABLE[mask[cube][:, None], 3 * local[:, None] + np.arange(3)].astype(np.int64)     # (#f, 3) cube edges
    a, b = idx[cube[:, None], EDGES[edges, 0]], idx[cube[:, None], EDGES[edges, 1]]
    lo, hi = np.minimum(a, b), np.maximum(a, b)
    key = lo * len(P) + hi
    uniq, inverse = np.unique(key.reshape(-1), return_inverse=True)
    ulo, uhi = uniq // len(P), uniq % len(P)
    with np.errstate(all="ignore"):
        t = (iso - S[ulo]) / (S[uhi] - S[ulo])
        v = P[ulo] + t[:, None] * (P[uhi] - P[ulo])
    assert v.dtype == P.dtype
    return np.ascontiguousarray(v), np.ascontiguousarray(inverse.reshape(-1, 3).astype(C.dtype))


# ---- 3. the hex mesh
def hex_mesh(grid_coordinates, voxel_size=1.0, origin=(0.0, 0.0, 0.0), dtype=np.float64):
    """(vertices, cubes): the unique integer corners of all voxels ascending by Morton code, positions in double rounded once to dtype;
    cubes (k, 8) int64, the rank of each corner, row for row the input."""
    rows = [tuple(int(x) for x in r) for r in np.asarray(grid_coordinates)]
    for r in rows:
        if not all(-RANGE <= x < RANGE - 1 for x in r):
            raise ValueError("Invalid vertex leads to an overflow integer. Perhaps grid_size is too small.")
    corners = set()
    for x, y, z in rows:
        for dx, dy, dz in CORNERS.tolist():
            corners.add((x + dx, y + dy, z + dz))
    verts = np.array(sorted(corners), dtype=np.int64)
    verts = verts[np.argsort(vc.morton(verts), kind="stable")]
    rank = {tuple(v): i for i, v in enumerate(verts.tolist())}
    cubes = np.array([[rank[(x + dx, y + dy, z + dz)] for dx, dy, dz in CORNERS.tolist()] for x, y, z in rows], dtype=np.int64)
    size = np.asarray(voxel_size, dtype=np.float64) * np.ones(3)
    org = np.asarray(origin, dtype=np.float64)
    pos = verts.astype(np.float64) * size
    pos = pos + org
    pos = pos - 0.5 * size
    return np.ascontiguousarray(pos.astype(dtype)), cubes


# ---- 4. what the tests measure on a surface
def dense_grid(n, lo=-1.0, hi=1.0, dtype=np.float64):
    """n^3 vertices over [lo, hi]^3 (x fastest) and the (n-1)^3 cubes in the contract's corner order."""
    ax = np.linspace(lo, hi, n)
    z, y, x = np.meshgrid(ax, ax, ax, indexing="ij")
    P = np.stack([x, y, z], axis=-1).reshape(-1, 3).astype(dtype)
    k, j, i = np.meshgrid(np.arange(n - 1), np.arange(n - 1), np.arange(n - 1), indexing="ij")
    base = np.stack([i, j, k], axis=-1).reshape(-1, 1, 3) + CORNERS[None]
    cubes = base[..., 0] + n * (base[..., 1] + n * base[..., 2])
    return np.ascontiguousarray(P), np.ascontiguousarray(cubes.astype(np.int64))


def directed_edges(f):
    f = np.asarray(f).astype(np.int64)
    return collections.Counter(map(tuple, np.concatenate([f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]]).tolist()))


def is_closed_and_oriented(f):
    """Every directed edge occurs once and its reverse once."""
    e = directed_edges(f)
    return all(c == 1 for c in e.values()) and all((b, a) in e for a, b in e)


def is_closed(f):
    """Every directed edge occurs as often as its reverse: closed and consistently oriented, whether or not two sheets touch along an edge."""
    e = directed_edges(f)
    return all(e.get((b, a), 0) == c for (a, b), c in e.items())


def euler_characteristic(v, f):
    e = directed_edges(f)
    return len(v) - len({(min(a, b), max(a, b)) for a, b in e}) + len(f)


def signed_volume(v, f):
    v = np.asarray(v, dtype=np.float64)
    f = np.asarray(f).astype(np.int64)
    return float(np.einsum("ij,ij->i", v[f[:, 0]], np.cross(v[f[:, 1]], v[f[:, 2]])).sum() / 6.0)


def merged_faces(mask):
    """The faces (indices into FACES) of a case that are ambiguous -- two diagonal inside corners -- and whose two segments lie on ONE loop of
    the cube: only across such a face can a fan diagonal of the loop join two vertices of the face."""
    succ = dict(_segments(mask))
    loop_of, seen = {}, 0
    for e0 in sorted(succ):
        if e0 not in loop_of:
            e = e0
            while e not in loop_of:
                loop_of[e] = seen
                e = succ[e]
            seen += 1
    edge_of = {frozenset((int(a), int(b))): e for e, (a, b) in enumerate(EDGES)}
    out = []
    for k, cyc in enumerate(FACES):
        sign = [bool(mask >> c & 1) for c in cyc]
        if sign[0] == sign[2] and sign[1] == sign[3] and sign[0] != sign[1]:
            if len({loop_of[edge_of[frozenset((cyc[j], cyc[(j + 1) % 4]))]] for j in range(4)}) == 1:
                out.append(k)
    return out


def faces_merged_from_both_sides(grid_scalars, cube_indices, isovalue):
    """How many grid faces are merged_faces of BOTH cubes that share them. Where there is none, no two cubes can emit the same mesh edge as
    a fan diagonal, so every directed mesh edge of a closed surface occurs exactly once: a face segment once from either cube, in opposite
    directions, a fan diagonal twice inside its own cube, in opposite directions. Where there are some, two sheets of the surface may
    touch along one segment inside such a face: that edge then occurs twice in either direction (closed and oriented, not manifold)."""
    S = np.asarray(grid_scalars).reshape(-1)
    idx = np.asarray(cube_indices).astype(np.int64)
    mask = ((S[idx] > S.dtype.type(isovalue)).astype(np.int64) << np.arange(8)).sum(axis=1)
    merged = [merged_faces(m) for m in range(256)]
    keys = [tuple(sorted(idx[c, FACES[k]].tolist())) for c in np.nonzero([len(merged[m]) > 0 for m in mask])[0] for k in merged[mask[c]]]
    return len(keys) - len(set(keys))


def has_repeated_indices(f):
    f = np.asarray(f)
    return bool(((f[:, 0] == f[:, 1]) | (f[:, 1] == f[:, 2]) | (f[:, 0] == f[:, 2])).any())
