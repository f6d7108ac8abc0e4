"""The contract of remove_mesh_vertices, remove_unreferenced_mesh_vertices, deduplicate_mesh_vertices and orient_mesh_faces (DESIGN.md, row
f16) in plain numpy and Python. It is not a port of anything: the three vertex calls are written as the loops of the reference's .cpp files
read, orient is a serial breadth-first search per patch over a dict of edges. Held to hand-worked cases by tests/test_mesh_repair_contract.py;
the GPU kernels are held to it by tests/test_gpu_mesh_repair.py. Also the seeded generators both files use."""
from collections import deque

import numpy as np

import mesh_smooth_contract as S

MESH_NAMES = ("tetrahedron", "defective", "fan700", "book300", "bunny", "cube_twist")


def mesh(name):
    """(v float64, f int64) of a named mesh of tests/mesh_smooth_contract.py, made once there."""
    return S.mesh(name)


# ---------------------------------------------------------------------------------------------------- the three vertex calls
def remove_mesh_vertices(v, f, mask):
    """src/remove_mesh_vertices.cpp:37-70."""
    mask = np.asarray(mask).reshape(-1)
    new = np.full(len(v), -1, dtype=np.int64)
    rows = []
    for i in range(len(v)):
        if mask[i]:
            new[i] = len(rows)
            rows.append(i)
    faces = []
    for face in f.tolist():
        mapped = [int(new[j]) for j in face]
        if all(m != -1 for m in mapped):
            faces.append(mapped)
    return v[np.array(rows, dtype=np.int64)].reshape(-1, 3), np.array(faces, dtype=f.dtype).reshape(-1, 3)


def remove_unreferenced(v, f):
    """(v_new, f_new, corr_v, corr_f): a vertex stays when a face lists it; those that stay keep their order. corr_f holds -1, wrapped for
    an unsigned dtype, for a vertex that no face lists."""
    seen = np.zeros(len(v), dtype=bool)
    for face in f.tolist():
        for j in face:
            seen[j] = True
    new = np.full(len(v), -1, dtype=np.int64)
    rows = []
    for i in range(len(v)):
        if seen[i]:
            new[i] = len(rows)
            rows.append(i)
    rows = np.array(rows, dtype=np.int64)
    return v[rows], new[f.astype(np.int64)].astype(f.dtype), rows.astype(f.dtype), new.astype(f.dtype)


def round_half_away(p, eps):
    """round(p / eps) as C's round() gives it, in p's dtype, then + 0 (so that -0.0 and 0.0 are one key); p itself for eps <= 0."""
    T = p.dtype.type
    r = p
    if eps > 0:
        q = p / T(eps)
        t = np.trunc(q)
        r = t + np.where(np.abs(q - t) >= 0.5, np.sign(q), 0).astype(p.dtype)
    return r + T(0)


def dedup_points(v, eps):
    """(v_out, svi, svj) of deduplicate_point_cloud: unique rows of the rounded coordinates in lexicographic order, the lowest row of every
    group, int32. For finite coordinates."""
    _, svi, svj = np.unique(round_half_away(np.ascontiguousarray(v), eps), axis=0, return_index=True, return_inverse=True)
    return v[svi], svi.astype(np.int32), svj.reshape(-1).astype(np.int32)


def dedup_mesh(v, f, eps):
    """src/remove_duplicates.cpp:59-80: (v_out, f_out, svi, svj)."""
    v_out, svi, svj = dedup_points(v, eps)
    faces = []
    for face in f.tolist():
        a, b, c = (int(svj[j]) for j in face)
        if a != b and a != c and b != c:
            faces.append([a, b, c])
    return v_out, np.array(faces, dtype=f.dtype).reshape(-1, 3), svi, svj


# ---------------------------------------------------------------------------------------------------- orient
def manifold_edges(f):
    """{(lo, hi): [(face, ascends), (face, ascends)]} of the undirected edges that exactly two faces list. A face that lists a vertex twice
    has no edges. ascends: the face runs along the edge from lo to hi."""
    edges = {}
    for i, (a, b, c) in enumerate(f.tolist()):
        if a == b or b == c or a == c:
            continue
        for x, y in ((a, b), (b, c), (c, a)):
            edges.setdefault((min(x, y), max(x, y)), []).append((i, x < y))
    return {e: fs for e, fs in edges.items() if len(fs) == 2 and fs[0][0] != fs[1][0]}


def orient(f):
    """(oriented faces, patch of every face, number of patches that are not orientable): one breadth-first search per patch from its smallest
    face; a patch in which two ways round disagree is returned as it came."""
    nf = len(f)
    nbrs = [[] for _ in range(nf)]
    for (i, ai), (j, aj) in manifold_edges(f).values():
        flip = ai == aj                                   # the same direction along the edge: one of the two must turn
        nbrs[i].append((j, flip))
        nbrs[j].append((i, flip))
    patch = np.full(nf, -1, dtype=np.int64)
    rev = np.zeros(nf, dtype=bool)
    count = twisted = 0
    for start in range(nf):
        if patch[start] != -1:
            continue
        members, ok = [start], True
        patch[start] = count
        queue = deque([start])
        while queue:
            i = queue.popleft()
            for j, flip in nbrs[i]:
                want = rev[i] != flip
                if patch[j] == -1:
                    patch[j], rev[j] = count, want
                    members.append(j)
                    queue.append(j)
                elif rev[j] != want:
                    ok = False
        if not ok:
            rev[members] = False
            twisted += 1
        count += 1
    out = np.where(rev[:, None], f[:, ::-1], f)
    return np.ascontiguousarray(out).astype(f.dtype), patch.astype(f.dtype), twisted


# ---------------------------------------------------------------------------------------------------- properties, vectorised
def edge_table(f):
    """Per corner of the faces that list three different vertices: (key lo * N + hi, face, ascends), sorted by key."""
    f = np.asarray(f).astype(np.int64)
    good = np.flatnonzero((f[:, 0] != f[:, 1]) & (f[:, 1] != f[:, 2]) & (f[:, 0] != f[:, 2]))
    a = f[good][:, [0, 1, 2]].reshape(-1)
    b = f[good][:, [1, 2, 0]].reshape(-1)
    face = np.repeat(good, 3)
    key = np.minimum(a, b) * (int(f.max()) + 1) + np.maximum(a, b)
    order = np.argsort(key, kind="stable")
    return key[order], face[order], (a < b)[order]


def manifold_pairs(f):
    """(i, j, same direction) of the manifold edges, as arrays."""
    key, face, asc = edge_table(f)
    if len(key) == 0:
        return (np.zeros(0, dtype=np.int64),) * 2 + (np.zeros(0, dtype=bool),)
    head = np.concatenate([[True], key[1:] != key[:-1]])
    starts = np.flatnonzero(head)
    lengths = np.diff(np.concatenate([starts, [len(key)]]))
    two = starts[lengths == 2]
    return face[two], face[two + 1], asc[two] == asc[two + 1]


def patches_by_scipy(f):
    """Patch of every face from scipy's labelling of the manifold-edge graph, renumbered by smallest face."""
    from scipy.sparse import coo_matrix
    from scipy.sparse.csgraph import connected_components
    nf = len(f)
    i, j, _ = manifold_pairs(f)
    _, label = connected_components(coo_matrix((np.ones(len(i), dtype=np.int8), (i, j)), shape=(nf, nf)), directed=False)
    first = np.full(label.max() + 1, nf, dtype=np.int64)
    np.minimum.at(first, label, np.arange(nf))
    rank = np.empty_like(first)
    rank[np.argsort(first)] = np.arange(len(first))
    return rank[label]


def check_orientation(f, oriented, patch):
    """The properties of an oriented result: rows are their input or its reverse; patch numbers ascend with smallest face; the smallest face
    of each patch has its input row; the two faces of a manifold edge are in one patch and run along it in opposite directions, except in
    patches that came back unchanged (an oriented patch has no such edge, so these are the ones that cannot be oriented). Returns their
    number."""
    f, oriented, patch = np.asarray(f).astype(np.int64), np.asarray(oriented).astype(np.int64), np.asarray(patch).astype(np.int64)
    kept, turned = (oriented == f).all(axis=1), (oriented == f[:, ::-1]).all(axis=1)
    assert (kept | turned).all()
    first = np.full(patch.max() + 1, len(f), dtype=np.int64)
    np.minimum.at(first, patch, np.arange(len(f)))
    assert (first < len(f)).all() and (np.diff(first) > 0).all()
    assert kept[first].all()
    i, j, same = manifold_pairs(oriented)
    assert np.array_equal(patch[i], patch[j])
    twisted = np.unique(patch[i][same])
    assert kept[np.isin(patch, twisted)].all()
    return len(twisted)


# ---------------------------------------------------------------------------------------------------- generators
def reverse_some(f, seed):
    """f with about half of its rows reversed."""
    turn = np.random.default_rng(seed).random(len(f)) < 0.5
    return np.ascontiguousarray(np.where(turn[:, None], f[:, ::-1], f))


def moebius(k=3, first_vertex=0):
    """A Moebius band of 2 k triangles over 2 k vertices: a strip of k quads whose last quad is glued to the first with a half turn."""
    top, bot = np.arange(k), k + np.arange(k)
    faces = []
    for i in range(k):
        a, b = top[i], bot[i]
        c, d = (top[i + 1], bot[i + 1]) if i + 1 < k else (bot[0], top[0])
        faces += [[a, b, c], [b, d, c]]
    return np.array(faces, dtype=np.int64) + first_vertex


def strip(n):
    """n triangles (i, i + 1, i + 2): every second one runs the other way round, every inner edge is manifold, one patch."""
    i = np.arange(n, dtype=np.int64)
    return np.stack([i, i + 1, i + 2], axis=1)


def strip_mesh(nv):
    """nv vertices on a zigzag and the nv - 2 triangles of strip(); nv >= 3."""
    i = np.arange(nv)
    return np.stack([0.5 * i, (i % 2).astype(np.float64), 0.01 * i * i], axis=1), strip(nv - 2)


def closed_book(k=6):
    """Closed and orientable, with an edge that 2 k faces share: k tetrahedra that have the edge (0, 1) in common and nothing else. The two
    faces of a tetrahedron at that edge are joined through its other two faces, so there are k patches, each a sphere."""
    faces = []
    for t in range(k):
        a, b = 2 + 2 * t, 3 + 2 * t
        faces += [[0, 1, a], [1, 0, b], [0, a, b], [1, b, a]]
    return np.array(faces, dtype=np.int64)


def soup(v, f):
    """Every face with three vertices of its own: deduplication must weld it back."""
    return np.ascontiguousarray(v[f.reshape(-1)]), np.arange(3 * len(f), dtype=f.dtype).reshape(-1, 3)


def with_unreferenced(v, f, seed):
    """The mesh with a tail of vertices that no face lists and some in the middle. Returns (v, f, their ids)."""
    rng = np.random.default_rng(seed)
    n = len(v)
    at = np.sort(rng.choice(np.arange(1, n), size=min(5, n - 1), replace=False))
    shift = np.searchsorted(at, np.arange(n), side="right")            # how many are put in before old vertex i
    extra = rng.random((len(at) + 3, 3))
    big = np.empty((n + len(extra), 3), dtype=v.dtype)
    old = np.arange(n) + shift
    big[old] = v
    ids = np.setdiff1d(np.arange(len(big)), old)
    big[ids] = extra
    return big, (np.arange(n) + shift)[f].astype(f.dtype), ids


def grid_faces(n, first_vertex=0):
    """The 2 (n - 1)^2 triangles of an n x n grid of vertices."""
    i, j = np.meshgrid(np.arange(n - 1), np.arange(n - 1), indexing="ij")
    a = (i * n + j).ravel() + first_vertex
    return np.stack([np.stack([a, a + 1, a + n], axis=1), np.stack([a + 1, a + n + 1, a + n], axis=1)], axis=1).reshape(-1, 3)
