"""decimate_triangle_mesh: the contract in numpy, executable. The GPU reproduces it byte for byte
(tests/test_gpu_decimate.py); tests/test_decimate_contract.py holds it to its invariants and to a sequential greedy yardstick.

A round-synchronous shortest-edge collapse. State: positions P (v's dtype), faces F, an alive flag per face; vertex ids never change during
the rounds. While more than max_faces faces are alive:
  1 edges     the distinct undirected pairs (lo, hi) of the alive faces in lexicographic order; an edge's position in that list is its rank.
              An edge with one face is a boundary edge, its ends are boundary vertices.
  2 closure   one extra vertex INF and a face (x, y, INF) on every boundary edge (x, y). INF is never collapsed and never stored.
  3 cost      d = double(P[lo]) - double(P[hi]); c = (d0*d0 + d1*d1) + d2*d2 in double, every operation rounded on its own; c rounded to
              float32; key = bits(c) << 32 | rank. A non-finite c makes the edge invalid.
  4 validity  the link condition on the closed mesh: |N(lo) & N(hi)| == 2 (INF counts for boundary vertices), and no face of hi that does
              not hold lo becomes, with hi replaced by lo, the vertex set of an existing face (virtual faces included). Normal flips are
              not tested (igl's shortest-edge heuristic does not test them either).
  5 claims    every valid edge writes its key, by minimum, to every real vertex of {lo, hi} | N(lo) | N(hi); it wins iff it holds them all.
  6 budget    the winners in ascending key order; one is taken iff the winners before it remove fewer than alive - max_faces faces
              (an interior edge removes 2, a boundary edge 1).
  7 apply     P[lo] = (P[lo] + P[hi]) * 0.5 in v's dtype; faces that hold both ends die; in the others hi becomes lo in place.
A round without a winner ends the loop. Output: the alive faces in input order (f_correspondences: their input rows), the vertices they
list in input order (v_correspondences: their ids), the faces re-indexed.

Only the order of the keys reaches the output, so any rank that is monotone in (lo, hi) gives the same bytes.
Every round in which the budget takes all winners does not depend on max_faces, and the round in which it does not is the last: a
Decimation keeps the winners of those rounds and answers every max_faces of one mesh from them."""
import heapq
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
EMPTY_TEXT = "decimate_triangle_mesh_doc produced an empty mesh. This can happen if the input is non-manifold."
DEGENERATE_TEXT = "f must not hold a face that lists a vertex twice"
NO_KEY = np.uint64(0xFFFFFFFFFFFFFFFF)


# ---------------------------------------------------------------------------------------------------- helpers
def _expand(start, count):
    """For rows i with `count[i]` items from `start[i]` on: (row of every item, index of every item)."""
    count = count.astype(np.int64)
    row = np.repeat(np.arange(len(count), dtype=np.int64), count)
    first = np.cumsum(count) - count
    return row, np.repeat(start.astype(np.int64), count) + (np.arange(int(count.sum()), dtype=np.int64) - np.repeat(first, count))


def _csr(rows, n):
    """Order that sorts `rows` (stable) and the start of every row in it."""
    order = np.argsort(rows, kind="stable")
    start = np.zeros(n + 1, dtype=np.int64)
    np.cumsum(np.bincount(rows, minlength=n), out=start[1:])
    return order, start


def _member(sorted_codes, codes):
    at = np.searchsorted(sorted_codes, codes)
    at[at == len(sorted_codes)] = 0
    return (sorted_codes[at] == codes) if len(sorted_codes) else np.zeros(len(codes), dtype=bool)


def edge_cost(P, lo, hi):
    """Step 3: the float32 the key carries."""
    d = P[lo].astype(np.float64) - P[hi].astype(np.float64)
    with np.errstate(over="ignore", invalid="ignore"):
        c = (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]
        return c.astype(np.float32)


def edges_of(F, nv):
    """Step 1: (lo, hi, number of faces) of the distinct undirected edges, in lexicographic order."""
    a, b = F.reshape(-1), F[:, [1, 2, 0]].reshape(-1)
    code, count = np.unique(np.minimum(a, b) * nv + np.maximum(a, b), return_counts=True)
    return code // nv, code % nv, count


def check_input(f, nv):
    """What the call refuses whatever max_faces is: an index outside [0, nv), a face that lists a vertex twice, an edge of three faces."""
    F = np.asarray(f).astype(np.int64)
    if F.min() < 0 or F.max() >= nv:
        raise ValueError(f"f must hold row indices of v: found a face index outside [0, {nv})")
    if ((F[:, 0] == F[:, 1]) | (F[:, 1] == F[:, 2]) | (F[:, 0] == F[:, 2])).any():
        raise ValueError(DEGENERATE_TEXT)
    if edges_of(F, nv)[2].max() > 2:
        raise ValueError(EMPTY_TEXT)
    return F


# ---------------------------------------------------------------------------------------------------- one round
def valid_edges(P, F, nv):
    """Steps 1 to 4 on the alive faces F: (lo, hi, faces per edge, key, valid, the neighbours as (columns, row starts))."""
    assert nv + 1 < 2 ** 20
    lo, hi, count = edges_of(F, nv)
    ne = len(lo)
    c = edge_cost(P, lo, hi)
    key = (c.view(np.uint32).astype(np.uint64) << np.uint64(32)) | np.arange(ne, dtype=np.uint64)
    boundary = np.zeros(nv, dtype=bool)
    boundary[lo[count == 1]] = True
    boundary[hi[count == 1]] = True
    # the neighbours as CSR; every pair of neighbours of one vertex is a wedge, and the wedges over (a, b) are the common neighbours of a and b
    src, dst = np.concatenate([lo, hi]), np.concatenate([hi, lo])
    order, start = _csr(src, nv)
    dst = dst[order]
    deg = np.diff(start)
    ent_row = np.repeat(np.arange(nv, dtype=np.int64), deg)
    i, j = _expand(start[ent_row], deg[ent_row])
    a, b = dst[i], dst[j]
    keep = a < b
    wcode, wcount = np.unique(a[keep] * nv + b[keep], return_counts=True)
    ecode = lo * nv + hi
    at = np.searchsorted(wcode, ecode)
    at[at == len(wcode)] = 0
    common = np.where(wcode[at] == ecode, wcount[at], 0) if len(wcode) else np.zeros(ne, dtype=np.int64)
    link = common + (boundary[lo] & boundary[hi]) == 2
    # the faces of the closed mesh as sorted triples (INF = nv), and the faces of every real vertex
    bnd = count == 1
    T = np.sort(np.concatenate([F, np.stack([lo[bnd], hi[bnd], np.full(int(bnd.sum()), nv, dtype=np.int64)], axis=1)]), axis=1)
    m = nv + 1
    fcode = np.sort((T[:, 0] * m + T[:, 1]) * m + T[:, 2])
    corner, cface = T.reshape(-1), np.repeat(np.arange(len(T), dtype=np.int64), 3)
    real = corner < nv
    forder, fstart = _csr(corner[real], nv)
    vface = cface[real][forder]
    cand = np.flatnonzero(link & np.isfinite(c))
    e, g = _expand(fstart[hi[cand]], np.diff(fstart)[hi[cand]])
    G = T[vface[g]]
    elo, ehi = lo[cand][e][:, None], hi[cand][e][:, None]
    moved = np.sort(np.where(G == ehi, elo, G), axis=1)
    twice = ~(G == elo).any(axis=1) & _member(fcode, (moved[:, 0] * m + moved[:, 1]) * m + moved[:, 2])
    valid = np.zeros(ne, dtype=bool)
    valid[cand] = np.bincount(e, weights=twice, minlength=len(cand)) == 0
    return lo, hi, count, key, valid, (dst, start)


def round_winners(P, F, nv):
    """Steps 1 to 5: (lo, hi, faces removed) of the winners in ascending key order, and the number of valid edges."""
    lo, hi, count, key, valid, (dst, start) = valid_edges(P, F, nv)
    ve = np.flatnonzero(valid)
    deg = np.diff(start)
    e1, i1 = _expand(start[lo[ve]], deg[lo[ve]])
    e2, i2 = _expand(start[hi[ve]], deg[hi[ve]])
    own = np.arange(len(ve), dtype=np.int64)
    who = np.concatenate([e1, e2, own, own])
    where = np.concatenate([dst[i1], dst[i2], lo[ve], hi[ve]])
    owner = np.full(nv, NO_KEY, dtype=np.uint64)
    np.minimum.at(owner, where, key[ve][who])
    wins = np.bincount(who, weights=owner[where] != key[ve][who], minlength=len(ve)) == 0
    w = ve[wins]
    w = w[np.argsort(key[w])]
    return lo[w], hi[w], count[w], len(ve)


def apply_collapses(P, F, lo, hi, nv):
    """Step 7, in place on P; returns the faces with hi replaced and which of them stay alive."""
    P[lo] = (P[lo] + P[hi]) * P.dtype.type(0.5)
    to = np.arange(nv, dtype=np.int64)
    to[hi] = lo
    F = to[F]
    return F, (F[:, 0] != F[:, 1]) & (F[:, 1] != F[:, 2]) & (F[:, 0] != F[:, 2])


def finish(v, f, P, F, rows):
    """The output: alive faces F (input rows `rows`) re-indexed over the vertices they list."""
    ids = np.unique(F)
    ft = np.asarray(f).dtype
    return (np.ascontiguousarray(P[ids]).astype(np.asarray(v).dtype, copy=False), np.searchsorted(ids, F).astype(ft).reshape(-1, 3),
            ids.astype(ft), rows.astype(ft))


class Decimation:
    """The contract for one mesh and every max_faces: decimate(max_faces) -> (v_out, f_out, v_correspondences, f_correspondences) and
    self.rounds / self.collapses / self.valid_left / self.touched (the vertices that were an end of a collapse) of that run."""

    def __init__(self, v, f):
        self.v, self.f = np.ascontiguousarray(v), np.ascontiguousarray(f)
        self.nv = len(self.v)
        self.F0 = check_input(self.f, self.nv)
        self._winners = []          # per round of the run without a budget: (lo, hi, removed) in key order, valid edges

    def decimate(self, max_faces):
        if max_faces <= 0:
            raise ValueError(f"max_faces must be greater than 0, got {max_faces}.")
        if max_faces > len(self.f):
            raise ValueError(f"max_faces must be less than or equal to the number of input faces ({len(self.f)}), got {max_faces}.")
        P, F, rows = self.v.copy(), self.F0, np.arange(len(self.f), dtype=np.int64)
        self.rounds = self.collapses = 0
        self.valid_left = None
        self.touched = np.zeros(self.nv, dtype=bool)
        while len(F) > max_faces:
            if self.rounds == len(self._winners):
                self._winners.append(round_winners(P, F, self.nv))
            lo, hi, removed, n_valid = self._winners[self.rounds]
            if len(lo) == 0:
                self.valid_left = n_valid
                break
            take = np.cumsum(removed) - removed < len(F) - max_faces
            F, alive = apply_collapses(P, F, lo[take], hi[take], self.nv)
            self.touched[lo[take]] = self.touched[hi[take]] = True
            F, rows = F[alive], rows[alive]
            self.rounds += 1
            self.collapses += int(take.sum())
        return finish(self.v, self.f, P, F, rows)


def decimate(v, f, max_faces):
    return Decimation(v, f).decimate(max_faces)


# ---------------------------------------------------------------------------------------------------- the rule, literally (small meshes, and the yardstick)
INF = -1


class SetMesh:
    """Faces as sets: the validity rule of step 4 word for word, for the yardstick and for checking valid_edges."""

    def __init__(self, P, F):
        self.P = P
        self.faces = {i: tuple(int(x) for x in row) for i, row in enumerate(F)}
        self.vf = {}
        for i, t in self.faces.items():
            for x in t:
                self.vf.setdefault(x, set()).add(i)

    def edge_faces(self, x, y):
        return self.vf[x] & self.vf[y]

    def neighbours(self, x):
        """N(x), INF included for a boundary vertex."""
        n = set()
        for i in self.vf[x]:
            n.update(self.faces[i])
        n.discard(x)
        if any(len(self.edge_faces(x, y)) == 1 for y in n):
            n.add(INF)
        return n

    def closed_faces(self, x):
        """The vertex sets of the faces of x on the closed mesh."""
        out = [frozenset(self.faces[i]) for i in self.vf[x]]
        for y in self.neighbours(x) - {INF}:
            if len(self.edge_faces(x, y)) == 1:
                out.append(frozenset((x, y, INF)))
        return out

    def valid(self, lo, hi):
        if not np.isfinite(edge_cost(self.P, np.array([lo]), np.array([hi]))[0]):
            return False
        if len(self.neighbours(lo) & self.neighbours(hi)) != 2:
            return False
        have = set(self.closed_faces(lo))
        return not any(lo not in g and (g - {hi}) | {lo} in have for g in self.closed_faces(hi))

    def collapse(self, lo, hi):
        self.P[lo] = (self.P[lo] + self.P[hi]) * self.P.dtype.type(0.5)
        for i in list(self.vf[hi]):
            t = self.faces[i]
            if lo in t:
                for x in t:
                    self.vf[x].discard(i)
                del self.faces[i]
            else:
                self.faces[i] = tuple(lo if x == hi else x for x in t)
                self.vf[lo].add(i)
        del self.vf[hi]


def valid_edges_literal(P, F):
    m = SetMesh(P, F)
    lo, hi, _ = edges_of(np.asarray(F, dtype=np.int64), len(P))
    return np.array([m.valid(int(a), int(b)) for a, b in zip(lo, hi)], dtype=bool)


def greedy_decimate(v, f, max_faces):
    """The yardstick: one collapse at a time, always the valid edge of the smallest (cost, lo, hi), same validity rule, same midpoint."""
    v, f = np.ascontiguousarray(v), np.ascontiguousarray(f)
    m = SetMesh(v.copy(), check_input(f, len(v)))
    version = {x: 0 for x in m.vf}
    heap = []

    def push_around(x):
        for y in m.neighbours(x) - {INF}:
            a, b = min(x, y), max(x, y)
            heapq.heappush(heap, (float(edge_cost(m.P, np.array([a]), np.array([b]))[0]), a, b, version[a], version[b]))

    for x in list(m.vf):
        push_around(x)
    while len(m.faces) > max_faces and heap:
        c, lo, hi, sa, sb = heapq.heappop(heap)
        if lo not in m.vf or hi not in m.vf or version[lo] != sa or version[hi] != sb or not m.edge_faces(lo, hi) or not m.valid(lo, hi):
            continue
        m.collapse(lo, hi)
        ring = {lo} | (m.neighbours(lo) - {INF})         # every edge whose cost or validity can have changed has an end in here
        for x in ring:
            version[x] += 1
        for x in ring:
            push_around(x)
    rows = np.array(sorted(m.faces), dtype=np.int64)
    return finish(v, f, m.P, np.array([m.faces[i] for i in rows], dtype=np.int64).reshape(-1, 3), rows)


# ---------------------------------------------------------------------------------------------------- measures
def edge_face_counts(f):
    f = np.asarray(f).astype(np.int64)
    return edges_of(f, int(f.max()) + 1)[2]


def euler_per_component(f):
    """Sorted list of V - E + F over the connected components of the faces."""
    f = np.asarray(f).astype(np.int64)
    n = int(f.max()) + 1
    parent = np.arange(n)

    def find(x):
        while parent[x] != x:
            parent[x] = parent[parent[x]]
            x = parent[x]
        return x

    for a, b, c in f:
        ra, rb, rc = find(a), find(b), find(c)
        r = min(ra, rb, rc)
        parent[ra] = parent[rb] = parent[rc] = r
    root = np.array([find(x) for x in range(n)])
    lo, hi, _ = edges_of(f, n)
    used = np.unique(f)
    out = []
    for r in np.unique(root[used]):
        out.append(int((root[used] == r).sum()) - int((root[lo] == r).sum()) + int((root[f[:, 0]] == r).sum()))
    return sorted(out)


def point_triangle_distances(p, v, f, chunk=256):
    """For every point of p the distance to the nearest triangle of (v, f): brute force, in float64 (Ericson's closest point on a triangle)."""
    p, v = np.asarray(p, dtype=np.float64), np.asarray(v, dtype=np.float64)
    f = np.asarray(f).astype(np.int64)
    A, B, C = v[f[:, 0]][None], v[f[:, 1]][None], v[f[:, 2]][None]
    ab, ac = B - A, C - A
    out = np.empty(len(p))
    for s in range(0, len(p), chunk):
        q = p[s:s + chunk, None, :]
        ap, bp, cp = q - A, q - B, q - C
        d1, d2 = (ab * ap).sum(-1), (ac * ap).sum(-1)
        d3, d4 = (ab * bp).sum(-1), (ac * bp).sum(-1)
        d5, d6 = (ab * cp).sum(-1), (ac * cp).sum(-1)
        va, vb, vc = d3 * d6 - d5 * d4, d5 * d2 - d1 * d6, d1 * d4 - d3 * d2
        with np.errstate(divide="ignore", invalid="ignore"):
            den = va + vb + vc
            best = A + ab * (vb / den)[..., None] + ac * (vc / den)[..., None]         # inside
            w = (d4 - d3) / ((d4 - d3) + (d5 - d6))
            best = np.where(((va <= 0) & (d4 - d3 >= 0) & (d5 - d6 >= 0))[..., None], B + (C - B) * w[..., None], best)
            best = np.where(((vb <= 0) & (d2 >= 0) & (d6 <= 0))[..., None], A + ac * (d2 / (d2 - d6))[..., None], best)
            best = np.where(((vc <= 0) & (d1 >= 0) & (d3 <= 0))[..., None], A + ab * (d1 / (d1 - d3))[..., None], best)
        best = np.where(((d6 >= 0) & (d5 <= d6))[..., None], C, best)
        best = np.where(((d3 >= 0) & (d4 <= d3))[..., None], B, best)
        best = np.where(((d1 <= 0) & (d2 <= 0))[..., None], A, best)
        out[s:s + chunk] = np.sqrt(((q - best) ** 2).sum(-1)).min(axis=1)
    return out


# ---------------------------------------------------------------------------------------------------- the named meshes
def icosphere(subdivisions):
    t = (1.0 + 5.0 ** 0.5) / 2.0
    v = [(-1, t, 0), (1, t, 0), (-1, -t, 0), (1, -t, 0), (0, -1, t), (0, 1, t), (0, -1, -t), (0, 1, -t), (t, 0, -1), (t, 0, 1), (-t, 0, -1), (-t, 0, 1)]
    f = [(0, 11, 5), (0, 5, 1), (0, 1, 7), (0, 7, 10), (0, 10, 11), (1, 5, 9), (5, 11, 4), (11, 10, 2), (10, 7, 6), (7, 1, 8),
         (3, 9, 4), (3, 4, 2), (3, 2, 6), (3, 6, 8), (3, 8, 9), (4, 9, 5), (2, 4, 11), (6, 2, 10), (8, 6, 7), (9, 8, 1)]
    v = [np.array(x, dtype=np.float64) / np.linalg.norm(x) for x in v]
    for _ in range(subdivisions):
        mid, g = {}, []

        def middle(a, b):
            k = (min(a, b), max(a, b))
            if k not in mid:
                x = v[a] + v[b]
                v.append(x / np.linalg.norm(x))
                mid[k] = len(v) - 1
            return mid[k]

        for a, b, c in f:
            ab, bc, ca = middle(a, b), middle(b, c), middle(c, a)
            g += [(a, ab, ca), (b, bc, ab), (c, ca, bc), (ab, bc, ca)]
        f = g
    return np.array(v), np.array(f, dtype=np.int64)


def grid_patch(n):
    """An open n x n patch of the equilateral lattice (i + j / 2, j * sqrt(3) / 2, 0). In float64 every edge's squared length is within
    a few 1e-16 of 1, so every cost of the first round is the float32 1.0 and the rank alone orders the keys."""
    ij = np.stack(np.meshgrid(np.arange(n + 1), np.arange(n + 1), indexing="ij"), axis=-1).reshape(-1, 2).astype(np.float64)
    v = np.stack([ij[:, 0] + 0.5 * ij[:, 1], ij[:, 1] * (3.0 ** 0.5 / 2.0), np.zeros(len(ij))], axis=1)
    idx = lambda i, j: i * (n + 1) + j
    f = []
    for i in range(n):
        for j in range(n):
            f += [(idx(i, j), idx(i + 1, j), idx(i, j + 1)), (idx(i + 1, j), idx(i + 1, j + 1), idx(i, j + 1))]
    return v, np.array(f, dtype=np.int64)


def cylinder(segments=12, rings=5):
    """Open at both ends."""
    a = 2 * np.pi * np.arange(segments) / segments
    v = np.array([(np.cos(t), np.sin(t), 0.37 * r) for r in range(rings + 1) for t in a])
    f = []
    for r in range(rings):
        for s in range(segments):
            p, q = r * segments + s, r * segments + (s + 1) % segments
            f += [(p, q, q + segments), (p, q + segments, p + segments)]
    return v, np.array(f, dtype=np.int64)


def moebius(segments=17):
    a = 2 * np.pi * np.arange(segments) / segments
    v = []
    for t in a:
        for w in (-0.4, 0.4):
            v.append(((1 + w * np.cos(t / 2)) * np.cos(t), (1 + w * np.cos(t / 2)) * np.sin(t), w * np.sin(t / 2)))
    f = []
    for s in range(segments):
        p0, p1 = 2 * s, 2 * s + 1
        if s + 1 < segments:
            q0, q1 = 2 * s + 2, 2 * s + 3
        else:
            q0, q1 = 1, 0
        f += [(p0, q0, q1), (p0, q1, p1)]
    return np.array(v), np.array(f, dtype=np.int64)


def strip(nf):
    """nf triangles in a row between two rails."""
    k = np.arange(nf + 2)
    v = np.stack([0.5 * k * (1 + 0.013 * np.sin(k)), (k % 2) * (0.8 + 0.01 * np.cos(3 * k)), 0.05 * np.sin(0.7 * k)], axis=1)
    f = np.array([(i, i + 1, i + 2) if i % 2 == 0 else (i + 1, i, i + 2) for i in range(nf)], dtype=np.int64)
    return v, f


def fan(nf):
    """nf triangles around vertex 0, open."""
    t = 1.7 * np.pi * np.arange(nf + 1) / (nf + 1)
    rim = np.stack([(1 + 0.1 * np.sin(5 * t)) * np.cos(t), (1 + 0.1 * np.sin(5 * t)) * np.sin(t), 0.1 * np.cos(3 * t)], axis=1)
    v = np.concatenate([np.zeros((1, 3)), rim])
    return v, np.array([(0, i + 1, i + 2) for i in range(nf)], dtype=np.int64)


def _join(*meshes):
    vs, fs, base = [], [], 0
    for v, f in meshes:
        vs.append(v)
        fs.append(f + base)
        base += len(v)
    return np.concatenate(vs), np.concatenate(fs)


def with_unreferenced(v, f, seed):
    """Vertices that no face lists, inserted at random places and at both ends."""
    rng = np.random.default_rng(seed)
    n = len(v)
    extra = max(3, n // 10)
    slot = np.sort(np.concatenate([[0, n + extra - 1], rng.choice(np.arange(1, n + extra - 1), extra - 2, replace=False)]))
    keep = np.ones(n + extra, dtype=bool)
    keep[slot] = False
    ids = np.flatnonzero(keep)
    w = rng.normal(size=(n + extra, 3))
    w[ids] = v
    return w, ids[f]


def bunny():
    return np.load(os.path.join(GOLDEN, "bunny_v.npy")).astype(np.float64), np.load(os.path.join(GOLDEN, "bunny_f.npy")).astype(np.int64)


MESH_NAMES = ["tetrahedron", "octahedron", "icosphere2", "grid", "cylinder", "two_components", "triangle_and_sphere", "moebius", "bowtie"]
MANIFOLD_NAMES = [n for n in MESH_NAMES if n != "bowtie"] + ["bunny", "bunny_unreferenced"]


def mesh(name):
    if name == "tetrahedron":
        return np.array([(0, 0, 0), (1, 0, 0), (0, 1.1, 0), (0, 0, 1.2)]), np.array([(0, 2, 1), (0, 1, 3), (1, 2, 3), (2, 0, 3)], dtype=np.int64)
    if name == "octahedron":
        v = np.array([(1, 0, 0), (-1.1, 0, 0), (0, 1.2, 0), (0, -1.3, 0), (0, 0, 1.4), (0, 0, -1.5)])
        return v, np.array([(0, 2, 4), (2, 1, 4), (1, 3, 4), (3, 0, 4), (2, 0, 5), (1, 2, 5), (3, 1, 5), (0, 3, 5)], dtype=np.int64)
    if name == "icosphere2":
        v, f = icosphere(2)
        return v * np.array([1.0, 0.8, 1.3]), f
    if name == "grid":
        return grid_patch(6)
    if name == "cylinder":
        return cylinder()
    if name == "two_components":
        a, b = icosphere(1), cylinder(7, 3)
        return _join((a[0] * 0.7, a[1]), (b[0] + np.array([3.0, 0, 0]), b[1]))
    if name == "triangle_and_sphere":
        s = icosphere(1)
        return _join((np.array([(5.0, 0, 0), (5.001, 0, 0), (5.0, 0.001, 0)]), np.array([(0, 1, 2)], dtype=np.int64)), (s[0] * np.array([1.0, 1.1, 0.9]), s[1]))
    if name == "moebius":
        return moebius()
    if name == "bowtie":            # two fans that share their centre only: the centre is no manifold vertex
        (av, af), (bv, bf) = fan(5), fan(6)
        rim = bv[1:] * np.array([1.0, 1.0, -1.0])
        rim[:, 2] += 0.9 * np.linalg.norm(rim[:, :2], axis=1)
        return np.concatenate([av, rim]), np.concatenate([af, np.where(bf == 0, 0, bf + len(av) - 1)])
    if name == "bunny":
        return bunny()
    if name == "bunny_unreferenced":
        return with_unreferenced(*bunny(), seed=5)
    raise KeyError(name)
