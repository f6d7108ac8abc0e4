"""The contract of orient_point_cloud_normals in numpy: this file is the definition, the GPU path equals it to the byte.

    orient(points, normals, nbr) -> (normals_out, flipped)

nbr is the (n, m) int64 array, m = min(k + 1, n), that k_nearest_neighbors(points, points, m, max_points_per_leaf=...) returns (reshaped when it
comes back squeezed; neighbours(nbr, n) does that). It is an argument: ties in k-NN order are the k-NN's business, and k-NN is pinned elsewhere.

1. Edges. Every (i, nbr[i, c]) with nbr[i, c] != i is the undirected edge {lo, hi}; a pair listed from both sides, or twice, is one edge.
   (Coincident copies may push i out of its own row: then all m entries are edges. An entry outside [0, n) is no edge.)
2. Agreement. d = (ni0*nj0 + ni1*nj1) + ni2*nj2 in float64, the inputs converted exactly, every multiply and add rounded on its own (no FMA).
   An edge whose d is not finite is not an edge: a row with a NaN or infinite normal ends up alone. w = 1.0 - |d|; flip(e) = (d < 0).
3. Forest. The minimum spanning forest of the edges under the strict total order (w, lo, hi). It is unique.
4. Reference row of a tree. The row with the largest points[r, 2], compared in the input dtype with >; the first such row wins among equal
   ones. base = (normals[r, 2] < 0).
5. Result. flipped[i] = base XOR (XOR of flip(e) over the tree path from i to r). A row with no edges is its own tree and follows rule 4.
   normals_out[i] is normals[i], negated (the three sign bits inverted, nothing else) where flipped[i].

Kruskal over a union-find that carries the parity of a row relative to its set's representative."""
import numpy as np


def neighbours(nbr, n):
    """k_nearest_neighbors' index result as (n, m) int64, whatever it squeezed."""
    return np.ascontiguousarray(np.asarray(nbr, dtype=np.int64).reshape(n, -1))


def edges(normals, nbr):
    """(lo, hi, w, flip) of rules 1 and 2, sorted by (w, lo, hi)."""
    n, m = nbr.shape
    i = np.repeat(np.arange(n, dtype=np.int64), m)
    j = nbr.reshape(-1)
    keep = (j != i) & (j >= 0) & (j < n)
    i, j = i[keep], j[keep]
    key = np.unique(np.minimum(i, j) * n + np.maximum(i, j))
    lo, hi = key // n, key % n
    nd = np.asarray(normals).astype(np.float64)
    with np.errstate(all="ignore"):
        d = (nd[lo, 0] * nd[hi, 0] + nd[lo, 1] * nd[hi, 1]) + nd[lo, 2] * nd[hi, 2]
    ok = np.isfinite(d)
    lo, hi, d = lo[ok], hi[ok], d[ok]
    w = 1.0 - np.abs(d)
    order = np.lexsort((hi, lo, w))
    return lo[order], hi[order], w[order], (d < 0)[order]


def forest(n, lo, hi, flip):
    """Kruskal over edges sorted by the total order. Returns (rep, par, tree): rep[i] a representative row of i's tree, par[i] the XOR of the
    flips on the tree path from i to rep[i], tree the indices of the edges taken."""
    parent = list(range(n))
    parity = [0] * n                 # of a row relative to parent[row]

    def find(x):
        path = []
        while parent[x] != x:
            path.append(x)
            x = parent[x]
        p = 0
        for y in reversed(path):     # from the root's child down: parity to the root
            p ^= parity[y]
            parity[y] = p
            parent[y] = x
        return x

    taken = []
    for e, (a, b, f) in enumerate(zip(lo.tolist(), hi.tolist(), flip.tolist())):
        ra, rb = find(a), find(b)
        if ra == rb:
            continue
        parent[ra] = rb
        parity[ra] = parity[a] ^ parity[b] ^ int(f)
        taken.append(e)
    rep = np.array([find(x) for x in range(n)], dtype=np.int64)
    par = np.array([parity[x] if parent[x] != x else 0 for x in range(n)], dtype=bool)
    return rep, par, np.array(taken, dtype=np.int64)


def reference_rows(points, rep):
    """Rule 4: per row, the reference row of its tree."""
    z = np.asarray(points)[:, 2]
    n = len(z)
    top = {}
    for i in range(n):
        r = int(rep[i])
        if r not in top or z[i] > z[top[r]]:
            top[r] = i
    return np.array([top[int(r)] for r in rep], dtype=np.int64)


def orient(points, normals, nbr):
    points, normals = np.asarray(points), np.asarray(normals)
    n = points.shape[0]
    nbr = neighbours(nbr, n)
    lo, hi, _, flip = edges(normals, nbr)
    rep, par, _ = forest(n, lo, hi, flip)
    ref = reference_rows(points, rep)
    base = normals[ref, 2] < 0
    flipped = base ^ par ^ par[ref]
    out = normals.copy()
    out[flipped] = -out[flipped]
    return out, flipped


def num_trees(points, normals, nbr):
    n = np.asarray(points).shape[0]
    lo, hi, _, flip = edges(np.asarray(normals), neighbours(nbr, n))
    return len(np.unique(forest(n, lo, hi, flip)[0]))
