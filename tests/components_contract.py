"""Plain numpy / Python restatements of the connected_components and flood_fill_3d contracts: what the GPU tests are held
to, bit for bit. components() is the reference's loop (src/connected_components.cpp:11-66, :99-105) over an adjacency built from the faces;
flood_fill() walks the grid from the seed, with true 6-connectivity by default and with the reference's offset arithmetic
(src/flood_fill_3d.cpp:31-49) on request. components_fast() and flood_fill_fast() state the same two contracts over scipy's labelling, for
inputs of millions of elements; tests/test_components_contract.py holds them to the plain ones."""
import os
from collections import deque

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
BLOCK = 256                   # threads per block of the library's kernels (csrc/grid.h: kBlock); a wave is 64 of them
SC_TILE = 4096                # the tile of the library's inclusive scan (csrc/radix.h: kScTile)


def golden_mesh(name, dtype=np.float64):
    v = np.load(os.path.join(GOLDEN, f"{name}_v.npy")).astype(dtype)
    f = np.load(os.path.join(GOLDEN, f"{name}_f.npy")).astype(np.int64)
    return np.ascontiguousarray(v), np.ascontiguousarray(f)


def doubled(v, f):
    """The mesh of the reference's own test (tests/test_examples.py:719-730): two copies, the second one shifted."""
    return np.concatenate([v, v + 1.0]), np.concatenate([f, f + v.shape[0]])


def components(nv, f):
    """(cv, nv, cf, nf) as int64 for nv vertices and the faces f (m, 3): vertices are visited in ascending order, each unvisited one starts
    component len(counts) and a breadth-first search over the adjacency (two vertices are adjacent when a face lists both) collects it."""
    f = np.asarray(f).astype(np.int64).reshape(-1, 3)
    e = np.concatenate([f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]])
    e = np.concatenate([e, e[:, ::-1]])
    order = np.argsort(e[:, 0], kind="stable")
    src, dst = e[order, 0], e[order, 1].tolist()
    start = np.searchsorted(src, np.arange(nv + 1)).tolist()
    cv = [nv] * nv                              # nv means not yet visited
    counts = []
    for s in range(nv):
        if cv[s] < nv:
            continue
        current, num = len(counts), 0
        q = deque([s])
        while q:
            g = q.popleft()
            if cv[g] < nv:
                continue
            cv[g] = current
            num += 1
            for n in dst[start[g]:start[g + 1]]:
                if cv[n] < nv:
                    continue
                q.append(n)
        counts.append(num)
    cv = np.array(cv, dtype=np.int64)
    cf = cv[f[:, 0]]
    return cv, np.array(counts, dtype=np.int64), cf, np.bincount(cf, minlength=len(counts)).astype(np.int64)


def components_fast(nv, f):
    """components() for meshes of a million faces: scipy's labelling of the undirected graph of the edges (f0, f1) and (f1, f2) of every face (the
    third edge joins nothing new), relabelled by rank of each component's smallest vertex."""
    from scipy.sparse import coo_matrix
    from scipy.sparse.csgraph import connected_components
    f = np.asarray(f).astype(np.int64).reshape(-1, 3)
    src, dst = np.concatenate([f[:, 0], f[:, 1]]), np.concatenate([f[:, 1], f[:, 2]])
    graph = coo_matrix((np.ones(src.size, dtype=np.int64), (src, dst)), shape=(nv, nv))     # (int64: a repeated edge sums, and must not wrap to 0)
    count, label = connected_components(graph, directed=False)
    smallest = np.full(count, nv, dtype=np.int64)
    np.minimum.at(smallest, label, np.arange(nv, dtype=np.int64))
    rank = np.empty(count, dtype=np.int64)
    rank[np.argsort(smallest)] = np.arange(count, dtype=np.int64)
    cv = rank[label]
    cf = cv[f[:, 0]]
    return cv, np.bincount(cv, minlength=count).astype(np.int64), cf, np.bincount(cf, minlength=count).astype(np.int64)


def fill_scalar(fill_value, dtype):
    """float(fill_value) to double, then to the grid's dtype: the reference's `(npe_Scalar_grid) flood_value`."""
    return np.array(float(fill_value), dtype=np.float64).astype(dtype)[()]


def flood_fill(grid, seed, fill_value, reference_offsets=False):
    """A copy of grid [w, h, d] in which the cells that == the seed cell's value and can be reached from the seed are set to fill_value.
    Default: a cell's neighbours are its six face neighbours inside the grid. reference_offsets: the reference's arithmetic -- the neighbours
    of offset o are o +- h d, o +- d and o +- 1 wherever 0 <= that offset < w h d, so the last cell of a z row is next to the first cell of
    the following row. Cells are visited once, so fill_value == the seed's value ends (the reference's queue would not) and changes nothing."""
    grid = np.ascontiguousarray(grid)
    w, h, d = grid.shape
    sx, sy, sz = (int(c) for c in seed)
    if not (0 <= sx < w and 0 <= sy < h and 0 <= sz < d):
        raise ValueError("seed point must be inside grid")
    flat = grid.ravel().copy()
    n = flat.size
    start = (sx * h + sy) * d + sz
    match = flat == flat[start]                 # (C++'s ==: -0.0 equals 0.0, NaN equals nothing -- not even the seed itself)
    seen = np.zeros(n, dtype=bool)
    front = np.array([start], dtype=np.int64)
    front = front[match[front]]
    seen[front] = True
    while front.size:
        z, y, x = front % d, (front // d) % h, front // (h * d)
        nxt = []
        for step, coord, size in ((h * d, x, w), (d, y, h), (1, z, d)):
            for sign in (1, -1):
                o = front + sign * step
                ok = (o >= 0) & (o < n) if reference_offsets else (coord + sign >= 0) & (coord + sign < size)
                nxt.append(o[ok])
        o = np.unique(np.concatenate(nxt))
        o = o[match[o] & ~seen[o]]
        seen[o] = True
        front = o
    flat[seen] = fill_scalar(fill_value, grid.dtype)
    return flat.reshape(w, h, d)


def flood_fill_fast(grid, seed, fill_value):
    """flood_fill() (true 6-connectivity) for grids of millions of cells: scipy's labelling of the cells that == the seed's value -- its default
    structure is the six face neighbours --, and the fill value wherever the label is the seed's. A NaN seed equals nothing: no label, no change."""
    from scipy import ndimage
    grid = np.ascontiguousarray(grid)
    seed = tuple(int(c) for c in seed)
    if len(seed) != 3 or not all(0 <= c < s for c, s in zip(seed, grid.shape)):
        raise ValueError("seed point must be inside grid")
    out = grid.copy()
    label, _ = ndimage.label(grid == grid[seed])
    if label[seed] != 0:
        out[label == label[seed]] = fill_scalar(fill_value, grid.dtype)
    return out


def serpentine(n):
    """A corridor one cell wide through an n x n x n grid of walls (0), as one walk from (0, 0, 0): along z on every second y row of every
    second x slab, back and forth, each row joined to the next at the end the walk arrives at, the y order reversed from slab to slab.
    Returns (grid, first cell, number of corridor cells): the last cell is that many steps less one from the first."""
    g = np.zeros((n, n, n), dtype=np.int32)
    k = 0                                                          # rows walked so far: an even one runs towards +z
    for xi, x in enumerate(range(0, n, 2)):
        ys = list(range(0, n, 2))[::-1 if xi % 2 else 1]
        for yi, y in enumerate(ys):
            g[x, y, :] = 1
            end = n - 1 if k % 2 == 0 else 0
            k += 1
            if yi + 1 < len(ys):
                g[x, (y + ys[yi + 1]) // 2, end] = 1
            elif x + 2 < n:
                g[x + 1, y, end] = 1
    return g, (0, 0, 0), int(g.sum())
