"""The contract of cluster_point_cloud_dbscan in numpy, by brute force on radius_contract's arithmetic. With T the dtype:
  j is a neighbour of i iff d2(i, j) < r2, d2 = ((dx*dx) + (dy*dy)) + (dz*dz) in T, r2 = T(eps) * T(eps) (strict; a point is its own neighbour
  when eps > 0; d2 is symmetric, so the graph is undirected; a non-finite d2 is never below r2);
  i is core iff it has at least min_points neighbours, itself included;
  the clusters are the connected components of the core points under that relation, numbered from 0 in the order of their smallest core row;
  a point that is not core takes the label of its nearest core neighbour -- smallest (d2, row) -- or -1 when it has none.
What the library refuses is not this module's business."""
import numpy as np

from radius_contract import _CHUNK, r2_of, squared_distances


def _rows_in_blocks(n):
    step = max(1, _CHUNK // max(n, 1))
    return [(a, min(a + step, n)) for a in range(0, n, step)]


def membership(p, eps):
    """(n, n) bool: member[i, j] iff j is a neighbour of i."""
    n = len(p)
    r2 = r2_of(eps, p.dtype)
    member = np.empty((n, n), dtype=bool)
    for a, b in _rows_in_blocks(n):
        with np.errstate(all="ignore"):
            member[a:b] = squared_distances(p[a:b], p) < r2
    return member


def dbscan(points, eps, min_points):
    """labels (n,) int64 (-1: noise), is_core (n,) bool."""
    p = np.ascontiguousarray(points)
    n = len(p)
    member = membership(p, eps)
    core = member.sum(axis=1, dtype=np.int64) >= int(min_points)
    rows = np.flatnonzero(core)                                  # ascending: position among them orders as the dataset row does
    among = member[np.ix_(rows, rows)]
    lab = np.full(len(rows), -1, dtype=np.int64)
    k = 0
    for s in range(len(rows)):                                   # the smallest core row not reached yet opens the next cluster
        if lab[s] >= 0:
            continue
        lab[s] = k
        frontier = np.array([s])
        while frontier.size:                                     # breadth first, a level at a time over rows of the membership matrix
            frontier = np.flatnonzero(among[frontier].any(axis=0) & (lab < 0))
            lab[frontier] = k
        k += 1
    labels = np.full(n, -1, dtype=np.int64)
    labels[rows] = lab
    rest = np.flatnonzero(~core)
    if len(rows) and len(rest):
        r2 = r2_of(eps, p.dtype)
        step = max(1, _CHUNK // len(rows))
        for a in range(0, len(rest), step):
            mine = rest[a:a + step]
            d2 = squared_distances(p[mine], p[rows])
            with np.errstate(all="ignore"):
                near = np.where(d2 < r2, d2, np.inf)
            j = near.argmin(axis=1)                              # the first of equal minima: the smaller row
            has = np.isfinite(near[np.arange(len(mine)), j])
            labels[mine[has]] = lab[j[has]]
    return labels, core
