"""The contract of radius_search / radius_count in numpy, by brute force. With T the input dtype:
  d2 = ((dx*dx) + (dy*dy)) + (dz*dz) in T, query minus dataset (numpy rounds every elementwise product and sum on its own: no FMA);
  r2 = T(radius) * T(radius), one multiply rounded in T; dataset row j is a member of query i iff d2 < r2 (strict);
  a row is ascending by (d2, dataset row); dists = sqrt(d2) correctly rounded in T (numpy's sqrt is), or d2 itself.
A non-finite d2 (a non-finite query or dataset row) is never below r2. What the library refuses is not this module's business."""
import numpy as np

_CHUNK = 1 << 22          # pairs per block of the brute force


def squared_distances(q, p):
    """(len(q), len(p)) array of d2 in the inputs' dtype."""
    assert q.dtype == p.dtype and q.dtype in (np.float32, np.float64)
    with np.errstate(all="ignore"):
        dx = q[:, None, 0] - p[None, :, 0]
        dy = q[:, None, 1] - p[None, :, 1]
        dz = q[:, None, 2] - p[None, :, 2]
        d2 = ((dx * dx) + (dy * dy)) + (dz * dz)
    assert d2.dtype == q.dtype
    return d2


def r2_of(radius, dtype):
    T = np.dtype(dtype).type
    with np.errstate(all="ignore"):
        return T(T(radius) * T(radius))


def radius_search(q, p, radius, squared_distances_out=False):
    """offsets (n + 1,) int64, indices (total,) int64, dists (total,) in the input dtype; every row ascending by (d2, dataset row)."""
    q, p = np.ascontiguousarray(q), np.ascontiguousarray(p)
    n, m = len(q), len(p)
    r2 = r2_of(radius, q.dtype)
    counts = np.zeros(n, dtype=np.int64)
    idx_parts, d2_parts = [], []
    step = max(1, _CHUNK // max(m, 1))
    for a in range(0, n, step):
        d2 = squared_distances(q[a:a + step], p)
        with np.errstate(all="ignore"):
            member = d2 < r2
        i, j = np.nonzero(member)                    # i ascending, j ascending inside a row
        v = d2[i, j]
        order = np.lexsort((j, v, i))                # by row, then d2, then dataset row
        counts[a:a + step] = np.bincount(i, minlength=len(d2))
        idx_parts.append(j[order].astype(np.int64)); d2_parts.append(v[order])
    offsets = np.zeros(n + 1, dtype=np.int64)
    np.cumsum(counts, out=offsets[1:])
    indices = np.concatenate(idx_parts) if idx_parts else np.zeros(0, np.int64)
    d2 = np.concatenate(d2_parts) if d2_parts else np.zeros(0, q.dtype)
    dists = d2 if squared_distances_out else np.sqrt(d2)
    assert dists.dtype == q.dtype
    return offsets, indices, dists


def radius_count(q, p, radius):
    off = radius_search(q, p, radius)[0]
    return off[1:] - off[:-1]


def rows(offsets, *arrays):
    """The rows of a ragged result as a list of tuples of arrays."""
    return [tuple(a[offsets[i]:offsets[i + 1]] for a in arrays) for i in range(len(offsets) - 1)]
