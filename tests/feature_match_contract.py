"""The contract of match_point_features in numpy. With T the input dtype, a the (n, D) query rows and b the (m, D) dataset rows:
  d2(i, j) = the sum over c = 0 .. D - 1, left to right, of (a_ic - b_jc) * (a_ic - b_jc) in T (numpy rounds every elementwise product and sum
  on its own: no FMA; the columns are added one at a time, no pairwise or blocked sum);
  nearest[i] = the j of the smallest (d2, j); a pair whose d2 is NaN is no candidate (+inf is one); a row with no candidate gets -1 and T(inf);
  is_mutual[i] iff nearest[i] >= 0 and the same rule from the dataset to the queries sends row nearest[i] back to i.
What the library refuses is not this module's business."""
import numpy as np

_CHUNK = 1 << 22          # pairs per block of the brute force


def squared_distances(a, b):
    """(len(a), len(b)) array of d2 in the inputs' dtype."""
    assert a.dtype == b.dtype and a.dtype in (np.float32, np.float64) and a.shape[1] == b.shape[1]
    d2 = np.zeros((len(a), len(b)), dtype=a.dtype)
    with np.errstate(all="ignore"):
        for c in range(a.shape[1]):
            df = a[:, None, c] - b[None, :, c]
            d2 = d2 + df * df              # (the first step adds to +0: exact)
    assert d2.dtype == a.dtype
    return d2


def _one_way(a, b):
    n, m = len(a), len(b)
    nearest = np.full(n, -1, dtype=np.int64)
    best = np.full(n, np.inf, dtype=a.dtype)
    step = max(1, _CHUNK // max(m, 1))
    for lo in range(0, n, step):
        d2 = squared_distances(a[lo:lo + step], b)
        cand = ~np.isnan(d2)
        key = np.where(cand, d2, np.inf)
        j = (cand & (key == key.min(axis=1, keepdims=True))).argmax(axis=1)       # the first candidate at the minimum: the lower row (+inf is one)
        rows = np.arange(len(d2))
        has = cand.any(axis=1)
        nearest[lo:lo + step] = np.where(has, j, -1)
        best[lo:lo + step] = np.where(has, d2[rows, j], np.inf)
    return nearest, best


def match(query_features, dataset_features, mutual=False):
    """nearest (n,) int64, d2 (n,) in the input dtype and, with mutual, is_mutual (n,) bool."""
    a, b = np.ascontiguousarray(query_features), np.ascontiguousarray(dataset_features)
    nearest, best = _one_way(a, b)
    if not mutual:
        return nearest, best
    back, _ = _one_way(b, a)
    is_mutual = (nearest >= 0) & (back[np.maximum(nearest, 0)] == np.arange(len(a)))
    return nearest, best, is_mutual
