"""The contract of downsample_point_cloud_farthest_point, restated in numpy. No library import: the GPU is held to this file
byte for byte (tests/test_gpu_fps.py), and this file to first principles (tests/test_fps_contract.py).

With T the input dtype: d2(i, s) = ((dx*dx) + (dy*dy)) + (dz*dz) in T, dx = x_i - x_s, separate multiplies and adds (numpy fuses nothing).
mind[i] = +inf for every row and idx[0] = start_index. After row s is selected, mind[i] = min(mind[i], d2(i, s)) for every row and s is
excluded from all later arg-maxes; the next sample is the unselected row of largest mind, the lowest row among exactly equal values.
dists[0] = +inf; dists[t] = mind[idx[t]] at the moment of its selection, as the correctly rounded sqrt in T, or as it is."""
import numpy as np


def d2_to(points, s):
    """d2(i, s) for every row i, in the dtype of points."""
    with np.errstate(over="ignore", invalid="ignore"):
        d = points - points[s]
        return ((d[:, 0] * d[:, 0]) + (d[:, 1] * d[:, 1])) + (d[:, 2] * d[:, 2])


def farthest_point_sample(points, num_samples, start_index=0, squared_distances=False):
    """(idx int64 (num_samples,), dists (num_samples,) in the dtype of points)."""
    points = np.ascontiguousarray(points)
    T = points.dtype.type
    n = points.shape[0]
    assert points.ndim == 2 and points.shape[1] == 3 and 1 <= num_samples <= n and 0 <= start_index < n
    mind = np.full(n, np.inf, dtype=T)
    selected = np.zeros(n, dtype=bool)
    idx = np.empty(num_samples, dtype=np.int64)
    dists = np.empty(num_samples, dtype=T)
    idx[0], dists[0] = start_index, np.inf
    for t in range(1, num_samples):
        s = int(idx[t - 1])
        mind = np.minimum(mind, d2_to(points, s))
        selected[s] = True
        cand = np.where(selected, T(-1), mind)          # mind is never negative: a selected row loses to every unselected one
        nxt = int(np.argmax(cand))                      # (numpy: the first, i.e. lowest, row among equal maxima)
        idx[t], dists[t] = nxt, mind[nxt]
    if not squared_distances:
        dists = np.sqrt(dists)                          # correctly rounded (IEEE 754) in T
    return idx, dists


def box_lower_bound(lo, hi, s):
    """The bound of the grid path for a box [lo, hi] and a sample s, in their dtype: lb = ((gx*gx) + (gy*gy)) + (gz*gz), g = max(lo - s, s - hi, 0)
    per axis. Claim: lb <= d2(p, s) as computed, for every p with lo <= p <= hi, because rounded subtraction, multiplication and addition are
    monotone. So a bucket with lb >= its largest mind cannot change, exactly."""
    T = lo.dtype.type
    with np.errstate(over="ignore", invalid="ignore"):
        g = np.maximum(np.maximum(lo - s, s - hi), T(0))
        return ((g[..., 0] * g[..., 0]) + (g[..., 1] * g[..., 1])) + (g[..., 2] * g[..., 2])
