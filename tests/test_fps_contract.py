"""tests/fps_contract.py held to first principles (CPU): a scalar loop that cannot be misread, the properties the documentation promises, the
inputs where the tie rule decides, and the monotone-bound claim the grid path's pruning rests on. The import of the package is only there so
that this file, like every test of the operator, fails where the operator is missing."""
import numpy as np
import pytest

import point_cloud_utils_amd as pcu
from fps_contract import box_lower_bound, d2_to, farthest_point_sample

assert callable(pcu.downsample_point_cloud_farthest_point)
DTYPES = [np.float32, np.float64]


def scalar_fps(points, m, start):
    """Pure Python over numpy scalars of the input dtype: one rounding per operation, nothing vectorised."""
    T = points.dtype.type
    n = len(points)
    mind = [T(np.inf)] * n
    chosen, dists = [start], [T(np.inf)]
    while len(chosen) < m:
        s = chosen[-1]
        for i in range(n):
            dx, dy, dz = points[i, 0] - points[s, 0], points[i, 1] - points[s, 1], points[i, 2] - points[s, 2]
            d = ((dx * dx) + (dy * dy)) + (dz * dz)
            if d < mind[i]:
                mind[i] = d
        best = None
        for i in range(n):                      # ascending rows, strict improvement: the lowest row among equals
            if i not in chosen and (best is None or mind[i] > mind[best]):
                best = i
        chosen.append(best)
        dists.append(mind[best])
    return np.array(chosen, np.int64), np.array(dists, points.dtype)


def lattice(k, dtype, seed=None):
    g = np.arange(k, dtype=dtype)
    p = np.stack(np.meshgrid(g, g, g, indexing="ij"), -1).reshape(-1, 3)
    if seed is not None:
        p = p[np.random.default_rng(seed).permutation(len(p))]
    return np.ascontiguousarray(p)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("n, start", [(1, 0), (2, 1), (7, 3), (40, 0), (40, 39)])
def test_equals_the_scalar_loop(dtype, n, start):
    p = np.random.default_rng(n).random((n, 3)).astype(dtype)
    p[n // 2] = p[0]                                        # a duplicate point
    i0, d0 = scalar_fps(p, n, start)
    i1, d1 = farthest_point_sample(p, n, start, squared_distances=True)
    assert np.array_equal(i0, i1) and d0.tobytes() == d1.tobytes()
    i2, d2 = farthest_point_sample(p, n, start)
    assert np.array_equal(i0, i2) and d2.dtype == dtype and d2.tobytes() == np.sqrt(d0).tobytes()


@pytest.mark.parametrize("dtype", DTYPES)
def test_properties(dtype):
    p = np.random.default_rng(5).random((300, 3)).astype(dtype)
    idx, d = farthest_point_sample(p, 300, 17)
    assert idx[0] == 17 and np.isposinf(d[0]) and idx.dtype == np.int64
    assert sorted(idx.tolist()) == list(range(300))                          # num_samples == n: every row once
    assert np.all(d[1:-1] >= d[2:])                                          # non-increasing
    for j in (1, 2, 150):                                                    # prefix property
        ij, dj = farthest_point_sample(p, j, 17)
        assert np.array_equal(ij, idx[:j]) and dj.tobytes() == d[:j].tobytes()
    # dists[t] is the covering radius of the first t samples
    for t in (1, 5, 60):
        cover = np.min(np.stack([d2_to(p, int(s)) for s in idx[:t]]), axis=0).max()
        assert np.sqrt(cover) == d[t]


@pytest.mark.parametrize("dtype", DTYPES)
def test_a_cloud_concatenated_with_itself(dtype):
    """Every point twice: the first n picks are distinct points; then every remaining mind is 0 and the rows follow in ascending order."""
    a = np.random.default_rng(9).random((50, 3)).astype(dtype)
    p = np.concatenate([a, a])
    idx, d = farthest_point_sample(p, 100, 60)
    assert sorted(idx.tolist()) == list(range(100))
    assert len({int(i) % 50 for i in idx[:50]}) == 50 and np.all(d[1:50] > 0) and np.all(d[50:] == 0)
    assert np.array_equal(idx[50:], np.sort(idx[50:]))
    assert np.array_equal(farthest_point_sample(np.zeros((9, 3), dtype), 9, 4)[0], [4, 0, 1, 2, 3, 5, 6, 7, 8])      # all identical


def test_the_lattice_is_decided_by_the_tie_rule():
    """9^3 integer lattice: the arg-max is tied at 189 of the first 200 steps, so the lowest-row rule decides nearly every pick."""
    p = lattice(9, np.float32)
    idx, d = farthest_point_sample(p, 201, 0, squared_distances=True)
    tied, mind, sel = 0, np.full(len(p), np.inf, np.float32), np.zeros(len(p), bool)
    for t in range(1, 201):
        mind = np.minimum(mind, d2_to(p, int(idx[t - 1]))); sel[idx[t - 1]] = True
        c = np.where(sel, -1, mind)
        tied += int(np.sum(c == c.max()) > 1)
        assert idx[t] == np.flatnonzero(c == c.max())[0]
    assert tied == 189


def test_overflowing_distances_follow_the_rule():
    # rows at least 1e20 apart along x: every d2 is 1e40 at least, +inf in float32; all ties, all the time
    p = np.random.default_rng(2).permutation(20).astype(np.float32)[:, None] * np.array([1e20, -2e20, 5e19], np.float32)
    idx, d = farthest_point_sample(p, 20, 5)
    assert np.all(np.isinf(d)) and np.array_equal(idx, [5] + [i for i in range(20) if i != 5])


@pytest.mark.parametrize("dtype", DTYPES)
def test_the_box_bound_is_never_above_a_computed_distance(dtype):
    """2000 random boxes per dtype, 64 points each, scales 1e-3 .. 1e6, offsets up to 1e6, and integer lattices (exact ties with the bound)."""
    rng = np.random.default_rng(11)
    T = dtype
    for trial in range(2000):
        scale, off = T(10.0 ** rng.uniform(-3, 6)), T(rng.uniform(-1, 1) * 10.0 ** rng.uniform(0, 6))
        if trial % 4 == 0:
            pts = rng.integers(-4, 5, (64, 3)).astype(T) * scale + off
            s = rng.integers(-8, 9, 3).astype(T) * scale + off
        else:
            pts = (rng.random((64, 3)).astype(T) * scale + off).astype(T)
            s = ((rng.random(3).astype(T) * T(3) - T(1)) * scale + off).astype(T)
        lo, hi = pts.min(axis=0), pts.max(axis=0)
        d = pts - s
        d2 = ((d[:, 0] * d[:, 0]) + (d[:, 1] * d[:, 1])) + (d[:, 2] * d[:, 2])
        assert box_lower_bound(lo, hi, s) <= d2.min(), (trial, scale, off)
