"""tests/radius_contract.py against what DESIGN.md row f18 says, on inputs where every d2 is exact (small integers): strictness, radius 0, an
independent exact computation, radius_count, and the order of ties. No GPU."""
import itertools

import numpy as np
import pytest

import radius_contract as rc


def lattice(k, dtype):
    return np.array(list(itertools.product(range(k), repeat=3)), dtype=dtype)


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("radius", [1.0, 2.0, 3.0])
def test_strict_on_an_integer_lattice(dtype, radius):
    p = lattice(7, dtype)
    off, idx, d2 = rc.radius_search(p, p, radius, squared_distances_out=True)
    exact = ((p[:, None, :].astype(np.int64) - p[None, :, :].astype(np.int64)) ** 2).sum(-1)
    r2 = int(radius * radius)
    assert (exact == r2).sum() > 300                         # many pairs at exactly the radius ...
    assert np.array_equal(off[1:] - off[:-1], (exact < r2).sum(1))
    assert not (d2 == r2).any() and (d2 < r2).all()         # ... and none of them is a member
    for i, (j, v) in enumerate(rc.rows(off, idx, d2)):
        assert np.array_equal(np.sort(j), np.nonzero(exact[i] < r2)[0])
        assert np.array_equal(v, exact[i, j].astype(dtype))
        key = list(zip(v.tolist(), j.tolist()))
        assert key == sorted(key)                            # ascending by (d2, row): ties by row
    ties = sum(len(v) - len(np.unique(v)) for _, v in rc.rows(off, idx, d2))
    assert radius == 1.0 or ties > 1000


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_radius_zero_gives_empty_rows(dtype):
    p = lattice(3, dtype)
    off, idx, d = rc.radius_search(p, p, 0.0)                # every query coincides with a dataset row
    assert np.array_equal(off, np.zeros(len(p) + 1, np.int64)) and idx.shape == (0,) and d.shape == (0,)
    assert idx.dtype == np.int64 and d.dtype == dtype
    assert np.array_equal(rc.radius_count(p, p, 0.0), np.zeros(len(p), np.int64))


def test_against_an_exact_float64_computation():
    rng = np.random.default_rng(5)
    q = rng.integers(-40, 40, (200, 3)).astype(np.float32)
    p = rng.integers(-40, 40, (900, 3)).astype(np.float32)
    exact = ((q[:, None, :].astype(np.float64) - p[None, :, :].astype(np.float64)) ** 2).sum(-1)      # integers below 2^24: exact in both types
    for radius in (0.5, 7.0, 13.0, 200.0):
        off, idx, d = rc.radius_search(q, p, radius)
        r2 = float(np.float32(radius) * np.float32(radius))
        assert np.array_equal(rc.radius_count(q, p, radius), (exact < r2).sum(1))
        for i, (j, v) in enumerate(rc.rows(off, idx, d)):
            want = np.nonzero(exact[i] < r2)[0]
            want = want[np.lexsort((want, exact[i, want]))]
            assert np.array_equal(j, want)
            assert np.array_equal(v, np.sqrt(exact[i, want]).astype(np.float32))       # (sqrt of an exact float32 value: double rounding cannot change it at 53 >= 2 * 24 + 2 bits)


def test_count_equals_row_lengths_and_dtypes():
    rng = np.random.default_rng(6)
    for dtype in (np.float32, np.float64):
        q, p = rng.random((50, 3)).astype(dtype), rng.random((400, 3)).astype(dtype)
        off, idx, d = rc.radius_search(q, p, 0.3)
        c = rc.radius_count(q, p, 0.3)
        assert c.dtype == np.int64 and off.dtype == np.int64 and idx.dtype == np.int64 and d.dtype == dtype
        assert np.array_equal(c, off[1:] - off[:-1]) and off[-1] == len(idx) == len(d) and off[-1] > 0
        off2, idx2, d2 = rc.radius_search(q, p, 0.3, squared_distances_out=True)
        assert np.array_equal(off2, off) and np.array_equal(idx2, idx) and np.array_equal(np.sqrt(d2), d)


def test_ties_are_ordered_by_dataset_row():
    p = np.zeros((9, 3), np.float32)
    p[[1, 4, 6]] = [3.0, 0.0, 0.0]                           # rows 0 2 3 5 7 8 at distance 0, rows 1 4 6 at distance 3
    off, idx, d = rc.radius_search(np.zeros((1, 3), np.float32), p, 4.0)
    assert idx.tolist() == [0, 2, 3, 5, 7, 8, 1, 4, 6] and d.tolist() == [0.0] * 6 + [3.0] * 3


def test_nonfinite_rows_are_nobodys_members():
    p = np.array([[0, 0, 0], [np.inf, 0, 0], [1, 0, 0]], np.float64)
    q = np.array([[0, 0, 0], [np.nan, 0, 0], [np.inf, 0, 0]], np.float64)
    off, idx, _ = rc.radius_search(q, p, 1e300)              # (r2 overflows to +inf: every finite d2 is below it, no other)
    assert off.tolist() == [0, 2, 2, 2] and idx.tolist() == [0, 2]
