"""tests/feature_match_contract.py, the definition of match_point_features, against np.argmin of a float64 distance matrix where both are
exact, and on its edges: ties, NaN rows, +inf distances, D = 1. No GPU."""
import numpy as np
import pytest

import feature_match_contract as mc


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("D", [1, 3, 33, 128])
def test_integer_valued_features_against_argmin(dtype, D):
    """Integers below 2^6 in up to 128 columns: every difference, square and partial sum is an integer below 2^24, exact in both dtypes and in
    any order, so a float64 matrix product form and np.argmin give the same answer."""
    rng = np.random.default_rng(D)
    a = rng.integers(0, 64, (70, D)).astype(dtype)
    b = rng.integers(0, 64, (90, D)).astype(dtype)
    a64, b64 = a.astype(np.float64), b.astype(np.float64)
    full = (a64 * a64).sum(axis=1)[:, None] + (b64 * b64).sum(axis=1)[None, :] - 2.0 * (a64 @ b64.T)
    nearest, d2, mutual = mc.match(a, b, mutual=True)
    assert nearest.dtype == np.int64 and d2.dtype == dtype and mutual.dtype == np.bool_
    assert np.array_equal(nearest, full.argmin(axis=1))
    assert np.array_equal(d2, full.min(axis=1).astype(dtype))
    back = full.argmin(axis=0)
    assert np.array_equal(mutual, back[nearest] == np.arange(len(a)))


def test_ties_go_to_the_lower_row():
    a = np.array([[0.0, 0.0], [5.0, 5.0]], dtype=np.float32)
    b = np.array([[1.0, 0.0], [0.0, 1.0], [-1.0, 0.0], [5.0, 5.0], [5.0, 5.0]], dtype=np.float32)
    nearest, d2, mutual = mc.match(a, b, mutual=True)
    assert nearest.tolist() == [0, 3] and d2.tolist() == [1.0, 0.0]
    assert mutual.tolist() == [True, True]              # dataset rows 0 and 3 send back 0 and 1; the duplicate row 4 has no say
    nearest, _, mutual = mc.match(b, a, mutual=True)
    assert nearest.tolist() == [0, 0, 0, 1, 1] and mutual.tolist() == [True, False, False, True, False]


def test_nan_rows_match_nothing_and_nothing_matches_them():
    a = np.array([[0.0, 0.0], [np.nan, 1.0], [3.0, 3.0]], dtype=np.float64)
    b = np.array([[np.nan, 0.0], [3.0, 2.0]], dtype=np.float64)
    nearest, d2, mutual = mc.match(a, b, mutual=True)
    assert nearest.tolist() == [1, -1, 1] and d2.tolist() == [13.0, np.inf, 1.0]
    assert mutual.tolist() == [False, False, True]
    nearest, d2 = mc.match(a, b[:1])
    assert nearest.tolist() == [-1, -1, -1] and np.isposinf(d2).all() and d2.dtype == np.float64


def test_an_infinite_distance_is_a_candidate():
    big = np.finfo(np.float32).max
    a = np.array([[big]], dtype=np.float32)
    b = np.array([[np.nan], [-big], [-big]], dtype=np.float32)
    nearest, d2 = mc.match(a, b)
    assert nearest.tolist() == [1] and np.isposinf(d2[0])


def test_one_column_and_one_row():
    a = np.array([[0.25], [10.0], [-4.0]], dtype=np.float32)
    b = np.array([[9.0], [0.0], [-3.5]], dtype=np.float32)
    nearest, d2, mutual = mc.match(a, b, mutual=True)
    assert nearest.tolist() == [1, 0, 2] and d2.tolist() == [0.0625, 1.0, 0.25] and mutual.all()
    nearest, d2 = mc.match(a[:1], b[:1])
    assert nearest.tolist() == [0] and d2.tolist() == [76.5625]


def test_the_sum_runs_left_to_right_in_the_input_dtype():
    """(2^12)^2 + 1 + 1 in float32: left to right both ones are lost, right to left they add up first and survive."""
    a = np.zeros((1, 3), np.float32)
    b = np.array([[4096.0, 1.0, 1.0]], dtype=np.float32)
    assert mc.match(a, b)[1].tolist() == [16777216.0]
    assert mc.match(a, b[:, ::-1].copy())[1].tolist() == [16777218.0]
