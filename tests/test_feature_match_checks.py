"""The refusals of match_point_features, every text in full, raised before anything touches the device: the library is replaced by an object
that fails the test when it is asked for anything. No GPU."""
import inspect

import numpy as np
import pytest

import point_cloud_utils_amd as pcu
from point_cloud_utils_amd import _checks, _lib


@pytest.fixture(autouse=True)
def no_device(monkeypatch):
    def refuse(*a, **k):
        raise AssertionError("the call reached the library")
    monkeypatch.setattr(_lib, "lib", refuse)
    monkeypatch.setattr(_lib, "ctx", refuse)


def raises(text, *args, **kw):
    with pytest.raises(ValueError) as e:
        pcu.match_point_features(*args, **kw)
    assert str(e.value) == text


A = np.random.default_rng(1).random((10, 33))
B = np.random.default_rng(2).random((7, 33))


def test_scalar_types():
    raises("Invalid scalar type (int64) for argument 'query_features'. Expected one of ['float32', 'float64'].", np.zeros((10, 33), np.int64), B)
    raises("Invalid scalar type (float16) for argument 'query_features'. Expected one of ['float32', 'float64'].", A.astype(np.float16), B)
    raises("Invalid scalar type (float32) for argument 'dataset_features'. Expected it to match argument 'query_features' which is of type float64.",
           A, B.astype(np.float32))
    raises("Invalid scalar type (int32) for argument 'dataset_features'. Expected it to match argument 'query_features' which is of type float32.",
           A.astype(np.float32), B.astype(np.int32), mutual=True)


def test_shapes():
    raises("Invalid input set with zero elements: query_features and dataset_features must have shape (n, D) and (m, D). "
           "Got query_features.shape = (0, 33), dataset_features.shape = (7, 33).", A[:0], B)
    raises("Invalid input set with zero elements: query_features and dataset_features must have shape (n, D) and (m, D). "
           "Got query_features.shape = (10, 33), dataset_features.shape = (0, 5).", A, B[:0, :5])
    raises("Invalid feature dimension: query_features and dataset_features must have the same number of columns. "
           "Got query_features.shape = (10, 33), dataset_features.shape = (7, 32).", A, B[:, :32])
    raises("Invalid feature dimension: query_features and dataset_features must have the same number of columns. "
           "Got query_features.shape = (10, 1), dataset_features.shape = (7, 33).", A[:, 0], B)          # (a 1-D array is one column)
    raises("Invalid feature dimension (0): must be in [1, 128].", A[:, :0], B[:, :0])
    raises("Invalid feature dimension (129): must be in [1, 128].", np.zeros((4, 129)), np.zeros((3, 129)), True)
    raises("Invalid number of dimensions (3): expected a matrix of shape (n, 3).", np.zeros((4, 3, 3)), B)
    big = np.broadcast_to(np.zeros((1, 1), np.float32), (2 ** 27 - 15, 1))
    raises("point clouds with more than 2^27-16 rows are not supported", big, np.zeros((1, 1), np.float32))
    raises("point clouds with more than 2^27-16 rows are not supported", np.zeros((1, 1), np.float32), big)


def test_the_order_of_the_checks():
    """Scalar types, zero rows, one D for both, the range of D, the row limit."""
    raises("Invalid scalar type (float32) for argument 'dataset_features'. Expected it to match argument 'query_features' which is of type float64.",
           A[:0], B[:, :2].astype(np.float32))
    raises("Invalid input set with zero elements: query_features and dataset_features must have shape (n, D) and (m, D). "
           "Got query_features.shape = (0, 33), dataset_features.shape = (7, 2).", A[:0], B[:, :2])
    big = np.broadcast_to(np.zeros((1, 129), np.float32), (2 ** 27 - 15, 129))
    raises("Invalid feature dimension (129): must be in [1, 128].", big, big)


def test_accepted_edges():
    assert _checks._check_features(A, B) == (10, 7, 33)
    assert _checks._check_features(A[:, :1], B[:1, :1]) == (10, 1, 1)
    assert _checks._check_features(np.zeros((2, 128), np.float32), np.zeros((1, 128), np.float32)) == (2, 1, 128)
    assert _checks._check_features(A[:, 0], B[:, 0]) == (10, 7, 1)
    assert "match_point_features" in pcu.__all__ and callable(pcu.match_point_features)
    assert str(inspect.signature(pcu.match_point_features)) == "(query_features, dataset_features, mutual=False)"
    # NaN and infinite VALUES are allowed: the contract says what they match (the call goes on to the library, which this test has replaced)
    bad = A.copy()
    bad[3, 3] = np.nan
    with pytest.raises(AssertionError, match="the call reached the library"):
        pcu.match_point_features(bad, B)
