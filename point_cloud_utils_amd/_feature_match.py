"""match_point_features: the nearest row in a feature space of up to 128 dimensions over the HIP kernels of csrc/feature_match.h. Not in the
reference's API; the values follow this library's stated contract (in numpy: tests/feature_match_contract.py)."""
import numpy as np

from ._call import _Dev, _call, _int_out
from ._checks import _check_features


def match_point_features(query_features, dataset_features, mutual=False):
    """
    For every row of query_features, find the nearest row of dataset_features (squared L2 distance over all D columns)

    Args:
        query_features : n by D array (float32 or float64; numpy, or a CUDA/HIP torch tensor), 1 <= D <= 128, for instance compute_point_cloud_fpfh's
        dataset_features : m by D array of the same dtype and kind
        mutual : If True, also return which matches hold in both directions. Default is False.

    Returns:
        nearest : (n,) int64: the row of dataset_features nearest to every query row, -1 where there is none
        d2 : (n,) array in the input dtype: the squared distance to it, +inf where there is none
        is_mutual : (if mutual) (n,) bool: nearest[i] >= 0 and query row i is the nearest query row of dataset row nearest[i]
        (numpy arrays in, numpy arrays out; CUDA/HIP torch tensors in, tensors on the same device out)

    Notes:
        The contract, exact to the byte, T the input dtype: d2(i, j) is the sum over c = 0 .. D - 1, left to right, of
        (a_ic - b_jc) * (a_ic - b_jc) in T, separate multiplies and adds. nearest[i] is the j of the smallest (d2, j): among equal distances
        the lower row wins. A pair whose d2 is NaN is no candidate (+inf is one), so a row with a NaN matches nothing and nothing matches it.
        The search in the other direction uses the same d2 and the same rule with queries and dataset exchanged.
        ValueError: a dtype that is not float32 or float64, or two that differ; zero rows; two arrays with different D; D outside [1, 128];
        more than 2^27-16 rows.
    """
    n, m, dims = _check_features(query_features, dataset_features)
    d = _Dev(query_features, dataset_features)
    nearest = d.empty((n,), "i64")
    d2 = d.empty((n,), "T")
    is_mutual = _int_out(d, (n,), np.bool_) if mutual else None
    _call("match_features", d, d.pa, n, d.pb, m, dims, _Dev.ptr(nearest), _Dev.ptr(d2), _Dev.ptr(is_mutual))
    return (nearest, d2, is_mutual) if mutual else (nearest, d2)
