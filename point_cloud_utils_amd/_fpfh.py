"""compute_point_cloud_fpfh: Fast Point Feature Histograms of an oriented cloud over the HIP kernels of csrc/fpfh.h. Not in the reference's API;
the values follow this library's stated contract (in numpy: tests/fpfh_contract.py)."""
import numpy as np

from ._call import _Dev, _call, _int_out, _is_torch
from ._checks import _check_normals, _check_radius, _check_rows, _host_searched_cloud


def compute_point_cloud_fpfh(points, normals, radius, return_spfh=False):
    """
    Describe the local shape around every point of an oriented cloud by a Fast Point Feature Histogram (Rusu et al. 2009): 33 numbers per point

    Args:
        points : n by 3 array of points (float32 or float64; numpy, or a CUDA/HIP torch tensor)
        normals : n by 3 array of normals (the points' dtype and kind), for instance orient_point_cloud_normals'; used as given, not renormalised
        radius : the neighbourhood radius (L2 distance); finite and not negative
        return_spfh : If True, also return the integer histograms of every point's own pairs. Default is False.

    Returns:
        features : (n, 33) array in the input dtype: three histograms of 11 bins, [theta 0..10 | f2 11..21 | f3 22..32]
        spfh_counts : (if return_spfh) (n, 33) int32
        (numpy arrays in, numpy arrays out; CUDA/HIP torch tensors in, tensors on the same device out)
        These are what match_point_features takes as features.

    Notes:
        The contract, T the input dtype. The neighbours of point i are its row of radius_search(points, points, radius) without
        i: d2 = ((dx*dx) + (dy*dy)) + (dz*dz) < T(radius) * T(radius) in T, strict: radius == 0 gives all zeros, a point exactly at the radius
        is out. A row whose normal has a non-finite component or is (0, 0, 0) is invalid: it takes part in no pair and its rows are zero.
        For a pair (i, j), in float64 on values promoted from T, every product, sum, division and square root rounded once and none fused:
        dp = p_j - p_i, len = |dp| (len == 0: no pair), a1 = (n_i . dp) / len, a2 = (n_j . dp) / len; if |a1| < |a2| the roles swap (n1 = n_j,
        n2 = n_i, dp = -dp, f3 = -a2), else n1 = n_i, n2 = n_j, f3 = a1; u = dp / len, v = u x n1 (|v| == 0: no pair), v = v / |v|, w = n1 x v,
        f2 = v . n2, theta = atan2(w . n2, n1 . n2). f2 and f3 fall into bin min(max(floor(11 * ((f + 1) * 0.5)), 0), 10) (a NaN: bin 0). The
        bin of theta is decided without atan2, by the signs of C_b * y - S_b * x against the ten inner bin edges (C_b, S_b the float64 nearest
        cosine and sine of -pi + 2 pi b / 11): y < 0 counts the edges 1..5 it has passed, any other y gives 5 plus the count over 6..10. So
        x = y = 0 lands in bin 10, and so does y = -0.0 with x < 0: stated, not an accident.
        spfh_counts[i] counts the bins of the pairs (i, j) over the valid neighbours j and equals the contract exactly; k_i is the sum of one
        group. S_i = 100 * c_i / k_i (0 where k_i == 0), W_i = the sum over the neighbours j with d2 > 0 of S_j / float64(d2), and group by
        group F_i = S_i + 100 * W_i / sum(W_i over the group) (the second term 0 where that sum is 0); features = T(F). This is the paper's
        weighted form with PCL's normalisation per group -- every group of a row with pairs and weights sums to 200 -- and it is this
        library's stated contract, not PCL's or Open3D's bytes: neither was on hand to compare with. The order of the sums W is the grid
        walk's, a function of the arguments: equal arguments give equal bytes, numpy and tensors alike, and against the contract's ascending
        j an entry differs by at most (2 * m_i + 8) * 2**-52 * 200 before it is rounded to T (m_i: the neighbours of row i).
        last_stats(): n_tie_flagged / n_tie_true are the waves of the first walk that staged the union of their lanes' cells / that did not.
        ValueError: the scalar-type and shape checks of orient_point_cloud_normals, with its texts; the row limit; a radius that is NaN,
        negative or infinite (radius_search's text); a cloud with NaN, or with +inf and -inf on one axis (the k-NN calls' text).
    """
    _, n = _check_normals(points, normals, False)
    _check_rows(n)
    radius = _check_radius(radius)
    if not (_is_torch(points) or _is_torch(normals)):
        _host_searched_cloud(np.asarray(points))
    d = _Dev(points, normals)
    features = d.empty((n, 33), "T")
    counts = _int_out(d, (n, 33), np.int32) if return_spfh else None
    _call("fpfh", d, d.pa, d.pb, n, radius, _Dev.ptr(features), _Dev.ptr(counts))
    return (features, counts) if return_spfh else features
