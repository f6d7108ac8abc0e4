"""tests/dbscan_contract.py itself, the numpy statement of cluster_point_cloud_dbscan's contract: hand-made cases with known
answers, the core mask against radius_contract.radius_count, and scikit-learn's DBSCAN where it is installed -- core mask, core labels and
noise set are equal; a border point may go to another of its neighbouring clusters there (first reached, not nearest). No GPU."""
import numpy as np
import pytest

import dbscan_contract as dc
import radius_contract as rc

DTYPES = [np.float32, np.float64]


def answer(points, eps, min_points, labels, core):
    got_labels, got_core = dc.dbscan(points, eps, min_points)
    assert got_labels.dtype == np.int64 and got_core.dtype == np.bool_
    assert got_labels.tolist() == list(labels), got_labels
    assert got_core.tolist() == [bool(c) for c in core], got_core


# Two clusters of four cores each and one point between them (DBSCAN's border case), min_points = 4: a hub at x = -+1 and three points 0.9
# beyond it. Each hub has itself, its three and the middle point within eps; each of the three has itself, the other two and its hub. The
# middle point has itself and the two hubs: three, so it is not core.
def _hub(x, sign):
    return [[x, 0.0, 0.0], [x + sign * 0.9, 0.0, 0.0], [x + sign * 0.9, 0.1, 0.0], [x + sign * 0.9, -0.1, 0.0]]


@pytest.mark.parametrize("dtype", DTYPES)
def test_two_blobs_and_a_far_point(dtype):
    rng = np.random.default_rng(0)
    a = rng.random((5, 3)) * 0.1
    b = rng.random((5, 3)) * 0.1 + [10.0, 0.0, 0.0]
    p = np.concatenate([a, b, [[100.0, 100.0, 100.0]]]).astype(dtype)
    answer(p, 0.5, 3, [0] * 5 + [1] * 5 + [-1], [1] * 10 + [0])
    order = [5, 0, 10, 6, 1, 7, 2, 8, 3, 9, 4]                      # the second blob now holds the smallest row: it is cluster 0
    answer(p[order], 0.5, 3, [0, 1, -1, 0, 1, 0, 1, 0, 1, 0, 1], [1, 1, 0] + [1] * 8)


@pytest.mark.parametrize("dtype", DTYPES)
def test_chain_is_linked_below_eps_and_not_at_eps(dtype):
    n = 20
    p = np.zeros((n, 3), dtype)
    p[:, 0] = 0.25 * np.arange(n)                                    # spacing 0.25: the next point is in, the one after it lies at exactly eps and is out
    answer(p, 0.5, 2, [0] * n, [1] * n)
    answer(p, 0.5, 3, [0] * n, [0] + [1] * (n - 2) + [0])           # the two ends have two neighbours: border points of the one cluster
    p[:, 0] = 0.5 * np.arange(n)                                     # spacing exactly eps: d2 == r2, strict comparison, nothing is linked
    answer(p, 0.5, 1, list(range(n)), [1] * n)
    answer(p, 0.5, 2, [-1] * n, [0] * n)


@pytest.mark.parametrize("dtype", DTYPES)
def test_coincident_copies(dtype):
    for min_points in (2, 5):
        far = np.array([[50.0, 0.0, 0.0]], dtype)
        few = np.concatenate([np.full((min_points - 1, 3), 0.25, dtype), far])
        answer(few, 0.1, min_points, [-1] * min_points, [0] * min_points)
        enough = np.concatenate([far, np.full((min_points, 3), 0.25, dtype)])
        answer(enough, 0.1, min_points, [-1] + [0] * min_points, [0] + [1] * min_points)


@pytest.mark.parametrize("dtype", DTYPES)
def test_border_tie_goes_to_the_lower_row_not_the_lower_cluster(dtype):
    left, right = _hub(-1.0, -1.0), _hub(1.0, 1.0)
    # rows 0-2: the left three (cluster 0), 3: the right hub, 4-6: the right three (cluster 1), 7: the left hub, 8: the middle, at distance
    # exactly 1 from both hubs (d2 == 1 in either dtype)
    p = np.array(left[1:] + right + left[:1] + [[0.0, 0.0, 0.0]], dtype)
    answer(p, 1.05, 4, [0, 0, 0, 1, 1, 1, 1, 0, 1], [1] * 8 + [0])
    # the hubs swapped: the left hub has the lower row now
    p = np.array(left[1:] + left[:1] + right[1:] + right[:1] + [[0.0, 0.0, 0.0]], dtype)
    answer(p, 1.05, 4, [0, 0, 0, 0, 1, 1, 1, 1, 0], [1] * 8 + [0])


@pytest.mark.parametrize("dtype", DTYPES)
def test_border_goes_to_the_nearer_core_in_the_higher_cluster(dtype):
    left, right = _hub(-1.0, -1.0), _hub(1.0, 1.0)
    p = np.array(left + right + [[0.125, 0.0, 0.0]], dtype)           # 1.125 from the left hub (row 0, cluster 0), 0.875 from the right one (row 4)
    answer(p, 1.2, 4, [0] * 4 + [1] * 4 + [1], [1] * 8 + [0])
    p = np.array(left + right + [[-0.125, 0.0, 0.0]], dtype)
    answer(p, 1.2, 4, [0] * 4 + [1] * 4 + [0], [1] * 8 + [0])


@pytest.mark.parametrize("dtype", DTYPES)
def test_eps_zero_and_min_points_one(dtype):
    p = np.concatenate([np.zeros((3, 3)), np.ones((2, 3)), [[5.0, 5.0, 5.0]]]).astype(dtype)
    answer(p, 0.0, 1, [-1] * 6, [0] * 6)                            # not even a point's own distance 0 is below 0
    answer(p, 0.5, 1, [0, 0, 0, 1, 1, 2], [1] * 6)                  # everybody is core: no noise, a lone point is a cluster
    answer(p, 2.0, 1, [0, 0, 0, 0, 0, 1], [1] * 6)                  # sqrt(3) < 2 joins the first two groups


def test_non_finite_rows_are_noise_and_nobodys_neighbour():
    p = np.array([[0, 0, 0], [0.1, 0, 0], [np.inf, 0, 0], [0, 0.1, 0], [np.nan, 0, 0], [np.inf, 0, 0]], np.float32)
    answer(p, 0.5, 1, [0, 0, -1, 0, -1, -1], [1, 1, 0, 1, 0, 0])
    answer(p, 0.5, 3, [0, 0, -1, 0, -1, -1], [1, 1, 0, 1, 0, 0])


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("seed, n, eps, min_points", [(0, 400, 0.12, 5), (1, 700, 0.1, 4), (2, 300, 0.2, 8), (3, 500, 0.08, 1)])
def test_core_is_radius_count_and_the_rest_follows(dtype, seed, n, eps, min_points):
    p = np.random.default_rng(seed).random((n, 3)).astype(dtype)
    labels, core = dc.dbscan(p, eps, min_points)
    assert np.array_equal(core, rc.radius_count(p, p, eps) >= min_points)
    member = dc.membership(p, eps)
    assert np.array_equal(member, member.T)
    # cores joined by an edge share a label; a cluster's number is the rank of its smallest core row; no label is skipped
    i, j = np.nonzero(member & core[:, None] & core[None, :])
    assert np.array_equal(labels[i], labels[j]) and (labels[core] >= 0).all()
    firsts = [np.flatnonzero(core & (labels == k))[0] for k in range(labels.max() + 1)]
    assert firsts == sorted(firsts)
    # a point that is not core: noise iff it has no core neighbour, else the label of the nearest one
    d2 = rc.squared_distances(p, p)
    for b in np.flatnonzero(~core):
        nb = np.flatnonzero(member[b] & core)
        if not len(nb):
            assert labels[b] == -1
        else:
            assert labels[b] == labels[nb[np.lexsort((nb, d2[b, nb]))[0]]]


def test_five_thousand_points_one_cluster_and_one_chain():
    """The sizes the GPU tests use: every point in one cluster, and a chain as long as the cloud (a breadth-first level per link)."""
    p = np.random.default_rng(5).random((5000, 3)).astype(np.float32)
    labels, core = dc.dbscan(p, 4.0, 5000)
    assert not labels.any() and core.all()
    chain = np.zeros((5000, 3), np.float64)
    chain[:, 0] = np.random.default_rng(6).permutation(5000) * 0.9
    labels, core = dc.dbscan(chain, 1.0, 2)
    assert not labels.any() and core.all()


SKLEARN_CASES = [(0, 1500, 0.08, 5), (1, 2000, 0.06, 4), (2, 2500, 0.1, 8), (3, 3000, 0.05, 3)]


@pytest.mark.parametrize("seed, n, eps, min_points", SKLEARN_CASES)
def test_against_scikit_learn(seed, n, eps, min_points):
    cluster = pytest.importorskip("sklearn.cluster")
    p = np.random.default_rng(seed).random((n, 3))
    labels, core = dc.dbscan(p, eps, min_points)
    sk = cluster.DBSCAN(eps=eps, min_samples=min_points, algorithm="brute").fit(p)
    sk_core = np.zeros(n, bool)
    sk_core[sk.core_sample_indices_] = True
    assert np.array_equal(core, sk_core)
    assert np.array_equal(labels[core], sk.labels_[core])
    assert np.array_equal(labels == -1, sk.labels_ == -1)
    member = dc.membership(p, eps)
    border = np.flatnonzero(~core & (labels >= 0))
    assert len(border) > 0
    for b in border:                                                 # each of the two labels is the label of one of b's core neighbours
        around = set(labels[member[b] & core].tolist())
        assert labels[b] in around and sk.labels_[b] in around
