"""tests/ransac_contract.py, the definition of register_point_clouds_ransac, tested on its own: the recovery of a planted
motion, the prefix property of the draws, refit off, the strict comparison, the edge pre-check, triples without a frame and inputs without
an alignment. No GPU. The inputs built here are the ones tests/test_gpu_point_cloud_ransac.py hands to the library."""
import collections
import math
import struct

import numpy as np
import pytest

import plane_contract as pc
import ransac_contract as rc

DTYPES = (np.float32, np.float64)
THR = 0.01
ANGLE = 2.5                                              # radians: 143 degrees


def rotation(axis, angle):
    a = np.asarray(axis, dtype=np.float64)
    a = a / np.linalg.norm(a)
    K = np.array([[0.0, -a[2], a[1]], [a[2], 0.0, -a[0]], [-a[1], a[0], 0.0]])
    return np.eye(3) + math.sin(angle) * K + (1.0 - math.cos(angle)) * (K @ K)


TRUTH_R, TRUTH_T = rotation([1.0, 2.0, 3.0], ANGLE), np.array([0.3, -0.2, 0.5])

Planted = collections.namedtuple("Planted", "source target corr true")


def planted(c, dtype, share=0.3, seed=31):
    """c correspondences between c source points in [-1, 1)^3 and c target points. A share of them (three at least), `true`, are pairs under
    (TRUTH_R, TRUTH_T) with the target point moved by less than 0.2 * THR; the target point of every other pair lies 0.2 to 1.0 away from the
    image of its source point. Target rows and correspondence rows are both shuffled."""
    rng = np.random.default_rng(seed)
    k = min(c, max(3, int(round(share * c))))
    S = (rng.random((c, 3)) * 2.0 - 1.0).astype(dtype)
    img = S.astype(np.float64) @ TRUTH_R.T + TRUTH_T
    true = np.zeros(c, dtype=bool)
    true[rng.permutation(c)[:k]] = True
    dirs = rng.normal(size=(c, 3))
    dirs /= np.linalg.norm(dirs, axis=1)[:, None]
    mag = np.where(true, 0.2 * THR * rng.random(c), 0.2 + 0.8 * rng.random(c))
    perm = rng.permutation(c)                            # target row perm[i] is the partner of source row i
    T = np.empty((c, 3), dtype=dtype)
    T[perm] = (img + dirs * mag[:, None]).astype(dtype)
    order = rng.permutation(c)
    corr = np.stack([np.arange(c), perm], axis=1).astype(np.int64)[order]
    return Planted(np.ascontiguousarray(S), np.ascontiguousarray(T), np.ascontiguousarray(corr), true[order])


def truth_distances(P):
    p, q = rc.packed(P.source, P.target, P.corr)
    return np.sqrt(rc.squared_distances(p, q, TRUTH_R.tolist(), TRUTH_T.tolist()))


def seed_for(c, triple):
    """The lowest seed whose hypothesis 0 over c correspondences draws `triple`, in that order."""
    for seed in range(1, 100000):
        if tuple(int(j[0]) for j in pc.triples(seed, c, 1)) == tuple(triple):
            return seed
    raise AssertionError("no seed draws %r" % (triple,))


def lattice(dtype, extra=()):
    """Three pairs whose triangles (0,0,0), (3,0,0), (0,3,0) and the same moved by (1, 2, 3) give, drawn in this order, the frames of the axes,
    the centroids (1, 1, 0) and (2, 3, 3), R = I and tr = (1, 2, 3) without a rounding; then one pair per offset in `extra`: a source point
    whose target point lies that far off its image."""
    S = [[0.0, 0.0, 0.0], [3.0, 0.0, 0.0], [0.0, 3.0, 0.0]] + [[1.0 + i, 2.0, 1.0] for i in range(len(extra))]
    S = np.array(S)
    T = S + np.array([1.0, 2.0, 3.0])
    for i, off in enumerate(extra):
        T[3 + i] += np.array(off)
    c = len(S)
    return np.ascontiguousarray(S.astype(dtype)), np.ascontiguousarray(T.astype(dtype)), np.stack([np.arange(c), np.arange(c)], axis=1).astype(np.int64)


def collinear(dtype, c=50):
    S = np.array([[i, 2.0 * i, -i] for i in range(c)])
    return np.ascontiguousarray(S.astype(dtype)), np.ascontiguousarray((S + 1.0).astype(dtype)), np.stack([np.arange(c), np.arange(c)], axis=1).astype(np.int64)


def packed_bytes(r):
    return (struct.pack("16d", *r.transform.reshape(-1).tolist()), r.inliers.tobytes(), struct.pack("2d", r.fitness, r.inlier_rmse), r.best_iteration, r.status)


@pytest.fixture(scope="module", params=DTYPES, ids=lambda d: np.dtype(d).name)
def case(request):
    P = planted(1000, request.param)
    return P, rc.register_ransac(P.source, P.target, P.corr, THR, 1024, 7)


def test_the_margin_of_the_planted_pairs():
    for dtype in DTYPES:
        P = planted(1000, dtype)
        d = truth_distances(P)
        assert np.count_nonzero(P.true) == 300
        assert d[P.true].max() < 0.25 * THR and d[~P.true].min() > 2.0 * THR


def test_planted_motion_is_recovered(case):
    P, r = case
    assert r.status == "ok" and r.random_seed == 7
    assert r.inliers.dtype == np.int64 and np.array_equal(r.inliers, np.flatnonzero(P.true))
    assert r.fitness == 300 / 1000
    d = truth_distances(P)[P.true]
    planted_rmse = math.sqrt(float(np.sum(d * d)) / 300)
    top = max(float(np.abs(P.source).max()), float(np.abs(P.target).max()))
    print("inlier_rmse", r.inlier_rmse, "planted", planted_rmse)
    assert r.inlier_rmse <= planted_rmse + 64 * np.finfo(np.float64).eps * top
    M = r.transform
    assert M.dtype == np.float64 and M.shape == (4, 4) and M[3].tolist() == [0.0, 0.0, 0.0, 1.0]
    assert np.abs(M[:3, :3] - TRUTH_R).max() < 1e-3 and np.abs(M[:3, 3] - TRUTH_T).max() < 1e-3
    assert abs(np.linalg.det(M[:3, :3]) - 1.0) < 1e-12


def test_prefix_property(case):
    P, r = case
    for a, b in zip(pc.triples(7, 1000, 100), pc.triples(7, 1000, 1024)):
        assert np.array_equal(a, b[:100])
    short = rc.register_ransac(P.source, P.target, P.corr, THR, r.best_iteration + 1, 7)
    assert packed_bytes(short) == packed_bytes(r)
    if r.best_iteration > 0:
        assert rc.register_ransac(P.source, P.target, P.corr, THR, r.best_iteration, 7).best_iteration < r.best_iteration


def test_refit_off_returns_the_winner(case):
    P, r = case
    off = rc.register_ransac(P.source, P.target, P.corr, THR, 1024, 7, refit=False)
    p, q = rc.packed(P.source, P.target, P.corr)
    R, tr, bound = rc.hypotheses(p, q, THR, 7, 1024, 0.9)
    sc = rc.scores(p, q, R, tr, bound)
    h = off.best_iteration
    assert h == r.best_iteration == int(np.argmax(sc)) and sc[h] == sc.max() and (sc[:h] < sc[h]).all()
    assert off.transform[:3, :3].tobytes() == R[h].tobytes() and off.transform[:3, 3].tobytes() == tr[h].tobytes()
    assert np.array_equal(off.inliers, np.flatnonzero(rc.inlier_mask(p, q, R[h], tr[h], bound[h]))) and len(off.inliers) == sc[h]
    assert P.true[off.inliers].all() and 3 <= len(off.inliers) <= 300
    assert off.fitness == len(off.inliers) / 1000 and 0.0 < off.inlier_rmse < THR


@pytest.mark.parametrize("dtype", DTYPES)
def test_the_comparison_is_strict(dtype):
    """Pairs at exactly the threshold 0.5 from the image of their source point, and one at 0.25: refit off, the one hypothesis is exact."""
    S, T, corr = lattice(dtype, extra=((0.5, 0.0, 0.0), (0.0, -0.5, 0.0), (0.0, 0.0, 0.25), (0.0, 0.0, 0.5)))
    seed = seed_for(len(corr), (0, 1, 2))
    p, q = rc.packed(S, T, corr)
    R, tr, bound = rc.hypotheses(p, q, 0.5, seed, 1, 0.9)
    assert R[0].tolist() == np.eye(3).tolist() and tr[0].tolist() == [1.0, 2.0, 3.0] and bound[0] == 0.25
    assert rc.squared_distances(p, q, R[0], tr[0]).tolist() == [0.0, 0.0, 0.0, 0.25, 0.25, 0.0625, 0.25]
    r = rc.register_ransac(S, T, corr, 0.5, 1, seed, refit=False)
    assert r.status == "ok" and r.inliers.tolist() == [0, 1, 2, 5] and r.fitness == 4 / 7 and r.inlier_rmse == math.sqrt(0.0625 / 4)
    assert np.flatnonzero(rc.inlier_mask(p, q, R[0], tr[0], bound[0], strict=False)).tolist() == [0, 1, 2, 3, 4, 5, 6]


@pytest.mark.parametrize("dtype", DTYPES)
def test_edge_length_ratio(dtype):
    """A target triangle of 0.8 times the size: rejected at 0.9 (0.64 * 9 < 0.81 * 9), tried at 0.75 and at 0."""
    S, T, corr = lattice(dtype)
    T = np.ascontiguousarray((T.astype(np.float64) * 0.8).astype(dtype))
    seed = seed_for(3, (0, 1, 2))
    p, q = rc.packed(S, T, corr)
    assert rc.hypotheses(p, q, 1.0, seed, 1, 0.9)[2][0] == 0.0
    assert rc.hypotheses(p, q, 1.0, seed, 1, 0.0)[2][0] == 1.0
    assert rc.register_ransac(S, T, corr, 1.0, 1, seed, edge_length_ratio=0.9).status == "no_alignment"
    for ratio in (0.0, 0.75):
        r = rc.register_ransac(S, T, corr, 1.0, 1, seed, edge_length_ratio=ratio)
        assert r.status == "ok" and r.inliers.tolist() == [0, 1, 2]
    # and the other way round: the source triangle is the smaller one
    assert rc.hypotheses(q, p, 1.0, seed, 1, 0.9)[2][0] == 0.0 and rc.hypotheses(q, p, 1.0, seed, 1, 0.0)[2][0] == 1.0


@pytest.mark.parametrize("dtype", DTYPES)
def test_triples_without_a_frame_score_zero(dtype):
    S, T, corr = lattice(dtype)
    seed = seed_for(3, (0, 1, 2))
    for rows, col in (((0, 0, 2), 0), ((0, 1, 1), 1), ((2, 1, 2), 0)):          # two equal points, in the source or in the target
        c2 = corr.copy()
        c2[:, col] = rows
        p, q = rc.packed(S, T, c2)
        for ratio in (0.0, 0.9):
            R, tr, bound = rc.hypotheses(p, q, 10.0, seed, 1, ratio)
            assert bound[0] == 0.0 and rc.scores(p, q, R, tr, bound)[0] == 0
        assert rc.register_ransac(S, T, c2, 10.0, 1, seed, edge_length_ratio=0.0).status == "no_alignment"
    S, T, corr = collinear(dtype, 3)
    p, q = rc.packed(S, T, corr)
    assert rc.hypotheses(p, q, 10.0, seed, 1, 0.0)[2][0] == 0.0


@pytest.mark.parametrize("dtype", DTYPES)
def test_no_alignment(dtype):
    r = rc.register_ransac(*collinear(dtype), 0.5, 64, 1)
    assert r.status == "no_alignment" and r.transform.tolist() == np.eye(4).tolist() and r.transform.dtype == np.float64
    assert r.inliers.dtype == np.int64 and r.inliers.shape == (0,) and r.fitness == 0.0 and r.inlier_rmse == 0.0 and r.best_iteration == 0
    P = planted(300, dtype)
    assert rc.register_ransac(P.source, P.target, P.corr, 0.0, 64, 1).status == "no_alignment"          # a threshold of 0: d2 < 0 never holds


@pytest.mark.parametrize("dtype", DTYPES)
def test_repeated_correspondences(dtype):
    """Every row three times: a draw of two copies has no frame; the inliers are the copies of the planted pairs."""
    P = planted(100, dtype, share=0.5)
    corr, true = np.ascontiguousarray(np.tile(P.corr, (3, 1))), np.tile(P.true, 3)
    r = rc.register_ransac(P.source, P.target, corr, THR, 256, 3)
    assert r.status == "ok" and np.array_equal(r.inliers, np.flatnonzero(true))


def test_a_winner_of_fewer_than_three_inliers_keeps_its_transform():
    """A target triangle stretched to twice the height: the centroids meet, two vertices end 1.0 from their partners and the third 2.0. At a
    threshold of 1.5 the winner has two inliers: no refit on two points."""
    S, T, corr = lattice(np.float64)
    T[2] += np.array([0.0, 3.0, 0.0])
    seed = seed_for(3, (0, 1, 2))
    on, off = (rc.register_ransac(S, T, corr, 1.5, 1, seed, edge_length_ratio=0.0, refit=f) for f in (True, False))
    assert off.status == "ok" and off.inliers.tolist() == [0, 1] and off.inlier_rmse == 1.0
    assert packed_bytes(on) == packed_bytes(off)
