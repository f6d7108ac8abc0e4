"""tests/plane_contract.py, the definition of segment_point_cloud_plane, tested on its own: the draws, the prefix property,
the recovery of a planted plane, the strict comparison, the degenerate clouds and the 3x3 Jacobi iteration. No GPU. The clouds built here are
the ones tests/test_gpu_point_cloud_plane.py hands to the library."""
import math

import numpy as np
import pytest

import plane_contract as pc

DTYPES = (np.float32, np.float64)
TRUTH = np.array([0.3, -0.2, -1.0]) / math.sqrt(0.3 * 0.3 + 0.2 * 0.2 + 1.0)      # the normal of z = 0.3x - 0.2y + 0.5


def planted(n, dtype, offset=0.0, seed=22):
    """60 % of the rows on z = 0.3x - 0.2y + 0.5 with Gaussian noise 0.002, the rest uniform in [0, 1)^3, shuffled; then moved by `offset`."""
    rng = np.random.default_rng(seed)
    k = (6 * n) // 10
    xy = rng.random((k, 2))
    z = 0.3 * xy[:, 0] - 0.2 * xy[:, 1] + 0.5 + rng.normal(0.0, 0.002, k)
    P = np.concatenate([np.column_stack([xy, z]), rng.random((n - k, 3))])
    rng.shuffle(P)
    return np.ascontiguousarray((P + offset).astype(dtype))


def angle_deg(plane):
    c = abs(float(np.dot(plane[:3], TRUTH))) / float(np.linalg.norm(plane[:3]))
    return math.degrees(math.acos(min(1.0, c)))


def strictness_grid(dtype):
    """An 8x8 integer grid at z = 0, plus 8 points at z = +0.5 (on the diagonal) and 8 at z = -0.5 (on the diagonal moved by five rows), at
    x, y offsets of 0.25: the plane through three grid points has the 16 others at exactly the threshold 0.5, and the best tilted plane
    through an offset point holds 65 rows. Everything is exact in float32."""
    g = np.array([[x, y, 0.0] for x in range(8) for y in range(8)])
    up = np.array([[i + 0.25, i + 0.25, 0.5] for i in range(8)])
    dn = np.array([[i + 0.25, (i + 5) % 8 + 0.25, -0.5] for i in range(8)])
    return np.ascontiguousarray(np.concatenate([g, up, dn]).astype(dtype))


def coplanar_grid(dtype):
    return np.ascontiguousarray(np.array([[x, y, 3.0] for x in range(9) for y in range(7)]).astype(dtype))


def collinear(dtype):
    return np.ascontiguousarray(np.array([[i, 2 * i, -i] for i in range(50)]).astype(dtype))


def identical(dtype):
    return np.ascontiguousarray(np.tile(np.array([[1.0, 2.0, 3.0]]), (10, 1)).astype(dtype))


def half_repeated(dtype):
    """n = 200, every second row equal to row 0: a draw with two equal points is a hypothesis without a plane."""
    P = np.random.default_rng(5).random((200, 3))
    P[::2] = P[0]
    return np.ascontiguousarray(P.astype(dtype))


@pytest.mark.parametrize("n", [3, 4, 65])
def test_triples_are_distinct_and_in_range(n):
    for seed in (1, 7, 2 ** 32 - 1):
        i0, i1, i2 = pc.triples(seed, n, 512)
        for i in (i0, i1, i2):
            assert i.dtype == np.int64 and i.min() >= 0 and i.max() < n
        assert np.all(i0 != i1) and np.all(i0 != i2) and np.all(i1 != i2)
    if n == 3:
        assert len({(a, b, c) for a, b, c in zip(i0, i1, i2)}) == 6          # every order of the three rows is drawn


def test_prefix_property():
    P = planted(300, np.float32)
    a, b = pc.hypotheses(P, 0.01, 3, 64), pc.hypotheses(P, 0.01, 3, 128)
    for x, y in zip(a, b):
        assert x.tobytes() == y[:64].tobytes()
    assert np.array_equal(pc.scores(P, 0.01, 3, 64), pc.scores(P, 0.01, 3, 128)[:64])


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("offset", [0.0, 1000.0])
def test_planted_plane_is_recovered(dtype, offset):
    """Within 0.05 degrees at n = 4097 with refit (this cloud measures 0.019 degrees, 0.23 without the refit); the refit improves on the
    three-point plane. The
    float32 cloud moved by 1000 has its noise rounded to the grid of 2^-14 there: the sums are centred on a data point, so that is all it costs."""
    P = planted(4097, dtype, offset)
    r = pc.segment_plane(P, 0.01, 128, 3, refit=True)
    q = pc.segment_plane(P, 0.01, 128, 3, refit=False)
    assert r.status == q.status == "ok" and r.best_iteration == q.best_iteration
    print(dtype.__name__, offset, "angle with refit", angle_deg(r.plane), "without", angle_deg(q.plane), "inliers", len(r.inliers), len(q.inliers))
    assert angle_deg(r.plane) < 0.05
    assert angle_deg(q.plane) > angle_deg(r.plane)
    for res in (r, q):
        assert abs(float(np.linalg.norm(res.plane[:3])) - 1.0) < 1e-12
        d = np.abs(P.astype(np.float64) @ res.plane[:3] + res.plane[3])
        assert np.all(d[res.inliers] < 0.01 * (1 + 1e-9)) and np.all(np.diff(res.inliers) > 0)


@pytest.mark.parametrize("dtype", DTYPES)
def test_the_comparison_is_strict(dtype):
    P = strictness_grid(dtype)
    assert int(pc.scores(P, 0.5, 1, 64).max()) == 65
    assert int(pc.scores(P, 0.5, 1, 64, strict=False).max()) == 80


@pytest.mark.parametrize("dtype", DTYPES)
def test_coplanar_grid(dtype):
    P = coplanar_grid(dtype)
    sc = pc.scores(P, 0.25, 1, 64)
    assert set(sc.tolist()) <= {0, len(P)} and (sc == len(P)).any() and (sc == 0).any()
    for refit in (False, True):
        r = pc.segment_plane(P, 0.25, 64, 1, refit=refit)
        assert r.status == "ok" and r.best_iteration == int(np.flatnonzero(sc == len(P))[0])
        assert np.array_equal(r.inliers, np.arange(len(P)))
        assert np.array_equal(r.plane, np.array([0.0, 0.0, 1.0, -3.0]))       # (a zero may carry either sign: the negation is of the bits)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("cloud", [collinear, identical])
def test_no_plane(dtype, cloud):
    r = pc.segment_plane(cloud(dtype), 0.5, 64, 1)
    assert r.status == "no_plane" and r.best_iteration == 0 and r.inliers.shape == (0,) and r.inliers.dtype == np.int64
    assert r.plane.tobytes() == np.zeros(4).tobytes()


@pytest.mark.parametrize("dtype", DTYPES)
def test_a_threshold_of_zero_gives_no_plane(dtype):
    for P in (planted(300, dtype), coplanar_grid(dtype)):
        assert pc.segment_plane(P, 0.0, 64, 1).status == "no_plane"


@pytest.mark.parametrize("dtype", DTYPES)
def test_hypotheses_without_a_plane_score_zero(dtype):
    P = half_repeated(dtype)
    sc = pc.scores(P, 0.05, 1, 64)
    assert int(np.count_nonzero(sc == 0)) == 31
    assert pc.segment_plane(P, 0.05, 64, 1).status == "ok"


def test_jacobi3_against_eigh():
    """Residuals of jacobi3 against numpy.linalg.eigh over 4000 random symmetric 3x3 matrices (Gaussian entries; every fourth scaled by 1e6,
    every fourth other by 1e-6; every tenth a covariance of nearly coplanar points, the case the refit meets). Measured on the CPU: the
    largest eigenvalue difference relative to the largest absolute eigenvalue was 1.84e-15, the largest |A v - lambda v| relative to it
    1.43e-15, the largest departure of |v| from 1 was 1.11e-15. The bound is the largest of them with a margin of ten, rounded up: 2e-14."""
    rng = np.random.default_rng(3)
    worst = [0.0, 0.0, 0.0]
    for t in range(4000):
        if t % 10 == 9:
            X = rng.random((50, 3)) * np.array([1.0, 1.0, 1e-4])
            X = X - X.mean(axis=0)
            A = X.T @ X
        else:
            B = rng.normal(size=(3, 3))
            A = (B + B.T) * (1e6 if t % 4 == 1 else 1e-6 if t % 4 == 2 else 1.0)
        diag, V = pc.jacobi3([[float(A[i][j]) for j in range(3)] for i in range(3)])
        w = np.linalg.eigh(A)[0]
        scale = float(np.abs(w).max())
        worst[0] = max(worst[0], float(np.abs(np.sort(diag) - w).max()) / scale)
        Vn = np.array(V)
        for i in range(3):
            worst[1] = max(worst[1], float(np.abs(A @ Vn[:, i] - diag[i] * Vn[:, i]).max()) / scale)
            worst[2] = max(worst[2], abs(float(np.linalg.norm(Vn[:, i])) - 1.0))
    print("jacobi3 worst: eigenvalues %.3g, residual %.3g, length %.3g" % tuple(worst))
    assert worst[0] < 2e-14 and worst[1] < 2e-14 and worst[2] < 2e-14
