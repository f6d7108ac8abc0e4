"""tests/icp_contract.py (the definition of register_point_clouds_icp) against independent numpy: the order of fold64 against a
plain Python pairing, Horn's step against np.linalg.svd Kabsch, the plane step against np.linalg.solve, the recovery of a known motion, the four
named outcomes, and the indifference of the plane system to the normals' sign. No GPU."""
import math

import numpy as np
import pytest

import icp_contract as ic
import radius_contract as rc

DTYPES = [np.float32, np.float64]


# ------------------------------------------------------------------------------------------------ fold64
def fold64_plain(terms):
    """The same tree, one Python float addition at a time."""
    y = [float(v) for v in terms]
    while True:
        y += [0.0] * ((-len(y)) % 64)
        nxt = []
        for r in range(0, len(y), 64):
            row = y[r:r + 64]
            w = 32
            while w >= 1:
                row = [row[i] + row[i + w] for i in range(w)]
                w //= 2
            nxt.append(row[0])
        y = nxt
        if len(y) == 1:
            return y[0]


@pytest.mark.parametrize("n", [1, 63, 64, 65, 4096, 4097, 262145])
def test_fold64_is_the_stated_tree(n):
    x = np.random.default_rng(n).standard_normal(n) * 10.0 ** np.random.default_rng(n + 1).integers(-6, 7, n)
    got, want = ic.fold64(x), fold64_plain(x)
    assert math.copysign(1.0, got) == math.copysign(1.0, want) and got == want
    assert abs(got - math.fsum(x)) <= 1e-9 * float(np.abs(x).sum())


def test_fold64_of_a_lone_negative_zero_is_positive_zero():
    got = ic.fold64(np.array([-0.0]))
    assert got == 0.0 and math.copysign(1.0, got) == 1.0


# ------------------------------------------------------------------------------------------------ Horn
def rotation(axis, angle):
    a = np.asarray(axis, np.float64)
    a = a / np.linalg.norm(a)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    return np.eye(3) + math.sin(angle) * K + (1 - math.cos(angle)) * (K @ K)


def kabsch(P, Q):
    """R, t minimising sum |R p + t - q|^2 by SVD, and the singular values of the covariance."""
    mp, mq = P.mean(0), Q.mean(0)
    H = (P - mp).T @ (Q - mq)
    U, S, Vt = np.linalg.svd(H)
    d = 1.0 if np.linalg.det(Vt.T @ U.T) >= 0 else -1.0
    R = Vt.T @ np.diag([1.0, 1.0, d]) @ U.T
    return R, mq - R @ mp, S


def sums_point(P, Q):
    """The 17 sums of the contract for an all-inlier pair, through its own fold."""
    terms = [np.ones(len(P)), np.zeros(len(P))] + ic.terms_point(P, Q)
    return [ic.fold64(t) for t in terms]


def is_rotation(R):
    R = np.asarray(R)
    return abs(np.linalg.det(R) - 1.0) < 1e-12 and np.abs(R @ R.T - np.eye(3)).max() < 1e-12


def test_horn_equals_kabsch_on_2000_cases():
    """Generic, exactly planar, exactly collinear clouds and H = 0. Where the optimum is unique (the two largest singular values of the
    covariance are not tiny) the two rotations must agree entry by entry; for a collinear cloud every rotation about the line is optimal, so
    there the image of the line's direction is compared, which is unique; for H = 0 both must only be rotations (Horn's rule gives the identity)."""
    rng = np.random.default_rng(2026)
    worst = 0.0
    kinds = {"generic": 0, "planar": 0, "collinear": 0, "zero": 0}
    for case in range(2000):
        n = int(rng.integers(3, 201))
        kind = ("generic", "generic", "generic", "generic", "generic", "generic", "planar", "planar", "collinear", "zero")[case % 10]
        P = rng.standard_normal((n, 3))
        if kind == "planar":
            P[:, 2] = 0.0
        if kind == "collinear":
            P[:, 1:] = 0.0
        if kind == "zero":
            P[:] = 0.0                      # (every source point at the origin: the covariance is exactly zero)
        R0 = rotation(rng.standard_normal(3), rng.uniform(-3.0, 3.0))
        Q = P @ R0.T + rng.standard_normal(3) + (rng.standard_normal((n, 3)) * 1e-3 if case % 3 == 0 and kind == "generic" else 0.0)
        kinds[kind] += 1
        R, t = ic.horn(sums_point(P, Q), n)
        Rk, tk, S = kabsch(P, Q)
        assert is_rotation(R) and is_rotation(Rk), (case, kind)
        R = np.array(R)
        if kind == "zero":
            assert np.array_equal(R, np.eye(3))
            continue
        if kind == "collinear":
            u = np.array([1.0, 0.0, 0.0])
            dev = np.abs(R @ u - Rk @ u).max()
        else:
            assert S[1] > 1e-3 * S[0]
            dev = max(np.abs(R - Rk).max(), np.abs(np.array(t) - tk).max())
        worst = max(worst, dev)
    print("horn against kabsch: max deviation", worst, kinds)
    assert min(kinds.values()) >= 200
    assert worst < 1e-12


# ------------------------------------------------------------------------------------------------ plane step
def ellipsoid(n, dtype, seed=5):
    """n points on the ellipsoid with semi-axes (0.5, 0.35, 0.25) centred at 0.5, and its unit normals."""
    rng = np.random.default_rng(seed)
    u = rng.standard_normal((n, 3))
    u /= np.linalg.norm(u, axis=1)[:, None]
    ax = np.array([0.5, 0.35, 0.25])
    p = 0.5 + u * ax
    nrm = u / ax
    nrm /= np.linalg.norm(nrm, axis=1)[:, None]
    return p.astype(dtype), nrm.astype(dtype)


MOTION_R = rotation((1.0, 2.0, 3.0), 0.1)
MOTION_T = np.array([0.02, -0.01, 0.03])


def moved_back(target, dtype):
    """The source: the target moved back by MOTION, so that MOTION is what the registration has to find."""
    return ((target.astype(np.float64) - MOTION_T) @ MOTION_R).astype(dtype)


def test_plane_step_equals_linalg_solve():
    """The 6x6 Cholesky solve against np.linalg.solve on the same A, b, for the systems the recovery test meets and random well-conditioned ones;
    the bound is Horn's (1e-12), on x relative to its largest entry. Measured: see the printed figure."""
    rng = np.random.default_rng(7)
    worst = 0.0
    for case in range(2000):
        n = int(rng.integers(20, 201))
        tgt, nrm = ellipsoid(n, np.float64, seed=case)
        P = moved_back(tgt, np.float64) + rng.standard_normal((n, 3)) * (1e-3 if case % 2 else 0.0)
        terms = [np.ones(n), np.zeros(n)] + ic.terms_plane(P, tgt, nrm)
        S = [ic.fold64(t) for t in terms]
        A, b = ic.plane_system(S)
        x = ic.cholesky_solve(A, b)
        assert x is not None
        want = np.linalg.solve(np.array(A), -np.array(b))
        worst = max(worst, np.abs(np.array(x) - want).max() / np.abs(want).max())
        R, t = ic.plane_step(S)
        assert is_rotation(R)
    print("plane step against linalg.solve: max relative deviation", worst)
    assert worst < 1e-12


def test_plane_system_ignores_the_sign_of_a_normal():
    """r and J both change sign with the normal, so every term J_u J_v, J_u r and r r keeps its bytes."""
    tgt, nrm = ellipsoid(500, np.float32)
    src = moved_back(tgt, np.float32)
    flipped = nrm.copy()
    flipped[::2] *= -1
    a = ic.evaluate(np.eye(4).tolist(), src, tgt, nrm, math.inf, ic.brute_nearest)
    b = ic.evaluate(np.eye(4).tolist(), src, tgt, flipped, math.inf, ic.brute_nearest)
    assert np.array(a.sums).tobytes() == np.array(b.sums).tobytes()
    ra = ic.register_icp(src, tgt, nrm)
    rb = ic.register_icp(src, tgt, flipped)
    assert ra.transform.tobytes() == rb.transform.tobytes() and ra[1:5] == rb[1:5]


# ------------------------------------------------------------------------------------------------ recovery
def no_ties_nearest(p, target):
    d2 = rc.squared_distances(p, target)
    part = np.partition(d2, 1, axis=1) if d2.shape[1] > 1 else None
    assert part is None or (part[:, 0] < part[:, 1]).all(), "the test's inputs must have no exact ties"
    return ic.brute_nearest(p, target)


@pytest.mark.parametrize("max_distance", [math.inf, 0.1])
@pytest.mark.parametrize("plane", [False, True])
@pytest.mark.parametrize("n", [257, 1000])
@pytest.mark.parametrize("dtype", DTYPES)
def test_recovers_a_known_motion(dtype, n, plane, max_distance):
    tgt, nrm = ellipsoid(n, dtype)
    src = moved_back(tgt, dtype)
    r = ic.register_icp(src, tgt, nrm if plane else None, max_correspondence_distance=max_distance, return_correspondences=True,
                        nearest=no_ties_nearest)
    want = np.eye(4)
    want[:3, :3], want[:3, 3] = MOTION_R, MOTION_T
    err = np.abs(r.transform - want).max()
    print(dtype.__name__, n, "plane" if plane else "point", max_distance, r.status, r.iterations, r.fitness, r.inlier_rmse, err)
    assert r.status == "converged" and r.fitness == 1.0
    assert err < (1e-12 if dtype == np.float64 else 1e-6)
    assert r.transform.dtype == np.float64 and r.transform.shape == (4, 4) and np.array_equal(r.transform[3], [0, 0, 0, 1])
    assert type(r.fitness) is float and type(r.inlier_rmse) is float and type(r.iterations) is int
    assert r.correspondences.dtype == np.int64 and np.array_equal(r.correspondences, np.arange(n))


# ------------------------------------------------------------------------------------------------ named outcomes
@pytest.mark.parametrize("dtype", DTYPES)
def test_named_outcomes(dtype):
    tgt, nrm = ellipsoid(300, dtype)
    src = moved_back(tgt, dtype)
    r = ic.register_icp(src, tgt, max_correspondence_distance=0.0, return_correspondences=True)
    assert (r.status, r.fitness, r.inlier_rmse, r.iterations) == ("no_correspondences", 0.0, 0.0, 0)
    assert (r.correspondences == -1).all() and np.array_equal(r.transform, np.eye(4))
    init = np.eye(4)
    init[:3, :3], init[:3, 3] = rotation((0, 0, 1), 0.05), (0.01, 0.0, -0.01)
    r = ic.register_icp(src, tgt, nrm, init_transform=init, max_iterations=0)
    assert r.status == "max_iterations" and r.iterations == 0 and r.transform.tobytes() == init.tobytes() and r.fitness == 1.0
    flat = np.random.default_rng(3).random((200, 3)).astype(dtype)
    flat[:, 2] = 0
    up = np.zeros((200, 3), dtype)
    up[:, 2] = 1
    r = ic.register_icp(src, flat, up)
    assert r.status == "degenerate" and r.iterations == 0 and np.array_equal(r.transform, np.eye(4)) and r.fitness == 1.0
    for normals in (None, nrm):
        r = ic.register_icp(tgt, tgt, normals, return_correspondences=True)
        assert (r.status, r.iterations, r.inlier_rmse, r.fitness) == ("converged", 1, 0.0, 1.0)
        assert np.array_equal(r.correspondences, np.arange(300))
