"""CPU tests of tests/pc_winding_contract.py, the numpy statement of point_cloud_fast_winding_number and estimate_mesh_face_normals (DESIGN.md
row f10): the model is checked against its own definitions and against the mesh the fixture clouds were sampled from, so that the GPU tests
(tests/test_gpu_pc_winding.py) hold the kernels to something that has been held to something itself. No GPU."""
import numpy as np
import pytest

import mesh_contract as mc
import pc_winding_contract as pw
import ray_contract as rc
import winding_contract as wc

INF = float("inf")
N_CLOUD, N_QUERIES = 20000, 2000


@pytest.fixture(scope="module")
def clouds():
    out = {}
    for name, make in (("cube_twist", rc.cube_twist), ("bunny", mc.bunny)):
        v, f = make(np.float32)
        p, n, a, h = pw.mesh_cloud(v, f, N_CLOUD)
        q = pw.f32_grid(wc.box_queries(v, N_QUERIES, seed=31))
        out[name] = dict(v=v, f=f, p=p, n=n, a=a, h=h, q=q, W=pw.exact(q, p, n, a), tree=pw.build_tree(p, n, a))
    return out


def test_moments_of_a_node_equal_its_childrens_shifted():
    rng = np.random.default_rng(1)
    p, n, a = rng.random((1000, 3)), rng.normal(size=(1000, 3)), rng.normal(size=1000)
    t = pw.build_tree(p, n, a)
    P = t["P"]
    assert P == 128 and t["pad"][P - 1 + 125:].all() and not t["pad"][P - 1:P - 1 + 125].any() and not t["pad"][0]
    first = {}                                      # sorted positions below every node
    for node in range(2 * P - 2, -1, -1):
        first[node] = (pw.LEAF * (node - (P - 1)), pw.LEAF * (node - (P - 1) + 1)) if node >= P - 1 else (first[2 * node + 1][0], first[2 * node + 2][1])
    scale = np.abs(t["D"]).sum()
    for node in range(2 * P - 1):
        s0, s1 = first[node][0], min(first[node][1], 1000)
        if s0 >= 1000:
            assert t["pad"][node] and t["r"][node] == -1.0
            continue
        pts, D = t["pts"][s0:s1], t["D"][s0:s1]
        w = np.linalg.norm(D, axis=1)
        assert np.allclose(t["ctr"][node], (w[:, None] * pts).sum(0) / w.sum(), rtol=1e-12, atol=1e-14)
        assert np.array_equal(t["lo"][node], pts.min(0)) and np.array_equal(t["hi"][node], pts.max(0))
        far = np.maximum(np.abs(t["ctr"][node] - t["lo"][node]), np.abs(t["hi"][node] - t["ctr"][node]))
        assert np.isclose(t["r"][node], np.linalg.norm(far), rtol=1e-14)
        assert t["r"][node] >= np.linalg.norm(pts - t["ctr"][node], axis=1).max() * (1 - 1e-14)
        for got, want in zip((t["M0"][node], t["M1"][node], t["M2"][node]), pw.direct_moments(pts - t["ctr"][node], D)):
            assert np.abs(got - want).max() <= 1e-12 * scale, node


def test_beta_inf_is_the_exact_sum():
    rng = np.random.default_rng(2)
    p, n, a = rng.random((777, 3)), rng.normal(size=(777, 3)), rng.normal(size=777)
    q = np.concatenate([wc.box_queries(p, 200, seed=3), p[:50]])
    t = pw.build_tree(p, n, a)
    visits = np.zeros(len(q), np.int64)
    W = pw.exact(q, p, n, a)
    assert np.abs(pw.fast(t, q, INF, visits=visits) - W).max() <= 1e-10 * max(1.0, np.abs(W).max())
    assert (visits == visits[0]).all() and 777 + 2 * 98 - 1 <= visits[0] <= 777 + 2 * t["P"] - 1      # every point and every node that holds one
    assert np.isfinite(W).all()                                # (a query on a point gets nothing from that point)


def test_sign_and_normalisation_on_a_sphere():
    count = 4096
    p, n, a = pw.fibonacci_sphere(count, radius=1.5)
    W = pw.exact(np.zeros((1, 3)), p, n, a)
    assert abs(W[0] - 1.0) <= count * np.finfo(np.float64).eps
    assert abs(pw.exact(np.array([[0.0, 0.0, 40.0]]), p, n, a)[0]) < 1e-3
    assert abs(pw.exact(np.zeros((1, 3)), p, -n, a)[0] + 1.0) <= count * np.finfo(np.float64).eps


@pytest.mark.parametrize("name", ["cube_twist", "bunny"])
def test_tolerance_refuses_an_evaluation_without_m2(clouds, name):
    c = clouds[name]
    e2 = np.abs(pw.fast(c["tree"], c["q"], 2.0, terms=2) - c["W"])
    worst = int(np.argmax(e2))
    for T in (np.float32, np.float64):
        tol, err, most = pw.tolerance(c["tree"], c["q"], c["W"], 2.0, T)
        print(f"\n{name} {np.dtype(T).name}: three-term error {err:.3e}, two-term error {e2.max():.3e}, most terms {most}, tol at the worst query {tol[worst]:.3e}")
        assert tol.shape == (N_QUERIES,) and tol[worst] < e2[worst], "the tolerance must refuse an evaluation without M2"
    t4, err4, _ = pw.tolerance(c["tree"], c["q"], c["W"], 4.0, np.float64)
    assert err4 < 0.2 * err
    tinf, zero, m = pw.tolerance(c["tree"], c["q"], c["W"], INF, np.float32)
    assert zero == 0.0 and m == N_CLOUD and (tinf >= 8 * np.finfo(np.float32).eps * N_CLOUD).all()


@pytest.mark.parametrize("name", ["cube_twist", "bunny"])
def test_cloud_against_the_mesh_it_was_sampled_from(clouds, name):
    """Away from the samples (farther than 2h, h the sample spacing) the dipole sum is the mesh's winding number to a quarter."""
    c = clouds[name]
    keep = pw.held(c["q"], c["p"], c["h"])
    W_mesh = wc.exact_winding(c["q"], c["v"], c["f"])
    worst = float(np.abs(c["W"] - W_mesh)[keep].max())
    print(f"\n{name}: {100.0 * keep.mean():.1f} % of the queries held, worst |W_cloud - W_mesh| = {worst:.3f}")
    assert keep.mean() >= 0.9
    assert worst < 0.25
    assert np.array_equal(c["W"][keep] > 0.5, W_mesh[keep] > 0.5)
    assert (W_mesh[keep] > 0.5).any() and (W_mesh[keep] < 0.5).any()


def test_face_normals_restated():
    for make in (rc.cube_twist, mc.bunny):
        for T in (np.float32, np.float64):
            v, f = make(T)
            got = pw.face_normals(v, f)
            assert got.dtype == T and got.shape == (len(f), 3)
            tri = v.astype(np.float64)[f]
            N = np.cross(tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0])
            want = N / np.linalg.norm(N, axis=1, keepdims=True)
            assert np.abs(got - want).max() <= 64 * np.finfo(T).eps      # (the differences of the cross product cancel: a few eps of the edges' products)
            assert np.abs(np.linalg.norm(got.astype(np.float64), axis=1) - 1).max() <= 4 * np.finfo(T).eps
    v, f = mc.bunny(np.float32)
    deg = mc.degenerate_faces(10, 20)
    got = pw.face_normals(v, np.concatenate([f[:3], deg]))
    assert np.array_equal(got[3:], np.zeros((len(deg), 3), np.float32)) and (np.abs(got[:3]).max(axis=1) > 0).all()
    tiny = np.array([[0, 0, 0], [1e-30, 0, 0], [0, 1e-30, 0]], np.float32)       # the cross product underflows: a zero normal (a documented limit)
    assert np.array_equal(pw.face_normals(tiny, np.array([[0, 1, 2]])), np.zeros((1, 3), np.float32))
