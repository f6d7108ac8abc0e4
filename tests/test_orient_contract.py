"""tests/orient_contract.py against an independent construction and its own properties. No GPU: small generic clouds and a brute-force k-NN.

The independent construction builds the same forest in the rounds the GPU path uses (every tree takes its least outgoing edge under
(w, lo, hi); mutual choices join once), keeps the chosen edges as an adjacency list and walks each tree from its reference row: no sorted
edge list, no union-find with parities. Disconnected clouds, n <= k, coincident copies and non-finite normals are among the inputs."""
import math
from collections import deque

import numpy as np
import pytest

import orient_contract as oc


def brute_knn(points, m):
    """(n, m) rows of nearest neighbours by (d2, row), in float64."""
    p = np.asarray(points, dtype=np.float64)
    d2 = ((p[:, None, :] - p[None, :, :]) ** 2).sum(axis=2)
    return np.argsort(d2, axis=1, kind="stable")[:, :m].astype(np.int64)


def by_rounds(points, normals, nbr):
    """(flipped, rounds, trees) by Boruvka rounds and a walk per tree."""
    n = len(points)
    nd = np.asarray(normals).astype(np.float64)
    pairs = set()
    for i in range(n):
        for j in nbr[i].tolist():
            if j != i and 0 <= j < n:
                pairs.add((min(i, j), max(i, j)))
    graph = []
    for lo, hi in pairs:
        with np.errstate(all="ignore"):
            d = (nd[lo, 0] * nd[hi, 0] + nd[lo, 1] * nd[hi, 1]) + nd[lo, 2] * nd[hi, 2]
        if math.isfinite(d):
            graph.append((1.0 - abs(d), lo, hi, bool(d < 0)))
    label = list(range(n))
    adj = [[] for _ in range(n)]
    rounds = 0
    while True:
        best = {}
        for e in graph:
            a, b = label[e[1]], label[e[2]]
            if a == b:
                continue
            for t in (a, b):
                if t not in best or e[:3] < best[t][:3]:
                    best[t] = e
        if not best:
            break
        rounds += 1
        for e in set(best.values()):
            adj[e[1]].append((e[2], e[3]))
            adj[e[2]].append((e[1], e[3]))
        # relabel: the components of the chosen edges
        seen = [False] * n
        for s in range(n):
            if seen[s]:
                continue
            seen[s] = True
            queue = deque([s])
            while queue:
                x = queue.popleft()
                label[x] = s
                for y, _ in adj[x]:
                    if not seen[y]:
                        seen[y] = True
                        queue.append(y)
    flipped = np.zeros(n, dtype=bool)
    z = np.asarray(points)[:, 2]
    trees = sorted(set(label))
    for t in trees:
        rows = [i for i in range(n) if label[i] == t]
        ref = rows[0]
        for i in rows[1:]:
            if z[i] > z[ref]:
                ref = i
        state = {ref: bool(normals[ref, 2] < 0)}
        queue = deque([ref])
        while queue:
            x = queue.popleft()
            for y, f in adj[x]:
                if y not in state:
                    state[y] = state[x] ^ f
                    queue.append(y)
        assert len(state) == len(rows)
        for i in rows:
            flipped[i] = state[i]
    return flipped, rounds, len(trees)


def cloud(seed, n, dtype, clusters=1):
    rng = np.random.default_rng(seed)
    p = rng.random((n, 3))
    if clusters > 1:
        p = p * 0.05 + rng.integers(0, clusters, size=(n, 1)) * 10.0
    return p.astype(dtype), rng.standard_normal((n, 3)).astype(dtype)


CASES = [(1, 1, 3, 1), (2, 2, 1, 1), (3, 3, 10, 1), (4, 17, 4, 1), (5, 64, 70, 1), (6, 200, 1, 1), (7, 200, 2, 1), (8, 300, 6, 4), (9, 257, 10, 3)]


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("seed,n,k,clusters", CASES)
def test_kruskal_equals_the_rounds(seed, n, k, clusters, dtype):
    p, nrm = cloud(seed, n, dtype, clusters)
    nbr = brute_knn(p, min(k + 1, n))
    out, flipped = oc.orient(p, nrm, nbr)
    want, rounds, trees = by_rounds(p, nrm, nbr)
    assert flipped.dtype == np.bool_ and out.dtype == dtype and out.shape == (n, 3)
    assert np.array_equal(flipped, want)
    assert out.tobytes() == np.where(want[:, None], -nrm, nrm).tobytes()
    assert trees == oc.num_trees(p, nrm, nbr) and (clusters == 1 or k == 1 or trees >= clusters or n <= k)
    assert rounds <= max(1, math.ceil(math.log2(max(n, 2))))


def test_disconnected_clouds_have_a_reference_row_per_tree():
    p, nrm = cloud(20, 240, np.float64, clusters=3)
    nbr = brute_knn(p, 7)
    out, flipped = oc.orient(p, nrm, nbr)
    assert oc.num_trees(p, nrm, nbr) == 3
    which = np.round(p[:, 0] / 10.0).astype(int)
    for c in range(3):
        rows = np.flatnonzero(which == c)
        top = rows[np.argmax(p[rows, 2])]
        assert out[top, 2] >= 0 and flipped[top] == (nrm[top, 2] < 0)


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_input_signs_do_not_matter(dtype):
    """Generic data: no agreement and no reference normal_z is exactly 0."""
    for seed, n, k, clusters in ((30, 150, 5, 1), (31, 150, 1, 1), (32, 200, 8, 3), (33, 9, 20, 1)):
        p, nrm = cloud(seed, n, dtype, clusters)
        nbr = brute_knn(p, min(k + 1, n))
        out, _ = oc.orient(p, nrm, nbr)
        rng = np.random.default_rng(seed + 100)
        for _ in range(3):
            sign = rng.choice(np.array([-1.0, 1.0], dtype), size=(n, 1))
            again, _ = oc.orient(p, nrm * sign, nbr)
            assert again.tobytes() == out.tobytes()


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_a_sphere_comes_back_outward(dtype):
    rng = np.random.default_rng(40)
    true = rng.standard_normal((1500, 3))
    true /= np.linalg.norm(true, axis=1, keepdims=True)
    p = true.astype(dtype)
    sign = rng.choice([-1.0, 1.0], size=(1500, 1))
    nrm = (true * sign).astype(dtype)
    out, flipped = oc.orient(p, nrm, brute_knn(p, 9))
    assert ((out.astype(np.float64) * true).sum(axis=1) > 0).all()
    assert np.array_equal(flipped, sign[:, 0] < 0)


def test_coincident_copies_and_non_finite_normals():
    p, nrm = cloud(50, 40, np.float64)
    nrm /= np.linalg.norm(nrm, axis=1, keepdims=True)
    # a row and its negated copy: d = -1 to rounding, the least edge at both ends, so it is in the forest and one of the two ends flipped
    p2, n2 = np.concatenate([p, p]), np.concatenate([nrm, -nrm])
    nbr = brute_knn(p2, 4)
    out, flipped = oc.orient(p2, n2, nbr)
    assert np.array_equal(flipped, by_rounds(p2, n2, nbr)[0])
    assert out[:40].tobytes() == out[40:].tobytes() and (flipped[:40] != flipped[40:]).all()
    # a NaN or infinite normal makes every agreement of its row non-finite: the row is a tree of its own (normal_z is not < 0: it keeps its bytes);
    # a zero normal agrees with d = 0 and takes part
    bad = nrm.copy()
    bad[3] = [np.nan, 1.0, 1.0]
    bad[7] = [np.inf, 0.0, 0.0]
    bad[9] = 0.0
    nbr = brute_knn(p, 6)
    out, flipped = oc.orient(p, bad, nbr)
    assert np.array_equal(flipped, by_rounds(p, bad, nbr)[0])
    assert not flipped[3] and out[3].tobytes() == bad[3].tobytes()
    assert not flipped[7] and out[7].tobytes() == bad[7].tobytes()
    assert oc.num_trees(p, bad, nbr) == 3
    alone = bad.copy()
    alone[3, 2] = -1.0                                                        # rule 4 holds for a lone row too
    assert oc.orient(p, alone, nbr)[1][3]
