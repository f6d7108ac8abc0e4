"""The contract of point_cloud_fast_winding_number and estimate_mesh_face_normals in numpy: the exact dipole sum W the
operator is judged by (float64), a float64 model of the fast evaluation, the face normals restated in the input dtype, and the tolerance.
Helper module (no tests): tests/test_pc_winding_contract.py checks it on the CPU, tests/test_gpu_pc_winding.py holds the kernels to it.

Exact. D_i = a_i n_i;  W(q) = (1/4pi) sum_i TERM(q, p_i, D_i);  with R = p - q, d2 = R.R: TERM = 0 if not d2 > 0, else D.R / d2^(3/2).

Model. Points in the order of the 63-bit Morton code of their position in the bounding box of all points (stable), leaves of LEAF consecutive
points, the implicit balanced binary tree of winding_contract over the leaves padded to a power of two P. Per node, over the points below it,
with weight w_i = |D_i|: centre c = sum w_i p_i / sum w_i (the centre of its box if the weight is 0; for an inner node the weighted mean of its
children's centres, which is the same point), radius r = the distance from c to the farthest corner of the box of its points, and with
x = p_i - c:  M0 = sum D_i,  M1_ij = sum x_i D_j,  M2_ijk = sum x_i x_j D_k.  Leaves take their moments from the points, an inner node moves its
children's to its own centre (winding_contract.shift_moments). Per query, from the root: a node with |c - q| > beta r contributes
winding_contract.expansion, any other inner node is opened, any other leaf contributes TERM of its points, padding nodes nothing.

LEAF = 8 is csrc/pc_winding.h's kPcLeaf. It was chosen on this model (one expansion is 34 loads, 8 dipoles are 48) and has not been timed on
the GPU."""
import numpy as np

from winding_contract import FOUR_PI, _levels, _split21, expansion, shift_moments

LEAF = 8


# ---- exact
def dipoles(n, a):
    return np.asarray(n, dtype=np.float64) * np.asarray(a, dtype=np.float64).reshape(-1, 1)


def dipole_terms(q, p, D):
    """4pi TERM for (..., 3) float64 arrays that broadcast against each other."""
    R = p - q
    d2 = np.einsum("...k,...k->...", R, R)
    with np.errstate(all="ignore"):
        t = np.einsum("...k,...k->...", np.broadcast_to(D, R.shape), R) / (d2 * np.sqrt(d2))
    return np.where(d2 > 0, t, 0.0)


def exact(q, p, n, a, chunk=None, absolute=False):
    """W of every row of q in float64: the plain sum over all points. `absolute`: the sum of |TERM| / 4pi instead."""
    q64, p64, D = np.asarray(q, dtype=np.float64), np.asarray(p, dtype=np.float64), dipoles(n, a)
    out = np.empty(len(q64))
    step = chunk or max(1, 2_000_000 // len(p64))
    for i0 in range(0, len(q64), step):
        t = dipole_terms(q64[i0:i0 + step, None, :], p64[None], D[None])
        out[i0:i0 + step] = (np.abs(t) if absolute else t).sum(axis=1) / FOUR_PI
    return out


# ---- the model's tree
def point_order(p64):
    lo, ext = p64.min(0), p64.max(0) - p64.min(0)
    with np.errstate(all="ignore"):
        cell = np.where(ext > 0, (p64 - lo) / np.where(ext > 0, ext, 1.0) * 2097152.0, 0.0)
    cell = np.clip(cell, 0, 2097151).astype(np.uint64)
    code = _split21(cell[:, 0]) | _split21(cell[:, 1]) << np.uint64(1) | _split21(cell[:, 2]) << np.uint64(2)
    return np.argsort(code, kind="stable")


def direct_moments(x, D):
    """M0, M1, M2 of the dipoles D (m, 3) at x (m, 3) relative to the centre, from the definition."""
    return D.sum(0), np.einsum("mi,mj->ij", x, D), np.einsum("mi,mj,mk->ijk", x, x, D)


def build_tree(p, n, a):
    """The tree of the module docstring in float64. Returns a dict: P, pts and D (sorted), pad (node is padding), lo, hi, ctr, r, weight, M0,
    M1, M2 per node."""
    p64 = np.asarray(p, dtype=np.float64)
    order = point_order(p64)
    pts, D = p64[order], dipoles(n, a)[order]
    m = len(pts)
    leaves = (m + LEAF - 1) // LEAF
    P = 1
    while P < leaves:
        P *= 2
    nn = 2 * P - 1
    t = dict(P=P, pts=pts, D=D, pad=np.ones(nn, bool), lo=np.full((nn, 3), np.inf), hi=np.full((nn, 3), -np.inf), ctr=np.zeros((nn, 3)),
             r=np.zeros(nn), weight=np.zeros(nn), M0=np.zeros((nn, 3)), M1=np.zeros((nn, 3, 3)), M2=np.zeros((nn, 3, 3, 3)))
    leaf = P - 1 + np.arange(m) // LEAF
    np.minimum.at(t["lo"], leaf, pts); np.maximum.at(t["hi"], leaf, pts)
    t["pad"][leaf] = False
    for lv in _levels(P):
        nodes = np.arange(lv - 1, 2 * lv - 1)
        t["lo"][nodes] = np.minimum(t["lo"][2 * nodes + 1], t["lo"][2 * nodes + 2])
        t["hi"][nodes] = np.maximum(t["hi"][2 * nodes + 1], t["hi"][2 * nodes + 2])
        t["pad"][nodes] = t["pad"][2 * nodes + 1] & t["pad"][2 * nodes + 2]
    w = np.linalg.norm(D, axis=1)
    np.add.at(t["weight"], leaf, w)
    wsum = np.zeros((nn, 3))
    np.add.at(wsum, leaf, w[:, None] * pts)
    real = ~t["pad"]
    with np.errstate(all="ignore"):
        box_mid = np.where(real[:, None], 0.5 * t["lo"] + 0.5 * t["hi"], 0.0)
    ln = np.arange(P - 1, nn)
    has = t["weight"][ln, None] > 0
    t["ctr"][ln] = np.where(has, wsum[ln] / np.where(has, t["weight"][ln, None], 1.0), box_mid[ln])
    x = pts - t["ctr"][leaf]
    np.add.at(t["M0"], leaf, D)
    np.add.at(t["M1"], leaf, np.einsum("mi,mj->mij", x, D))
    np.add.at(t["M2"], leaf, np.einsum("mi,mj,mk->mijk", x, x, D))
    for lv in _levels(P):
        nodes = np.arange(lv - 1, 2 * lv - 1)
        l, r = 2 * nodes + 1, 2 * nodes + 2
        wl, wr = t["weight"][l], t["weight"][r]
        ws = wl + wr
        t["weight"][nodes] = ws
        mean = (wl[:, None] * t["ctr"][l] + wr[:, None] * t["ctr"][r]) / np.where(ws > 0, ws, 1.0)[:, None]
        t["ctr"][nodes] = np.where(ws[:, None] > 0, mean, box_mid[nodes])
        for c in (l, r):
            M0, M1, M2 = shift_moments(t["M0"][c], t["M1"][c], t["M2"][c], t["ctr"][c] - t["ctr"][nodes])
            t["M0"][nodes] += M0; t["M1"][nodes] += M1; t["M2"][nodes] += M2
    with np.errstate(all="ignore"):
        far = np.maximum(np.abs(t["ctr"] - t["lo"]), np.abs(t["hi"] - t["ctr"]))
    t["r"] = np.where(real, np.linalg.norm(np.where(real[:, None], far, 0.0), axis=1), -1.0)
    return t


def fast(tree, q, beta=2.0, terms=3, visits=None, mag=None):
    """The model's w for every row of q (float64). `visits` (int array of len(q)) receives the number of nodes and points each query
    touched, `mag` (float array) the sum of |contribution| / 4pi over what its walk added."""
    q64 = np.asarray(q, dtype=np.float64)
    P, pts, D = tree["P"], tree["pts"], tree["D"]
    m = len(pts)
    acc = np.zeros(len(q64))
    qi, node = np.arange(len(q64)), np.zeros(len(q64), np.int64)
    while len(qi):
        if visits is not None:
            np.add.at(visits, qi, 1)
        keep = ~tree["pad"][node]
        qi, node = qi[keep], node[keep]
        R = tree["ctr"][node] - q64[qi]
        with np.errstate(invalid="ignore"):
            far = np.linalg.norm(R, axis=1) > beta * tree["r"][node]
        if far.any():
            e = expansion(R[far], tree["M0"][node[far]], tree["M1"][node[far]], tree["M2"][node[far]], terms)
            np.add.at(acc, qi[far], e)
            if mag is not None:
                np.add.at(mag, qi[far], np.abs(e) / FOUR_PI)
        qi, node = qi[~far], node[~far]
        is_leaf = node >= P - 1
        lq, ln = qi[is_leaf], node[is_leaf]
        for t in range(LEAF):
            s = LEAF * (ln - (P - 1)) + t
            ok = s < m
            if ok.any():
                e = dipole_terms(q64[lq[ok]], pts[s[ok]], D[s[ok]])
                np.add.at(acc, lq[ok], e)
                if visits is not None:
                    np.add.at(visits, lq[ok], 1)
                if mag is not None:
                    np.add.at(mag, lq[ok], np.abs(e) / FOUR_PI)
        qi, node = qi[~is_leaf], node[~is_leaf]
        qi, node = np.concatenate([qi, qi]), np.concatenate([2 * node + 1, 2 * node + 2])
    return acc / FOUR_PI


ROUNDING = 8.0          # the factor of the mesh winding tests (winding_contract.tolerance); not measured for dipoles


def walk_stats(tree, q, W, beta):
    """What tolerance() needs of the model's walk at `beta`, the same for every dtype: (E, terms(q), mag(q)). At beta = +inf the walk adds
    every point and no expansion: E = 0 (tests/test_pc_winding_contract.py), terms = #p, mag = the plain sum of |TERM| / 4pi."""
    if not np.isfinite(beta):
        q64, m = np.asarray(q, dtype=np.float64), len(tree["pts"])
        mag = np.empty(len(q64))
        step = max(1, 2_000_000 // m)
        for i0 in range(0, len(q64), step):
            mag[i0:i0 + step] = np.abs(dipole_terms(q64[i0:i0 + step, None, :], tree["pts"][None], tree["D"][None])).sum(axis=1) / FOUR_PI
        return 0.0, np.full(len(q64), m, np.int64), mag
    visits, mag = np.zeros(len(q), np.int64), np.zeros(len(q))
    err = float(np.abs(fast(tree, q, beta, visits=visits, mag=mag) - W).max())
    return err, visits, mag


def tolerance(tree, q, W, beta, dtype, walk=None):
    """Per query: tol(q) = 2 E + ROUNDING eps(T) terms(q) max(1, mag(q)), E the model's largest |fast - exact| over the queries, terms(q) the
    nodes and points the model's walk touches, mag(q) = (1/4pi) sum |contribution| over what that walk adds (a dipole term grows like
    a / d^2 near a sample, unlike a solid angle). At beta = +inf that is ROUNDING eps(T) #p max(1, mag(q)). `walk`: walk_stats of the same
    arguments, if the caller has it. Returns (tol (len(q),), E, the most terms of a query)."""
    err, visits, mag = walk if walk is not None else walk_stats(tree, q, W, beta)
    return 2.0 * err + ROUNDING * float(np.finfo(dtype).eps) * visits * np.maximum(1.0, mag), err, int(visits.max())


# ---- face normals, in T
def face_normals(v, f):
    """estimate_mesh_face_normals restated: every operation rounded on its own in v's dtype."""
    T = v.dtype.type
    f = np.asarray(f).astype(np.int64)
    a, b, c = v[f[:, 0]], v[f[:, 1]], v[f[:, 2]]
    with np.errstate(all="ignore"):
        e1, e2 = b - a, c - a
        N = np.stack([e1[:, 1] * e2[:, 2] - e1[:, 2] * e2[:, 1], e1[:, 2] * e2[:, 0] - e1[:, 0] * e2[:, 2],
                      e1[:, 0] * e2[:, 1] - e1[:, 1] * e2[:, 0]], axis=1)
        r = np.sqrt((N[:, 0] * N[:, 0] + N[:, 1] * N[:, 1]) + N[:, 2] * N[:, 2])
        out = np.where(r[:, None] == 0, T(0), N / r[:, None])
    assert out.dtype == v.dtype
    return np.ascontiguousarray(out)


# ---- the fixture clouds
def f32_grid(x):
    return np.ascontiguousarray(np.asarray(x).astype(np.float32).astype(np.float64))


def mesh_cloud(v, f, count, seed=5):
    """`count` samples of sampling_contract.sample_mesh_random on the float32 mesh (v, f): positions, the face normal of the sample's face,
    a = total area / count; everything on the float32 grid, returned in float64. Also returns h = sqrt(total area / count)."""
    import sampling_contract as sc
    v32 = np.ascontiguousarray(np.asarray(v).astype(np.float32))
    fi, bc = sc.sample_mesh_random(v32, f, count, seed)
    p = sc.positions(v32, f, fi, bc)
    n = face_normals(v32, f)[fi]
    tri = v32.astype(np.float64)[np.asarray(f).astype(np.int64)]
    area = 0.5 * np.linalg.norm(np.cross(tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0]), axis=1).sum()
    a = np.full(count, np.float32(area / count))
    return f32_grid(p), f32_grid(n), f32_grid(a), float(np.sqrt(area / count))


def held(q, p, h, chunk=200):
    """Which queries are farther than 2h from every sample."""
    q64, p64 = np.asarray(q, dtype=np.float64), np.asarray(p, dtype=np.float64)
    out = np.empty(len(q64), bool)
    for i0 in range(0, len(q64), chunk):
        d2 = ((q64[i0:i0 + chunk, None, :] - p64[None]) ** 2).sum(-1).min(axis=1)
        out[i0:i0 + chunk] = d2 > (2.0 * h) ** 2
    return out


def fibonacci_sphere(count, radius=1.0):
    """Points, outward unit normals and equal areas 4 pi r^2 / count."""
    i = np.arange(count) + 0.5
    z = 1.0 - 2.0 * i / count
    phi = i * np.pi * (3.0 - np.sqrt(5.0))
    s = np.sqrt(1.0 - z * z)
    n = np.stack([s * np.cos(phi), s * np.sin(phi), z], axis=1)
    return radius * n, n, np.full(count, FOUR_PI * radius * radius / count)
