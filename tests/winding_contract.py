"""The contract of triangle_soup_fast_winding_number and signed_distance_to_mesh in float64 numpy: the exact generalized
winding number W the operators are judged by, and a model of the fast evaluation. Helper module (no tests): tests/test_winding_contract.py
checks it on the CPU, tests/test_gpu_winding.py measures its error on its own queries and holds the kernels to twice that.

Exact. W(q) = (1/4pi) sum over faces of OMEGA(q, a, b, c), the signed solid angle by Van Oosterom and Strackee:
  A = a - q, B = b - q, C = c - q,  OMEGA = 2 atan2(A.(BxC), |A||B||C| + (A.B)|C| + (B.C)|A| + (C.A)|B|),  atan2(0, 0) = 0.

Model. A tree built by the library's rule: faces in the order of the Morton code of their centroid, leaves of LEAF consecutive faces, an
implicit balanced binary tree over the leaves padded to a power of two P (node i has children 2i+1 and 2i+2, leaf j is node P-1+j). Per node,
over the faces t below it, with N_t = (b-a)x(c-a)/2, A_t = |N_t|, g_t = (a+b+c)/3:
  centre p = sum A_t g_t / sum A_t (the centre of its box if the area is 0; for an inner node the area-weighted mean of its children's
  centres, which is the same point), radius r = the distance from p to the farthest corner of its box,
  M0 = sum N_t,  M1_ij = sum (g_t - p)_i N_t,j,  M2_ijk = sum Q_t,ij N_t,k,
  Q_t = (xa xa' + xb xb' + xc xc' + (xa+xb+xc)(xa+xb+xc)')/12 with x = vertex - p.
Leaves take their moments from the faces; an inner node moves its children's to its own centre, with delta = p_child - p_parent:
  M0' = M0,  M1'_ij = M1_ij + delta_i M0_j,  M2'_ijk = M2_ijk + delta_i M1_jk + delta_j M1_ik + delta_i delta_j M0_k.
Per query, from the root: with R = p - q, d = |R|, a node with d > beta r contributes
  (1/4pi) [ M0.R/d^3 + sum_ij M1_ij (delta_ij/d^3 - 3 R_i R_j/d^5)
            + 1/2 sum_ijk M2_ijk (-3 (delta_ij R_k + delta_ik R_j + delta_jk R_i)/d^5 + 15 R_i R_j R_k/d^7) ],
any other inner node is opened, any other leaf contributes sum OMEGA/4pi of its faces, padding nodes contribute nothing."""
import os

import numpy as np

LEAF = 4
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
FOUR_PI = 4.0 * np.pi


# ---- exact
def solid_angle(q, a, b, c):
    """OMEGA for (..., 3) float64 arrays that broadcast against each other."""
    A, B, C = a - q, b - q, c - q
    la, lb, lc = (np.sqrt(np.einsum("...k,...k->...", x, x)) for x in (A, B, C))
    det = np.einsum("...k,...k->...", A, np.cross(B, C))
    den = (la * lb * lc + np.einsum("...k,...k->...", A, B) * lc + np.einsum("...k,...k->...", B, C) * la
           + np.einsum("...k,...k->...", C, A) * lb)
    return 2.0 * np.arctan2(det, den + 0.0)


def exact_winding(p, v, f, chunk=None):
    """W of every row of p in float64: the plain sum over all faces."""
    p64, v64 = np.asarray(p, dtype=np.float64), np.asarray(v, dtype=np.float64)
    f = np.asarray(f).astype(np.int64)
    a, b, c = v64[f[:, 0]][None], v64[f[:, 1]][None], v64[f[:, 2]][None]
    out = np.empty(len(p64))
    step = chunk or max(1, 1_000_000 // len(f))
    for i0 in range(0, len(p64), step):
        out[i0:i0 + step] = solid_angle(p64[i0:i0 + step, None, :], a, b, c).sum(axis=1) / FOUR_PI
    return out


# ---- the model's tree
def _split21(x):
    x = x.astype(np.uint64)
    out = np.zeros_like(x)
    for bit in range(21):
        out |= ((x >> np.uint64(bit)) & np.uint64(1)) << np.uint64(3 * bit)
    return out


def face_order(v64, f):
    """Faces by the 63-bit Morton code of their centroid in the bounding box of the referenced vertices (stable: ties keep face order)."""
    ref = v64[np.unique(f)]
    lo, ext = ref.min(0), ref.max(0) - ref.min(0)
    g = v64[f].mean(axis=1)
    with np.errstate(all="ignore"):
        cell = np.where(ext > 0, (g - lo) / np.where(ext > 0, ext, 1.0) * 2097152.0, 0.0)
    cell = np.clip(cell, 0, 2097151).astype(np.uint64)
    code = _split21(cell[:, 0]) | _split21(cell[:, 1]) << np.uint64(1) | _split21(cell[:, 2]) << np.uint64(2)
    return np.argsort(code, kind="stable")


def face_terms(tri, p):
    """Per face of tri (m, 3 corners, 3) about the points p (m, 3) or (3,): N (m, 3), g - p (m, 3), Q (m, 3, 3)."""
    x = tri - np.reshape(p, (-1, 1, 3))
    N = 0.5 * np.cross(x[:, 1] - x[:, 0], x[:, 2] - x[:, 0])
    sx = x.sum(axis=1)
    Q = (np.einsum("mci,mcj->mij", x, x) + np.einsum("mi,mj->mij", sx, sx)) / 12.0
    return N, sx / 3.0, Q


def direct_moments(tri, p):
    """M0, M1, M2 of the faces tri (m, 3, 3) about the one point p, from the definition."""
    N, gy, Q = face_terms(tri, p)
    return N.sum(0), np.einsum("mi,mj->ij", gy, N), np.einsum("mij,mk->ijk", Q, N)


def shift_moments(M0, M1, M2, delta):
    """The moments (n, ...) about p_child moved to p_parent, delta = p_child - p_parent (n, 3)."""
    S1 = M1 + np.einsum("ni,nj->nij", delta, M0)
    S2 = (M2 + np.einsum("ni,njk->nijk", delta, M1) + np.einsum("nj,nik->nijk", delta, M1)
          + np.einsum("ni,nj,nk->nijk", delta, delta, M0))
    return M0, S1, S2


def build_tree(v, f):
    """The tree of the module docstring in float64. Returns a dict: P, tri (sorted faces' corners), nleaf (faces per leaf), pad (node is padding),
    lo, hi, ctr, r, area, M0, M1, M2 per node."""
    v64 = np.asarray(v, dtype=np.float64)
    f = np.asarray(f).astype(np.int64)
    tri = v64[f[face_order(v64, f)]]
    nf = len(tri)
    leaves = (nf + LEAF - 1) // LEAF
    P = 1
    while P < leaves:
        P *= 2
    n = 2 * P - 1
    t = dict(P=P, tri=tri, pad=np.ones(n, bool), lo=np.full((n, 3), np.inf), hi=np.full((n, 3), -np.inf), ctr=np.zeros((n, 3)), r=np.zeros(n),
             area=np.zeros(n), M0=np.zeros((n, 3)), M1=np.zeros((n, 3, 3)), M2=np.zeros((n, 3, 3, 3)))
    leaf = P - 1 + np.arange(nf) // LEAF
    np.minimum.at(t["lo"], leaf, tri.min(axis=1)); np.maximum.at(t["hi"], leaf, tri.max(axis=1))
    t["pad"][leaf] = False
    for m in _levels(P):
        nodes = np.arange(m - 1, 2 * m - 1)
        t["lo"][nodes] = np.minimum(t["lo"][2 * nodes + 1], t["lo"][2 * nodes + 2])
        t["hi"][nodes] = np.maximum(t["hi"][2 * nodes + 1], t["hi"][2 * nodes + 2])
        t["pad"][nodes] = t["pad"][2 * nodes + 1] & t["pad"][2 * nodes + 2]
    N = 0.5 * np.cross(tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0])
    A = np.linalg.norm(N, axis=1)
    np.add.at(t["area"], leaf, A)
    wsum = np.zeros((n, 3))
    np.add.at(wsum, leaf, A[:, None] * tri.mean(axis=1))
    real = ~t["pad"]
    with np.errstate(all="ignore"):
        box_mid = np.where(real[:, None], 0.5 * t["lo"] + 0.5 * t["hi"], 0.0)
        leaf_nodes = np.arange(P - 1, n)
        t["ctr"][leaf_nodes] = np.where(t["area"][leaf_nodes, None] > 0, wsum[leaf_nodes] / np.where(t["area"][leaf_nodes, None] > 0, t["area"][leaf_nodes, None], 1.0),
                                        box_mid[leaf_nodes])
    Nf, gy, Q = face_terms(tri, t["ctr"][leaf])
    np.add.at(t["M0"], leaf, Nf)
    np.add.at(t["M1"], leaf, np.einsum("mi,mj->mij", gy, Nf))
    np.add.at(t["M2"], leaf, np.einsum("mij,mk->mijk", Q, Nf))
    for m in _levels(P):
        nodes = np.arange(m - 1, 2 * m - 1)
        l, r = 2 * nodes + 1, 2 * nodes + 2
        al, ar = t["area"][l], t["area"][r]
        a = al + ar
        t["area"][nodes] = a
        with np.errstate(all="ignore"):
            mean = (al[:, None] * t["ctr"][l] + ar[:, None] * t["ctr"][r]) / np.where(a > 0, a, 1.0)[:, None]
        t["ctr"][nodes] = np.where(a[:, None] > 0, mean, box_mid[nodes])
        for c in (l, r):
            M0, M1, M2 = shift_moments(t["M0"][c], t["M1"][c], t["M2"][c], t["ctr"][c] - t["ctr"][nodes])
            t["M0"][nodes] += M0; t["M1"][nodes] += M1; t["M2"][nodes] += M2
    with np.errstate(all="ignore"):
        far = np.maximum(np.abs(t["ctr"] - t["lo"]), np.abs(t["hi"] - t["ctr"]))
    t["r"] = np.where(real, np.linalg.norm(np.where(real[:, None], far, 0.0), axis=1), -1.0)
    return t


def _levels(P):
    m = P // 2
    while m >= 1:
        yield m
        m //= 2


def expansion(R, M0, M1, M2, terms=3):
    """4pi times the contribution of far nodes: R (n, 3) = centre - query, the nodes' moments (n, ...). terms = 2 leaves M2 out."""
    d = np.linalg.norm(R, axis=1)
    eye = np.eye(3)
    out = np.einsum("nk,nk->n", M0, R) / d ** 3
    G1 = eye[None] / d[:, None, None] ** 3 - 3.0 * np.einsum("ni,nj->nij", R, R) / d[:, None, None] ** 5
    out = out + np.einsum("nij,nij->n", M1, G1)
    if terms >= 3:
        G2 = (-3.0 * (np.einsum("ij,nk->nijk", eye, R) + np.einsum("ik,nj->nijk", eye, R) + np.einsum("jk,ni->nijk", eye, R)) / d[:, None, None, None] ** 5
              + 15.0 * np.einsum("ni,nj,nk->nijk", R, R, R) / d[:, None, None, None] ** 7)
        out = out + 0.5 * np.einsum("nijk,nijk->n", M2, G2)
    return out


def fast_winding(tree, p, beta=2.0, terms=3, visits=None):
    """The model's w for every row of p (float64). `visits`, an int array of len(p), receives the number of nodes and faces each query touched."""
    p64 = np.asarray(p, dtype=np.float64)
    P, tri = tree["P"], tree["tri"]
    nf = len(tri)
    acc = np.zeros(len(p64))
    qi, node = np.arange(len(p64)), np.zeros(len(p64), np.int64)
    while len(qi):
        if visits is not None:
            np.add.at(visits, qi, 1)
        keep = ~tree["pad"][node]
        qi, node = qi[keep], node[keep]
        R = tree["ctr"][node] - p64[qi]
        with np.errstate(invalid="ignore"):
            far = np.linalg.norm(R, axis=1) > beta * tree["r"][node]
        if far.any():
            np.add.at(acc, qi[far], expansion(R[far], tree["M0"][node[far]], tree["M1"][node[far]], tree["M2"][node[far]], terms))
        qi, node = qi[~far], node[~far]
        is_leaf = node >= P - 1
        lq, ln = qi[is_leaf], node[is_leaf]
        for t in range(LEAF):
            s = LEAF * (ln - (P - 1)) + t
            ok = s < nf
            if ok.any():
                face = tri[s[ok]]
                np.add.at(acc, lq[ok], solid_angle(p64[lq[ok]], face[:, 0], face[:, 1], face[:, 2]))
                if visits is not None:
                    np.add.at(visits, lq[ok], 1)
        qi, node = qi[~is_leaf], node[~is_leaf]
        qi, node = np.concatenate([qi, qi]), np.concatenate([2 * node + 1, 2 * node + 2])
    return acc / FOUR_PI


# ---- meshes and queries
def box_queries(v, n, seed, dtype=np.float64):
    """n points uniform in the bounding box of v enlarged by a quarter of its extent per side."""
    rng = np.random.default_rng(seed)
    v64 = np.asarray(v, dtype=np.float64)
    lo, hi = v64.min(0), v64.max(0)
    ext = hi - lo
    return np.ascontiguousarray((lo - 0.25 * ext + rng.random((n, 3)) * 1.5 * ext).astype(dtype))


def tetrahedron(dtype):
    """Outward-oriented."""
    v = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [0, 0, 1]], dtype=dtype)
    f = np.array([[0, 2, 1], [0, 1, 3], [0, 3, 2], [1, 2, 3]], dtype=np.int64)
    return v, f


def tolerance(tree, q, W, beta, dtype):
    """TOL(beta) on these queries: twice the model's largest error (a maximum over a few thousand queries is a noisy statistic and the
    kernel's boxes, hence radii, are padded), plus the rounding of the sum in the kernel's type: a term has an absolute error of a few eps
    and a query adds as many terms as the model's walk touches nodes and faces, so 8 * (most terms of any query) * eps -- for float32 and
    finite beta no more than 1e-4. Returns (tol, the model's largest error, the most terms of a query)."""
    visits = np.zeros(len(q), np.int64)
    err = float(np.abs(fast_winding(tree, q, beta, visits=visits) - W).max())
    rounding = 8.0 * int(visits.max()) * np.finfo(dtype).eps
    if np.dtype(dtype) == np.float32 and np.isfinite(beta):
        rounding = min(rounding, 1e-4)
    return 2.0 * err + rounding, err, int(visits.max())
