"""The contract of closest_points_on_mesh restated in numpy, the independent float64 formulation it is judged by, and the
meshes both test files use. Helper module (no tests): tests/test_mesh_contract.py checks it on the CPU, tests/test_gpu_mesh.py holds the
kernels to it bit for bit.

Contract. Per face D2(q, a, b, c) -> (d2, v, w) in the input type T, every product and sum rounded on its own, IEEE division:
  dot(x, y) = (x0*y0 + x1*y1) + x2*y2
  ab = b - a, ac = c - a, ap = q - a, bp = q - b, cp = q - c
  d1 = dot(ab, ap), d2 = dot(ac, ap), d3 = dot(ab, bp), d4 = dot(ac, bp), d5 = dot(ab, cp), d6 = dot(ac, cp)
  vc = d1*d4 - d3*d2, vb = d5*d2 - d1*d6, va = d3*d6 - d5*d4
  the first of these regions whose test holds (Ericson, Real-Time Collision Detection 5.1.5; an edge region needs a denominator > 0, so a
  collapsed edge falls through, and an interior denominator that is not > 0 gives vertex A):
    vertex A   d1 <= 0 and d2 <= 0                                              v = 0, w = 0
    vertex B   d3 >= 0 and d4 <= d3                                             v = 1, w = 0
    edge AB    vc <= 0 and d1 >= 0 and d3 <= 0 and d1 - d3 > 0                  v = d1 / (d1 - d3), w = 0
    vertex C   d6 >= 0 and d5 <= d6                                             v = 0, w = 1
    edge AC    vb <= 0 and d2 >= 0 and d6 <= 0 and d2 - d6 > 0                  v = 0, w = d2 / (d2 - d6)
    edge BC    va <= 0 and d4 - d3 >= 0 and d5 - d6 >= 0 and (d4-d3)+(d5-d6) > 0   w = (d4 - d3) / ((d4 - d3) + (d5 - d6)), v = 1 - w
    interior   (va + vb) + vc > 0                                               v = vb / ((va + vb) + vc), w = vc / ((va + vb) + vc)
    otherwise                                                                   v = 0, w = 0
  u = (1 - v) - w, closest = (u*a + v*b) + w*c, d2 = dot(q - closest, q - closest).
Per query: the lowest face index among the faces of minimal d2 (exact equality), d = sqrt(d2) and bc = (u, v, w) of that face."""
import os

import numpy as np

# |d - d64| <= B * eps(T) * scale against the independent float64 formulation below: four times the largest excess measured with this
# restatement on the inputs of tests/test_mesh_contract.py, which prints every figure (well-shaped meshes: 0.912 in float32 -- surface samples
# of the bunny --, 1.001 in float64 -- box queries of the 8192-face sphere; the largest of all: 1.040, a face collapsed to a point, float32).
B = 4 * 1.040

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def _dot(x, y):
    return (x[..., 0] * y[..., 0] + x[..., 1] * y[..., 1]) + x[..., 2] * y[..., 2]


def face_d2(q, a, b, c):
    """D2 of the contract; q, a, b, c: (..., 3) arrays of one float dtype (broadcast against each other). Returns d2, v, w."""
    T = q.dtype
    assert a.dtype == T and b.dtype == T and c.dtype == T and T in (np.float32, np.float64)
    ab, ac, ap, bp, cp = b - a, c - a, q - a, q - b, q - c
    d1, d2, d3, d4, d5, d6 = _dot(ab, ap), _dot(ac, ap), _dot(ab, bp), _dot(ac, bp), _dot(ab, cp), _dot(ac, cp)
    with np.errstate(all="ignore"):
        vc, vb, va = d1 * d4 - d3 * d2, d5 * d2 - d1 * d6, d3 * d6 - d5 * d4
        e_ab, e_ac, e_b, e_c = d1 - d3, d2 - d6, d4 - d3, d5 - d6
        e_bc, den = e_b + e_c, (va + vb) + vc
        regions = [(d1 <= 0) & (d2 <= 0),
                   (d3 >= 0) & (d4 <= d3),
                   (vc <= 0) & (d1 >= 0) & (d3 <= 0) & (e_ab > 0),
                   (d6 >= 0) & (d5 <= d6),
                   (vb <= 0) & (d2 >= 0) & (d6 <= 0) & (e_ac > 0),
                   (va <= 0) & (e_b >= 0) & (e_c >= 0) & (e_bc > 0),
                   den > 0]
        zero, one = np.zeros_like(d1), np.ones_like(d1)
        w_bc = e_b / e_bc
        v = np.select(regions, [zero, one, d1 / e_ab, zero, zero, one - w_bc, vb / den], default=zero).astype(T, copy=False)
        w = np.select(regions, [zero, zero, zero, one, d2 / e_ac, w_bc, vc / den], default=zero).astype(T, copy=False)
        u = (one - v) - w
        r = q - ((u[..., None] * a + v[..., None] * b) + w[..., None] * c)
        out = _dot(r, r)
    assert out.dtype == T and v.dtype == T and w.dtype == T
    return out, v, w


def closest_brute(p, v, f, faces=None, chunk=None):
    """The contract's answer for every row of p: a serial minimum over all faces (or, for row i, over the ascending candidate list faces[i]).
    Returns d (#p,), fi (#p,) int64, bc (#p, 3)."""
    T = p.dtype
    f = np.asarray(f).astype(np.int64)
    n = len(p)
    d = np.empty(n, T); fi = np.empty(n, np.int64); bc = np.empty((n, 3), T)
    if faces is None:
        a, b, c = v[f[:, 0]], v[f[:, 1]], v[f[:, 2]]
        step = chunk or max(1, 4_000_000 // len(f))
        for i0 in range(0, n, step):
            q = p[i0:i0 + step, None, :]
            d2, vv, ww = face_d2(q, a[None], b[None], c[None])
            assert not np.isnan(d2).any()
            j = np.argmin(d2, axis=1)                       # (the first occurrence of the minimum: the lowest face index)
            rows = np.arange(len(j))
            d[i0:i0 + step] = np.sqrt(d2[rows, j]); fi[i0:i0 + step] = j
            vj, wj = vv[rows, j], ww[rows, j]
            bc[i0:i0 + step] = np.stack([(T.type(1) - vj) - wj, vj, wj], axis=1)
        return d, fi, bc
    for i in range(n):
        cand = np.asarray(faces[i], dtype=np.int64)
        assert len(cand) and np.all(np.diff(cand) > 0)
        ff = f[cand]
        d2, vv, ww = face_d2(p[i][None], v[ff[:, 0]], v[ff[:, 1]], v[ff[:, 2]])
        assert not np.isnan(d2).any()
        j = int(np.argmin(d2))
        d[i] = np.sqrt(d2[j]); fi[i] = cand[j]
        bc[i] = ((T.type(1) - vv[j]) - ww[j], vv[j], ww[j])
    return d, fi, bc


# ---- the independent float64 formulation: distance to the plane where the projection falls inside the triangle (three edge-function signs),
# else the minimum over the three clamped segments. Not the region code in double.
def _segment64(q, p0, p1):
    e = p1 - p0
    ee = np.einsum("...k,...k->...", e, e)
    with np.errstate(all="ignore"):
        t = np.where(ee > 0, np.einsum("...k,...k->...", q - p0, e) / ee, 0.0)
    t = np.clip(t, 0.0, 1.0)
    r = q - (p0 + t[..., None] * e)
    return np.sqrt(np.einsum("...k,...k->...", r, r))


def triangle_distance64(q, a, b, c):
    q, a, b, c = (np.asarray(x, dtype=np.float64) for x in (q, a, b, c))
    n = np.cross(b - a, c - a)
    nn = np.einsum("...k,...k->...", n, n)
    e0 = np.einsum("...k,...k->...", np.cross(b - a, q - a), n)
    e1 = np.einsum("...k,...k->...", np.cross(c - b, q - b), n)
    e2 = np.einsum("...k,...k->...", np.cross(a - c, q - c), n)
    inside = (nn > 0) & (e0 >= 0) & (e1 >= 0) & (e2 >= 0)
    with np.errstate(all="ignore"):
        plane = np.abs(np.einsum("...k,...k->...", q - a, n)) / np.sqrt(nn)
    seg = np.minimum(np.minimum(_segment64(q, a, b), _segment64(q, b, c)), _segment64(q, c, a))
    return np.where(inside, plane, seg)


def mesh_distance64(p, v, f, chunk=None):
    """min over all faces of triangle_distance64, per row of p."""
    p64, v64 = p.astype(np.float64), v.astype(np.float64)
    f = np.asarray(f).astype(np.int64)
    a, b, c = v64[f[:, 0]], v64[f[:, 1]], v64[f[:, 2]]
    out = np.empty(len(p))
    step = chunk or max(1, 2_000_000 // len(f))
    for i0 in range(0, len(p), step):
        out[i0:i0 + step] = triangle_distance64(p64[i0:i0 + step, None, :], a[None], b[None], c[None]).min(axis=1)
    return out


def reproduce64(p, v, f, fi, bc):
    """|q - bc . triangle(fi)| in float64: the distance the returned (fi, bc) stand for."""
    f = np.asarray(f).astype(np.int64)
    tri = v.astype(np.float64)[f[np.asarray(fi).astype(np.int64)]]               # (#p, 3 corners, 3)
    x = np.einsum("ij,ijk->ik", np.asarray(bc, dtype=np.float64), tri)
    return np.linalg.norm(p.astype(np.float64) - x, axis=1)


# ---- meshes and queries
def bunny(dtype):
    v = np.load(os.path.join(GOLDEN, "bunny_v.npy")).astype(dtype)
    f = np.load(os.path.join(GOLDEN, "bunny_f.npy"))
    return np.ascontiguousarray(v), np.ascontiguousarray(f.astype(np.int64))


def sphere(n, dtype):
    """The octahedron with every face cut into n * n triangles, pushed onto the unit sphere: 8 n^2 faces (n = 32: 8192, n = 160: 204,800)."""
    ii, jj = np.meshgrid(np.arange(n + 1), np.arange(n + 1), indexing="ij")
    keep = ii + jj <= n
    i, j = ii[keep], jj[keep]
    k = n - i - j
    idx = -np.ones((n + 1, n + 1), np.int64)
    idx[i, j] = np.arange(len(i))
    iu, ju = np.nonzero(ii + jj <= n - 1)
    idn, jdn = np.nonzero(ii + jj <= n - 2)
    local = np.concatenate([np.stack([idx[iu, ju], idx[iu + 1, ju], idx[iu, ju + 1]], 1),
                            np.stack([idx[idn + 1, jdn], idx[idn + 1, jdn + 1], idx[idn, jdn + 1]], 1)])
    pts, tris = [], []
    for sx in (1, -1):
        for sy in (1, -1):
            for sz in (1, -1):
                tris.append(local + len(pts) * len(i))
                pts.append(np.stack([sx * i, sy * j, sz * k], 1))
    uniq, inv = np.unique(np.concatenate(pts), axis=0, return_inverse=True)     # (lattice points shared by neighbouring octants are one vertex)
    f = inv.reshape(-1)[np.concatenate(tris)]
    v = uniq / np.linalg.norm(uniq, axis=1, keepdims=True)
    return np.ascontiguousarray(v.astype(dtype)), np.ascontiguousarray(f.astype(np.int64))


def surface_samples(v, f, n, seed):
    """n area-weighted samples on the triangles, in float64 (tests/conftest.py: mesh_samples)."""
    rng = np.random.default_rng(seed)
    tri = v.astype(np.float64)[f]
    areas = 0.5 * np.linalg.norm(np.cross(tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0]), axis=1)
    fi = rng.choice(len(f), n, p=areas / areas.sum())
    u = rng.random(n); w = rng.random(n); su = np.sqrt(u)
    return (1 - su)[:, None] * tri[fi, 0] + (su * (1 - w))[:, None] * tri[fi, 1] + (su * w)[:, None] * tri[fi, 2]


def query_sets(v, f, n, dtype, seed=11):
    """The four kinds of queries of the issue, n rows each: a box twice the bounding box, surface samples, vertices, a far Gaussian (50 extents)."""
    rng = np.random.default_rng(seed)
    v64 = v.astype(np.float64)
    lo, hi = v64.min(0), v64.max(0)
    mid, ext = (lo + hi) / 2, (hi - lo)
    box = mid + (rng.random((n, 3)) - 0.5) * 2 * ext
    surf = surface_samples(v, f, n, seed + 1)
    vert = v64[rng.integers(0, len(v), n)]
    far = mid + rng.normal(size=(n, 3)) * 50 * ext.max()
    return {k: np.ascontiguousarray(a.astype(dtype)) for k, a in (("box", box), ("surface", surf), ("vertex", vert), ("far", far))}


def degenerate_faces(i, j):
    """The five kinds of degenerate faces over vertex rows i, j (and, for the collinear one, a third row the caller puts on their line)."""
    return np.array([[i, j, j], [i, i, i], [i, i, j], [i, j, i]], dtype=np.int64)


def needle_soup(n, height, dtype, seed):
    """n triangles in the unit box with two edges of about 0.1 and a height of `height` (relative to the box): vertices (3n, 3), faces (n, 3)."""
    rng = np.random.default_rng(seed)
    a = rng.random((n, 3))
    d = rng.normal(size=(n, 3)); d /= np.linalg.norm(d, axis=1, keepdims=True)
    o = np.cross(d, rng.normal(size=(n, 3))); o /= np.linalg.norm(o, axis=1, keepdims=True)
    b = a + 0.1 * d
    c = a + 0.05 * d + height * o
    v = np.stack([a, b, c], axis=1).reshape(-1, 3).astype(dtype)
    return np.ascontiguousarray(v), np.arange(3 * n, dtype=np.int64).reshape(n, 3)
