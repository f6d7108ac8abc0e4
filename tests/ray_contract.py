"""The contract of ray_mesh_intersection restated in numpy, the independent float64 formulation it is judged by, and the
ray generators both test files use. Helper module (no tests): tests/test_ray_contract.py checks it on the CPU, tests/test_gpu_rays.py holds the
kernels to it bit for bit.

Contract. All arithmetic in the input type T, every product, sum and difference rounded on its own, IEEE division.
  per mesh   S = the largest absolute coordinate of a referenced vertex
  per ray    kz = the dominant axis of d (0 if |d0| >= |d1| and |d0| >= |d2|, else 1 if |d1| >= |d2|, else 2), kx = (kz+1)%3, ky = (kx+1)%3,
             kx and ky swapped if d[kz] < 0; Sx = d[kx]/d[kz], Sy = d[ky]/d[kz], Sz = 1/d[kz]; inv[k] = 1/d[k];
             pad = max(16 eps S, 16 eps max_k |o[k]|)
  per (ray, face a b c)
    1 watertight test (Woop, Benthin, Wald, JCGT 2013, no double fallback): A = a - o (B, C alike); Ax = A[kx] - Sx*A[kz], Ay = A[ky] - Sy*A[kz],
      Az = Sz*A[kz]; U = Cx*By - Cy*Bx, V = Ax*Cy - Ay*Cx, W = Bx*Ay - By*Ax; reject if (U<0 or V<0 or W<0) and (U>0 or V>0 or W>0);
      det = (U+V)+W, reject if det == 0; t = ((U*Az + V*Bz) + W*Cz)/det, b1 = V/det, b2 = W/det
    2 window: accept only if t >= near and t <= far
    3 box clip: flo = min(a,b,c) - pad, fhi = max(a,b,c) + pad; per axis t1 = (flo[k]-o[k])*inv[k], t2 = (fhi[k]-o[k])*inv[k], n_k = fmin(t1,t2),
      f_k = fmax(t1,t2); t_in = fmax(fmax(n_0,n_1),n_2), t_out = fmin(fmin(f_0,f_1),f_2); accept only if t_in <= t and t <= t_out
  per ray    the smallest accepted t, the LOWEST face index among equal t (a serial loop with a strict `<` that starts at +inf);
             hit: f_id, bc = ((1-b1)-b2, b1, b2), t; miss: f_id = -1, bc = 0, t = +inf."""
import os
from concurrent.futures import ThreadPoolExecutor

import numpy as np

import mesh_contract as mc

# |o + t d - x64| and |bc . tri - x64| <= B_RAY * eps(T) * max(S, |o|) against the independent float64 formulation below: four times the
# largest figure tests/test_ray_contract.py::test_accuracy_against_independent_float64 prints. Measured there (1500 rays from a box of three
# extents at surface samples; along the ray / bc . tri): bunny 34.7 / 34.9 in float32 and 36.8 / 36.4 in float64, sphere(32) 170.2 / 170.5 and
# 179.2 / 180.0, cube_twist 5.5 / 4.7 and 65.2 / 65.6. The two figures of a set are nearly equal because t and bc come from the same edge
# functions; the tail is made of grazing rays and of small faces seen from afar (the error of an edge function is eps |a - o|^2).
B_RAY = 4 * 180.0

GOLDEN = mc.GOLDEN


def mesh_scale(v, f):
    """S of the contract, in v's dtype."""
    return np.abs(v[np.unique(np.asarray(f).astype(np.int64))]).max()


def ray_setup(o, d, S):
    """Per-ray constants: o, d (n, 3) of one float dtype. Returns kx, ky, kz (n,) and Sx, Sy, Sz (n,), inv (n, 3), pad (n,)."""
    T = d.dtype
    eps = np.finfo(T).eps
    ad = np.abs(d)
    kz = np.where((ad[:, 0] >= ad[:, 1]) & (ad[:, 0] >= ad[:, 2]), 0, np.where(ad[:, 1] >= ad[:, 2], 1, 2))
    kx = (kz + 1) % 3
    ky = (kx + 1) % 3
    rows = np.arange(len(d))
    neg = d[rows, kz] < 0
    kx, ky = np.where(neg, ky, kx), np.where(neg, kx, ky)
    with np.errstate(all="ignore"):
        dz = d[rows, kz]
        Sx, Sy, Sz = d[rows, kx] / dz, d[rows, ky] / dz, T.type(1) / dz
        inv = T.type(1) / d
    pad = np.maximum(T.type(16) * eps * T.type(S), T.type(16) * eps * np.abs(o).max(axis=1))
    assert all(x.dtype == T for x in (Sx, Sy, Sz, inv, pad))
    return kx, ky, kz, Sx, Sy, Sz, inv, pad


def hit_faces(o, d, near, far, setup, a, b, c, clip=True):
    """HIT of the contract, elementwise: o, d (..., 3), the entries of `setup` (...) (inv (..., 3)), a, b, c (..., 3), all broadcast against
    each other. Returns accepted (bool), t, b1, b2."""
    T = d.dtype
    assert o.dtype == T and a.dtype == T and b.dtype == T and c.dtype == T
    kx, ky, kz, Sx, Sy, Sz, inv, pad = setup
    near, far = T.type(near), T.type(far)

    def shear(P):
        P, ix, iy, iz = np.broadcast_arrays(P, kx[..., None], ky[..., None], kz[..., None])
        pz = np.take_along_axis(P, iz[..., :1], -1)[..., 0]
        px = np.take_along_axis(P, ix[..., :1], -1)[..., 0] - Sx * pz
        py = np.take_along_axis(P, iy[..., :1], -1)[..., 0] - Sy * pz
        return px, py, Sz * pz

    with np.errstate(all="ignore"):
        Ax, Ay, Az = shear(a - o)
        Bx, By, Bz = shear(b - o)
        Cx, Cy, Cz = shear(c - o)
        U = Cx * By - Cy * Bx
        V = Ax * Cy - Ay * Cx
        W = Bx * Ay - By * Ax
        ok = ~(((U < 0) | (V < 0) | (W < 0)) & ((U > 0) | (V > 0) | (W > 0)))
        det = (U + V) + W
        ok &= det != 0
        t = ((U * Az + V * Bz) + W * Cz) / det
        b1, b2 = V / det, W / det
        ok &= (t >= near) & (t <= far)
        if clip:
            flo = np.minimum(np.minimum(a, b), c) - pad[..., None]
            fhi = np.maximum(np.maximum(a, b), c) + pad[..., None]
            t1, t2 = (flo - o) * inv, (fhi - o) * inv
            n, fk = np.fmin(t1, t2), np.fmax(t1, t2)
            t_in = np.fmax(np.fmax(n[..., 0], n[..., 1]), n[..., 2])
            t_out = np.fmin(np.fmin(fk[..., 0], fk[..., 1]), fk[..., 2])
            ok &= (t_in <= t) & (t <= t_out)
    assert t.dtype == T and b1.dtype == T and b2.dtype == T
    return ok, t, b1, b2


def _rows(o, n, T):
    o = np.asarray(o)
    assert o.dtype == T
    return np.broadcast_to(o.reshape(-1, 3), (n, 3)) if o.size == 3 else o


def hit_brute(o, d, near, far, v, f, faces=None, clip=True, chunk=None):
    """The contract's answer for every ray: a serial loop over all faces (or, for ray i, over the ascending candidate list faces[i]) with a
    strict `<` starting at +inf. o: (n, 3), (1, 3) or (3,). Returns f_id (n,) int64, bc (n, 3), t (n,)."""
    T = d.dtype
    f = np.asarray(f).astype(np.int64)
    n = len(d)
    o = _rows(o, n, T)
    S = mesh_scale(v, f)
    fid = np.full(n, -1, np.int64); bc = np.zeros((n, 3), T); tt = np.full(n, np.inf, T)
    one = T.type(1)
    o = np.ascontiguousarray(o)
    if faces is None:
        # Step 1's sign test on every (ray, face) pair, the rays grouped by their axis permutation so that it is plain broadcasting; the few
        # pairs that pass go through hit_faces like a candidate list (the same arithmetic again, so the filter changes nothing).
        kx, ky, kz, Sx, Sy = ray_setup(np.ascontiguousarray(o), d, S)[:5]
        corners = [v[f[:, j]] for j in range(3)]
        step = chunk or max(1, 200_000 // len(f))
        pr, pf = [], []
        with np.errstate(all="ignore"):
            for cls in np.unique(kx * 3 + kz):
                rows = np.flatnonzero(kx * 3 + kz == cls)
                ix, iy, iz = kx[rows[0]], ky[rows[0]], kz[rows[0]]
                for i0 in range(0, len(rows), step):
                    r = rows[i0:i0 + step]
                    sx, sy = Sx[r, None], Sy[r, None]
                    P = []
                    for q in corners:
                        pz = q[None, :, iz] - o[r, iz, None]
                        P.append(((q[None, :, ix] - o[r, ix, None]) - sx * pz, (q[None, :, iy] - o[r, iy, None]) - sy * pz))
                    (Ax, Ay), (Bx, By), (Cx, Cy) = P
                    U, V, W = Cx * By - Cy * Bx, Ax * Cy - Ay * Cx, Bx * Ay - By * Ax
                    keep = ~(((U < 0) | (V < 0) | (W < 0)) & ((U > 0) | (V > 0) | (W > 0)))
                    a_, b_ = np.nonzero(keep)
                    pr.append(r[a_]); pf.append(b_)
        pr, pf = np.concatenate(pr), np.concatenate(pf)
        order = np.lexsort((pf, pr))
        pr, pf = pr[order], pf[order]
        cuts = np.searchsorted(pr, np.arange(n + 1))
        faces = [pf[cuts[i]:cuts[i + 1]] for i in range(n)]
    # candidate lists: every (ray, face) pair in one flat pass, then the minimum per ray
    lens = np.array([len(x) for x in faces], dtype=np.int64)
    if lens.sum() == 0:
        return fid, bc, tt
    ray = np.repeat(np.arange(n), lens)
    cand = np.concatenate([np.asarray(x, dtype=np.int64) for x in faces if len(x)])
    setup = tuple(x[ray] for x in ray_setup(np.ascontiguousarray(o), d, S))
    ff = f[cand]
    ok, t, b1, b2 = hit_faces(o[ray], d[ray], near, far, setup, v[ff[:, 0]], v[ff[:, 1]], v[ff[:, 2]], clip)
    key = np.where(ok, t, T.type(np.inf))
    order = np.lexsort((cand, key, ray))                        # per ray: by t, then by face index
    first = order[np.concatenate([[0], np.flatnonzero(np.diff(ray[order])) + 1])]
    hit = key[first] < np.inf
    r = ray[first][hit]; j = first[hit]
    fid[r] = cand[j]; tt[r] = t[j]
    bc[r] = np.stack([(one - b1[j]) - b2[j], b1[j], b2[j]], 1)
    return fid, bc, tt


# ---- the independent float64 formulation: the ray meets the face's plane at t = n.(a - o) / n.d, and the point lies in the face if the three
# edge functions cross(edge, x - corner) . n are all >= 0. Shares no code with the sheared test above.
def hit64(o, d, near, far, v, f, chunk=None):
    """Returns f_id (n,) int64 (-1: miss), t (n,), x (n, 3) the hit point, all float64; the nearest face, the lowest index among equal t."""
    f = np.asarray(f).astype(np.int64)
    d64, v64 = d.astype(np.float64), v.astype(np.float64)
    n = len(d64)
    o64 = np.broadcast_to(np.asarray(o, dtype=np.float64).reshape(-1, 3), (n, 3)) if np.asarray(o).size == 3 else o.astype(np.float64)
    a, b, c = v64[f[:, 0]][None], v64[f[:, 1]][None], v64[f[:, 2]][None]
    nrm = np.cross(b - a, c - a)
    fid = np.full(n, -1, np.int64); tt = np.full(n, np.inf); xx = np.zeros((n, 3))
    step = chunk or max(1, 1_000_000 // len(f))
    dot = lambda x, y: np.einsum("...k,...k->...", x, y)
    for i0 in range(0, n, step):
        oo, dd = o64[i0:i0 + step, None, :], d64[i0:i0 + step, None, :]
        with np.errstate(all="ignore"):
            den = dot(nrm, dd)
            t = dot(nrm, a - oo) / den
            x = oo + t[..., None] * dd
            inside = (dot(np.cross(b - a, x - a), nrm) >= 0) & (dot(np.cross(c - b, x - b), nrm) >= 0) & (dot(np.cross(a - c, x - c), nrm) >= 0)
        ok = inside & (den != 0) & (t >= near) & (t <= far)
        key = np.where(ok, t, np.inf)
        j = np.argmin(key, axis=1)
        r = np.arange(len(j))
        hit = key[r, j] < np.inf
        sl = slice(i0, i0 + len(j))
        fid[sl] = np.where(hit, j, -1); tt[sl] = key[r, j]; xx[sl] = np.where(hit[:, None], x[r, j], 0.0)
    return fid, tt, xx


def excess(o, d, v, f, got, T, what=""):
    """The two accuracy figures of a set of rays against hit64, in units of eps(T) * max(S, |o|), and the share of rays left out (those whose
    hit/miss or face differs between the contract and float64)."""
    fid, bc, t = got
    n = len(d)
    o = _rows(o, n, T)
    f = np.asarray(f).astype(np.int64)
    fid64, t64, x64 = hit64(o, d, 0.0, np.inf, v, f)
    same = (fid == fid64) & (fid >= 0)
    left_out = float(np.mean(fid != fid64))
    scale = np.finfo(T).eps * np.maximum(float(mesh_scale(v, f)), np.abs(o.astype(np.float64)).max(axis=1))
    along = o.astype(np.float64) + t.astype(np.float64)[:, None] * d.astype(np.float64)
    tri = v.astype(np.float64)[f[np.where(same, fid, 0)]]
    surf = np.einsum("ij,ijk->ik", bc.astype(np.float64), tri)
    e_ray = float((np.abs(along - x64).max(axis=1) / scale)[same].max())
    e_bc = float((np.abs(surf - x64).max(axis=1) / scale)[same].max())
    return e_ray, e_bc, left_out, int(same.sum())


# ---- meshes and rays
def cube_twist(dtype):
    """The reference's data/cube_twist.obj (tests/golden/make_golden_rays.py), normalised as the reference's test does: into [-1, 1]^3."""
    v = np.load(os.path.join(GOLDEN, "cube_twist_v.npy"))
    f = np.load(os.path.join(GOLDEN, "cube_twist_f.npy"))
    v = v - v.min(0)
    v /= v.max(0)
    v -= 0.5
    v *= 2.0
    return np.ascontiguousarray(v.astype(dtype)), np.ascontiguousarray(f.astype(np.int64))


def octahedron(dtype):
    v = np.array([[1, 0, 0], [-1, 0, 0], [0, 1, 0], [0, -1, 0], [0, 0, 1], [0, 0, -1]], dtype=dtype)
    f = np.array([[0, 2, 4], [2, 1, 4], [1, 3, 4], [3, 0, 4], [2, 0, 5], [1, 2, 5], [3, 1, 5], [0, 3, 5]], dtype=np.int64)
    return v, f


def _frame(v):
    v64 = v.astype(np.float64)
    lo, hi = v64.min(0), v64.max(0)
    return (lo + hi) / 2, hi - lo


def rays_box_to_surface(v, f, n, dtype, seed, extents=3.0):
    """Origins uniform in a box of `extents` bounding-box extents, aimed at area-weighted surface samples (directions not normalised)."""
    rng = np.random.default_rng(seed)
    mid, ext = _frame(v)
    o = mid + (rng.random((n, 3)) - 0.5) * extents * ext
    x = mc.surface_samples(v, f, n, seed + 1)
    return np.ascontiguousarray(o.astype(dtype)), np.ascontiguousarray((x - o).astype(dtype))


def rays_far_to_surface(v, f, n, dtype, seed, extents=1000.0):
    """Origins on a sphere `extents` extents away, aimed at surface samples."""
    rng = np.random.default_rng(seed)
    mid, ext = _frame(v)
    u = rng.normal(size=(n, 3)); u /= np.linalg.norm(u, axis=1, keepdims=True)
    o = mid + u * extents * ext.max()
    x = mc.surface_samples(v, f, n, seed + 1)
    return np.ascontiguousarray(o.astype(dtype)), np.ascontiguousarray((x - o).astype(dtype))


def edge_and_vertex_targets(v, f, n, seed):
    """n random points on random edges and n vertices of referenced rows, float64."""
    rng = np.random.default_rng(seed)
    f = np.asarray(f).astype(np.int64)
    v64 = v.astype(np.float64)
    fi, e, s = rng.integers(0, len(f), n), rng.integers(0, 3, n), rng.random(n)
    p0, p1 = v64[f[fi, e]], v64[f[fi, (e + 1) % 3]]
    return p0 + s[:, None] * (p1 - p0), v64[f[rng.integers(0, len(f), n), rng.integers(0, 3, n)]]


def rays_at_edges_and_vertices(v, f, origin, n, dtype, seed):
    """From one origin: n rays at random edge points, then n rays at vertices. Returns o (3,), d (2n, 3)."""
    edges, verts = edge_and_vertex_targets(v, f, n, seed)
    o = np.asarray(origin, dtype=np.float64)
    return o.astype(dtype), np.ascontiguousarray((np.concatenate([edges, verts]) - o).astype(dtype))


def box_candidates(o, d, v, f, slack=1e-3, workers=8):
    """A sound float64 filter for meshes too large for brute force: per ray the ascending list of faces whose bounding box, padded by `slack`
    of the mesh's scale and 64 eps(T) of the origins' (step 3 of the contract pads by 16 eps of the larger), the ray's line crosses."""
    f = np.asarray(f).astype(np.int64)
    n = len(d)
    o64 = np.broadcast_to(np.asarray(o, dtype=np.float64).reshape(-1, 3), (n, 3)) if np.asarray(o).size == 3 else o.astype(np.float64)
    d64 = d.astype(np.float64)
    tri = v.astype(np.float64)[f]
    pad = slack * float(np.abs(tri).max()) + 64 * float(np.finfo(d.dtype).eps) * float(np.abs(o64).max())
    lo, hi = tri.min(axis=1) - pad, tri.max(axis=1) + pad
    def one(i):
        with np.errstate(all="ignore"):
            inv = 1.0 / d64[i]
            t1, t2 = (lo - o64[i]) * inv, (hi - o64[i]) * inv
            nn, ff = np.fmin(t1, t2), np.fmax(t1, t2)
            t_in = np.fmax(np.fmax(nn[:, 0], nn[:, 1]), nn[:, 2])
            t_out = np.fmin(np.fmin(ff[:, 0], ff[:, 1]), ff[:, 2])
            return np.flatnonzero(~(t_in > t_out))

    with ThreadPoolExecutor(workers) as ex:                      # (numpy releases the GIL inside its loops)
        return list(ex.map(one, range(n)))
