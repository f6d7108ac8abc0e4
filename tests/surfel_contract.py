"""The contract of ray_surfel_intersection and pointcloud_surfel_geometry restated in numpy. Helper module (no tests):
tests/test_surfel_contract.py checks it on the CPU, tests/test_gpu_surfels.py holds the kernels to it bit for bit.

Contract. All arithmetic in the input type T, every product, sum and difference rounded on its own, IEEE division and square root,
dot(x, y) = (x0*y0 + x1*y1) + x2*y2, cross(a, b) = (a1*b2 - a2*b1, a2*b0 - a0*b2, a0*b1 - a1*b0).
  table      c_j = cos(6.283185307179586 * j / subdivs), s_j = sin(...) for j in [0, subdivs), in double with the C library (math.cos and
             math.sin call the one the library's host code calls), rounded to T once
  per point  l = sqrt(dot(n, n)); ni = n / l component by component, or 0 if l == 0; e = (1,0,0) if fabs(fabs(ni[1]) - 1) < T(1e-5), else
             (0,1,0); right0 = cross(ni, e), right = right0 / |right0| (0 if that length is 0); up0 = cross(ni, right), up = up0 / |up0|
             (or 0); A = r * right, B = r * up; rim vertex j = (c_j * A + s_j * B) + p per component; the centre vertex is p
  geometry   point i owns vertices [i (subdivs + 1), (i + 1)(subdivs + 1)), the rim vertices first, then the centre, and faces
             [i subdivs, (i + 1) subdivs): face j = (centre, rim j, rim (j + 1) % subdivs)
  rays       (pid, t) = (f_id // subdivs, t) of ray_contract.hit_brute on that geometry; misses give (-1, +inf)."""
import math

import numpy as np

import ray_contract as rc


def table(subdivs, T):
    """(c, s), each (subdivs,) in T."""
    T = np.dtype(T)
    c = np.array([math.cos(6.283185307179586 * j / subdivs) for j in range(subdivs)], dtype=np.float64).astype(T)
    s = np.array([math.sin(6.283185307179586 * j / subdivs) for j in range(subdivs)], dtype=np.float64).astype(T)
    return c, s


def _dot(x, y):
    return (x[..., 0] * y[..., 0] + x[..., 1] * y[..., 1]) + x[..., 2] * y[..., 2]


def _cross(a, b):
    return np.stack([a[..., 1] * b[..., 2] - a[..., 2] * b[..., 1], a[..., 2] * b[..., 0] - a[..., 0] * b[..., 2],
                     a[..., 0] * b[..., 1] - a[..., 1] * b[..., 0]], axis=-1)


def _unit(x):
    T = x.dtype
    with np.errstate(all="ignore"):
        l = np.sqrt(_dot(x, x))
        return np.where((l == 0)[..., None], T.type(0), x / l[..., None]), l


def basis(n):
    """n (N, 3) in T -> (right, up, ni, l), the reference's local_basis minus its NaN for a zero normal."""
    T = n.dtype
    assert T in (np.dtype(np.float32), np.dtype(np.float64))
    ni, l = _unit(n)
    along_y = np.abs(np.abs(ni[:, 1]) - T.type(1)) < T.type(1e-5)
    e = np.zeros_like(n)
    e[:, 0] = along_y
    e[:, 1] = ~along_y
    right, _ = _unit(_cross(ni, e))
    up, _ = _unit(_cross(ni, right))
    assert right.dtype == T and up.dtype == T and ni.dtype == T and l.dtype == T
    return right, up, ni, l


def geometry(p, n, r, subdivs):
    """p, n (N, 3) and r (N,) of one float dtype -> v (N (subdivs + 1), 3) in that dtype, f (N subdivs, 3) int32."""
    T = p.dtype
    assert n.dtype == T and r.dtype == T and r.shape == (len(p),) and subdivs >= 4
    N = len(p)
    right, up, _, _ = basis(n)
    c, s = table(subdivs, T)
    with np.errstate(all="ignore"):
        A, B = r[:, None] * right, r[:, None] * up
        rim = (c[None, :, None] * A[:, None, :] + s[None, :, None] * B[:, None, :]) + p[:, None, :]
    v = np.concatenate([rim, p[:, None, :]], axis=1).reshape(-1, 3)
    assert v.dtype == T
    base = (np.arange(N, dtype=np.int64) * (subdivs + 1))[:, None]
    j = np.arange(subdivs, dtype=np.int64)[None, :]
    f = np.stack([np.broadcast_to(base + subdivs, (N, subdivs)), base + j, base + (j + 1) % subdivs], axis=-1).reshape(-1, 3)
    return np.ascontiguousarray(v), np.ascontiguousarray(f.astype(np.int32))


def hit(p, n, r, subdivs, o, d, near=0.0, far=np.inf):
    """The contract's (pid (int32), t) for every ray: hit_brute on the fan geometry, then // subdivs."""
    T = d.dtype
    if len(p) == 0:
        return np.full(len(d), -1, np.int32), np.full(len(d), np.inf, T)
    v, f = geometry(p, n, r, subdivs)
    fid, _, t = rc.hit_brute(o, d, near, far, v, f)
    return np.where(fid >= 0, fid // subdivs, -1).astype(np.int32), t


def radii(r, N, T):
    """What the package makes of its argument r (a scalar, a list or an array of shape (N,) or (N, 1), of any float dtype): (N,) in T."""
    if np.isscalar(r):
        return np.full(N, r, dtype=np.float64).astype(T)
    return np.asarray(r).reshape(-1).astype(T)
