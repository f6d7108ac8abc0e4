"""The contract of mesh_face_areas, sample_mesh_random and sample_mesh_poisson_disk (csrc/mesh_sample.h), restated in
numpy: areas in the type of v, uint64 weights and their cumsum, the three 64-bit draws of a row, the high half of a 128-bit product, the
barycentric coordinates, the candidates' positions and the composition with the Poisson-disk greedy. Everything the GPU returns is compared
with these functions bit for bit (tests/test_gpu_mesh_sampling.py); tests/test_sampling_contract.py tests the restatement itself."""
import math
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
MAX_ROWS = 2 ** 27 - 16
WEIGHT_BITS = 36
GOLDEN_GAMMA = 0x9E3779B97F4A7C15
M64 = (1 << 64) - 1
SC_TILE = 4096                # csrc/radix.h: kScTile, the tile of the inclusive scan
TABLE = 1024                  # csrc/mesh_sample.h: kMsTable, the entries of the search's LDS table


def golden_mesh(name, dtype):
    v = np.load(os.path.join(GOLDEN, f"{name}_v.npy")).astype(dtype)
    f = np.load(os.path.join(GOLDEN, f"{name}_f.npy")).astype(np.int64)
    return np.ascontiguousarray(v), np.ascontiguousarray(f)


# ---- 1. areas, in T
def face_areas(v, f):
    T = v.dtype.type
    f = np.asarray(f).astype(np.int64)
    v1, v2, v3 = v[f[:, 0]], v[f[:, 1]], v[f[:, 2]]

    def norm(d):
        return np.sqrt((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2])

    def m(x):                                       # std::max(x, 0): (x < 0) ? 0 : x, a NaN passes through
        return np.where(x < 0, T(0), x)

    with np.errstate(all="ignore"):
        a, b, c = norm(v2 - v1), norm(v3 - v2), norm(v1 - v3)
        p = T(0.5) * ((a + b) + c)
        return np.sqrt(((p * m(p - a)) * m(p - b)) * m(p - c)).astype(v.dtype)


# ---- 2. weights
def weights(areas):
    """(w, C, W, A_max); raises what the library raises."""
    if not np.all(np.isfinite(areas)):
        raise ValueError("face areas overflow the scalar type of v")
    amax = areas.max()
    if amax == 0:
        raise ValueError("Mesh has zero area")
    w = np.floor((areas.astype(np.float64) / np.float64(amax)) * np.float64(2 ** WEIGHT_BITS)).astype(np.uint64)
    C = np.cumsum(w, dtype=np.uint64)
    return w, C, int(C[-1]), amax


# ---- 3. samples
def mix(z):
    """The splitmix64 finalizer (csrc/poisson.h: pd_mix) on a uint64 array."""
    z = z.copy()
    z ^= z >> np.uint64(30); z *= np.uint64(0xBF58476D1CE4E5B9)
    z ^= z >> np.uint64(27); z *= np.uint64(0x94D049BB133111EB)
    z ^= z >> np.uint64(31)
    return z


def priority(seed, n):
    return mix((np.uint64(seed) << np.uint64(32)) ^ np.arange(n, dtype=np.uint64))


def draws(seed, n):
    p = priority(seed, n)
    return tuple(mix(p + np.uint64(((j + 1) * GOLDEN_GAMMA) & M64)) for j in range(3))


def hi64(h, W):
    """High 64 bits of h * W (h: uint64 array, W: Python int <= 2^63), by 32-bit limbs."""
    lo32 = np.uint64(0xFFFFFFFF); s32 = np.uint64(32)
    hl, hh = h & lo32, h >> s32
    wl, wh = np.uint64(W & 0xFFFFFFFF), np.uint64(W >> 32)
    ll, lh, hl_, hh_ = hl * wl, hl * wh, hh * wl, hh * wh
    mid = (ll >> s32) + (lh & lo32) + (hl_ & lo32)
    return hh_ + (lh >> s32) + (hl_ >> s32) + (mid >> s32)


def sample_rows(C, W, seed, n, dtype):
    """(f_idx int64, bc in dtype) of the rows 0 .. n-1."""
    h0, h1, h2 = draws(seed, n)
    fi = np.searchsorted(C, hi64(h0, W), side="right").astype(np.int64)        # the first t with C_t > x
    r = (h1 >> np.uint64(11)).astype(np.float64) * 2.0 ** -53
    s = (h2 >> np.uint64(11)).astype(np.float64) * 2.0 ** -53
    q = np.sqrt(r)
    bc = np.stack([1.0 - q, (1.0 - s) * q, s * q], axis=1).astype(dtype)
    return fi, np.ascontiguousarray(bc)


def sample_mesh_random(v, f, n, seed):
    _, C, W, _ = weights(face_areas(v, f))
    return sample_rows(C, W, seed, n, v.dtype)


def positions(v, f, fi, bc):
    """interpolate_barycentric_coords(f, fi, bc, v) in numpy: (bc0 * v1 + bc1 * v2) + bc2 * v3 in T."""
    tri = v[np.asarray(f).astype(np.int64)[fi]]
    return np.ascontiguousarray((bc[:, 0:1] * tri[:, 0] + bc[:, 1:2] * tri[:, 1]) + bc[:, 2:3] * tri[:, 2])


# ---- 4. Poisson-disk samples
def candidate_count(oversampling_factor, num_samples, radius, W, amax):
    of = float(np.float32(oversampling_factor))
    total_area = (float(W) * 2.0 ** -WEIGHT_BITS) * float(amax)
    with np.errstate(all="ignore"):
        n_est = np.ceil(np.float64(total_area) / np.float64(0.7 * math.pi * radius * radius)) if radius > 0 else np.float64(0)
        n_c = np.ceil(np.float64(of) * max(np.float64(num_samples), n_est, np.float64(1)))
    if not n_c <= MAX_ROWS:
        raise ValueError("more than 2^27-16 rows are not supported")
    return int(n_c)


def count_limits(target, tol, dtype):
    """f5's own rounding rule: (int)((T)target * (T)(1 -/+ tol)) with tol a float32."""
    T = np.dtype(dtype).type
    tolf = np.float32(tol)
    return int(T(target) * T(np.float32(1.0) - tolf)), int(T(target) * T(np.float32(1.0) + tolf))


def radius_search(P, target, seed, tol, greedy):
    """The reference's radius search (src/sample_point_cloud.cpp:281-329) as tests/test_gpu_poisson_disk.py: greedy_target restates it, driving
    `greedy`; returns (kept rows, the radius of the last run)."""
    T = P.dtype.type
    nmin, nmax = count_limits(target, tol, P.dtype)
    e = P.max(axis=0) - P.min(axis=0)
    bb = np.sqrt((e[0] * e[0] + e[1] * e[1]) + e[2] * e[2])
    rmin = T(float(bb) / 50.0); rmax = rmin
    while True:
        rmin = T(float(rmin) / 2.0); r = rmin
        s = greedy(P, r, seed)
        if len(s) >= target:
            break
    while True:
        rmax = T(float(rmax) * 2.0); r = rmax
        s = greedy(P, r, seed)
        if len(s) <= target:
            break
    it = 0
    while it < 20 and (len(s) < nmin or len(s) > nmax):
        it += 1
        r = T(float(T(rmin + rmax)) / 2.0)
        s = greedy(P, r, seed)
        if len(s) > target:
            rmin = r
        if len(s) < target:
            rmax = r
    return s, r


def sample_mesh_poisson_disk(v, f, num_samples, seed, greedy, radius=0.0, tol=0.04, oversampling_factor=40.0):
    """(f_idx, bc, P, kept candidate rows, N_c, radius of the last run or None); `greedy`: the restated greedy of
    tests/test_gpu_poisson_disk.py."""
    _, C, W, amax = weights(face_areas(v, f))
    n_c = candidate_count(oversampling_factor, num_samples, radius, W, amax)
    fi, bc = sample_rows(C, W, seed, n_c, v.dtype)
    P = positions(v, f, fi, bc)
    r = None
    if radius > 0:
        keep, r = greedy(P, radius, seed), radius
    elif num_samples >= n_c:
        keep = np.arange(n_c, dtype=np.int32)
    else:
        keep, r = radius_search(P, num_samples, seed, tol, greedy)
    return fi[keep], bc[keep], P, keep, n_c, r
