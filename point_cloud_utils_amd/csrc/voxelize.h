// csrc/voxelize.h -- voxelize_triangle_mesh, sparse_voxel_grid_boundary and voxel_grid_geometry (src/voxelize_triangle_mesh.cpp,
// src/sparse_voxel_grid.cpp:473-522, src/mesh_for_voxels.cpp:11-79): kernels and contract. Host side: voxelize_host.h.
//
// Voxelization. Voxel ijk is the box with centre origin + ijk * size and half size size / 2 (what the reference's code does; its docstring
// says "corner"). A face's candidates are the integer boxes lo..hi on all three axes, lo = floor((min - origin) / size), hi = ceil((max -
// origin) / size) over its three corners -- the reference's formula, applied to x as well (the reference's x loop runs `widx <= inix` and only
// ever visits the first column: a bug that is not reproduced). A candidate is kept iff the triangle-box overlap test of Akenine-Moller as the
// reference evaluates it (src/common/tribox.h:112-187) says so: in double without FMA, on the corners less the box centre, the edges taken
// from those already-rounded differences, the nine edge-axis tests in the reference's order, then the three box axes, then the plane; touching
// counts. Nothing of that arithmetic is shared between the candidates of a face: its bits depend on the box. The result is the set of kept
// ijk, each once, ascending by MortonCode64.
//
// Device shape: one thread per face writes its extent and candidate count (k_vx_extent), the counts are scanned, and candidate RANKS --
// positions in the concatenation of all faces' candidates, x outermost and z innermost within a face -- are cut into slices of kVxSlice. A
// block of the test pass finds its slice's first face with one binary search in the scan, stages the slice's part of the scan in LDS (a face
// has at least one candidate: at most kVxSlice faces), and every lane finds its face there, decodes its rank into a box and runs the test.
// Verdicts leave as one ballot word per wave and one count per block; the emit pass scans the counts, reads the words back and writes the
// kept boxes' Morton codes, which are sorted (radix.h) on as many bits as the extent of the candidates needs, and made unique.
#pragma once
#include "pcu_types.h"
#include "morton.h"
#include "radix.h"

namespace pcu {

constexpr int kVxThreads = 256, kVxItems = 8;
constexpr int kVxSlice = kVxThreads * kVxItems;             // 2048 candidate ranks per block of the test and emit passes
constexpr int kVxWords = kVxSlice / 64;                     // ballot words per slice
constexpr double kVxRange = 1048576.0;                      // voxel coordinates live in [-2^20, 2^20): the 21 bits per axis of MortonCode64
constexpr unsigned long long kVxMaxCandidates = 1ull << 32; // the candidate cap of one call. A choice (it bounds the time one call can hold a GPU), not a measured limit.
constexpr unsigned long long kVxFaceSat = 1ull << 33;       // a face's count saturates here, above the cap: 2^27 faces cannot overflow the 64-bit scan
constexpr int kVxBadRange = 4;                              // next to kMeshBadVertex / kMeshBadFace in the call's flag word
constexpr int kVxBadCoord = 8;                              // a voxel coordinate of the input outside [-2^20, 2^20) (k_vb_codes, k_hx_codes of marching_cubes.h)

struct VxGrid { double size[3], origin[3]; };
struct VxHead { int lo[3], hi[3]; };                        // extent of all candidates (atomics; lo starts at INT_MAX, hi at INT_MIN)

// ---------------------------------------------------------------------------------------------------- the overlap test
// One separating-axis test: the projections pa, pb of two corners against the box's radius on that axis.
__device__ __forceinline__ bool vx_apart(double pa, double pb, double rad) {
    const double mn = pa < pb ? pa : pb, mx = pa < pb ? pb : pa;
    return mn > rad || mx < -rad;
}
__device__ __forceinline__ bool vx_apart3(double a, double b, double c, double h) {
    double mn = a, mx = a;
    if (b < mn) mn = b;
    if (b > mx) mx = b;
    if (c < mn) mn = c;
    if (c > mx) mx = c;
    return mn > h || mx < -h;
}
// triangle (t0, t1, t2) against the box of centre c and half size h
__device__ __forceinline__ bool vx_tribox(const double* c, const double* h, const double* t0, const double* t1, const double* t2) {
    double v0[3], v1[3], v2[3], e0[3], e1[3], e2[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) { v0[k] = t0[k] - c[k]; v1[k] = t1[k] - c[k]; v2[k] = t2[k] - c[k]; }
#pragma unroll
    for (int k = 0; k < 3; ++k) { e0[k] = v1[k] - v0[k]; e1[k] = v2[k] - v1[k]; e2[k] = v0[k] - v2[k]; }
    // axis e x (1,0,0): corners p, q projected as a*y - b*z; e x (0,1,0): -a*x + b*z; e x (0,0,1): a*x - b*y
    auto ax = [&](const double* e, const double* p, const double* q) {
        const double a = e[2], b = e[1];
        return vx_apart(a * p[1] - b * p[2], a * q[1] - b * q[2], fabs(e[2]) * h[1] + fabs(e[1]) * h[2]);
    };
    auto ay = [&](const double* e, const double* p, const double* q) {
        const double a = e[2], b = e[0];
        return vx_apart(-a * p[0] + b * p[2], -a * q[0] + b * q[2], fabs(e[2]) * h[0] + fabs(e[0]) * h[2]);
    };
    auto az = [&](const double* e, const double* p, const double* q) {
        const double a = e[1], b = e[0];
        return vx_apart(a * p[0] - b * p[1], a * q[0] - b * q[1], fabs(e[1]) * h[0] + fabs(e[0]) * h[1]);
    };
    if (ax(e0, v0, v2) || ay(e0, v0, v2) || az(e0, v1, v2)) return false;
    if (ax(e1, v0, v2) || ay(e1, v0, v2) || az(e1, v0, v1)) return false;
    if (ax(e2, v0, v1) || ay(e2, v0, v1) || az(e2, v1, v2)) return false;
    if (vx_apart3(v0[0], v1[0], v2[0], h[0]) || vx_apart3(v0[1], v1[1], v2[1], h[1]) || vx_apart3(v0[2], v1[2], v2[2], h[2])) return false;
    // the triangle's plane against the box: normal = e0 x e1, the box corners farthest along -normal and +normal, relative to v0
    const double n[3] = {e0[1] * e1[2] - e0[2] * e1[1], e0[2] * e1[0] - e0[0] * e1[2], e0[0] * e1[1] - e0[1] * e1[0]};
    double lo[3], hi[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        if (n[k] > 0.0) { lo[k] = -h[k] - v0[k]; hi[k] = h[k] - v0[k]; }
        else { lo[k] = h[k] - v0[k]; hi[k] = -h[k] - v0[k]; }
    }
    if ((n[0] * lo[0] + n[1] * lo[1]) + n[2] * lo[2] > 0.0) return false;
    return (n[0] * hi[0] + n[1] * hi[1]) + n[2] * hi[2] >= 0.0;
}

// ---------------------------------------------------------------------------------------------------- extent pass
__global__ void k_vx_head_init(VxHead* h) {
    if (threadIdx.x < 3) { h->lo[threadIdx.x] = 0x7fffffff; h->hi[threadIdx.x] = (int)0x80000000; }
}
// ext (nf, 6): lo[3] and the number of boxes n[3] per axis; cnt (nf): n0 * n1 * n2 (0 for a face that raised a flag). The bounds are compared
// in double before any conversion to an integer.
template <typename T>
__global__ __launch_bounds__(kBlock) void k_vx_extent(const T* __restrict__ v, const int* __restrict__ fidx, int nf, VxGrid g, int* __restrict__ ext,
                                                      unsigned long long* __restrict__ cnt, int* __restrict__ bad, VxHead* __restrict__ head) {
    const int i = blockIdx.x * kBlock + threadIdx.x;
    int lo[3] = {0x7fffffff, 0x7fffffff, 0x7fffffff}, hi[3] = {(int)0x80000000, (int)0x80000000, (int)0x80000000};
    bool out = false;
    if (i < nf) {
        const size_t a = 3 * (size_t)fidx[3 * (size_t)i], b = 3 * (size_t)fidx[3 * (size_t)i + 1], c = 3 * (size_t)fidx[3 * (size_t)i + 2];
        double l[3], h[3];
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            const double x0 = (double)v[a + k], x1 = (double)v[b + k], x2 = (double)v[c + k];
            double mn = x1 < x2 ? x1 : x2, mx = x1 > x2 ? x1 : x2;
            mn = x0 < mn ? x0 : mn; mx = x0 > mx ? x0 : mx;
            l[k] = floor((mn - g.origin[k]) / g.size[k]);
            h[k] = ceil((mx - g.origin[k]) / g.size[k]);
            if (!(l[k] >= -kVxRange && h[k] < kVxRange && l[k] <= h[k])) out = true;          // (a NaN fails every comparison)
        }
        unsigned long long n = 0ull;
        int e[6] = {0, 0, 0, 0, 0, 0};
        if (!out) {
#pragma unroll
            for (int k = 0; k < 3; ++k) { lo[k] = (int)l[k]; hi[k] = (int)h[k]; e[k] = lo[k]; e[3 + k] = hi[k] - lo[k] + 1; }
            n = (unsigned long long)e[3] * (unsigned long long)e[4];                          // < 2^42
            n = n >= kVxFaceSat ? kVxFaceSat : n * (unsigned long long)e[5];                  // < 2^54
            n = n > kVxFaceSat ? kVxFaceSat : n;
        }
#pragma unroll
        for (int k = 0; k < 6; ++k) ext[6 * (size_t)i + k] = e[k];
        cnt[i] = n;
    }
#pragma unroll
    for (int k = 0; k < 3; ++k) {
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            const int p = __shfl_xor(lo[k], o, 64), q = __shfl_xor(hi[k], o, 64);
            lo[k] = p < lo[k] ? p : lo[k]; hi[k] = q > hi[k] ? q : hi[k];
        }
    }
    const bool any_out = __ballot(out) != 0ull;
    if ((threadIdx.x & 63) == 0) {
#pragma unroll
        for (int k = 0; k < 3; ++k) {           // (an atomic only where it would move the extent: a stale read costs one atomic more, never a wrong extent)
            if (lo[k] > hi[k]) continue;
            if (lo[k] < __atomic_load_n(&head->lo[k], __ATOMIC_RELAXED)) atomicMin(&head->lo[k], lo[k]);
            if (hi[k] > __atomic_load_n(&head->hi[k], __ATOMIC_RELAXED)) atomicMax(&head->hi[k], hi[k]);
        }
        if (any_out) atomicOr(bad, kVxBadRange);
    }
}

// ---------------------------------------------------------------------------------------------------- test and emit passes
// What a block of either pass knows of its slice: the scan C of the faces [f0, f0 + n) in LDS and the scan's value before f0.
struct VxSlice { int f0, n; unsigned long long before; };
__device__ __forceinline__ VxSlice vx_stage(const unsigned long long* __restrict__ C, int nf, unsigned long long base, unsigned long long* s_C, int* s_f0) {
    if (threadIdx.x == 0) {                     // the first face whose candidates reach past `base`
        int lo = 0, hi = nf;
        while (lo < hi) { const int mid = lo + ((hi - lo) >> 1); if (C[mid] > base) hi = mid; else lo = mid + 1; }
        *s_f0 = lo;
    }
    __syncthreads();
    VxSlice s;
    s.f0 = *s_f0;
    s.n = nf - s.f0 < kVxSlice ? nf - s.f0 : kVxSlice;
    for (int j = threadIdx.x; j < s.n; j += kVxThreads) s_C[j] = C[s.f0 + j];
    s.before = s.f0 > 0 ? C[s.f0 - 1] : 0ull;
    __syncthreads();
    return s;
}
// The box of candidate `rank`: its face and integer coordinates. False for a rank beyond the slice's faces (never for rank < the total).
__device__ __forceinline__ bool vx_locate(const VxSlice& s, const unsigned long long* s_C, const int* __restrict__ ext, unsigned long long rank, int& face, int* ijk) {
    int lo = 0, hi = s.n;
    while (lo < hi) { const int mid = (lo + hi) >> 1; if (s_C[mid] > rank) hi = mid; else lo = mid + 1; }
    if (lo >= s.n) return false;
    const unsigned long long local = rank - (lo > 0 ? s_C[lo - 1] : s.before);
    face = s.f0 + lo;
    const int* e = ext + 6 * (size_t)face;
    const unsigned ny = (unsigned)e[4], nz = (unsigned)e[5];
    const unsigned long long t = local / nz;
    ijk[2] = e[2] + (int)(local - t * nz);
    const unsigned long long u = t / ny;
    ijk[1] = e[1] + (int)(t - u * ny);
    ijk[0] = e[0] + (int)u;
    return true;
}
// words (kVxWords per slice): bit l of word q * 4 + w is the verdict of rank base + q * 256 + w * 64 + l; bcnt (per slice): the kept ranks
template <typename T>
__global__ __launch_bounds__(kVxThreads) void k_vx_test(const T* __restrict__ v, const int* __restrict__ fidx, const int* __restrict__ ext,
                                                        const unsigned long long* __restrict__ C, int nf, unsigned long long total, unsigned long long slice0,
                                                        VxGrid g, unsigned long long* __restrict__ words, unsigned long long* __restrict__ bcnt) {
    __shared__ unsigned long long s_C[kVxSlice];
    __shared__ int s_f0;
    __shared__ unsigned s_k[kVxThreads / 64];
    const unsigned long long slice = slice0 + blockIdx.x, base = slice * (unsigned long long)kVxSlice;
    const VxSlice s = vx_stage(C, nf, base, s_C, &s_f0);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const double h[3] = {g.size[0] / 2, g.size[1] / 2, g.size[2] / 2};
    unsigned kept = 0;
#pragma unroll 1
    for (int q = 0; q < kVxItems; ++q) {
        const unsigned long long rank = base + (unsigned long long)(q * kVxThreads + threadIdx.x);
        bool yes = false;
        int face, ijk[3];
        if (rank < total && vx_locate(s, s_C, ext, rank, face, ijk)) {
            const size_t a = 3 * (size_t)fidx[3 * (size_t)face], b = 3 * (size_t)fidx[3 * (size_t)face + 1], c = 3 * (size_t)fidx[3 * (size_t)face + 2];
            double ctr[3], t0[3], t1[3], t2[3];
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                ctr[k] = g.origin[k] + (double)ijk[k] * g.size[k];
                t0[k] = (double)v[a + k]; t1[k] = (double)v[b + k]; t2[k] = (double)v[c + k];
            }
            yes = vx_tribox(ctr, h, t0, t1, t2);
        }
        const unsigned long long w = __ballot(yes);
        if (lane == 0) { words[slice * kVxWords + (unsigned)(q * (kVxThreads / 64) + wave)] = w; kept += (unsigned)__popcll(w); }
    }
    if (lane == 0) s_k[wave] = kept;
    __syncthreads();
    if (threadIdx.x == 0) { unsigned t = 0; for (int w = 0; w < kVxThreads / 64; ++w) t += s_k[w]; bcnt[slice] = t; }
}
// bscan: the inclusive scan of bcnt. The kept ranks' Morton codes, in rank order.
__global__ __launch_bounds__(kVxThreads) void k_vx_emit(const int* __restrict__ ext, const unsigned long long* __restrict__ C, int nf, unsigned long long slice0,
                                                        const unsigned long long* __restrict__ words, const unsigned long long* __restrict__ bcnt,
                                                        const unsigned long long* __restrict__ bscan, unsigned long long* __restrict__ codes) {
    __shared__ unsigned long long s_C[kVxSlice];
    __shared__ int s_f0;
    __shared__ unsigned long long s_w[kVxWords];
    __shared__ unsigned s_off[kVxWords];
    const unsigned long long slice = slice0 + blockIdx.x, base = slice * (unsigned long long)kVxSlice;
    if (bcnt[slice] == 0ull) return;            // (uniform: nothing of this slice was kept)
    if (threadIdx.x < kVxWords) s_w[threadIdx.x] = words[slice * kVxWords + threadIdx.x];
    const VxSlice s = vx_stage(C, nf, base, s_C, &s_f0);
    if (threadIdx.x == 0) { unsigned t = 0; for (int j = 0; j < kVxWords; ++j) { s_off[j] = t; t += (unsigned)__popcll(s_w[j]); } }
    __syncthreads();
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const unsigned long long first = bscan[slice] - bcnt[slice];
#pragma unroll 1
    for (int q = 0; q < kVxItems; ++q) {
        const int j = q * (kVxThreads / 64) + wave;
        const unsigned long long w = s_w[j];
        if (!((w >> lane) & 1ull)) continue;
        int face, ijk[3];
        if (!vx_locate(s, s_C, ext, base + (unsigned long long)(q * kVxThreads + threadIdx.x), face, ijk)) continue;
        codes[first + s_off[j] + (unsigned)__popcll(w & ((1ull << lane) - 1ull))] = morton_encode3(ijk[0], ijk[1], ijk[2]);
    }
}
// the run heads of the sorted codes, decoded: row scan[j] - 1 of out (m, 3)
__global__ __launch_bounds__(kBlock) void k_vx_rows(const unsigned long long* __restrict__ keys, const unsigned* __restrict__ flag, const unsigned* __restrict__ scan, int n,
                                                    int* __restrict__ out) {
    const int j = blockIdx.x * kBlock + threadIdx.x;
    if (j >= n || !flag[j]) return;
    int x, y, z;
    morton_decode3(keys[j], x, y, z);
    int* row = out + 3 * (size_t)(scan[j] - 1u);
    row[0] = x; row[1] = y; row[2] = z;
}

// ---------------------------------------------------------------------------------------------------- sparse_voxel_grid_boundary
// A coordinate of any of the four integer types (index_kinds.h), and whether it lies in [-2^20, 2^20). The window is signed for the signed
// kinds only: an unsigned value of 2^63 or more is out of range, not a negative coordinate.
__device__ __forceinline__ bool vx_coord(const void* __restrict__ p, int kind, size_t at, int& out) {
    const unsigned long long u = index_in(p, kind, at);
    const bool ok = index_kind_signed(kind) ? u + (1ull << 20) < (1ull << 21) : u < (1ull << 20);
    out = ok ? (int)(long long)u : 0;
    return ok;
}
__global__ __launch_bounds__(kBlock) void k_vb_codes(const void* __restrict__ ijk, int kind, int n, unsigned long long* __restrict__ codes, unsigned long long* __restrict__ sorted,
                                                     int* __restrict__ bad) {
    const int i = blockIdx.x * kBlock + threadIdx.x;
    bool out = false;
    if (i < n) {
        int x, y, z;
        out = !vx_coord(ijk, kind, 3 * (size_t)i, x);
        out |= !vx_coord(ijk, kind, 3 * (size_t)i + 1, y);
        out |= !vx_coord(ijk, kind, 3 * (size_t)i + 2, z);
        const unsigned long long c = morton_encode3(x, y, z);
        codes[i] = c; sorted[i] = c;
    }
    if (__ballot(out) != 0ull && (threadIdx.x & 63) == 0) atomicOr(bad, kVxBadCoord);
}
// flag[i] = 1 if one of the six face neighbours of row i is not among the codes (a neighbour outside [-2^20, 2^20) is absent)
__global__ __launch_bounds__(kBlock) void k_vb_flag(const unsigned long long* __restrict__ codes, const unsigned long long* __restrict__ sorted, int n, unsigned* __restrict__ flag) {
    const int i = blockIdx.x * kBlock + threadIdx.x;
    if (i >= n) return;
    int c[3];
    morton_decode3(codes[i], c[0], c[1], c[2]);
    bool missing = false;
#pragma unroll 1
    for (int o = 0; o < 6 && !missing; ++o) {
        int q[3] = {c[0], c[1], c[2]};
        q[o >> 1] += (o & 1) ? -1 : 1;
        if (q[o >> 1] < -(1 << 20) || q[o >> 1] >= (1 << 20)) { missing = true; break; }
        const unsigned long long want = morton_encode3(q[0], q[1], q[2]);
        int lo = 0, hi = n;
        while (lo < hi) { const int mid = lo + ((hi - lo) >> 1); if (sorted[mid] < want) lo = mid + 1; else hi = mid; }
        missing = lo >= n || sorted[lo] != want;
    }
    flag[i] = missing ? 1u : 0u;
}
// (bad: the finished flag word of k_vb_codes. With its bit raised the call will be refused, and nothing is written to out, which is the caller's
// own memory when the call's pointers are device memory.)
__global__ __launch_bounds__(kBlock) void k_vb_rows(const unsigned* __restrict__ flag, const unsigned* __restrict__ scan, int n, long long* __restrict__ out,
                                                    const int* __restrict__ bad) {
    const int i = blockIdx.x * kBlock + threadIdx.x;
    if (i < n && flag[i] && !(*bad & kVxBadCoord)) out[scan[i] - 1u] = i;
}

// ---------------------------------------------------------------------------------------------------- voxel_grid_geometry
// Thread t < 12 n writes face t, thread t < 8 n vertex t: ((unit * (1 - gap) + 0.5 * gap) + ijk) * size + origin in double, rounded once.
__global__ __launch_bounds__(kBlock) void k_vg_geometry(const void* __restrict__ ijk, int kind, long long n, VxGrid g, double gap, float* __restrict__ out_v, int* __restrict__ out_f) {
    const long long t = (long long)blockIdx.x * kBlock + threadIdx.x;
    if (t < 12 * n) {
        // the reference's twelve triangles (top, bottom, left, right, front, back), three 3-bit corner indices per entry
        constexpr unsigned tri[12] = {2 | 7 << 3 | 6 << 6, 2 | 3 << 3 | 7 << 6, 0 | 4 << 3 | 5 << 6, 0 | 5 << 3 | 1 << 6, 0 | 2 << 3 | 6 << 6, 0 | 6 << 3 | 4 << 6,
                                      1 | 7 << 3 | 3 << 6, 1 | 5 << 3 | 7 << 6, 0 | 3 << 3 | 2 << 6, 0 | 1 << 3 | 3 << 6, 4 | 6 << 3 | 7 << 6, 4 | 7 << 3 | 5 << 6};
        const long long row = t / 12;
        const unsigned e = tri[t - row * 12];
        const int b = (int)(8 * row);
        out_f[3 * t] = b + (int)(e & 7u); out_f[3 * t + 1] = b + (int)((e >> 3) & 7u); out_f[3 * t + 2] = b + (int)((e >> 6) & 7u);
    }
    if (t < 8 * n) {
        const long long row = t >> 3;
        const int vi = (int)(t & 7);
        // corner vi: x = bit 0, y = bit 1, z = 1 for the first four corners and 0 for the last four
        const double unit[3] = {(double)(vi & 1), (double)((vi >> 1) & 1), (double)(vi < 4 ? 1 : 0)};
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            const unsigned long long u = index_in(ijk, kind, 3 * (size_t)row + k);
            const double c = index_kind_signed(kind) ? (double)(long long)u : (double)u;
            double x = unit[k] * (1.0 - gap) + 0.5 * gap;
            x = x + c;
            x = x * g.size[k];
            x = x + g.origin[k];
            out_v[3 * t + k] = (float)x;
        }
    }
}

}  // namespace pcu
