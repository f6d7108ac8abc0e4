// csrc/mesh_sample.h -- mesh_face_areas, sample_mesh_random and the candidates of sample_mesh_poisson_disk (src/face_areas.cpp:17-79,
// src/sample_mesh.cpp:34-115).
//
// The reference draws its samples with libigl and rand(); this library states a deterministic contract instead, with
// T the type of v and everything rounded operation by operation (the translation unit is built without FMA contraction):
//   area      |d| = sqrt((d0*d0 + d1*d1) + d2*d2), a = |v2 - v1|, b = |v3 - v2|, c = |v1 - v3|, p = 0.5 * ((a + b) + c),
//             A = sqrt(((p * m(p - a)) * m(p - b)) * m(p - c)), m(x) = x < 0 ? 0 : x (std::max: a NaN passes through)       [in T]
//   weight    w_t = floor(((double)A_t / (double)A_max) * 2^36) as uint64; C = inclusive scan of w in face order, W = C[#f - 1]. Integer
//             weights make the scan associative: no result depends on how it is tiled.
//   sample i  h_j = mix(pd_priority(seed, i) + (j + 1) * 0x9E3779B97F4A7C15), j = 0, 1, 2 (mix: poisson.h);
//             face = the first t with C_t > hi64(h_0 * W);  r = (h_1 >> 11) * 2^-53, s = (h_2 >> 11) * 2^-53, q = sqrt(r) in double;
//             bc = (1 - q, (1 - s) * q, s * q), each rounded to T.
//   position  P_i = (bc0 * v1 + bc1 * v2) + bc2 * v3 in T (the candidates of the Poisson-disk path).
// Row i depends on (seed, i) and the mesh alone: no launch geometry, no atomics on floating-point values.
#pragma once
#include "pcu_types.h"
#include "poisson.h"

namespace pcu {

constexpr int kMsWeightBits = 36;
constexpr int kMsTable = 1024;             // entries of the LDS table over C (k_mesh_sample): every ceil(#f / 1024)-th one
constexpr int kMsPerLane = 4;              // samples per lane of k_mesh_sample: one table load serves 1024 samples

// What one call keeps on the device next to the areas: the largest area as an order-preserving bit pattern (areas are never negative, so the
// pattern without its sign bit orders them; a NaN sorts above +inf and surfaces in the same word).
template <typename T>
struct MsHead {
    typename EncT<T>::type amax;
};
__device__ __forceinline__ unsigned ms_bits(float x) { return __float_as_uint(x) & 0x7fffffffu; }
__device__ __forceinline__ unsigned long long ms_bits(double x) { return (unsigned long long)__double_as_longlong(x) & 0x7fffffffffffffffull; }
__device__ __forceinline__ float ms_unbits(unsigned u) { return __uint_as_float(u); }
__device__ __forceinline__ double ms_unbits(unsigned long long u) { return __longlong_as_double((long long)u); }

template <typename T>
__device__ __forceinline__ T ms_len(const T* __restrict__ p, const T* __restrict__ q) {
    const T d0 = p[0] - q[0], d1 = p[1] - q[1], d2 = p[2] - q[2];
    return sqrt((d0 * d0 + d1 * d1) + d2 * d2);
}
template <typename T> __device__ __forceinline__ T ms_max0(T x) { return x < (T)0 ? (T)0 : x; }

// One lane per face, through the range-checked int32 triples of k_mesh_faces. The largest area: a wave reduction and one integer atomic.
// bad (optional): the finished flag word of the launches before, where `area` is the caller's own memory: with a vertex or face bit raised
// the call will be refused, and no area is written.
template <typename T>
__global__ __launch_bounds__(kBlock) void k_mesh_areas(const T* __restrict__ v, const int* __restrict__ fidx, int nf, T* __restrict__ area,
                                                       MsHead<T>* __restrict__ h, const int* __restrict__ bad) {
    using E = typename EncT<T>::type;
    const int t = blockIdx.x * kBlock + threadIdx.x;
    const bool refused = bad && (*bad & (kMeshBadVertex | kMeshBadFace)) != 0;
    E key = 0;
    if (t < nf) {
        const T* v1 = v + 3 * (size_t)fidx[3 * (size_t)t];
        const T* v2 = v + 3 * (size_t)fidx[3 * (size_t)t + 1];
        const T* v3 = v + 3 * (size_t)fidx[3 * (size_t)t + 2];
        const T a = ms_len(v2, v1), b = ms_len(v3, v2), c = ms_len(v1, v3);
        const T p = (T)0.5 * ((a + b) + c);
        const T A = sqrt(((p * ms_max0(p - a)) * ms_max0(p - b)) * ms_max0(p - c));
        if (!refused) area[t] = A;
        key = ms_bits(A);
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) { const E w = (E)__shfl_xor(key, o, 64); key = w > key ? w : key; }
    if ((threadIdx.x & 63) == 0 && key != 0) atomicMax(&h->amax, key);
}

// w_t; all zero unless the largest area is finite and positive (the host refuses those meshes after its one wait).
template <typename T>
__global__ __launch_bounds__(kBlock) void k_mesh_weights(const T* __restrict__ area, int nf, const MsHead<T>* __restrict__ h,
                                                         unsigned long long* __restrict__ w) {
    const int t = blockIdx.x * kBlock + threadIdx.x;
    if (t >= nf) return;
    const T amax = ms_unbits(h->amax);
    const bool ok = amax > (T)0 && amax < Limits<T>::max_v * (T)2;          // (finite: inf and NaN fail the comparison)
    // y is an integer of at most 2^36: split exactly into two 32-bit halves (the compiler's own double -> uint64 conversion brings a fused
    // multiply-add, which test_mesh_kernels_fuse_only_inside_division_and_square_root does not allow in a k_mesh_* kernel)
    const double y = ok ? floor(((double)area[t] / (double)amax) * (double)(1ull << kMsWeightBits)) : 0.0;
    const unsigned hi = (unsigned)(y * 0x1p-32);
    const unsigned lo = (unsigned)(y - (double)hi * 0x1p32);
    w[t] = ((unsigned long long)hi << 32) | lo;
}

struct MsDraw { unsigned long long h0, h1, h2; };
__host__ __device__ __forceinline__ MsDraw ms_draw(unsigned seed, unsigned long long i) {
    const unsigned long long p = pd_priority(seed, i), g = 0x9E3779B97F4A7C15ull;
    return {pd_mix(p + g), pd_mix(p + 2ull * g), pd_mix(p + 3ull * g)};
}

// One lane per kMsPerLane samples. The face is an upper bound search over C: its top ten steps run over a table of every stride-th entry
// of C in LDS (stride = ceil(#f / 1024); entry k is C[min((k + 1) * stride, #f) - 1]), the rest over the stride entries in global memory.
// Measured against the plain binary search over C in global memory (profiles/f9_search_ab.txt): 41 against 51 us per million
// samples on 204,800 faces. The table fill is a strided gather (one cache line per entry from 16 faces per entry on), repeated by every block.
template <typename T>
__global__ __launch_bounds__(kBlock) void k_mesh_sample(const unsigned long long* __restrict__ C, int nf, unsigned seed, long long n,
                                                        long long* __restrict__ out_fi, T* __restrict__ out_bc) {
    const unsigned long long W = C[nf - 1];
    if (W == 0ull) return;                                                  // (a mesh the host refuses)
    const int stride = (nf + kMsTable - 1) / kMsTable;
    __shared__ unsigned long long s_top[kMsTable];
    for (int k = threadIdx.x; k < kMsTable; k += kBlock) {
        const long long e = (long long)(k + 1) * stride;
        s_top[k] = C[(e < nf ? e : (long long)nf) - 1];
    }
    __syncthreads();
    const long long i0 = (long long)blockIdx.x * (kBlock * kMsPerLane) + threadIdx.x;
#pragma unroll
    for (int q = 0; q < kMsPerLane; ++q) {
        const long long i = i0 + (long long)q * kBlock;
        if (i >= n) break;
        const MsDraw d = ms_draw(seed, (unsigned long long)i);
        const unsigned long long x = __umul64hi(d.h0, W);                    // < W = C[nf - 1]: the search always ends inside C
        int lo = 0, hi = kMsTable - 1;                                      // first k with s_top[k] > x
        while (lo < hi) { const int m = (lo + hi) >> 1; if (s_top[m] > x) hi = m; else lo = m + 1; }
        const long long b = (long long)lo * stride, e = b + stride;
        int tl = (int)b, th = (int)((e < nf ? e : (long long)nf) - 1);       // first t in the table entry's run with C[t] > x
        while (tl < th) { const int m = (int)(((long long)tl + th) >> 1); if (C[m] > x) th = m; else tl = m + 1; }
        const double r = (double)(d.h1 >> 11) * 0x1p-53, s = (double)(d.h2 >> 11) * 0x1p-53;
        const double sq = sqrt(r);
        out_fi[i] = tl;
        out_bc[3 * i] = (T)(1.0 - sq);
        out_bc[3 * i + 1] = (T)((1.0 - s) * sq);
        out_bc[3 * i + 2] = (T)(s * sq);
    }
}

// The candidates' positions, as interpolate_barycentric_coords gives them in numpy.
template <typename T>
__global__ __launch_bounds__(kBlock) void k_mesh_positions(const T* __restrict__ v, const int* __restrict__ fidx, const long long* __restrict__ fi,
                                                           const T* __restrict__ bc, int n, T* __restrict__ P) {
    const int i = blockIdx.x * kBlock + threadIdx.x;
    if (i >= n) return;
    const size_t t = (size_t)fi[i];
    const T* v1 = v + 3 * (size_t)fidx[3 * t];
    const T* v2 = v + 3 * (size_t)fidx[3 * t + 1];
    const T* v3 = v + 3 * (size_t)fidx[3 * t + 2];
    const T b0 = bc[3 * (size_t)i], b1 = bc[3 * (size_t)i + 1], b2 = bc[3 * (size_t)i + 2];
#pragma unroll
    for (int k = 0; k < 3; ++k) P[3 * (size_t)i + k] = (b0 * v1[k] + b1 * v2[k]) + b2 * v3[k];
}

// The kept candidates' rows, in ascending candidate order.
template <typename T>
__global__ __launch_bounds__(kBlock) void k_mesh_keep(const int32_t* __restrict__ idx, int m, const long long* __restrict__ fi, const T* __restrict__ bc,
                                                      long long* __restrict__ out_fi, T* __restrict__ out_bc) {
    const int k = blockIdx.x * kBlock + threadIdx.x;
    if (k >= m) return;
    const size_t i = (size_t)idx[k];
    out_fi[k] = fi[i];
    out_bc[3 * (size_t)k] = bc[3 * i]; out_bc[3 * (size_t)k + 1] = bc[3 * i + 1]; out_bc[3 * (size_t)k + 2] = bc[3 * i + 2];
}

}  // namespace pcu
