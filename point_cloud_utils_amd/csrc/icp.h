// csrc/icp.h -- the kernels of register_point_clouds_icp (the contract in numpy: tests/icp_contract.py; host loop: icp_host.h).
//
// One evaluation of the current transform M is: k_icp_transform (source rows to p = T(M * row)), the library's own k = 1 search of p in the
// target (knn_impl, untouched), k_icp_sums (inliers, their terms, the first two levels of the sum tree), k_icp_fold (the remaining levels and
// the record the host reads). The two levels are icp_sum_block, which plane.h's and ransac.h's sums use with their own terms. Everything is
// float64 with one rounding per operation (the unit is built with -ffp-contract=off), no square root.
//
// The order of every sum is the contract's fold64: the terms in source-row order, padded with +0.0 to rows of 64; six times the upper half of a
// row is added to its lower half; the row results are the next level's terms; until one value remains. On a wave that is the __shfl_xor
// butterfly with masks 32, 16, ..., 1: lane i < w computes v[i] + v[i + w] exactly as the slice addition does (the upper lanes compute the
// same sums with the operands swapped, which are the same bits, and are not used), and lane 0 ends with the row's value.
// A 1024-thread block owns 4096 consecutive rows: its 16 waves take four groups of 64 each (level 1), the 64 group values of a sum sit in LDS
// and one wave folds them (level 2). A block so emits one value per sum; k_icp_fold folds those by 64 until one is left.
// The sums, in the contract's order: [count, d2, ...] -- 17 in point mode, 30 in plane mode (icp_contract.py's header). The inlier count is the
// sum of 1.0 per inlier, folded like the rest: integers below 2^53 add exactly in any order.
#pragma once
#include "pcu_types.h"

namespace pcu {

constexpr int kIcpBlock = 1024;             // threads of a k_icp_sums / k_icp_fold block: 16 waves
constexpr int kIcpGroups = 64;              // level-1 values of a block
constexpr int kIcpRows = kIcpGroups * 64;   // rows of a block
constexpr int kIcpPoint = 0, kIcpPlane = 1;
constexpr int kIcpSumsPoint = 17, kIcpSumsPlane = 30;
constexpr int kIcpBadRow = 1;               // flag word: the search named a row outside the target for an inlier (internal)

struct IcpXform { double m[12]; };          // rows 0 .. 2 of M, row-major
// What the host reads after an evaluation.
struct IcpRecord { double sums[kIcpSumsPlane]; int flags; int pad[3]; };      // (sums[0] is the inlier count)
static_assert(sizeof(IcpRecord) == 256, "IcpRecord layout");

__device__ __forceinline__ double icp_fold_wave(double v) {
#pragma unroll
    for (int w = 32; w >= 1; w >>= 1) v = v + __shfl_xor(v, w, 64);
    return v;
}

// p[i] = T(M * src[i]): x' = ((M00*x + M01*y) + M02*z) + M03 in float64, one rounding to T. A lane per row.
template <typename T>
__global__ __launch_bounds__(256) void k_icp_transform(const T* __restrict__ src, int n, const IcpXform M, T* __restrict__ p) {
    const int i = (int)(blockIdx.x * 256u + threadIdx.x);
    if (i >= n) return;
    const size_t o = (size_t)i * 3;
    const double x = (double)src[o], y = (double)src[o + 1], z = (double)src[o + 2];
#pragma unroll
    for (int a = 0; a < 3; ++a) p[o + a] = (T)(((M.m[4 * a] * x + M.m[4 * a + 1] * y) + M.m[4 * a + 2] * z) + M.m[4 * a + 3]);
}

template <typename T>
struct IcpSumsArgs {
    const T* p; const T* d2; const long long* j;        // the transformed source, the search's squared distances and rows (n each)
    const T* target; const T* normals; long long m;     // the target's rows and (plane mode) normals
    int n; T r2;
    long long* corr;                                    // n, or null: the target row of an inlier, -1 elsewhere
    double* part; int nblocks;                          // [sum][block]
    int* flags;
};

// The first two levels of the sum tree of NS sums over n rows, for one block: the only copy of the tree's block shape. terms(i, t) fills the NS
// terms of row i < n into t, which arrives as +0.0 and stays so for a row that contributes nothing; rows past n are +0.0. part: [sum][block].
template <int NS, typename Terms>
__device__ __forceinline__ void icp_sum_block(int n, double* __restrict__ part, int nblocks, Terms terms) {
    __shared__ double lv1[NS][kIcpGroups];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (int g = 0; g < kIcpGroups / 16; ++g) {
        const int grp = g * 16 + wave;
        const long long i = (long long)blockIdx.x * kIcpRows + grp * 64 + lane;
        double t[NS];
#pragma unroll
        for (int k = 0; k < NS; ++k) t[k] = 0.0;
        if (i < n) terms(i, t);
#pragma unroll
        for (int k = 0; k < NS; ++k) {
            const double v = icp_fold_wave(t[k]);
            if (lane == 0) lv1[k][grp] = v;
        }
    }
    __syncthreads();
    // level 2 -- unless level 1 left one value (n <= 64): fold64 stops there
    const bool single = n <= 64;
    for (int k = wave; k < NS; k += kIcpBlock / 64) {
        double v = lv1[k][single ? 0 : lane];
        if (!single) v = icp_fold_wave(v);
        if (lane == 0) part[(size_t)k * nblocks + blockIdx.x] = v;
    }
}

template <typename T, int MODE>
__global__ __launch_bounds__(kIcpBlock) void k_icp_sums(const IcpSumsArgs<T> a) {
    icp_sum_block<MODE == kIcpPlane ? kIcpSumsPlane : kIcpSumsPoint>(a.n, a.part, a.nblocks, [&](long long i, double* t) {
        const T d2 = a.d2[i];
        const long long jj = a.j[i];
        bool in = d2 < a.r2;                            // strict; false for a non-finite d2
        if (in && (unsigned long long)jj >= (unsigned long long)a.m) { in = false; atomicOr(a.flags, kIcpBadRow); }
        if (a.corr) a.corr[i] = in ? jj : -1ll;
        if (in) {
            const size_t po = (size_t)i * 3, qo = (size_t)jj * 3;
            const double p0 = (double)a.p[po], p1 = (double)a.p[po + 1], p2 = (double)a.p[po + 2];
            const double q0 = (double)a.target[qo], q1 = (double)a.target[qo + 1], q2 = (double)a.target[qo + 2];
            t[0] = 1.0; t[1] = (double)d2;
            if (MODE == kIcpPoint) {
                const double pp[3] = {p0, p1, p2}, qq[3] = {q0, q1, q2};
#pragma unroll
                for (int u = 0; u < 3; ++u) { t[2 + u] = pp[u]; t[5 + u] = qq[u]; }
#pragma unroll
                for (int u = 0; u < 3; ++u)
#pragma unroll
                    for (int v = 0; v < 3; ++v) t[8 + 3 * u + v] = pp[u] * qq[v];
            } else {
                const double n0 = (double)a.normals[qo], n1 = (double)a.normals[qo + 1], n2 = (double)a.normals[qo + 2];
                const double e0 = p0 - q0, e1 = p1 - q1, e2 = p2 - q2;
                const double r = ((e0 * n0) + (e1 * n1)) + (e2 * n2);
                const double J[6] = {p1 * n2 - p2 * n1, p2 * n0 - p0 * n2, p0 * n1 - p1 * n0, n0, n1, n2};
                int k = 2;
#pragma unroll
                for (int u = 0; u < 6; ++u)
#pragma unroll
                    for (int v = u; v < 6; ++v) t[k++] = J[u] * J[v];
#pragma unroll
                for (int u = 0; u < 6; ++u) t[23 + u] = J[u] * r;
                t[29] = r * r;
            }
        }
    });
}

// One block. x holds [sum][count] values (row stride: count); they are folded by 64 into y ([sum][ceil(count / 64)]), the two change roles,
// until one value per sum is left; then the record. y has room for nsums * ceil(count / 64) values.
__global__ __launch_bounds__(kIcpBlock) void k_icp_fold(double* x, double* y, int count, int nsums, const int* flags, IcpRecord* rec) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    while (count > 1) {
        const int out = (count + 63) / 64;
        for (int w = wave; w < nsums * out; w += kIcpBlock / 64) {
            const int k = w / out, g = w - k * out, idx = g * 64 + lane;
            const double v = icp_fold_wave(idx < count ? x[(size_t)k * count + idx] : 0.0);
            if (lane == 0) y[(size_t)k * out + g] = v;
        }
        __syncthreads();
        double* z = x; x = y; y = z;
        count = out;
    }
    if ((int)threadIdx.x < nsums) rec->sums[threadIdx.x] = x[threadIdx.x];
    if (threadIdx.x == 0) rec->flags = *flags;
}

}  // namespace pcu
