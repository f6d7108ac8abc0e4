// csrc/feature_match.h -- match_point_features: the nearest dataset row of every query row in a feature space of 1 .. 128 dimensions (DESIGN.md
// row f24). Host side: feature_match_host.h.
//
// The contract (in numpy: tests/feature_match_contract.py), T the input type: d2(i, j) = the sum over c = 0 .. D - 1, left to right, of
// (a_ic - b_jc) * (a_ic - b_jc) in T, separate multiplies and adds (the TU is built with -ffp-contract=off; the form |a|^2 + |b|^2 - 2 a.b
// cancels and cannot give these bytes). nearest[i] is the j of the smallest (d2, j); a pair whose d2 is NaN is no candidate (+inf is one);
// a row without a candidate gets -1 and +inf. (a - b) * (a - b) == (b - a) * (b - a) exactly, so the search from the dataset to the queries
// sees the same d2: is_mutual[i] = nearest[i] >= 0 and the nearest query of dataset row nearest[i], by the same rule, is i.
//
// k_feature_match: a dense search on the vector ALU -- the 3-D grid is no help here. A block holds kFmQueries = 64 queries, a lane each, in
// every one of its four waves; the dataset passes through LDS in tiles of kFmTile rows that the four waves share out in groups of kFmRows
// rows, which a lane accumulates side by side (one LDS read, a broadcast, serves 64 queries; kFmRows independent sums hide the add latency).
// DF = 33 (the FPFH width): the query row in registers and the loops unrolled; DF = 0: any D, the query rows in LDS, transposed so that the
// 64 lanes read 64 consecutive words. The running minimum is (d2, j) under the full order, so which wave met a row first does not matter;
// the four waves fold through LDS, the blocks of a split dataset (gridDim.y) through k_feature_match_fold. The cancel word is looked at once
// per tile by one lane, read at most once per 200 us.
#pragma once
#include "pcu_types.h"
#include "grid.h"

namespace pcu {

constexpr int kFmQueries = 64;           // queries per block
constexpr int kFmTile = 32;              // dataset rows per LDS tile
constexpr int kFmRows = 4;               // dataset rows a lane accumulates side by side (float; float64 takes half: fm_rows)
constexpr int kFmMaxD = 128;
constexpr int kFmNone = 0x7fffffff;      // "no candidate yet": above every row

template <typename T>
struct FmArgs {
    const T* q; const T* d; int n, m, D;                                // n queries, m dataset rows, D values each
    int split_rows;                                                     // dataset rows per block along gridDim.y, a multiple of kFmTile
    T* part_d; int* part_j;                                             // (gridDim.y, n): the minimum of every split
    const unsigned* cancel_word; unsigned cancel_gen;
};

template <typename T> constexpr int fm_rows() { return sizeof(T) == 4 ? kFmRows : kFmRows / 2; }      // (four float64 rows beside a 33-value query row spill)
constexpr int fm_padded(int D) { return (D + 3) & ~3; }                 // a tile row starts on 16 bytes
template <typename T>
constexpr size_t fm_lds_bytes(int D, bool query_in_lds) {
    return ((size_t)kFmTile * fm_padded(D) + (query_in_lds ? (size_t)D * kFmQueries : 0) + (kBlock / 64) * kFmQueries) * sizeof(T) + (kBlock / 64) * kFmQueries * 4 + 16;
}

template <typename T, int DF>
__global__ __launch_bounds__(kBlock) void k_feature_match(const FmArgs<T> a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char s_fm[];
    const int D = DF ? DF : a.D, DP = fm_padded(D);
    T* const s_tile = reinterpret_cast<T*>(s_fm);                       // kFmTile x DP
    T* const s_q = s_tile + kFmTile * DP;                               // DF == 0: D x 64
    T* const s_bd = s_q + (DF ? 0 : D * kFmQueries);                    // 4 x 64
    int* const s_bj = reinterpret_cast<int*>(s_bd + (kBlock / 64) * kFmQueries);
    int* const s_stop = s_bj + (kBlock / 64) * kFmQueries;
    constexpr int kRows = fm_rows<T>();
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int qi = blockIdx.x * kFmQueries + lane;
    const T* const qrow = a.q + (size_t)min(qi, a.n - 1) * D;
    T qr[DF ? DF : 1];
    if (DF) {
#pragma unroll
        for (int c = 0; c < (DF ? DF : 1); ++c) qr[c] = qrow[c];
    } else {
        for (int c = wv; c < D; c += kBlock / 64) s_q[c * kFmQueries + lane] = qrow[c];
    }
    if (threadIdx.x == 0) *s_stop = 0;
    const int r_begin = blockIdx.y * a.split_rows, r_end = min(a.m, r_begin + a.split_rows);
    T bd = (T)INFINITY; int bj = kFmNone;
    long long t_poll = wall_clock64();
    for (int r0 = r_begin; r0 < r_end; r0 += kFmTile) {
        const int rows = min(kFmTile, r_end - r0);
        __syncthreads();                                                // (the tile before this one has been read)
        const T* const src = a.d + (size_t)r0 * D;
        for (int e = threadIdx.x; e < rows * D; e += kBlock) { const int rr = e / D; s_tile[rr * DP + (e - rr * D)] = src[e]; }
        if (threadIdx.x == 0) { const long long t_now = wall_clock64(); if (t_now - t_poll > 20000ll) { t_poll = t_now; if (cancel_seen(a.cancel_word, a.cancel_gen)) *s_stop = 1; } }
        __syncthreads();
        if (*s_stop) break;                                             // (the whole block)
        for (int g = wv * kRows; g < rows; g += (kBlock / 64) * kRows) {
            // (a group that reaches past `rows` reads rows of an earlier tile, or unwritten ones, inside the tile's room; their sums are dropped)
            T acc[kRows];
#pragma unroll
            for (int r = 0; r < kRows; ++r) acc[r] = (T)0;
            const T* const tr = s_tile + g * DP;
            if (DF) {
#pragma unroll
                for (int c = 0; c < (DF ? DF : 1); ++c) {
#pragma unroll
                    for (int r = 0; r < kRows; ++r) { const T df = qr[c] - tr[r * DP + c]; acc[r] = acc[r] + df * df; }
                }
            } else {
                for (int c = 0; c < D; ++c) {
                    const T qc = s_q[c * kFmQueries + lane];
#pragma unroll
                    for (int r = 0; r < kRows; ++r) { const T df = qc - tr[r * DP + c]; acc[r] = acc[r] + df * df; }
                }
            }
#pragma unroll
            for (int r = 0; r < kRows; ++r) {
                const int j = r0 + g + r;
                if (g + r < rows && (acc[r] < bd || (acc[r] == bd && j < bj))) { bd = acc[r]; bj = j; }      // (a NaN is neither)
            }
        }
    }
    s_bd[wv * kFmQueries + lane] = bd; s_bj[wv * kFmQueries + lane] = bj;
    __syncthreads();
    if (wv == 0 && qi < a.n) {
        for (int w = 1; w < kBlock / 64; ++w) {
            const T od = s_bd[w * kFmQueries + lane]; const int oj = s_bj[w * kFmQueries + lane];
            if (od < bd || (od == bd && oj < bj)) { bd = od; bj = oj; }
        }
        a.part_d[(size_t)blockIdx.y * a.n + qi] = bd; a.part_j[(size_t)blockIdx.y * a.n + qi] = bj;
    }
}

// the minimum over the splits; a row without a candidate leaves as (-1, +inf)
template <typename T>
__global__ __launch_bounds__(kBlock) void k_feature_match_fold(const T* __restrict__ part_d, const int* __restrict__ part_j, int splits, int n, long long* __restrict__ out_j,
                                                               T* __restrict__ out_d) {
    const int i = blockIdx.x * kBlock + threadIdx.x;
    if (i >= n) return;
    T bd = part_d[i]; int bj = part_j[i];
    for (int s = 1; s < splits; ++s) {
        const T od = part_d[(size_t)s * n + i]; const int oj = part_j[(size_t)s * n + i];
        if (od < bd || (od == bd && oj < bj)) { bd = od; bj = oj; }
    }
    out_j[i] = bj == kFmNone ? -1ll : (long long)bj;
    out_d[i] = bd;
}

__global__ __launch_bounds__(kBlock) void k_feature_match_mutual(const long long* __restrict__ nearest, const long long* __restrict__ back, int n, unsigned char* __restrict__ out) {
    const int i = blockIdx.x * kBlock + threadIdx.x;
    if (i >= n) return;
    const long long j = nearest[i];
    out[i] = (j >= 0 && back[j] == (long long)i) ? 1 : 0;
}

}  // namespace pcu
