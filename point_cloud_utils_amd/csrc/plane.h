// csrc/plane.h -- the kernels of segment_point_cloud_plane (the contract in numpy: tests/plane_contract.py; host: plane_host.h).
//
// RANSAC over H three-point hypotheses: k_plane_hypotheses (a lane per hypothesis: the draw of poisson.h / mesh_sample.h, the plane as
// {c, k, bound}), k_plane_score (every row against every hypothesis: the hot path), k_plane_best (the lowest h of the largest score; the
// winner stays on the device), then either k_plane_sums + icp.h's k_icp_fold (the ten sums of the refit, in the fold64 order) and a 3x3 solve
// on the host, or nothing; k_plane_mark / the scan of voxel_host.h / k_plane_emit write the inliers' rows in ascending order.
// Everything is float64 with one rounding per operation (the unit is built with -ffp-contract=off), without square root or division. The
// score is an integer count: no floating-point atomic anywhere, and no result depends on how a kernel was launched.
#pragma once
#include "pcu_types.h"
#include "poisson.h"
#include "mesh_sample.h"
#include "icp.h"

namespace pcu {

constexpr int kPlaneRows = 4;                       // R: rows a lane of k_plane_score keeps in registers
constexpr int kPlaneScoreBlock = 256;               // threads of a k_plane_score block: 4 waves, 4 * 64 * R rows
constexpr long long kPlaneLaunchTests = 1ll << 34;  // (row, hypothesis) tests of one k_plane_score launch, about: the host polls cancellation between launches
constexpr int kPlaneScoreWaves = 8192;              // waves a launch aims for (256 CUs x 32): short clouds split the hypothesis range over blockIdx.y
constexpr int kPlaneSums = 10;                      // [count, u0, u1, u2, u0u0, u0u1, u0u2, u1u1, u1u2, u2u2]

struct PlaneHyp { double c0, c1, c2, k, bound; };   // row i is an inlier iff e*e < bound, e = ((c0*x + c1*y) + c2*z) - k
static_assert(sizeof(PlaneHyp) == 40, "PlaneHyp layout");
// What k_plane_best leaves on the device (and the host reads with its first wait).
struct PlaneBest { PlaneHyp hyp; double o[3]; unsigned score, h; };
static_assert(sizeof(PlaneBest) == 72, "PlaneBest layout");

// h mod d in integers alone (the compiler's 64-bit remainder goes through floating point): m = floor((2^64 - 1) / d) from the host; the
// quotient estimate umulhi(h, m) is short by two at the most.
struct PlaneMods { unsigned long long m[3]; };      // of n, n - 1, n - 2 (plane_host.h: plane_mods)
__device__ __forceinline__ unsigned plane_mod(unsigned long long h, unsigned d, unsigned long long m) {
    unsigned long long r = h - __umul64hi(h, m) * d;
    while (r >= d) r -= d;
    return (unsigned)r;
}
// The three distinct rows of hypothesis h (tests/plane_contract.py: triples).
__device__ __forceinline__ void plane_draw(unsigned seed, unsigned h, unsigned n, const PlaneMods& md, unsigned& i0, unsigned& i1, unsigned& i2) {
    const MsDraw d = ms_draw(seed, (unsigned long long)h);
    i0 = plane_mod(d.h0, n, md.m[0]);
    i1 = plane_mod(d.h1, n - 1u, md.m[1]); i1 += i1 >= i0 ? 1u : 0u;
    const unsigned lo = i0 < i1 ? i0 : i1, hi = i0 < i1 ? i1 : i0;
    i2 = plane_mod(d.h2, n - 2u, md.m[2]); i2 += i2 >= lo ? 1u : 0u; i2 += i2 >= hi ? 1u : 0u;
}

__device__ __forceinline__ bool plane_inlier(const PlaneHyp& q, double x, double y, double z) {
    const double e = ((q.c0 * x + q.c1 * y) + q.c2 * z) - q.k;
    return e * e < q.bound;                         // strict; false for any NaN
}

// A lane per hypothesis. n >= 3.
template <typename T>
__global__ __launch_bounds__(256) void k_plane_hypotheses(const T* __restrict__ pts, unsigned n, const PlaneMods md, unsigned seed, unsigned H, double t2, PlaneHyp* __restrict__ out) {
    const unsigned h = blockIdx.x * 256u + threadIdx.x;
    if (h >= H) return;
    unsigned i0, i1, i2;
    plane_draw(seed, h, n, md, i0, i1, i2);
    const size_t o0 = (size_t)i0 * 3, o1 = (size_t)i1 * 3, o2 = (size_t)i2 * 3;
    const double p0x = (double)pts[o0], p0y = (double)pts[o0 + 1], p0z = (double)pts[o0 + 2];
    const double a0 = (double)pts[o1] - p0x, a1 = (double)pts[o1 + 1] - p0y, a2 = (double)pts[o1 + 2] - p0z;
    const double b0 = (double)pts[o2] - p0x, b1 = (double)pts[o2 + 1] - p0y, b2 = (double)pts[o2 + 2] - p0z;
    PlaneHyp q;
    q.c0 = a1 * b2 - a2 * b1; q.c1 = a2 * b0 - a0 * b2; q.c2 = a0 * b1 - a1 * b0;
    const double l2 = (q.c0 * q.c0 + q.c1 * q.c1) + q.c2 * q.c2;
    q.k = (q.c0 * p0x + q.c1 * p0y) + q.c2 * p0z;
    q.bound = (l2 > 0.0 && l2 < __builtin_inf()) ? t2 * l2 : 0.0;
    out[h] = q;
}

// The hot path. A wave owns 64 * R consecutive rows, lane l the rows base + r * 64 + l: read once, converted to float64, kept in registers
// over the launch's hypotheses [hbeg, hend) -- of which blockIdx.y takes one slice of `slice` (a multiple of 64). A row past n is NaN: never
// an inlier. The record of a hypothesis is read at a wave-uniform address (scalar loads). The wave's count for a hypothesis is the popcount
// of a ballot; the counts of 64 consecutive hypotheses are gathered into the 64 lanes and leave as one vector atomicAdd on unsigned counters.
template <typename T>
__global__ __launch_bounds__(kPlaneScoreBlock) void k_plane_score(const T* __restrict__ pts, unsigned n, const PlaneHyp* __restrict__ hyp, unsigned hbeg, unsigned hend,
                                                                  unsigned slice, unsigned* __restrict__ scores) {
    const unsigned lane = threadIdx.x & 63u;
    const unsigned long long wave = (unsigned long long)blockIdx.x * (kPlaneScoreBlock / 64) + (threadIdx.x >> 6);
    const unsigned long long base = wave * (64ull * kPlaneRows);
    if (base >= n) return;                          // (wave-uniform)
    double x[kPlaneRows], y[kPlaneRows], z[kPlaneRows];
#pragma unroll
    for (int r = 0; r < kPlaneRows; ++r) {
        const unsigned long long i = base + (unsigned)r * 64u + lane;
        const bool live = i < n;
        const size_t o = live ? (size_t)i * 3 : 0;
        x[r] = live ? (double)pts[o] : __builtin_nan("");
        y[r] = (double)pts[o + 1];
        z[r] = (double)pts[o + 2];
    }
    const unsigned long long s0 = (unsigned long long)hbeg + (unsigned long long)blockIdx.y * slice;
    const unsigned b = (unsigned)(s0 < hend ? s0 : hend);
    const unsigned e = (unsigned)(s0 + slice < hend ? s0 + slice : hend);
    for (unsigned hb = b; hb < e; hb += 64u) {
        const unsigned m = e - hb < 64u ? e - hb : 64u;
        unsigned cnt = 0;
        for (unsigned j = 0; j < m; ++j) {
            const PlaneHyp q = hyp[hb + j];         // (loading record j + 1 under the tests of record j changed nothing: DESIGN.md 8.14)
            unsigned c = 0;
#pragma unroll
            for (int r = 0; r < kPlaneRows; ++r) c += (unsigned)__popcll(__ballot(plane_inlier(q, x[r], y[r], z[r])));
            cnt = lane == j ? c : cnt;              // (c and j are wave-uniform: one compare and one select beside the 32 operations of the tests)
        }
        if (lane < m && cnt) atomicAdd(&scores[hb + lane], cnt);
    }
}

// One block: the largest score, the lowest h among equal ones; the winner's record and its first point o = p0, for the kernels that follow.
template <typename T>
__global__ __launch_bounds__(1024) void k_plane_best(const unsigned* __restrict__ scores, const PlaneHyp* __restrict__ hyp, unsigned H, const T* __restrict__ pts, unsigned n,
                                                     const PlaneMods md, unsigned seed, PlaneBest* __restrict__ out) {
    __shared__ unsigned long long top[16];
    unsigned long long key = 0;                     // (score, ~h): the maximum is the largest score at the lowest h
    for (unsigned h = threadIdx.x; h < H; h += 1024u) {
        const unsigned long long k = ((unsigned long long)scores[h] << 32) | (0xffffffffu - h);
        key = k > key ? k : key;
    }
#pragma unroll
    for (int w = 32; w >= 1; w >>= 1) { const unsigned long long o = __shfl_xor(key, w, 64); key = o > key ? o : key; }
    if ((threadIdx.x & 63) == 0) top[threadIdx.x >> 6] = key;
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int w = 1; w < 16; ++w) key = top[w] > key ? top[w] : key;
        const unsigned h = 0xffffffffu - (unsigned)(key & 0xffffffffull);
        unsigned i0, i1, i2;
        plane_draw(seed, h, n, md, i0, i1, i2);
        PlaneBest bst;
        bst.hyp = hyp[h]; bst.score = (unsigned)(key >> 32); bst.h = h;
        for (int a = 0; a < 3; ++a) bst.o[a] = (double)pts[(size_t)i0 * 3 + a];
        *out = bst;
    }
}

// The ten sums of the winner's inliers about o, in the fold64 order: the block shape and the two levels of k_icp_sums (icp.h); the further
// levels are k_icp_fold's. part: [sum][block].
template <typename T>
__global__ __launch_bounds__(kIcpBlock) void k_plane_sums(const T* __restrict__ pts, int n, const PlaneBest* __restrict__ best, double* __restrict__ part, int nblocks) {
    __shared__ double lv1[kPlaneSums][kIcpGroups];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const PlaneHyp q = best->hyp;
    const double o0 = best->o[0], o1 = best->o[1], o2 = best->o[2];
    for (int g = 0; g < kIcpGroups / 16; ++g) {
        const int grp = g * 16 + wave;
        const long long i = (long long)blockIdx.x * kIcpRows + grp * 64 + lane;
        double t[kPlaneSums];
#pragma unroll
        for (int k = 0; k < kPlaneSums; ++k) t[k] = 0.0;
        if (i < n) {
            const size_t po = (size_t)i * 3;
            const double x = (double)pts[po], y = (double)pts[po + 1], z = (double)pts[po + 2];
            if (plane_inlier(q, x, y, z)) {
                const double u0 = x - o0, u1 = y - o1, u2 = z - o2;
                t[0] = 1.0; t[1] = u0; t[2] = u1; t[3] = u2;
                t[4] = u0 * u0; t[5] = u0 * u1; t[6] = u0 * u2; t[7] = u1 * u1; t[8] = u1 * u2; t[9] = u2 * u2;
            }
        }
#pragma unroll
        for (int k = 0; k < kPlaneSums; ++k) {
            const double v = icp_fold_wave(t[k]);
            if (lane == 0) lv1[k][grp] = v;
        }
    }
    __syncthreads();
    const bool single = n <= 64;                    // level 1 left one value: fold64 stops there
    for (int k = wave; k < kPlaneSums; k += kIcpBlock / 64) {
        double v = lv1[k][single ? 0 : lane];
        if (!single) v = icp_fold_wave(v);
        if (lane == 0) part[(size_t)k * nblocks + blockIdx.x] = v;
    }
}

// flag[i] = 1 for an inlier of the final plane: the winner on the device (refit off), or the host's refitted one.
template <typename T>
__global__ __launch_bounds__(256) void k_plane_mark(const T* __restrict__ pts, int n, const PlaneBest* __restrict__ best, const PlaneHyp given, unsigned* __restrict__ flag) {
    const int i = (int)(blockIdx.x * 256u + threadIdx.x);
    if (i >= n) return;
    const PlaneHyp q = best ? best->hyp : given;
    const size_t o = (size_t)i * 3;
    flag[i] = plane_inlier(q, (double)pts[o], (double)pts[o + 1], (double)pts[o + 2]) ? 1u : 0u;
}

// rank: the inclusive scan of flag. out has room for n rows.
__global__ __launch_bounds__(256) void k_plane_emit(const unsigned* __restrict__ flag, const unsigned* __restrict__ rank, int n, long long* __restrict__ out) {
    const int i = (int)(blockIdx.x * 256u + threadIdx.x);
    if (i >= n) return;
    if (flag[i]) out[rank[i] - 1u] = (long long)i;
}

}  // namespace pcu
