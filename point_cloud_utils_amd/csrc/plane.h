// csrc/plane.h -- the model and the own kernels of segment_point_cloud_plane (the contract in numpy: tests/plane_contract.py;
// host: plane_host.h). The scoring, winner, mark and emit kernels are consensus.h's, instantiated for PlaneModel<T>.
//
// RANSAC over H three-point hypotheses: k_plane_hypotheses (a lane per hypothesis: the draw of poisson.h / mesh_sample.h, the plane as
// {c, k, bound}), k_consensus_score (every row against every hypothesis: the hot path), k_consensus_best (the lowest h of the largest score;
// the winner stays on the device), then either k_plane_sums + icp.h's k_icp_fold (the ten sums of the refit, in the fold64 order) and a 3x3
// solve on the host, or nothing; k_consensus_mark / the scan of voxel_host.h / k_consensus_emit write the inliers' rows in ascending order.
// Everything is float64 with one rounding per operation (the unit is built with -ffp-contract=off), without square root or division.
#pragma once
#include "pcu_types.h"
#include "poisson.h"
#include "mesh_sample.h"
#include "icp.h"
#include "consensus.h"

namespace pcu {

constexpr int kPlaneRows = 4;                       // R: rows a lane of k_consensus_score keeps in registers
constexpr int kPlaneSums = 10;                      // [count, u0, u1, u2, u0u0, u0u1, u0u2, u1u1, u1u2, u2u2]

struct PlaneHyp { double c0, c1, c2, k, bound; };   // row i is an inlier iff e*e < bound, e = ((c0*x + c1*y) + c2*z) - k
static_assert(sizeof(PlaneHyp) == 40, "PlaneHyp layout");
// What k_consensus_best leaves on the device (and the host reads with its first wait).
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

// The plane as a model of consensus.h. The winner's extra is its first drawn point o = p0, about which k_plane_sums takes its sums.
template <typename T>
struct PlaneModel {
    using Elem = T; using Hyp = PlaneHyp; using Best = PlaneBest;
    static constexpr int kRows = kPlaneRows;
    struct Row { double x, y, z; };
    struct Draw { const T* pts; unsigned n; PlaneMods md; unsigned seed; };
    static __device__ __forceinline__ Row load(const T* __restrict__ pts, unsigned n, unsigned long long i) {
        const bool live = i < n;
        const size_t o = live ? (size_t)i * 3 : 0;
        return {live ? (double)pts[o] : __builtin_nan(""), (double)pts[o + 1], (double)pts[o + 2]};
    }
    static __device__ __forceinline__ bool inlier(const PlaneHyp& q, const Row& p) { return plane_inlier(q, p.x, p.y, p.z); }
    static __device__ __forceinline__ void won(const Draw& d, unsigned h, PlaneBest& bst) {
        unsigned i0, i1, i2;
        plane_draw(d.seed, h, d.n, d.md, i0, i1, i2);
        for (int a = 0; a < 3; ++a) bst.o[a] = (double)d.pts[(size_t)i0 * 3 + a];
    }
};

// The ten sums of the winner's inliers about o, in the fold64 order: icp.h's sum block over the terms of a row; the further levels are
// k_icp_fold's. part: [sum][block].
template <typename T>
__global__ __launch_bounds__(kIcpBlock) void k_plane_sums(const T* __restrict__ pts, int n, const PlaneBest* __restrict__ best, double* __restrict__ part, int nblocks) {
    const PlaneHyp q = best->hyp;
    const double o0 = best->o[0], o1 = best->o[1], o2 = best->o[2];
    icp_sum_block<kPlaneSums>(n, part, nblocks, [&](long long i, double* t) {
        const size_t po = (size_t)i * 3;
        const double x = (double)pts[po], y = (double)pts[po + 1], z = (double)pts[po + 2];
        if (plane_inlier(q, x, y, z)) {
            const double u0 = x - o0, u1 = y - o1, u2 = z - o2;
            t[0] = 1.0; t[1] = u0; t[2] = u1; t[3] = u2;
            t[4] = u0 * u0; t[5] = u0 * u1; t[6] = u0 * u2; t[7] = u1 * u1; t[8] = u1 * u2; t[9] = u2 * u2;
        }
    });
}

}  // namespace pcu
