// csrc/ransac.h -- the model and the own kernels of register_point_clouds_ransac (the contract in numpy:
// tests/ransac_contract.py; host: ransac_host.h). The winner, mark and emit kernels are consensus.h's, instantiated for RansacModel; the scoring kernel is its own.
//
// RANSAC over H three-correspondence hypotheses: k_ransac_gather (a lane per correspondence: both indices checked, the six coordinates as
// float64 into six planes of c values), k_ransac_hypotheses (a lane per hypothesis: the draw of plane.h over the c correspondences, the edge
// pre-check, the two frames, the rigid motion as {R, tr, bound}), k_ransac_score (every correspondence against every hypothesis: the hot
// path), k_consensus_best (the lowest h of the largest score; the winner stays on the device), k_ransac_sums + icp.h's k_icp_fold (the 17
// sums of Horn's solve, or [count, d2] alone, in the fold64 order), k_consensus_mark / the scan of voxel_host.h / k_consensus_emit for the
// inliers' rows in ascending order.
// Everything is float64 with one rounding per operation (the unit is built with -ffp-contract=off). Division and square root appear in
// k_ransac_hypotheses alone and are the IEEE ones.
#pragma once
#include "pcu_types.h"
#include "plane.h"
#include "icp.h"
#include "consensus.h"

namespace pcu {

#ifndef PCU_RANSAC_ROWS
#define PCU_RANSAC_ROWS 4                           // (2 and 8 measured: DESIGN.md 8.17)
#endif
constexpr int kRansacRows = PCU_RANSAC_ROWS;        // R: correspondences a lane of k_ransac_score keeps in registers (six doubles each)
constexpr int kRansacBadSource = 1, kRansacBadTarget = 2;      // flag word: column 0 / column 1 of correspondences names a row that is not there

struct RansacHyp { double R[9], tr[3], bound; };    // correspondence i is an inlier iff |R s + tr - t|^2 < bound
static_assert(sizeof(RansacHyp) == 104, "RansacHyp layout");
// What k_consensus_best leaves on the device (and the host reads with its first wait).
struct RansacBest { RansacHyp hyp; unsigned score, h; };
static_assert(sizeof(RansacBest) == 112, "RansacBest layout");

// The squared distance of the moved source point to its partner: x'_a = ((R[a][0]*x + R[a][1]*y) + R[a][2]*z) + tr[a] (register_point_clouds_icp's
// form, not rounded to T), d = x' - q, d2 = (d0*d0 + d1*d1) + d2*d2: 26 operations.
__device__ __forceinline__ double ransac_d2(const RansacHyp& q, double x, double y, double z, double qx, double qy, double qz) {
    const double d0 = (((q.R[0] * x + q.R[1] * y) + q.R[2] * z) + q.tr[0]) - qx;
    const double d1 = (((q.R[3] * x + q.R[4] * y) + q.R[5] * z) + q.tr[1]) - qy;
    const double d2 = (((q.R[6] * x + q.R[7] * y) + q.R[8] * z) + q.tr[2]) - qz;
    return (d0 * d0 + d1 * d1) + d2 * d2;
}
// (strict; false for any NaN)
__device__ __forceinline__ bool ransac_inlier(const RansacHyp& q, double x, double y, double z, double qx, double qy, double qz) {
    return ransac_d2(q, x, y, z, qx, qy, qz) < q.bound;
}

// A lane per correspondence. pk: six planes of c doubles [sx | sy | sz | tx | ty | tz]. An index outside its cloud raises its bit of the flag
// word and leaves NaN coordinates (never an inlier, never a usable frame): nothing is read through it.
template <typename T>
__global__ __launch_bounds__(256) void k_ransac_gather(const T* __restrict__ src, long long n, const T* __restrict__ tgt, long long m, const long long* __restrict__ corr,
                                                       unsigned c, double* __restrict__ pk, int* __restrict__ flags) {
    const unsigned i = blockIdx.x * 256u + threadIdx.x;
    if (i >= c) return;
    const long long a = corr[2 * (size_t)i], b = corr[2 * (size_t)i + 1];
    const bool oka = (unsigned long long)a < (unsigned long long)n, okb = (unsigned long long)b < (unsigned long long)m;
    if (!oka || !okb) atomicOr(flags, (oka ? 0 : kRansacBadSource) | (okb ? 0 : kRansacBadTarget));
    const size_t so = oka ? (size_t)a * 3 : 0, to = okb ? (size_t)b * 3 : 0;
#pragma unroll
    for (int u = 0; u < 3; ++u) {
        pk[(size_t)u * c + i] = oka ? (double)src[so + u] : __builtin_nan("");
        pk[(size_t)(3 + u) * c + i] = okb ? (double)tgt[to + u] : __builtin_nan("");
    }
}

struct RansacVec { double x, y, z; };
__device__ __forceinline__ RansacVec ransac_sub(const RansacVec& a, const RansacVec& b) { return {a.x - b.x, a.y - b.y, a.z - b.z}; }
__device__ __forceinline__ double ransac_len2(const RansacVec& a) { return (a.x * a.x + a.y * a.y) + a.z * a.z; }
__device__ __forceinline__ RansacVec ransac_cross(const RansacVec& a, const RansacVec& b) {
    return {a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x};
}
__device__ __forceinline__ RansacVec ransac_load(const double* __restrict__ pk, unsigned c, unsigned i, int plane) {
    return {pk[(size_t)plane * c + i], pk[(size_t)(plane + 1) * c + i], pk[(size_t)(plane + 2) * c + i]};
}
// The frame of a triple: e1 along p1 - p0, e3 along (p1 - p0) x (p2 - p0), e2 = e3 x e1; usable iff both lengths are finite and > 0.
__device__ __forceinline__ bool ransac_frame(const RansacVec& p0, const RansacVec& p1, const RansacVec& p2, RansacVec& e1, RansacVec& e2, RansacVec& e3) {
    const RansacVec a = ransac_sub(p1, p0), b = ransac_sub(p2, p0), nn = ransac_cross(a, b);
    const double la = sqrt(ransac_len2(a)), ln = sqrt(ransac_len2(nn));
    e1 = {a.x / la, a.y / la, a.z / la};
    e3 = {nn.x / ln, nn.y / ln, nn.z / ln};
    e2 = ransac_cross(e3, e1);
    return la > 0.0 && la < __builtin_inf() && ln > 0.0 && ln < __builtin_inf();
}

// A lane per hypothesis. c >= 3. r2 = edge_length_ratio^2, t2 = max_correspondence_distance^2.
__global__ __launch_bounds__(256) void k_ransac_hypotheses(const double* __restrict__ pk, unsigned c, const PlaneMods md, unsigned seed, unsigned H, double r2, double t2,
                                                           RansacHyp* __restrict__ out) {
    const unsigned h = blockIdx.x * 256u + threadIdx.x;
    if (h >= H) return;
    unsigned j0, j1, j2;
    plane_draw(seed, h, c, md, j0, j1, j2);
    const RansacVec s0 = ransac_load(pk, c, j0, 0), s1 = ransac_load(pk, c, j1, 0), s2 = ransac_load(pk, c, j2, 0);
    const RansacVec t0 = ransac_load(pk, c, j0, 3), t1 = ransac_load(pk, c, j1, 3), t2v = ransac_load(pk, c, j2, 3);
    // the pre-check: the three edges of the two triangles are of like length (no square root; any NaN fails)
    const double ls01 = ransac_len2(ransac_sub(s0, s1)), ls02 = ransac_len2(ransac_sub(s0, s2)), ls12 = ransac_len2(ransac_sub(s1, s2));
    const double lt01 = ransac_len2(ransac_sub(t0, t1)), lt02 = ransac_len2(ransac_sub(t0, t2v)), lt12 = ransac_len2(ransac_sub(t1, t2v));
    bool ok = ls01 >= r2 * lt01 && lt01 >= r2 * ls01 && ls02 >= r2 * lt02 && lt02 >= r2 * ls02 && ls12 >= r2 * lt12 && lt12 >= r2 * ls12;
    RansacVec e1s, e2s, e3s, e1t, e2t, e3t;
    ok = ransac_frame(s0, s1, s2, e1s, e2s, e3s) && ok;
    ok = ransac_frame(t0, t1, t2v, e1t, e2t, e3t) && ok;
    const double a1[3] = {e1s.x, e1s.y, e1s.z}, a2[3] = {e2s.x, e2s.y, e2s.z}, a3[3] = {e3s.x, e3s.y, e3s.z};
    const double b1[3] = {e1t.x, e1t.y, e1t.z}, b2[3] = {e2t.x, e2t.y, e2t.z}, b3[3] = {e3t.x, e3t.y, e3t.z};
    const double msx = ((s0.x + s1.x) + s2.x) / 3.0, msy = ((s0.y + s1.y) + s2.y) / 3.0, msz = ((s0.z + s1.z) + s2.z) / 3.0;
    const double mt[3] = {((t0.x + t1.x) + t2v.x) / 3.0, ((t0.y + t1.y) + t2v.y) / 3.0, ((t0.z + t1.z) + t2v.z) / 3.0};
    RansacHyp q;
#pragma unroll
    for (int i = 0; i < 3; ++i) {
#pragma unroll
        for (int j = 0; j < 3; ++j) q.R[3 * i + j] = (b1[i] * a1[j] + b2[i] * a2[j]) + b3[i] * a3[j];
        q.tr[i] = mt[i] - ((q.R[3 * i] * msx + q.R[3 * i + 1] * msy) + q.R[3 * i + 2] * msz);
    }
    q.bound = ok ? t2 : 0.0;
    out[h] = q;
}

// The motion as a model of consensus.h: a row is a correspondence, read from the six planes.
struct RansacModel {
    using Elem = double; using Hyp = RansacHyp; using Best = RansacBest;
    static constexpr int kRows = kRansacRows;
    struct Row { double sx, sy, sz, tx, ty, tz; };
    struct Draw {};
    static __device__ __forceinline__ Row load(const double* __restrict__ pk, unsigned c, unsigned long long i) {
        const bool live = i < c;
        const size_t o = live ? (size_t)i : 0;
        return {live ? pk[o] : __builtin_nan(""), pk[(size_t)c + o], pk[2 * (size_t)c + o], pk[3 * (size_t)c + o], pk[4 * (size_t)c + o], pk[5 * (size_t)c + o]};
    }
    static __device__ __forceinline__ bool inlier(const RansacHyp& q, const Row& p) { return ransac_inlier(q, p.sx, p.sy, p.sz, p.tx, p.ty, p.tz); }
    static __device__ __forceinline__ void won(const Draw&, unsigned, RansacBest&) {}
};

// The hot path: consensus.h's k_consensus_score with the motion's rows and test written out. It is kept as a kernel of its own because
// k_consensus_score<RansacModel> measured 0.6 to 1.6 % slower on every figure of profiles/ransac_record.py when the two ran alternately
// (profiles/consensus_frame_refactor.txt, part 5): the same opcodes, but the compiler orders the operands of twelve additions of the hypothesis
// loop differently and places the loop 12 bytes earlier -- which does not explain it: the cause is not found (look at the loop's alignment
// first). A change to the loop of k_consensus_score is to be made here too.
__global__ __launch_bounds__(kConsensusScoreBlock) void k_ransac_score(const double* __restrict__ pk, unsigned c, const RansacHyp* __restrict__ hyp, unsigned hbeg, unsigned hend,
                                                                    unsigned slice, unsigned* __restrict__ scores) {
    const unsigned lane = threadIdx.x & 63u;
    const unsigned long long wave = (unsigned long long)blockIdx.x * (kConsensusScoreBlock / 64) + (threadIdx.x >> 6);
    const unsigned long long base = wave * (64ull * kRansacRows);
    if (base >= c) return;                          // (wave-uniform)
    double sx[kRansacRows], sy[kRansacRows], sz[kRansacRows], tx[kRansacRows], ty[kRansacRows], tz[kRansacRows];
#pragma unroll
    for (int r = 0; r < kRansacRows; ++r) {
        const unsigned long long i = base + (unsigned)r * 64u + lane;
        const bool live = i < c;
        const size_t o = live ? (size_t)i : 0;
        sx[r] = live ? pk[o] : __builtin_nan("");
        sy[r] = pk[(size_t)c + o]; sz[r] = pk[2 * (size_t)c + o];
        tx[r] = pk[3 * (size_t)c + o]; ty[r] = pk[4 * (size_t)c + o]; tz[r] = pk[5 * (size_t)c + o];
    }
    const unsigned long long s0 = (unsigned long long)hbeg + (unsigned long long)blockIdx.y * slice;
    const unsigned b = (unsigned)(s0 < hend ? s0 : hend);
    const unsigned e = (unsigned)(s0 + slice < hend ? s0 + slice : hend);
    for (unsigned hb = b; hb < e; hb += 64u) {
        const unsigned m = e - hb < 64u ? e - hb : 64u;
        unsigned cnt = 0;
        for (unsigned j = 0; j < m; ++j) {
            const RansacHyp q = hyp[hb + j];
            unsigned k = 0;
#pragma unroll
            for (int r = 0; r < kRansacRows; ++r) k += (unsigned)__popcll(__ballot(ransac_inlier(q, sx[r], sy[r], sz[r], tx[r], ty[r], tz[r])));
            cnt = lane == j ? k : cnt;              // (k and j are wave-uniform)
        }
        if (lane < m && cnt) atomicAdd(&scores[hb + lane], cnt);
    }
}

// The sums of the inliers of a motion -- the winner on the device (best), or the host's (given) --, in the fold64 order: icp.h's sum block over
// the terms of a correspondence; the further levels are k_icp_fold's. NS = 17: [count, d2, p(3), q(3), p_u*q_v (9)] with p the source point as
// it is and q its partner (the point mode of icp.h); NS = 2: [count, d2]. A non-inlier contributes +0.0. part: [sum][block].
template <int NS>
__global__ __launch_bounds__(kIcpBlock) void k_ransac_sums(const double* __restrict__ pk, int c, const RansacBest* __restrict__ best, const RansacHyp given,
                                                           double* __restrict__ part, int nblocks) {
    const RansacHyp q = best ? best->hyp : given;
    icp_sum_block<NS>(c, part, nblocks, [&](long long i, double* t) {
        const size_t o = (size_t)i, C = (size_t)c;
        const double pp[3] = {pk[o], pk[C + o], pk[2 * C + o]}, qq[3] = {pk[3 * C + o], pk[4 * C + o], pk[5 * C + o]};
        const double d2 = ransac_d2(q, pp[0], pp[1], pp[2], qq[0], qq[1], qq[2]);
        if (d2 < q.bound) {
            t[0] = 1.0; t[1] = d2;
            if constexpr (NS == kIcpSumsPoint) {
#pragma unroll
                for (int u = 0; u < 3; ++u) { t[2 + u] = pp[u]; t[5 + u] = qq[u]; }
#pragma unroll
                for (int u = 0; u < 3; ++u)
#pragma unroll
                    for (int v = 0; v < 3; ++v) t[8 + 3 * u + v] = pp[u] * qq[v];
            }
        }
    });
}

}  // namespace pcu
