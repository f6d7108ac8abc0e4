// csrc/consensus.h -- the kernels that every RANSAC operator shares (host: consensus_host.h): H hypotheses, every row
// tested against every one of them, the lowest h of the largest score wins, the inliers of the final model leave as ascending rows.
//
// An operator brings a model M (plane.h: PlaneModel<T>; ransac.h: RansacModel) with
//   Elem, Hyp, Best      the scalar of the data it reads, the record of a hypothesis, what the winner kernel leaves on the device {hyp, ..., score, h}
//   Row, kRows           what a lane keeps of a row, and how many rows a lane of the scoring kernel keeps in registers
//   Draw                 what the winner kernel is given beside the scores (a kernel argument)
//   load(data, n, i)     row i of n as float64; NaN past the end: never an inlier
//   inlier(hyp, row)     the test: strict, false for any NaN
//   won(draw, h, best)   the winner's extras, by one thread
// and its own hypotheses kernel and sums. The motion (ransac.h) also keeps a scoring kernel of its own, k_ransac_score, and says why. The
// score is an integer count: no floating-point atomic anywhere, and no result depends on how a kernel was launched.
#pragma once
#include "pcu_types.h"

namespace pcu {

constexpr int kConsensusScoreBlock = 256;               // threads of a k_consensus_score block: 4 waves, 4 * 64 * R rows
constexpr long long kConsensusLaunchTests = 1ll << 34;  // (row, hypothesis) tests of one k_consensus_score launch, about: the host polls cancellation between launches
constexpr int kConsensusScoreWaves = 8192;              // waves a launch aims for (256 CUs x 32): short clouds split the hypothesis range over blockIdx.y

// The hot path. A wave owns 64 * R consecutive rows, lane l the rows base + r * 64 + l: read once, converted to float64, kept in registers
// over the launch's hypotheses [hbeg, hend) -- of which blockIdx.y takes one slice of `slice` (a multiple of 64). A row past n is NaN: never
// an inlier. The record of a hypothesis is read at a wave-uniform address (scalar loads). The wave's count for a hypothesis is the popcount
// of a ballot; the counts of 64 consecutive hypotheses are gathered into the 64 lanes and leave as one vector atomicAdd on unsigned counters.
template <typename M>
__global__ __launch_bounds__(kConsensusScoreBlock) void k_consensus_score(const typename M::Elem* __restrict__ data, unsigned n, const typename M::Hyp* __restrict__ hyp,
                                                                          unsigned hbeg, unsigned hend, unsigned slice, unsigned* __restrict__ scores) {
    const unsigned lane = threadIdx.x & 63u;
    const unsigned long long wave = (unsigned long long)blockIdx.x * (kConsensusScoreBlock / 64) + (threadIdx.x >> 6);
    const unsigned long long base = wave * (64ull * M::kRows);
    if (base >= n) return;                          // (wave-uniform)
    typename M::Row row[M::kRows];
#pragma unroll
    for (int r = 0; r < M::kRows; ++r) row[r] = M::load(data, n, base + (unsigned)r * 64u + lane);
    const unsigned long long s0 = (unsigned long long)hbeg + (unsigned long long)blockIdx.y * slice;
    const unsigned b = (unsigned)(s0 < hend ? s0 : hend);
    const unsigned e = (unsigned)(s0 + slice < hend ? s0 + slice : hend);
    for (unsigned hb = b; hb < e; hb += 64u) {
        const unsigned m = e - hb < 64u ? e - hb : 64u;
        unsigned cnt = 0;
        for (unsigned j = 0; j < m; ++j) {
            const typename M::Hyp q = hyp[hb + j];  // (loading record j + 1 under the tests of record j changed nothing: DESIGN.md 8.14)
            unsigned c = 0;
#pragma unroll
            for (int r = 0; r < M::kRows; ++r) c += (unsigned)__popcll(__ballot(M::inlier(q, row[r])));
            cnt = lane == j ? c : cnt;              // (c and j are wave-uniform: one compare and one select beside the 32 operations of the tests)
        }
        if (lane < m && cnt) atomicAdd(&scores[hb + lane], cnt);
    }
}

// One block: the largest score, the lowest h among equal ones; the winner's record (and what M::won adds to it), for the kernels that follow.
template <typename M>
__global__ __launch_bounds__(1024) void k_consensus_best(const unsigned* __restrict__ scores, const typename M::Hyp* __restrict__ hyp, unsigned H, const typename M::Draw draw,
                                                         typename M::Best* __restrict__ out) {
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
        typename M::Best bst;
        bst.hyp = hyp[h]; bst.score = (unsigned)(key >> 32); bst.h = h;
        M::won(draw, h, bst);
        *out = bst;
    }
}

// flag[i] = 1 for an inlier of the final model: the winner on the device (refit off), or the host's.
template <typename M>
__global__ __launch_bounds__(256) void k_consensus_mark(const typename M::Elem* __restrict__ data, unsigned n, const typename M::Best* __restrict__ best, const typename M::Hyp given,
                                                        unsigned* __restrict__ flag) {
    const unsigned i = blockIdx.x * 256u + threadIdx.x;
    if (i >= n) return;
    const typename M::Hyp q = best ? best->hyp : given;
    flag[i] = M::inlier(q, M::load(data, n, i)) ? 1u : 0u;
}

// rank: the inclusive scan of flag. out has room for n rows.
__global__ __launch_bounds__(256) void k_consensus_emit(const unsigned* __restrict__ flag, const unsigned* __restrict__ rank, int n, long long* __restrict__ out) {
    const int i = (int)(blockIdx.x * 256u + threadIdx.x);
    if (i >= n) return;
    if (flag[i]) out[rank[i] - 1u] = (long long)i;
}

}  // namespace pcu
