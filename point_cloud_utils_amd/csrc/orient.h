// csrc/orient.h -- the kernels of orient_point_cloud_normals (the contract in numpy: tests/orient_contract.py; host: orient_host.h).
//
// The normals' signs are propagated along the minimum spanning forest of the cloud's k-NN graph, an edge {lo, hi} weighing w = 1 - |d| with
// d = (n_lo0*n_hi0 + n_lo1*n_hi1) + n_lo2*n_hi2 in float64, one rounding per operation (the unit is built with -ffp-contract=off), and saying
// "the two rows disagree" iff d < 0. The forest under the strict total order (w, lo, hi) is unique, so it may be built in any way: here in
// Boruvka rounds over a union-find that carries one parity bit.
//
// State: word[x] = parent << 1 | parity, one uint32 per row (rows < 2^27), parity = "x is flipped relative to parent". A 4-byte load or store
// moves a consistent (ancestor, parity to that ancestor) pair. At the start of a round every word names its tree's root. A round:
//   k_orient_offer<T, 0>  a thread per slot (i, c) of the neighbour array whose ends lie in different trees offers the edge's w, as an
//                         order-preserving uint64, to both trees: atomicMin on best_w[root];
//   k_orient_offer<T, 1>  the slots that hold their tree's least w offer lo << 28 | hi << 1 | (d < 0): atomicMin on best_e[root];
//   k_orient_hook         a thread per root that was offered an edge (u in its tree r, v in tree s): if s chose the same edge, the larger
//                         root of the two hooks, the smaller stays (a strict total order leaves these mutual pairs as the only cycles); else r
//                         hooks: hook[r] = s << 1 | (par[u] ^ flip ^ par[v]). The kernel reads `word` and writes `hook`, so that no root reads
//                         a word another root is writing;
//   k_orient_flatten      every row walks to its new root, XORs the parities on the way and stores its own word.
// The flatten's walk: a word that still names its own row belongs to a root of the round's start, whose step is hook[row] (itself: the
// walk's end); any other word is a finished row's and names that row's final root. Every value a walk can read is an ancestor with the true
// parity to it, every step strictly approaches the root of a forest that is fixed within the launch, and a row's word is stored by its own
// thread alone, so after the launch every word names a root. The loads and stores of `word` in that launch are relaxed agent-scope atomics
// (components.h: eight L2s, and an L1 that no other CU's store refreshes). No thread waits for another; there is no grid barrier.
// components.h's cc_find cannot serve: its parent[x] <= x does not hold where a root hooks under whichever root its edge points to.
//
// The reference row of a tree -- the row with the largest z (compared in T; -0 == +0), the smallest row among equal ones -- travels with the
// rounds: top[root], a row of the tree, which a root that hooks hands to its new root in the flatten. (Found after the last round instead,
// it is one atomic per row on one address for a cloud that is one tree: 3.3 of the call's 7.0 ms at a million rows)
// k_orient_write: base = normals[ref, 2] < 0, flipped[x] = base ^ par[x] ^ par[ref]; a flipped normal has its three sign bits inverted,
// nothing else is touched.
#pragma once
#include "pcu_types.h"
#include "grid.h"
#include "components.h"

namespace pcu {

constexpr unsigned long long kOrNone = ~0ull;           // best_w / best_e: nothing offered
constexpr int kOrMaxRounds = 30;                        // rounds halve the trees that have an edge: at most 27 for 2^27 rows
constexpr int kOrCounts = kOrMaxRounds;                 // [r]: the roots that hooked in round r (every hook makes one tree of two)

// A double as a uint64 of the same order (no NaN reaches it, and no -0.0: w = 1.0 - |d|).
__device__ __forceinline__ unsigned long long orient_key(double v) {
    const unsigned long long b = (unsigned long long)__double_as_longlong(v);
    return (b >> 63) ? ~b : (b | 0x8000000000000000ull);
}
__device__ __forceinline__ unsigned long long or_load64(const unsigned long long* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

// q = idx / m without the compiler's 64-bit division (which goes through floating point): inv = floor((2^64 - 1) / m) from the host.
__device__ __forceinline__ unsigned orient_row_of(unsigned long long idx, unsigned m, unsigned long long inv) {
    unsigned long long q = __umul64hi(idx, inv), r = idx - q * m;
    while (r >= m) { r -= m; ++q; }
    return (unsigned)q;
}

__global__ __launch_bounds__(kBlock) void k_orient_init(unsigned* __restrict__ word, unsigned* __restrict__ top, unsigned long long* __restrict__ best_w, unsigned long long* __restrict__ best_e, unsigned n) {
    const unsigned i = blockIdx.x * kBlock + threadIdx.x;
    if (i >= n) return;
    word[i] = i << 1;
    top[i] = i;
    best_w[i] = kOrNone; best_e[i] = kOrNone;
}

// dead[slot] != 0: the slot offers nothing any more -- it names its own row or no row, its agreement is not finite, or its ends have met
// in one tree, which they never leave. Pass 0 finds that out and says so; from then on the slot costs its byte, not its 8-byte row and the
// gathers of two words.
template <typename T, int PASS>
__global__ __launch_bounds__(kBlock) void k_orient_offer(const T* __restrict__ nrm, const long long* __restrict__ nbr, unsigned n, unsigned m, unsigned long long m_inv,
                                                         unsigned long long slots, const unsigned* __restrict__ word, unsigned char* __restrict__ dead,
                                                         unsigned long long* best_w, unsigned long long* best_e) {
    const unsigned long long idx = (unsigned long long)blockIdx.x * kBlock + threadIdx.x;
    if (idx >= slots || dead[idx]) return;
    const unsigned i = orient_row_of(idx, m, m_inv);
    const long long jj = nbr[idx];
    const bool row = jj >= 0 && jj < (long long)n && jj != (long long)i;
    const unsigned j = row ? (unsigned)jj : i;
    const unsigned ri = word[i] >> 1, rj = word[j] >> 1;
    if (ri == rj) { if (PASS == 0) dead[idx] = 1; return; }           // (j == i included)
    const size_t oi = (size_t)i * 3, oj = (size_t)j * 3;
    const double d = ((double)nrm[oi] * (double)nrm[oj] + (double)nrm[oi + 1] * (double)nrm[oj + 1]) + (double)nrm[oi + 2] * (double)nrm[oj + 2];
    if (!(fabs(d) < __builtin_inf())) { if (PASS == 0) dead[idx] = 1; return; }       // not finite: not an edge
    const unsigned long long kw = orient_key(1.0 - fabs(d));
    if (PASS == 0) {
        if (or_load64(best_w + ri) > kw) atomicMin(best_w + ri, kw);
        if (or_load64(best_w + rj) > kw) atomicMin(best_w + rj, kw);
    } else {
        const unsigned lo = i < j ? i : j, hi = i < j ? j : i;
        const unsigned long long e = (unsigned long long)lo << 28 | (unsigned long long)hi << 1 | (d < 0.0 ? 1ull : 0ull);
        if (best_w[ri] == kw && or_load64(best_e + ri) > e) atomicMin(best_e + ri, e);
        if (best_w[rj] == kw && or_load64(best_e + rj) > e) atomicMin(best_e + rj, e);
    }
}

// hook[r], for every root r of the round's start: its step in the flatten (itself where it stays a root). *hooks += the roots that hook.
__global__ __launch_bounds__(kBlock) void k_orient_hook(const unsigned* __restrict__ word, const unsigned long long* __restrict__ best_w, const unsigned long long* __restrict__ best_e,
                                                        unsigned n, unsigned* __restrict__ hook, unsigned* __restrict__ hooks) {
    const unsigned r = blockIdx.x * kBlock + threadIdx.x;
    bool hooked = false;
    if (r < n && (word[r] >> 1) == r) {
        unsigned out = r << 1;
        const unsigned long long kw = best_w[r];
        const unsigned long long e = best_e[r];
        const unsigned lo = (unsigned)(e >> 28) & 0x07ffffffu, hi = (unsigned)(e >> 1) & 0x07ffffffu, flip = (unsigned)e & 1u;
        if (kw != kOrNone && e != kOrNone && lo < n && hi < n) {
            const unsigned wl = word[lo], wh = word[hi];
            const unsigned wv = (wl >> 1) == r ? wh : wl;       // v: the end in the other tree
            const unsigned s = wv >> 1;
            const bool mutual = best_w[s] == kw && best_e[s] == e;
            if (!(mutual && r < s)) { out = s << 1 | ((wl ^ wh ^ flip) & 1u); hooked = true; }
        }
        hook[r] = out;
    }
    // one add per block: in the first rounds every wave has roots that hook, and an add per wave is 16,384 adds to one address at a million rows
    __shared__ unsigned per_wave[kBlock / 64];
    const unsigned long long b = __ballot(hooked);
    if ((threadIdx.x & 63) == 0) per_wave[threadIdx.x >> 6] = (unsigned)__popcll(b);
    __syncthreads();
    if (threadIdx.x == 0) {
        unsigned t = 0;
        for (int w = 0; w < kBlock / 64; ++w) t += per_wave[w];
        if (t) atomicAdd(hooks, t);
    }
}

// The reference row of two: the larger z (compared in T: -0 == +0; no NaN reaches a searched cloud), the smaller row among equal ones.
template <typename T>
__device__ __forceinline__ bool orient_above(const T* __restrict__ pts, unsigned a, T za, unsigned b) {
    const T zb = pts[(size_t)b * 3 + 2];
    return za > zb || (za == zb && a < b);
}
// word[x] = the new root of x and the parity to it. A root of the round's start gets its offers cleared for the next round, and one that
// hooked hands its tree's reference row to its new root: top[x] is final by now (whoever hooked under x walks on to the same new root and
// hands over there), and top[root] moves by compare-and-swap towards the better row -- rows are compared by what they are, so the order of
// the hand-overs does not matter.
template <typename T>
__global__ __launch_bounds__(kBlock) void k_orient_flatten(const T* __restrict__ pts, unsigned* word, const unsigned* __restrict__ hook, unsigned long long* __restrict__ best_w,
                                                           unsigned long long* __restrict__ best_e, unsigned* top, unsigned n) {
    const unsigned x = blockIdx.x * kBlock + threadIdx.x;
    if (x >= n) return;
    unsigned cur = x, par = 0;
    bool was_root = false;
    for (;;) {
        unsigned w = cc_load(word + cur);
        if ((w >> 1) == cur) {                          // a root of the round's start (or a finished root): its step is the hook
            if (cur == x) { was_root = true; best_w[x] = kOrNone; best_e[x] = kOrNone; }
            w = hook[cur];
            if ((w >> 1) == cur) break;
        }
        par ^= w & 1u;
        cur = w >> 1;
    }
    __hip_atomic_store(word + x, cur << 1 | par, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (was_root && cur != x) {
        const unsigned mine = top[x];
        const T z = pts[(size_t)mine * 3 + 2];
        unsigned seen = cc_load(top + cur);
        while (orient_above(pts, mine, z, seen)) {
            const unsigned was = atomicCAS(top + cur, seen, mine);
            if (was == seen) break;
            seen = was;
        }
    }
}

// The outputs. flipped may be null.
template <typename T> struct OrientBits;
template <> struct OrientBits<float> { typedef unsigned type; static constexpr unsigned sign = 0x80000000u; };
template <> struct OrientBits<double> { typedef unsigned long long type; static constexpr unsigned long long sign = 0x8000000000000000ull; };
template <typename T>
__global__ __launch_bounds__(kBlock) void k_orient_write(const T* __restrict__ nrm, const unsigned* __restrict__ word, const unsigned* __restrict__ top, unsigned n,
                                                         T* __restrict__ out, unsigned char* __restrict__ flipped) {
    typedef typename OrientBits<T>::type B;
    const unsigned x = blockIdx.x * kBlock + threadIdx.x;
    if (x < n) {
        const unsigned w = word[x], root = w >> 1;
        const unsigned ref = top[root];
        const unsigned base = nrm[(size_t)ref * 3 + 2] < (T)0 ? 1u : 0u;
        const unsigned f = (base ^ w ^ word[ref]) & 1u;
        const B mask = f ? OrientBits<T>::sign : (B)0;
        const B* in = reinterpret_cast<const B*>(nrm) + (size_t)x * 3;
        B* o = reinterpret_cast<B*>(out) + (size_t)x * 3;
        o[0] = in[0] ^ mask; o[1] = in[1] ^ mask; o[2] = in[2] ^ mask;
        if (flipped) flipped[x] = (unsigned char)f;
    }
}

}  // namespace pcu
