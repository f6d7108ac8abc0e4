// csrc/fps.h -- farthest-point downsampling of a point cloud (in numpy: tests/fps_contract.py; host side: fps_host.h).
//
// The contract, with T the input type: d2(i, s) = ((dx*dx) + (dy*dy)) + (dz*dz) in T, dx = x_i - x_s, separate multiplies and adds (the unit
// is built with -ffp-contract=off). mind[i] starts at +inf; after row s is selected mind[i] = min(mind[i], d2(i, s)) for every row, and every
// selected row leaves all later arg-maxes. The next sample is the unselected row of largest mind, the LOWEST ROW among exactly equal values;
// its mind at that moment is its entry of dists (the first entry is +inf).
//
// In the kernels a selected row is mind = -1 (mind is never negative otherwise, and never NaN: the coordinates are finite, so a difference
// is finite or an infinity, its square +inf at most, and sums of non-negative terms stay ordered). A candidate is (value, row[, position]);
// "no candidate" is (-1, INT_MAX). fps_better is the total order of the contract, and it is the ONLY comparison between candidates, at every
// level: lane, wave, block, bucket, across blocks. It compares row ids, never positions in the cell order. float64 values do not fit a
// 64-bit key beside the row, so pairs are compared everywhere.
//
// Two shapes:
//   k_fps_block   one 1024-thread block holds the whole cloud in registers (x, y, z, mind per point, 16 points per lane in float32, 8 in
//                 float64) and runs every iteration inside one launch: lane arg-max, wave butterfly, one LDS round over the 16 waves
//                 (double-buffered: ONE __syncthreads per sample), the winner's coordinates travelling with its candidate.
//   k_fps_iter    one launch per sample over the cloud in the grid index's cell order, cut into buckets of kFpsBucket records. A bucket keeps
//                 its bounding box (computed once), the maximum of mind over its unselected rows and the row attaining it. Block b owns the
//                 buckets b, b + G, b + 2G, ... (neighbours in the cell order are neighbours in space: interleaving spreads the few buckets
//                 a sample touches over the blocks); their state lies owner-major, so a block reads its own contiguously. Every block first
//                 reduces the G partials of the previous launch (the other half of a ping-pong array) to the current sample, updates the
//                 buckets the sample can change and writes its own partial. No block waits for another inside a launch.
//   Pruning: a bucket is skipped when lb >= bucket_max, lb = ((gx*gx) + (gy*gy)) + (gz*gz), g = max(lo - s, s - hi, 0) per axis in T. For a
//   point p of the box and an axis with s < lo: lo - s <= p - s exactly, rounding is monotone, so fl(lo - s) <= fl(p - s) = |dx|; likewise for
//   s > hi; and g = 0 <= |dx| otherwise. Rounded multiplication and addition of non-negative values are monotone too, so the computed lb is
//   never above the computed d2 of any point of the box: min(mind, d2) changes nothing in a skipped bucket, exactly, with no slack term.
//   The bucket that holds the sample itself is never skipped (its row must be marked, and bucket_max == 0 == lb for duplicates of selected
//   points); a bucket whose rows are all selected has bucket_max = -1 and is always skipped.
#pragma once
#include <limits.h>
#include "pcu_types.h"

namespace pcu {

#ifndef PCU_FPS_BUCKET
#define PCU_FPS_BUCKET 128
#endif
#ifndef PCU_FPS_CHAIN
#define PCU_FPS_CHAIN 32
#endif
constexpr int kFpsBlockThreads = 1024;       // the one-block path: 16 waves
constexpr int kFpsBlockRows = 16384;         // L: its row limit in float32 (16 points per lane); float64 rows take two registers: L / 2
constexpr int kFpsBucket = PCU_FPS_BUCKET;   // B: records per bucket (a multiple of 64: a wave walks a bucket)
constexpr int kFpsBlocks = 256;              // G: blocks of an iteration launch = partials per sample = threads of a block
constexpr int kFpsChain = PCU_FPS_CHAIN;     // C: iteration launches per captured graph (even: the ping-pong half of a node is fixed)
constexpr int kFpsThreads = 256;
static_assert(kFpsBucket % 64 == 0 && kFpsChain % 2 == 0 && kFpsBlocks == kFpsThreads, "fps geometry");

template <typename T> __device__ __forceinline__ bool fps_better(T av, int ar, T bv, int br) { return av > bv || (av == bv && ar < br); }
template <typename T> __device__ __forceinline__ T fps_d2(T x, T y, T z, T sx, T sy, T sz) {
    const T dx = x - sx, dy = y - sy, dz = z - sz;
    return ((dx * dx) + (dy * dy)) + (dz * dz);
}
// every lane ends with the wave's best candidate (xor butterfly over `width` lanes)
template <typename T, int WIDTH = 64>
__device__ __forceinline__ void fps_wave_max(T& v, int& row, int& aux) {
#pragma unroll
    for (int o = WIDTH / 2; o > 0; o >>= 1) {
        const T ov = __shfl_xor(v, o, 64); const int orow = __shfl_xor(row, o, 64), oaux = __shfl_xor(aux, o, 64);
        if (fps_better(ov, orow, v, row)) { v = ov; row = orow; aux = oaux; }
    }
}

// ------------------------------------------------------------------------------------------------ one block
template <typename T> struct FpsSlot { T v, x, y, z; int row; };
// pts: (n, 3) rows, n <= 1024 * P. idx: m int64; dists: m T or null. *bad is set (and nothing else written) when a coordinate is not finite.
template <typename T, int P>
__global__ __launch_bounds__(kFpsBlockThreads) void k_fps_block(const T* __restrict__ pts, int n, int m, int start, long long* __restrict__ idx,
                                                                T* __restrict__ dists, int squared, int* __restrict__ bad) {
    __shared__ FpsSlot<T> slot[2][kFpsBlockThreads / 64];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    typedef T V2 __attribute__((ext_vector_type(2)));      // two points of a lane side by side: float32 differences, squares and sums are packed instructions
    static_assert(P % 2 == 0, "points per lane come in pairs");
    V2 x[P / 2], y[P / 2], z[P / 2]; T md[P];
    bool nf = false;
#pragma unroll
    for (int j = 0; j < P; ++j) {
        const int i = tid + kFpsBlockThreads * j;
        T px = (T)0, py = (T)0, pz = (T)0;
        if (i < n) {
            px = pts[3 * i]; py = pts[3 * i + 1]; pz = pts[3 * i + 2]; md[j] = (T)INFINITY;
            nf |= !(isfinite(px) && isfinite(py) && isfinite(pz));
        } else md[j] = (T)-1;
        x[j / 2][j % 2] = px; y[j / 2][j % 2] = py; z[j / 2][j % 2] = pz;
    }
    if (__syncthreads_or(nf ? 1 : 0)) { if (tid == 0) *bad = 1; return; }
    int s = start; T sv = (T)INFINITY;
    T sx = pts[3 * s], sy = pts[3 * s + 1], sz = pts[3 * s + 2];
    for (int t = 0, par = 0;; ++t, par ^= 1) {
        if (tid == 0) { idx[t] = s; if (dists) dists[t] = squared ? sv : (T)sqrt(sv); }
        if (t + 1 >= m) break;
        if ((s & (kFpsBlockThreads - 1)) == tid) {           // the sample is this lane's point s / 1024: out for good (min(-1, d2) stays -1); one lane of one wave
            const int sj = s / kFpsBlockThreads;
#pragma unroll
            for (int j = 0; j < P; ++j) if (j == sj) md[j] = (T)-1;
        }
        const V2 sx2 = {sx, sx}, sy2 = {sy, sy}, sz2 = {sz, sz};
        T bv = (T)-1; int bj = -1;
#pragma unroll
        for (int j = 0; j < P; j += 2) {
            const V2 dx = x[j / 2] - sx2, dy = y[j / 2] - sy2, dz = z[j / 2] - sz2;
            const V2 d = ((dx * dx) + (dy * dy)) + (dz * dz);
            const T m0 = d[0] < md[j] ? d[0] : md[j], m1 = d[1] < md[j + 1] ? d[1] : md[j + 1];
            md[j] = m0; md[j + 1] = m1;
            if (m0 > bv) { bv = m0; bj = j; }              // strict: the lowest row of the lane among equals
            if (m1 > bv) { bv = m1; bj = j + 1; }
        }
        T bx = (T)0, by = (T)0, bz = (T)0;
#pragma unroll
        for (int j = 0; j < P; ++j) if (j == bj) { bx = x[j / 2][j % 2]; by = y[j / 2][j % 2]; bz = z[j / 2][j % 2]; }
        const int brow = bj >= 0 ? tid + kFpsBlockThreads * bj : INT_MAX;
        T wv = bv; int wrow = brow, unused = 0;
        fps_wave_max(wv, wrow, unused);
        if (brow == wrow && (wrow != INT_MAX || lane == 0)) { FpsSlot<T> o; o.v = bv; o.x = bx; o.y = by; o.z = bz; o.row = brow; slot[par][wave] = o; }
        __syncthreads();
        constexpr int W = kFpsBlockThreads / 64;
        T cv = slot[par][lane & (W - 1)].v; int crow = slot[par][lane & (W - 1)].row, cw = lane & (W - 1);
        fps_wave_max<T, W>(cv, crow, cw);
        s = crow; sv = cv; sx = slot[par][cw].x; sy = slot[par][cw].y; sz = slot[par][cw].z;
    }
}

// ------------------------------------------------------------------------------------------------ grid path
// What the kernels of one call work on: FpsArgs, the layout, is a kernel argument (the captured chain of iteration launches is re-captured
// when it changes, fps_host.h); FpsCall, what differs between calls on one layout, lies at a fixed address of the context. An iteration's
// first loads -- the chain's base step, the call, the partials, the state of its buckets -- then depend on nothing but its arguments and
// leave together: after a kernel boundary every one of them is a miss in the XCD's L2, and a chain of dependent misses is what an
// iteration costs.
// A candidate travels with its position and its coordinates -- in a bucket's state and in a block's partial --, so that the sample of an
// iteration is known from the partials alone, without a dependent load of its record.
template <typename T>
struct FpsArgs {
    const Pt4<T>* rec;                 // the cloud in cell order, row ids beside the coordinates
    int n, nb, per;                    // records, buckets, bucket slots per block (ceil(nb / G))
    T* mind;                           // [n], by position
    T* box;                            // [G * per][6], by slot: lo x y z, hi x y z
    T* bmax; int* brow; int* bpos; T* bxyz;     // [G * per] ([G * per][3]), by slot: the bucket's best candidate
    T* pv; int* prow; int* ppos; T* pxyz;       // [2][G] ([2][G][3]): the blocks' partials, ping-pong
    int* start_pos;                    // the position of the start row (k_fps_init)
    const int* base;                   // the step of the chain's first node (written between replays)
    unsigned long long* counters;      // null, or [2]: bucket tests, bucket updates
};
template <typename T>
struct FpsCall {
    long long* out_idx; T* out_d;      // [m]; out_d may be null
    int m, start_row, squared;
};
__device__ __forceinline__ int fps_slot(int bucket, int per) { return (bucket % kFpsBlocks) * per + bucket / kFpsBlocks; }
template <typename T> struct FpsCand { T v; int row, pos; T x, y, z; };
template <typename T> __device__ __forceinline__ FpsCand<T> fps_none() { FpsCand<T> c; c.v = (T)-1; c.row = INT_MAX; c.pos = 0; c.x = c.y = c.z = (T)0; return c; }

template <typename T>
__global__ void k_fps_setup(FpsCall<T>* dst, FpsCall<T> c, unsigned long long* counters) {
    *dst = c;
    if (counters) { counters[0] = 0; counters[1] = 0; }
}
// One wave per bucket: its box, mind = +inf, its first candidate (+inf at its lowest row), and the position of the start row.
template <typename T>
__global__ __launch_bounds__(64) void k_fps_init(FpsArgs<T> a, int start_row) {
    const int bk = blockIdx.x, lane = threadIdx.x;
    T lo[3] = {(T)INFINITY, (T)INFINITY, (T)INFINITY}, hi[3] = {-(T)INFINITY, -(T)INFINITY, -(T)INFINITY};
    FpsCand<T> c = fps_none<T>();
    for (int j = 0; j < kFpsBucket / 64; ++j) {
        const int p = bk * kFpsBucket + lane + 64 * j;
        if (p >= a.n) continue;
        const Pt4<T> r = a.rec[p];
        a.mind[p] = (T)INFINITY;
        const T q[3] = {r.x, r.y, r.z};
#pragma unroll
        for (int k = 0; k < 3; ++k) { lo[k] = q[k] < lo[k] ? q[k] : lo[k]; hi[k] = q[k] > hi[k] ? q[k] : hi[k]; }
        if (fps_better((T)INFINITY, (int)r.idx, c.v, c.row)) { c.v = (T)INFINITY; c.row = (int)r.idx; c.pos = p; c.x = r.x; c.y = r.y; c.z = r.z; }
        if ((int)r.idx == start_row) *a.start_pos = p;
    }
#pragma unroll
    for (int k = 0; k < 3; ++k)
        for (int o = 32; o > 0; o >>= 1) {
            const T ol = __shfl_xor(lo[k], o, 64), oh = __shfl_xor(hi[k], o, 64);
            lo[k] = ol < lo[k] ? ol : lo[k]; hi[k] = oh > hi[k] ? oh : hi[k];
        }
    T wv = c.v; int wrow = c.row, wl = lane;
    fps_wave_max(wv, wrow, wl);
    if (lane == wl) {                  // the winner's lane has its position and coordinates
        const int sl = fps_slot(bk, a.per);
        for (int k = 0; k < 3; ++k) { a.box[6 * (size_t)sl + k] = lo[k]; a.box[6 * (size_t)sl + 3 + k] = hi[k]; }
        a.bmax[sl] = c.v; a.brow[sl] = c.row; a.bpos[sl] = c.pos;
        a.bxyz[3 * (size_t)sl] = c.x; a.bxyz[3 * (size_t)sl + 1] = c.y; a.bxyz[3 * (size_t)sl + 2] = c.z;
    }
}

// Sample `base + k` of the call: see the head of this file. Launched with kFpsBlocks blocks of kFpsThreads threads.
template <typename T>
__global__ __launch_bounds__(kFpsThreads) void k_fps_iter(const FpsArgs<T> a, const FpsCall<T>* __restrict__ call, int k) {
    constexpr int W = kFpsThreads / 64;
    __shared__ T red_v[2][W]; __shared__ int red_row[2][W], red_tid[2][W];
    __shared__ FpsCand<T> won[2];
    __shared__ FpsCand<T> upd[kFpsThreads];
    __shared__ int list[kFpsThreads], n_act;
    const FpsCall<T> cl = *call;
    const int step = *a.base + k;
    if (step >= cl.m) return;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, b = blockIdx.x;
    // the best of the block's candidates, in every thread: the winner is found by (value, row), its thread hands the rest over through LDS
    auto block_max = [&](FpsCand<T>& c, int which) {
        T v = c.v; int row = c.row, wt = tid;
        fps_wave_max(v, row, wt);
        if (lane == 0) { red_v[which][wave] = v; red_row[which][wave] = row; red_tid[which][wave] = wt; }
        __syncthreads();
        v = red_v[which][0]; row = red_row[which][0]; wt = red_tid[which][0];
#pragma unroll
        for (int w = 1; w < W; ++w) if (fps_better(red_v[which][w], red_row[which][w], v, row)) { v = red_v[which][w]; row = red_row[which][w]; wt = red_tid[which][w]; }
        if (tid == wt) won[which] = c;
        __syncthreads();
        c = won[which];
    };
    auto load_state = [&](int j, FpsCand<T>& c, T* bx) {      // slot j of this block: the bucket's candidate and its box
        const size_t sl = (size_t)b * a.per + j;
        c.v = a.bmax[sl]; c.row = a.brow[sl]; c.pos = a.bpos[sl];
        c.x = a.bxyz[3 * sl]; c.y = a.bxyz[3 * sl + 1]; c.z = a.bxyz[3 * sl + 2];
#pragma unroll
        for (int q = 0; q < 6; ++q) bx[q] = a.box[6 * sl + q];
    };
    const int mine = b < a.nb ? (a.nb - b + kFpsBlocks - 1) / kFpsBlocks : 0;       // buckets b, b + G, ...: slots [b * per, b * per + mine)
    const bool last = step + 1 >= cl.m;
    // the state of this thread's first bucket does not depend on the sample: its loads are in flight while the sample is found
    FpsCand<T> bc = fps_none<T>(); T bx[6] = {(T)0, (T)0, (T)0, (T)0, (T)0, (T)0};
    if (!last && tid < mine) load_state(tid, bc, bx);
    // the current sample: the start row, or the best of the partials the previous launch wrote (every block reduces them for itself)
    FpsCand<T> s;
    if (step == 0) {
        const Pt4<T> sp = a.rec[*a.start_pos];
        s.v = (T)INFINITY; s.row = cl.start_row; s.pos = *a.start_pos; s.x = sp.x; s.y = sp.y; s.z = sp.z;
    } else {
        const size_t h = (size_t)(k & 1) * kFpsBlocks + tid;             // (the chain's base step is even: the half is the node's)
        s.v = a.pv[h]; s.row = a.prow[h]; s.pos = a.ppos[h]; s.x = a.pxyz[3 * h]; s.y = a.pxyz[3 * h + 1]; s.z = a.pxyz[3 * h + 2];
        block_max(s, 0);
    }
    if (b == 0 && tid == 0) { cl.out_idx[step] = s.row; if (cl.out_d) cl.out_d[step] = cl.squared ? s.v : (T)sqrt(s.v); }
    if (last) return;
    const T sx = s.x, sy = s.y, sz = s.z;
    const int spos = s.pos, s_bucket = spos / kFpsBucket;
    FpsCand<T> best = fps_none<T>(); int updates = 0;
    for (int c0 = 0; c0 < mine; c0 += kFpsThreads) {
        if (tid == 0) n_act = 0;
        __syncthreads();
        const int j = c0 + tid; const bool have = j < mine;
        bool act = false;
        if (have) {
            if (c0 > 0) load_state(j, bc, bx);
#ifdef PCU_FPS_NO_PRUNE
            act = true;
#else
            const T s3[3] = {sx, sy, sz};
            T g[3];
#pragma unroll
            for (int q = 0; q < 3; ++q) {
                const T below = bx[q] - s3[q], above = s3[q] - bx[3 + q];
                const T m = below > above ? below : above;
                g[q] = m > (T)0 ? m : (T)0;
            }
            const T lb = ((g[0] * g[0]) + (g[1] * g[1])) + (g[2] * g[2]);
            act = b + kFpsBlocks * j == s_bucket || !(lb >= bc.v);       // (the sample's own bucket: its row is marked whatever the bound says)
#endif
            if (act) list[atomicAdd(&n_act, 1)] = tid;
        }
        __syncthreads();
        const int na = n_act;
        updates += na;
        for (int e = wave; e < na; e += W) {               // a wave per bucket to update
            const int li = list[e], bk = b + kFpsBlocks * (c0 + li);
            FpsCand<T> w = fps_none<T>();
#pragma unroll
            for (int q = 0; q < kFpsBucket / 64; ++q) {
                const int p = bk * kFpsBucket + lane + 64 * q;
                if (p < a.n) {
                    const Pt4<T> r = a.rec[p];
                    const T old = a.mind[p], d = fps_d2(r.x, r.y, r.z, sx, sy, sz);
                    T nm = d < old ? d : old;
                    if (p == spos) nm = (T)-1;
                    if (nm != old) a.mind[p] = nm;
                    if (nm >= (T)0 && fps_better(nm, (int)r.idx, w.v, w.row)) { w.v = nm; w.row = (int)r.idx; w.pos = p; w.x = r.x; w.y = r.y; w.z = r.z; }
                }
            }
            T wv = w.v; int wrow = w.row, wl = lane;
            fps_wave_max(wv, wrow, wl);
            if (lane == wl) {
                const size_t sl = (size_t)b * a.per + c0 + li;
                a.bmax[sl] = w.v; a.brow[sl] = w.row; a.bpos[sl] = w.pos;
                a.bxyz[3 * sl] = w.x; a.bxyz[3 * sl + 1] = w.y; a.bxyz[3 * sl + 2] = w.z;
                upd[li] = w;
            }
        }
        __syncthreads();
        if (have) {
            if (act) bc = upd[tid];
            if (bc.v >= (T)0 && fps_better(bc.v, bc.row, best.v, best.row)) best = bc;
        }
    }
    block_max(best, 1);
    if (tid == 0) {
        const size_t h = (size_t)((k + 1) & 1) * kFpsBlocks + b;
        a.pv[h] = best.v; a.prow[h] = best.row; a.ppos[h] = best.pos; a.pxyz[3 * h] = best.x; a.pxyz[3 * h + 1] = best.y; a.pxyz[3 * h + 2] = best.z;
        if (a.counters && mine > 0) { atomicAdd(&a.counters[0], (unsigned long long)mine); atomicAdd(&a.counters[1], (unsigned long long)updates); }
    }
}

}  // namespace pcu
