// csrc/poisson.h -- Poisson-disk downsampling of a point cloud (downsample_point_cloud_poisson_disk, src/sample_point_cloud.cpp:240-333).
//
// The reference runs libigl's serial blue_noise, whose sample set depends on libigl's RNG and on hash-table iteration order. This
// library implements a deterministic contract instead ("Poisson-disk downsampling"):
//   close(i, j)  iff  d2 < r * r, d2 = ((dx*dx)+(dy*dy))+(dz*dz) in T without FMA, dx = v[i,0] - v[j,0] in T (symmetric in i, j);
//   priority(i)  = splitmix64 finalizer of (uint64(seed) << 32) ^ i (a bijection: distinct for every row);
//   result       = the set the serial greedy builds visiting the rows by ascending priority, taking a row iff no row taken so far
//                  is close to it.
// It is computed by a parallel form of that greedy (Blelloch, Fineman and Shun: "Greedy sequential maximal independent set and
// matching are parallel on average") over the uniform grid of grid.h, whose cells are at least r wide, so that a point's r-ball lies in
// the box of cells around its own (`pd_box`; the reach includes the grid's face slack, as k_normals_ball's does). Every point is
// undecided, a sample or removed. One round is three launches, each reading what the previous one finished:
//   k_pd_cellmin  the lowest priority among the undecided points of every cell (wave-segmented min, one atomic per cell and wave);
//   k_pd_decide   an undecided point p becomes a sample iff no undecided point of lower priority is close to it: a box cell whose
//                 minimum is above p's priority holds none; a cell with a lower minimum is scanned exactly when it holds at most
//                 kPdExact points or is more than 2r wide, and otherwise makes p wait. (Samples of earlier rounds are never close
//                 to an undecided point: the previous k_pd_remove removed those.) Two points that decide in the same round are never close -- the higher one
//                 would have seen the lower one -- so the samples are exactly the greedy's;
//   k_pd_remove   an undecided point close to a sample (looked up in the per-cell sample lists) is removed; the undecided points
//                 left are counted for the host, which polls that counter every few rounds.
// The globally lowest undecided point always decides, so every round makes progress. A cell whose width is at least r holds a
// bounded number of samples, so the cost of a round does not grow with r: no kernel visits every point of every ball.
#pragma once
#include "pcu_types.h"
#include "grid.h"

namespace pcu {

__host__ __device__ __forceinline__ unsigned long long pd_mix(unsigned long long z) {        // the splitmix64 finalizer
    z ^= z >> 30; z *= 0xBF58476D1CE4E5B9ull;
    z ^= z >> 27; z *= 0x94D049BB133111EBull;
    z ^= z >> 31;
    return z;
}
__host__ __device__ __forceinline__ unsigned long long pd_priority(unsigned seed, unsigned long long row) {
    return pd_mix(((unsigned long long)seed << 32) ^ row);
}

constexpr unsigned char kPdUndecided = 0, kPdSample = 1, kPdRemoved = 2, kPdStateMask = 3;
constexpr unsigned char kPdHead = 4;       // the first record of its cell (k_pd_remove resets the cell's minimum through it)
constexpr unsigned kPdExact = 64;          // cells of at most this many points are scanned exactly by k_pd_decide

// Everything indexed by position in the cell-ordered cloud (`sorted`), except cellmin / nsamp (by cell).
template <typename T>
struct PdArgs {
    const GridParams<T>* gp; const Pt4<T>* sorted; const unsigned* cell_start;
    int n;
    T r2;                                  // r * r (in T): close iff d2 < r2
    T reach;                               // r * (1 + 8 eps): no coordinate of a close pair differs by this much
    unsigned long long* prio; unsigned char* state; unsigned* cell;
    unsigned long long* cellmin;           // lowest undecided priority per cell (~0: none); all ~0 between rounds
    unsigned* nsamp;                       // samples per cell ...
    unsigned* slist;                       // ... listed at slist[cell_start[c] + k] (sorted positions)
    unsigned* counters;                    // [0] undecided points after the round, [1] samples
};

template <typename T>
__device__ __forceinline__ T pd_d2(const Pt4<T>& a, const Pt4<T>& b) {
    const T dx = a.x - b.x, dy = a.y - b.y, dz = a.z - b.z;
    return ((dx * dx) + (dy * dy)) + (dz * dz);
}

// The cells that can hold a point close to q: [lo, hi] per axis.
template <typename T>
__device__ __forceinline__ void pd_box(const GridParams<T>& g, const Pt4<T>& q, T reach, int (&lo)[3], int (&hi)[3]) {
    const int R = (int)fmin(4096.0, ceil((double)(reach + g.slack[0] + g.slack[1] + g.slack[2]) * (double)g.inv_h));
    const T v[3] = {q.x, q.y, q.z};
#pragma unroll
    for (int j = 0; j < 3; ++j) {
        const int c = grid_cell(g, j, v[j]);
        lo[j] = max(c - R, 0); hi[j] = min(c + R, g.G[j] - 1);
    }
}

// Once per grid build: priorities, cell ids and states of the records.
template <typename T>
__global__ __launch_bounds__(kBlock) void k_pd_init(const PdArgs<T> a, unsigned seed) {
    const int p = blockIdx.x * kBlock + threadIdx.x;
    if (p >= a.n) return;
    const Pt4<T> q = a.sorted[p];
    const unsigned c = cell_linear(*a.gp, q.x, q.y, q.z);
    a.prio[p] = pd_priority(seed, (unsigned long long)q.idx);
    a.cell[p] = c;
    a.state[p] = a.cell_start[c] == (unsigned)p ? kPdHead : kPdUndecided;
}

// (a) cellmin[c] = min priority of the undecided points of cell c. A cell's records are consecutive: a segmented min across the wave,
// then one atomic per (wave, cell).
template <typename T>
__global__ __launch_bounds__(kBlock) void k_pd_cellmin(const PdArgs<T> a) {
    const int p = blockIdx.x * kBlock + threadIdx.x;
    if (p == 0) a.counters[0] = 0u;                  // (k_pd_remove of this round counts into it)
    const int lane = threadIdx.x & 63;
    const bool in = p < a.n;
    const unsigned c = in ? a.cell[p] : 0xffffffffu;
    unsigned long long m = (in && (a.state[p] & kPdStateMask) == kPdUndecided) ? a.prio[p] : ~0ull;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const unsigned long long mo = __shfl_down(m, o, 64);
        const unsigned co = __shfl_down(c, o, 64);
        if (lane + o < 64 && co == c && mo < m) m = mo;
    }
    const unsigned cp = __shfl_up(c, 1, 64);
    if (in && (lane == 0 || cp != c) && m != ~0ull) atomicMin(&a.cellmin[c], m);
}

// (b) undecided p becomes a sample iff no undecided point of lower priority is close to it.
template <typename T>
__global__ __launch_bounds__(kBlock) void k_pd_decide(const PdArgs<T> a) {
    const int p = blockIdx.x * kBlock + threadIdx.x;
    if (p >= a.n) return;
    const unsigned char st = a.state[p];
    if ((st & kPdStateMask) != kPdUndecided) return;
    const GridParams<T>& g = *a.gp;
    const Pt4<T> q = a.sorted[p];
    const unsigned long long pr = a.prio[p];
    int lo[3], hi[3];
    pd_box(g, q, a.reach, lo, hi);
    // Cells more than twice as wide as r (the occupancy rule, not r, set their width: clustered input, small r) can hold many samples
    // each: there every cell is scanned exactly, or a crowded cell would take one round per sample. Narrower cells hold a few samples
    // at most: a crowded one makes p wait, which bounds the work of a round whatever r is.
    const bool wide = g.h > (T)2 * a.reach;
    for (int cz = lo[2]; cz <= hi[2]; ++cz)
        for (int cy = lo[1]; cy <= hi[1]; ++cy) {
            const int c0 = row_run_lo(g.G[0], grid_row(g.G[1], cy, cz), lo[0], hi[0]);
            for (int c = c0; c <= c0 + (hi[0] - lo[0]); ++c) {
                if (a.cellmin[c] >= pr) continue;                  // no undecided point below p here (== pr: p itself)
                const unsigned s = a.cell_start[c], e = a.cell_start[c + 1];
                if (e - s > kPdExact && !wide) return;             // crowded: wait for its lower points to decide
                for (unsigned j = s; j < e; ++j) {
                    // (a record may turn from undecided into a sample during this launch: both count, a removed one does not)
                    if ((a.state[j] & kPdStateMask) == kPdRemoved || a.prio[j] >= pr) continue;
                    if (pd_d2(q, a.sorted[j]) < a.r2) return;
                }
            }
        }
    a.state[p] = (unsigned char)((st & kPdHead) | kPdSample);
    const unsigned c = a.cell[p];
    const unsigned k = atomicAdd(&a.nsamp[c], 1u);
    a.slist[a.cell_start[c] + k] = (unsigned)p;
    atomicAdd(&a.counters[1], 1u);
}

// (c) undecided points close to a sample are removed; the rest are counted. Cell heads reset their cell's minimum for the next round.
template <typename T>
__global__ __launch_bounds__(kBlock) void k_pd_remove(const PdArgs<T> a) {
    const int p = blockIdx.x * kBlock + threadIdx.x;
    const bool in = p < a.n;
    const unsigned char st = in ? a.state[p] : kPdRemoved;
    if (st & kPdHead) a.cellmin[a.cell[p]] = ~0ull;
    bool open = false;
    if ((st & kPdStateMask) == kPdUndecided) {
        const GridParams<T>& g = *a.gp;
        const Pt4<T> q = a.sorted[p];
        int lo[3], hi[3];
        pd_box(g, q, a.reach, lo, hi);
        open = true;
        for (int cz = lo[2]; cz <= hi[2] && open; ++cz)
            for (int cy = lo[1]; cy <= hi[1] && open; ++cy) {
                const int c0 = row_run_lo(g.G[0], grid_row(g.G[1], cy, cz), lo[0], hi[0]);
                for (int c = c0; c <= c0 + (hi[0] - lo[0]) && open; ++c) {
                    const unsigned k = a.nsamp[c], s = a.cell_start[c];
                    for (unsigned j = 0; j < k; ++j)
                        if (pd_d2(q, a.sorted[a.slist[s + j]]) < a.r2) { open = false; break; }
                }
            }
        if (!open) a.state[p] = (unsigned char)((st & kPdHead) | kPdRemoved);
    }
    const unsigned long long b = __ballot(open);
    if ((threadIdx.x & 63) == 0 && b) atomicAdd(&a.counters[0], (unsigned)__popcll(b));
}

// The samples as flags by original row (for the compaction), and the compaction itself: out[rank] = row, ascending.
template <typename T>
__global__ __launch_bounds__(kBlock) void k_pd_flags(const Pt4<T>* sorted, const unsigned char* state, int n, unsigned* flag) {
    const int p = blockIdx.x * kBlock + threadIdx.x;
    if (p >= n) return;
    flag[(size_t)sorted[p].idx] = (state[p] & kPdStateMask) == kPdSample ? 1u : 0u;
}
__global__ __launch_bounds__(kBlock) void k_pd_compact(const unsigned* flag, const unsigned* scan, int n, int32_t* out) {
    const int i = blockIdx.x * kBlock + threadIdx.x;
    if (i < n && flag[i]) out[scan[i] - 1] = i;
}
__global__ __launch_bounds__(kBlock) void k_pd_iota(int n, int32_t* out) {
    const int i = blockIdx.x * kBlock + threadIdx.x;
    if (i < n) out[i] = i;
}

}  // namespace pcu
