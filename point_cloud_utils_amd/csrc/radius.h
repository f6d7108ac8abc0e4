// csrc/radius.h -- radius_search / radius_count: every dataset point within a radius of every query.
//
// The contract: d2 = ((dx*dx) + (dy*dy)) + (dz*dz) in the input type T, query minus dataset, no FMA (the TU is built with -ffp-contract=off);
// row j is a member of query i iff d2 < r2 with r2 = T(radius) * T(radius) rounded once on the host; a row leaves sorted by (d2, dataset row).
//
// The walk (k_radius_walk, count and fill passes): the queries are taken in the cell order of the DATASET's grid, one wave per 64 of them.
// A query's candidates are the cells within R of its own along every axis (the reach and face-slack arithmetic of k_normals_ball). A wave
// takes the union of its lanes' boxes; when that union is at most kRadUnionFactor times the largest single box it is STAGED: every run of
// records of the union is loaded once, 64 records at a time as one coalesced Pt4 load per lane, and the wave's queries are broadcast over
// the tile from registers (v_readlane) -- lane = candidate, one query per step. The members of one (query, tile) step are compacted with a
// ballot and a popcount: they leave the wave together, into consecutive slots of that query's row. A wave whose queries do not share their
// cells (a query cloud that is sparse against the dataset, queries far outside it) would stage a union that grows with their spread: it
// walks per lane instead, every lane over its own box, as k_normals_ball does. Which of the two a wave takes is a function of the grid and
// its queries alone, the records of a cell are visited in ascending row order (k_cells_by_row), so the order of a filled row is a function
// of the arguments: two equal calls give equal bytes before any sort.
//
// The row order (k_radius_sort_wave / _block, the long-row kernels): rows of up to kRadWaveRow = 128 members sort in one wave's registers (a
// bitonic network of cross-lane moves; four rows of up to 16 or two of up to 32 share a wave, a row of more than 64 has two members to a
// lane), rows of up to kRadBlockRow = 2048 in a block's LDS, longer rows
// through the stable radix passes of radix.h (dataset row, then the bits of d2 -- non-negative IEEE patterns order as unsigned integers --
// then the query: the last pass puts every row back where it was).
#pragma once
#include "pcu_types.h"
#include "grid.h"
#include "radix.h"

namespace pcu {

constexpr int kRadWaveRow = 128;         // rows of up to this many members: one wave's registers, at most two members to a lane
constexpr int kRadSubRow = 16;           // ... four rows to a wave when all four are this short (two when both of a pair have at most 32)
constexpr int kRadBlockRow = 2048;       // rows of up to this many members: one block's LDS (24 KiB of (double, int) pairs)
constexpr int kRadUnionFactor = 8;       // a wave stages its union box while it holds at most this many times the cells of its largest own box:
                                         // a staged candidate costs a register broadcast and ten VALU steps, a gathered one a 16-byte load per
                                         // lane of its own; a chosen figure that nobody has timed

__device__ __forceinline__ int rad_bcast(int v, int l) { return __builtin_amdgcn_readlane(v, l); }
__device__ __forceinline__ unsigned rad_bcast(unsigned v, int l) { return (unsigned)__builtin_amdgcn_readlane((int)v, l); }
__device__ __forceinline__ float rad_bcast(float v, int l) { return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), l)); }
__device__ __forceinline__ double rad_bcast(double v, int l) {
    const unsigned long long b = (unsigned long long)__double_as_longlong(v);
    const unsigned lo = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)b, l), hi = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)(b >> 32), l);
    return __longlong_as_double((long long)(((unsigned long long)hi << 32) | lo));
}
__device__ __forceinline__ int rad_wave_min(int v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = min(v, __shfl_xor(v, o, 64));
    return uniform(v);
}
__device__ __forceinline__ int rad_wave_max(int v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = max(v, __shfl_xor(v, o, 64));
    return uniform(v);
}

// cell of every query in the dataset's grid: the key the queries are ordered by
template <typename T>
__global__ __launch_bounds__(kBlock) void k_radius_qkeys(const GridParams<T>* __restrict__ gp, const T* __restrict__ q, int nq, unsigned long long* __restrict__ keys) {
    const int i = blockIdx.x * kBlock + threadIdx.x;
    if (i >= nq) return;
    keys[i] = (unsigned long long)cell_linear(*gp, q[3 * (size_t)i], q[3 * (size_t)i + 1], q[3 * (size_t)i + 2]);
}

template <typename T>
struct RadiusArgs {
    const GridParams<T>* gp; const Pt4<T>* by_row; const unsigned* cell_start; int nr;      // the dataset's grid; records ascending by row inside a cell
    const T* query; const unsigned* order; int nq;                                          // the queries, and their rows in cell order
    T r2, reach;                                                                            // membership: d2 < r2; reach >= sqrt(r2), the box arithmetic's
    unsigned* counts;                                                                       // count pass: row lengths by query row
    const unsigned long long* offsets; T* d2; int* row;                                     // fill pass: where every row starts (nq + 1); the members
    const unsigned* cancel_word; unsigned cancel_gen;
};

// One wave per 64 queries in cell order. FILL = false: counts[query] = members; FILL = true: the members' (d2, row) from offsets[query] on.
template <typename T, bool FILL>
__global__ __launch_bounds__(kBlock) void k_radius_walk(const RadiusArgs<T> a) {
    const int lane = threadIdx.x & 63;
    const int t = (blockIdx.x * (kBlock / 64) + (threadIdx.x >> 6)) * 64 + lane;
    if (t - lane >= a.nq) return;                                       // (the whole wave)
    const bool active = t < a.nq;
    const GridParams<T> g = uniform_params(*a.gp);
    const int Gx = g.G[0], Gy = g.G[1], Gz = g.G[2];
    const size_t qi = active ? (size_t)a.order[t] : 0;
    const T qx = a.query[3 * qi], qy = a.query[3 * qi + 1], qz = a.query[3 * qi + 2];
    // cells that can hold a member: |coordinate difference| < reach (+ the face slack of the grid); a query outside the grid sits in a border cell
    const int R = (int)fmin(1073741824.0, ceil((double)(a.reach + g.slack[0] + g.slack[1] + g.slack[2]) * (double)g.inv_h));
    const int ccx = grid_cell(g, 0, qx), ccy = grid_cell(g, 1, qy), ccz = grid_cell(g, 2, qz);
    const int x0 = max(ccx - R, 0), x1 = min(ccx + R, Gx - 1);
    const int y0 = max(ccy - R, 0), y1 = min(ccy + R, Gy - 1);
    const int z0 = max(ccz - R, 0), z1 = min(ccz + R, Gz - 1);
    const int big = 0x7fffffff;
    const int ux0 = rad_wave_min(active ? x0 : big), ux1 = rad_wave_max(active ? x1 : -1);
    const int uy0 = rad_wave_min(active ? y0 : big), uy1 = rad_wave_max(active ? y1 : -1);
    const int uz0 = rad_wave_min(active ? z0 : big), uz1 = rad_wave_max(active ? z1 : -1);
    // (both products are at most the grid's cell count: they fit an int)
    const long long own = rad_wave_max(active ? (x1 - x0 + 1) * (y1 - y0 + 1) * (z1 - z0 + 1) : 0);
    const long long uni = (long long)(ux1 - ux0 + 1) * (uy1 - uy0 + 1) * (uz1 - uz0 + 1);
    const bool staged = uni <= (long long)kRadUnionFactor * own;
    const unsigned nr = (unsigned)a.nr;
    unsigned at = 0, end = 0;                                           // count pass: members so far; fill pass: the next slot of this lane's row and the row's end
    if (FILL && active) { at = (unsigned)a.offsets[qi]; end = (unsigned)a.offsets[qi + 1]; }
    long long t_poll = wall_clock64();
    if (staged) {
        const unsigned long long below = (1ull << lane) - 1ull;
        for (int cz = uz0; cz <= uz1; ++cz) {
            // (cancellation: one uncached host-memory load, at most once per 200 us of a wave's life, as the k-NN wave pass looks)
            { const long long t_now = wall_clock64(); if (t_now - t_poll > 20000ll) { t_poll = t_now; if (__ballot(cancel_seen(a.cancel_word, a.cancel_gen))) break; } }
            for (int cy = uy0; cy <= uy1; ++cy) {
                const unsigned long long in_row = __ballot(active && cy >= y0 && cy <= y1 && cz >= z0 && cz <= z1);      // queries whose box takes in this row of cells
                if (!in_row) continue;
                const int lo = row_run_lo(Gx, grid_row(Gy, cy, cz), ux0, ux1);
                const unsigned e = min((unsigned)uniform((int)a.cell_start[lo + (ux1 - ux0 + 1)]), nr), s = min((unsigned)uniform((int)a.cell_start[lo]), e);
                for (unsigned p = s; p < e; p += 64u) {
                    const bool valid = p + (unsigned)lane < e;
                    const Pt4<T> c = a.by_row[valid ? p + (unsigned)lane : s];             // one coalesced record per lane
                    for (unsigned long long qq = in_row; qq; qq &= qq - 1ull) {
                        const int j = __builtin_ctzll(qq);
                        const T dx = rad_bcast(qx, j) - c.x, dy = rad_bcast(qy, j) - c.y, dz = rad_bcast(qz, j) - c.z;
                        const T d2 = ((dx * dx) + (dy * dy)) + (dz * dz);
                        const bool member = valid && d2 < a.r2;
                        const unsigned long long mm = __ballot(member);
                        if (!mm) continue;
                        if (FILL) {
                            const unsigned pos = rad_bcast(at, j) + (unsigned)__popcll(mm & below);
                            if (member && pos < rad_bcast(end, j)) { a.d2[pos] = d2; a.row[pos] = (int)c.idx; }          // this query's members of the tile leave together
                        }
                        if (lane == j) at += (unsigned)__popcll(mm);
                    }
                }
            }
        }
    } else if (active) {
        for (int cz = z0; cz <= z1; ++cz) {
            { const long long t_now = wall_clock64(); if (t_now - t_poll > 20000ll) { t_poll = t_now; if (cancel_seen(a.cancel_word, a.cancel_gen)) break; } }
            for (int cy = y0; cy <= y1; ++cy) {
                const int lo = row_run_lo(Gx, grid_row(Gy, cy, cz), x0, x1);
                const unsigned e = min(a.cell_start[lo + (x1 - x0 + 1)], nr), s = min(a.cell_start[lo], e);
                for (unsigned p = s; p < e; ++p) {
                    const Pt4<T> c = a.by_row[p];
                    const T dx = qx - c.x, dy = qy - c.y, dz = qz - c.z;
                    const T d2 = ((dx * dx) + (dy * dy)) + (dz * dz);
                    if (d2 < a.r2) {
                        if (FILL && at < end) { a.d2[at] = d2; a.row[at] = (int)c.idx; }
                        ++at;
                    }
                }
            }
        }
    }
    if (!FILL && active) a.counts[qi] = at;
}

// Row lengths as 64-bit words for the scan, the rows of the LDS tier listed (in any order: each is sorted on its own), the long rows' lengths
// kept for their scan. tally[0] = rows listed, tally[1] = long rows.
__global__ __launch_bounds__(kBlock) void k_radius_lengths(const unsigned* __restrict__ counts, int nq, unsigned long long* __restrict__ len64, unsigned* __restrict__ mid_list,
                                                           unsigned* __restrict__ long_len, unsigned* __restrict__ tally) {
    const int i = blockIdx.x * kBlock + threadIdx.x;
    const int lane = threadIdx.x & 63;
    const unsigned len = i < nq ? counts[i] : 0u;
    if (i < nq) { len64[i] = len; long_len[i] = len > (unsigned)kRadBlockRow ? len : 0u; }
    const bool mid = len > (unsigned)kRadWaveRow && len <= (unsigned)kRadBlockRow;
    const unsigned long long mm = __ballot(mid), ml = __ballot(len > (unsigned)kRadBlockRow);
    if (mm) {                                                           // one atomic per wave
        const int first = __builtin_ctzll(mm);
        unsigned base = 0;
        if (lane == first) base = atomicAdd(&tally[0], (unsigned)__popcll(mm));
        base = rad_bcast(base, first);
        if (mid) mid_list[base + (unsigned)__popcll(mm & ((1ull << lane) - 1ull))] = (unsigned)i;
    }
    if (ml && lane == __builtin_ctzll(ml)) atomicAdd(&tally[1], (unsigned)__popcll(ml));
}
__global__ __launch_bounds__(kBlock) void k_radius_counts_out(const unsigned* __restrict__ counts, int nq, long long* __restrict__ out) {
    const int i = blockIdx.x * kBlock + threadIdx.x;
    if (i < nq) out[i] = (long long)counts[i];
}

// (d2, row) pairs in ascending order; a row's pairs are distinct (dataset rows are), the padding (+inf, INT_MAX) sorts last
template <typename T>
__device__ __forceinline__ bool rad_less(T da, int ra, T db, int rb) { return da < db || (da == db && ra < rb); }

// Bitonic network over groups of W lanes (W a power of two, wave-uniform): every group ends ascending, or descending with `down`.
template <typename T>
__device__ __forceinline__ void rad_bitonic_lanes(T& d, int& r, int lane, int W, bool down = false) {
    for (int k = 2; k <= W; k <<= 1)
        for (int j = k >> 1; j > 0; j >>= 1) {
            const T od = __shfl_xor(d, j, 64); const int orr = __shfl_xor(r, j, 64);
            const bool up = k == W ? !down : (lane & k) == 0, lower = (lane & j) == 0;
            const bool take = (lower == up) ? rad_less(od, orr, d, r) : rad_less(d, r, od, orr);       // the lower lane of an ascending pair keeps the smaller
            if (take) { d = od; r = orr; }
        }
}
// The last merge of a network over 128 members, two to a lane (member e = lane + 64 h): the halves arrive ascending and descending.
template <typename T>
__device__ __forceinline__ void rad_merge_two(T& d0, int& r0, T& d1, int& r1, int lane) {
    if (rad_less(d1, r1, d0, r0)) { const T td = d0; d0 = d1; d1 = td; const int tr = r0; r0 = r1; r1 = tr; }      // j = 64: inside the lane
#pragma unroll
    for (int h = 0; h < 2; ++h) {
        T& d = h ? d1 : d0; int& r = h ? r1 : r0;
        for (int j = 32; j > 0; j >>= 1) {
            const T od = __shfl_xor(d, j, 64); const int orr = __shfl_xor(r, j, 64);
            const bool take = (lane & j) == 0 ? rad_less(od, orr, d, r) : rad_less(d, r, od, orr);
            if (take) { d = od; r = orr; }
        }
    }
}
// Rows of 2 .. kRadWaveRow members: a wave takes four consecutive rows -- all at once in groups of 16 lanes when none is longer, two at once in
// groups of 32, one in 64 lanes, or one with two members to a lane.
template <typename T>
__global__ __launch_bounds__(kBlock) void k_radius_sort_wave(const unsigned long long* __restrict__ offsets, int nq, T* __restrict__ d2, int* __restrict__ row) {
    const int lane = threadIdx.x & 63;
    const int i0 = (blockIdx.x * (kBlock / 64) + (threadIdx.x >> 6)) * 4;
    if (i0 >= nq) return;
    const unsigned long long o = offsets[min(i0 + min(lane, 4), nq)];
    unsigned long long start[4]; unsigned len[4]; unsigned longest = 0;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const unsigned long long lo = uniform(__shfl(o, q, 64)), hi = uniform(__shfl(o, q + 1, 64));
        start[q] = lo; len[q] = (unsigned)(hi - lo); longest = max(longest, len[q]);
    }
    const T inf = (T)INFINITY;
    if (longest < 2u) return;
    if (longest <= (unsigned)kRadSubRow) {
        const int grp = lane >> 4, li = lane & 15;
        const unsigned long long st = grp == 0 ? start[0] : (grp == 1 ? start[1] : (grp == 2 ? start[2] : start[3]));
        const unsigned ln = grp == 0 ? len[0] : (grp == 1 ? len[1] : (grp == 2 ? len[2] : len[3]));
        const bool has = (unsigned)li < ln;
        T d = has ? d2[st + li] : inf; int r = has ? row[st + li] : 0x7fffffff;
        rad_bitonic_lanes(d, r, lane, kRadSubRow);
        if (has) { d2[st + li] = d; row[st + li] = r; }
        return;
    }
#pragma unroll
    for (int q = 0; q < 4; q += 2) {
        if (max(len[q], len[q + 1]) <= 32u) {                          // two rows, 32 lanes each
            if (max(len[q], len[q + 1]) < 2u) continue;
            const int li = lane & 31;
            const unsigned long long st = lane < 32 ? start[q] : start[q + 1];
            const bool has = (unsigned)li < (lane < 32 ? len[q] : len[q + 1]);
            T d = has ? d2[st + li] : inf; int r = has ? row[st + li] : 0x7fffffff;
            rad_bitonic_lanes(d, r, lane, 32);
            if (has) { d2[st + li] = d; row[st + li] = r; }
            continue;
        }
#pragma unroll
        for (int u = q; u < q + 2; ++u) {
            if (len[u] < 2u || len[u] > (unsigned)kRadWaveRow) continue;
            const bool has0 = (unsigned)lane < len[u], has1 = (unsigned)lane + 64u < len[u];
            T e0 = has0 ? d2[start[u] + lane] : inf; int r0 = has0 ? row[start[u] + lane] : 0x7fffffff;
            if (len[u] <= 64u) {
                rad_bitonic_lanes(e0, r0, lane, len[u] <= 32u ? 32 : 64);
            } else {
                T e1 = has1 ? d2[start[u] + 64 + lane] : inf; int r1 = has1 ? row[start[u] + 64 + lane] : 0x7fffffff;
                rad_bitonic_lanes(e0, r0, lane, 64);
                rad_bitonic_lanes(e1, r1, lane, 64, /*down=*/true);
                rad_merge_two(e0, r0, e1, r1, lane);
                if (has1) { d2[start[u] + 64 + lane] = e1; row[start[u] + 64 + lane] = r1; }
            }
            if (has0) { d2[start[u] + lane] = e0; row[start[u] + lane] = r0; }
        }
    }
}
// Rows of kRadWaveRow + 1 .. kRadBlockRow members (listed): one block per row, a bitonic network in LDS over the next power of two.
template <typename T>
__global__ __launch_bounds__(kBlock) void k_radius_sort_block(const unsigned* __restrict__ list, const unsigned long long* __restrict__ offsets, T* __restrict__ d2, int* __restrict__ row) {
    __shared__ T s_d[kRadBlockRow];
    __shared__ int s_r[kRadBlockRow];
    const unsigned i = list[blockIdx.x];
    const unsigned long long st = offsets[i];
    const int len = (int)(offsets[i + 1] - st);
    if (len > kRadBlockRow) return;                                    // (never: the list holds rows of this tier only)
    int P = 256;
    while (P < len) P <<= 1;
    for (int t = threadIdx.x; t < P; t += kBlock) { s_d[t] = t < len ? d2[st + t] : (T)INFINITY; s_r[t] = t < len ? row[st + t] : 0x7fffffff; }
    for (int k = 2; k <= P; k <<= 1)
        for (int j = k >> 1; j > 0; j >>= 1) {
            __syncthreads();
            for (int t = threadIdx.x; t < P / 2; t += kBlock) {
                const int lo = ((t & ~(j - 1)) << 1) | (t & (j - 1)), hi = lo | j;
                const T dl = s_d[lo], dh = s_d[hi]; const int rl = s_r[lo], rh = s_r[hi];
                const bool up = (lo & k) == 0;
                if (up ? rad_less(dh, rh, dl, rl) : rad_less(dl, rl, dh, rh)) { s_d[lo] = dh; s_r[lo] = rh; s_d[hi] = dl; s_r[hi] = rl; }
            }
        }
    __syncthreads();
    for (int t = threadIdx.x; t < len; t += kBlock) { d2[st + t] = s_d[t]; row[st + t] = s_r[t]; }
}

// ---- rows longer than kRadBlockRow: their members, numbered 0 .. nl - 1 in row order ("long slots"), go through the stable radix passes
template <typename T> struct RadBits;
template <> struct RadBits<float> { __device__ static unsigned long long of(float v) { return (unsigned long long)__float_as_uint(v); } };
template <> struct RadBits<double> { __device__ static unsigned long long of(double v) { return (unsigned long long)__double_as_longlong(v); } };
struct RadLong { const unsigned* scan; const unsigned* counts; const unsigned long long* offsets; int nq; unsigned nl; };       // scan: inclusive, of the long rows' lengths by query row
// the query row that holds long slot e, and the slot's place in the filled rows
__device__ __forceinline__ unsigned long long rad_long_place(const RadLong& L, unsigned e, unsigned* query) {
    int lo = 0, hi = L.nq - 1;                                         // first row whose inclusive scan exceeds e
    while (lo < hi) { const int mid = (lo + hi) >> 1; if (L.scan[mid] > e) hi = mid; else lo = mid + 1; }
    *query = (unsigned)lo;
    return L.offsets[lo] + (unsigned long long)(e - (L.scan[lo] - L.counts[lo]));
}
// stage 0: the dataset row, 1: the bits of d2, 2: the query row -- of the member that stands at sorted position i (ids: where it stood; none: the identity)
template <typename T>
__global__ __launch_bounds__(kBlock) void k_radius_long_key(const RadLong L, const unsigned* __restrict__ ids, int stage, const T* __restrict__ d2, const int* __restrict__ row,
                                                            unsigned long long* __restrict__ keys) {
    const unsigned i = blockIdx.x * (unsigned)kBlock + threadIdx.x;
    if (i >= L.nl) return;
    unsigned q;
    const unsigned long long at = rad_long_place(L, ids ? ids[i] : i, &q);
    keys[i] = stage == 0 ? (unsigned long long)(unsigned)row[at] : (stage == 1 ? RadBits<T>::of(d2[at]) : (unsigned long long)q);
}
// back == 0: the members in sorted order into (td, tr); back == 1: from there to the long slots' places, in order
template <typename T>
__global__ __launch_bounds__(kBlock) void k_radius_long_move(const RadLong L, const unsigned* __restrict__ ids, int back, T* __restrict__ d2, int* __restrict__ row, T* __restrict__ td,
                                                             int* __restrict__ tr) {
    const unsigned i = blockIdx.x * (unsigned)kBlock + threadIdx.x;
    if (i >= L.nl) return;
    unsigned q;
    const unsigned long long at = rad_long_place(L, back ? i : (ids ? ids[i] : i), &q);
    if (back) { d2[at] = td[i]; row[at] = tr[i]; } else { td[i] = d2[at]; tr[i] = row[at]; }
}

// the rows as returned: int64 indices, distances (correctly rounded sqrt) or squared distances; d may be d2 itself
template <typename T>
__global__ __launch_bounds__(kBlock) void k_radius_out(const T* d2, const int* __restrict__ row, unsigned long long total, int squared, long long* __restrict__ idx, T* d) {
    const unsigned long long p = (unsigned long long)blockIdx.x * kBlock + threadIdx.x;
    if (p >= total) return;
    idx[p] = (long long)row[p];
    const T v = d2[p];
    d[p] = squared ? v : (T)sqrt(v);
}

}  // namespace pcu
