// csrc/fpfh.h -- compute_point_cloud_fpfh: Fast Point Feature Histograms of an oriented cloud. Host side: fpfh_host.h.
//
// The contract (in numpy: tests/fpfh_contract.py), T the input type. The neighbourhood of row i is its row of radius_search(points, points,
// radius) without i itself: d2 = ((dx*dx) + (dy*dy)) + (dz*dz) < r2 in T, no FMA, r2 = T(radius) * T(radius). A row is VALID iff its normal
// has three finite components, not all zero; an invalid row takes part in no pair and its outputs are zero. Everything below is float64 on
// values converted exactly from T, one rounding per operation, no FMA, IEEE division and square root (fpfh_pair, the only copy on the device):
//   dp = p_j - p_i, len = sqrt(dp.dp); len == 0: no pair. a1 = (n_i.dp) / len, a2 = (n_j.dp) / len. |a1| < |a2|: the roles swap (n1 = n_j,
//   n2 = n_i, dp = -dp, f3 = -a2), else n1 = n_i, n2 = n_j, f3 = a1. u = dp / len, v = u x n1, |v| == 0: no pair; v = v / |v|, w = n1 x v,
//   f2 = v.n2, y = w.n2, x = n1.n2. Eleven bins per feature, [theta 0..10 | f2 11..21 | f3 22..32]: f2 and f3 by t = 11 * ((f + 1) * 0.5),
//   bin 0 unless t >= 1, bin 10 from t >= 10 on, else int(t) (a NaN lands in bin 0); theta = atan2(y, x) without atan2: with (C_b, S_b) the
//   float64 nearest (cos, sin) of -pi + 2 pi b / 11, y < 0 counts the b in 1..5 with C_b*y - S_b*x >= 0, any other y gives 5 plus that count
//   over b in 6..10 (so x = y = 0 lands in bin 10).
// spfh_counts[i] counts the bins of the pairs (i, j) over the valid neighbours j; k_i is the sum of one group. S_i[b] = 100 c_i[b] / k_i (0
// where k_i == 0); W_i[b] = sum over the neighbours j with d2 > 0 of S_j[b] / float64(d2); G_i[g] = the sum of W_i over group g;
// F_i[b] = S_i[b] + 100 W_i[b] / G_i[g] (the second term 0 where G_i[g] == 0); features = T(F). The counts are exact; the sums W run in the
// order of walk 2 (cells in grid order, rows ascending inside a cell): a function of the arguments, but not the contract's ascending j.
//
// Two walks over radius_impl's grid (cells of 1.01 r, records ascending by row inside a cell: k_cells_by_row), a wave per 64 records.
//   k_fpfh_walk1  finds the pairs the way k_dbscan_walk finds members -- the union box of the wave's lanes, staged 64 records at a time with
//                 one query broadcast per step, unless the union is more than kRadUnionFactor times the largest own box; then the lanes step
//                 through their own boxes side by side -- and PARKS them: a pair is some 150 float64 operations with eight divisions and two
//                 square roots, and a (query, tile) step has a handful of members among 64 lanes. The members of a step are compacted with
//                 a ballot into a queue in LDS, (candidate position, query lane); whenever it holds 64 pairs, every lane takes one. The three
//                 bins of a pair are integer adds into the wave's 64 x 33 histogram in LDS. The tail turns the counts into S, float64, by
//                 record position, and writes the counts by dataset row.
//   k_fpfh_walk2  a lane per record over its own box: for every member the 33 quotients S_j[b] / d2 into 33 float64 registers, then F.
//                 There is nothing to share between lanes here but the loads; see DESIGN.md 8.16.
// Both read the cancel word at most once per 200 us, as k_radius_walk does, but look at the clock per tile (walk 1) and per 64 candidates
// (walk 2) where that walk looks once per slab of cells: a candidate here can cost a thousand operations. No float atomics: equal arguments
// give equal bytes.
#pragma once
#include "pcu_types.h"
#include "grid.h"
#include "radius.h"

namespace pcu {

constexpr int kFpfhBins = 33;            // 3 features x 11 bins
constexpr int kFpfhQueue = 128;          // parked pairs per wave: fewer than 64 wait, a step adds at most 64

// (cos, sin) of -pi + 2 pi b / 11 for b = 1 .. 10, the float64 nearest the true values (tests/fpfh_contract.py holds the same literals)
__device__ __forceinline__ double fpfh_edge(double cb, double sb, double x, double y) { return cb * y - sb * x; }
__device__ __forceinline__ int fpfh_theta_bin(double x, double y) {
    if (y < 0.0)
        return (fpfh_edge(-0.8412535328311812, -0.5406408174555976, x, y) >= 0.0 ? 1 : 0) + (fpfh_edge(-0.41541501300188644, -0.9096319953545183, x, y) >= 0.0 ? 1 : 0) +
               (fpfh_edge(0.14231483827328514, -0.9898214418809327, x, y) >= 0.0 ? 1 : 0) + (fpfh_edge(0.6548607339452851, -0.7557495743542583, x, y) >= 0.0 ? 1 : 0) +
               (fpfh_edge(0.9594929736144974, -0.28173255684142967, x, y) >= 0.0 ? 1 : 0);
    return 5 + (fpfh_edge(0.9594929736144974, 0.28173255684142967, x, y) >= 0.0 ? 1 : 0) + (fpfh_edge(0.6548607339452851, 0.7557495743542583, x, y) >= 0.0 ? 1 : 0) +
           (fpfh_edge(0.14231483827328514, 0.9898214418809327, x, y) >= 0.0 ? 1 : 0) + (fpfh_edge(-0.41541501300188644, 0.9096319953545183, x, y) >= 0.0 ? 1 : 0) +
           (fpfh_edge(-0.8412535328311812, 0.5406408174555976, x, y) >= 0.0 ? 1 : 0);
}
__device__ __forceinline__ int fpfh_unit_bin(double f) {
    const double t = 11.0 * ((f + 1.0) * 0.5);
    return t >= 1.0 ? (t >= 10.0 ? 10 : (int)t) : 0;
}
__device__ __forceinline__ double fpfh_dot(double ax, double ay, double az, double bx, double by, double bz) { return ((ax * bx) + (ay * by)) + (az * bz); }

// The three bins of the pair (i, j), or false where the contract skips it. pi, ni: the row whose histogram is counted; pj, nj: its neighbour.
__device__ __forceinline__ bool fpfh_pair(double pix, double piy, double piz, double nix, double niy, double niz, double pjx, double pjy, double pjz, double njx, double njy,
                                          double njz, int* b_theta, int* b_f2, int* b_f3) {
    double dx = pjx - pix, dy = pjy - piy, dz = pjz - piz;
    const double len = sqrt(fpfh_dot(dx, dy, dz, dx, dy, dz));
    if (len == 0.0) return false;
    const double a1 = fpfh_dot(nix, niy, niz, dx, dy, dz) / len, a2 = fpfh_dot(njx, njy, njz, dx, dy, dz) / len;
    const bool swap = fabs(a1) < fabs(a2);
    const double n1x = swap ? njx : nix, n1y = swap ? njy : niy, n1z = swap ? njz : niz;
    const double n2x = swap ? nix : njx, n2y = swap ? niy : njy, n2z = swap ? niz : njz;
    const double f3 = swap ? -a2 : a1;
    if (swap) { dx = -dx; dy = -dy; dz = -dz; }
    const double ux = dx / len, uy = dy / len, uz = dz / len;
    double vx = uy * n1z - uz * n1y, vy = uz * n1x - ux * n1z, vz = ux * n1y - uy * n1x;
    const double vl = sqrt(fpfh_dot(vx, vy, vz, vx, vy, vz));
    if (vl == 0.0) return false;
    vx = vx / vl; vy = vy / vl; vz = vz / vl;
    const double wx = n1y * vz - n1z * vy, wy = n1z * vx - n1x * vz, wz = n1x * vy - n1y * vx;
    const double f2 = fpfh_dot(vx, vy, vz, n2x, n2y, n2z), y = fpfh_dot(wx, wy, wz, n2x, n2y, n2z), x = fpfh_dot(n1x, n1y, n1z, n2x, n2y, n2z);
    *b_theta = fpfh_theta_bin(x, y); *b_f2 = fpfh_unit_bin(f2); *b_f3 = fpfh_unit_bin(f3);
    return true;
}

template <typename T>
struct FpfhArgs {
    const GridParams<T>* gp; const Pt4<T>* by_row; const unsigned* cell_start; int n;      // the grid; records ascending by row inside a cell
    const Pt4<T>* nrm;                                                                      // the normals by record position; idx: 1 where the row is valid
    T r2, reach;                                                                            // membership: d2 < r2; reach >= sqrt(r2), the box arithmetic's
    double* spfh;                                                                           // S, n x 33 by record position
    int* counts;                                                                            // spfh_counts, n x 33 by dataset row, or null
    T* features;                                                                            // n x 33 by dataset row
    unsigned* n_staged;                                                                     // waves that staged their union box (a statistic)
    const unsigned* cancel_word; unsigned cancel_gen;
};

// the normals by record position, with the validity of every row
template <typename T>
__global__ __launch_bounds__(kBlock) void k_fpfh_normals(const Pt4<T>* __restrict__ by_row, const T* __restrict__ normals, int n, Pt4<T>* __restrict__ out) {
    const int t = blockIdx.x * kBlock + threadIdx.x;
    if (t >= n) return;
    const size_t r = (size_t)by_row[t].idx;
    Pt4<T> o; o.x = normals[3 * r]; o.y = normals[3 * r + 1]; o.z = normals[3 * r + 2];
    const bool finite = fabs(o.x) <= Limits<T>::max_v && fabs(o.y) <= Limits<T>::max_v && fabs(o.z) <= Limits<T>::max_v;      // (false for a NaN)
    o.idx = (finite && (o.x != (T)0 || o.y != (T)0 || o.z != (T)0)) ? 1 : 0;
    out[t] = o;
}

__device__ __forceinline__ void fpfh_wave_sync() {       // what one lane wrote to the wave's LDS, every lane may read
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// The lanes below `count` take one parked pair each: entry e = (candidate position, query lane).
template <typename T>
__device__ __forceinline__ void fpfh_drain(const FpfhArgs<T>& a, const unsigned* q_pos, const unsigned* q_lane, int* hist, unsigned count, int lane, double qx, double qy, double qz,
                                           double nx, double ny, double nz) {
    fpfh_wave_sync();
    const bool has = (unsigned)lane < count;
    const unsigned cp = has ? q_pos[lane] : 0u; const int ql = has ? (int)q_lane[lane] : lane;
    // (the shuffles are the whole wave's: a lane without a pair reads its own values)
    const double pix = __shfl(qx, ql, 64), piy = __shfl(qy, ql, 64), piz = __shfl(qz, ql, 64), nix = __shfl(nx, ql, 64), niy = __shfl(ny, ql, 64), niz = __shfl(nz, ql, 64);
    if (has) {
        const Pt4<T> c = a.by_row[cp], cn = a.nrm[cp];
        int b0, b1, b2;
        if (fpfh_pair(pix, piy, piz, nix, niy, niz, (double)c.x, (double)c.y, (double)c.z, (double)cn.x, (double)cn.y, (double)cn.z, &b0, &b1, &b2)) {
            int* const h = hist + ql * kFpfhBins;
            atomicAdd(h + b0, 1); atomicAdd(h + 11 + b1, 1); atomicAdd(h + 22 + b2, 1);
        }
    }
}

// One wave per 64 records in cell order: the counts of every record, then its S.
template <typename T>
__global__ __launch_bounds__(kBlock) void k_fpfh_walk1(const FpfhArgs<T> a) {
    __shared__ int s_hist[kBlock / 64][64 * kFpfhBins];
    __shared__ unsigned s_qpos[kBlock / 64][kFpfhQueue], s_qlane[kBlock / 64][kFpfhQueue];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int t = (blockIdx.x * (kBlock / 64) + wv) * 64 + lane;
    if (t - lane >= a.n) return;                                        // (the whole wave)
    const bool active = t < a.n;
    int* const hist = s_hist[wv]; unsigned* const q_pos = s_qpos[wv]; unsigned* const q_lane = s_qlane[wv];
    for (int e = lane; e < 64 * kFpfhBins; e += 64) hist[e] = 0;
    const GridParams<T> g = uniform_params(*a.gp);
    const int Gx = g.G[0], Gy = g.G[1], Gz = g.G[2];
    const Pt4<T> q = a.by_row[active ? t : t - lane], qn = a.nrm[active ? t : t - lane];
    const T qx = q.x, qy = q.y, qz = q.z;
    const double dqx = (double)q.x, dqy = (double)q.y, dqz = (double)q.z, dnx = (double)qn.x, dny = (double)qn.y, dnz = (double)qn.z;
    const bool wants = active && qn.idx != 0;                          // an invalid row takes part in no pair
    const unsigned long long below = (1ull << lane) - 1ull;
    unsigned parked = 0;                                                // pairs in the queue (wave-uniform)
    fpfh_wave_sync();
    // park the members of one step; with 64 of them parked, every lane takes one and the rest moves to the front
#define FPFH_PARK(member, cpos, qlane)                                                                                                   \
    do {                                                                                                                                 \
        const unsigned long long mm_ = __ballot(member);                                                                                 \
        if (mm_) {                                                                                                                       \
            if (member) { const unsigned at_ = parked + (unsigned)__popcll(mm_ & below); q_pos[at_] = (cpos); q_lane[at_] = (unsigned)(qlane); } \
            parked += (unsigned)__popcll(mm_);                                                                                           \
            if (parked >= 64u) {                                                                                                         \
                fpfh_drain(a, q_pos, q_lane, hist, 64u, lane, dqx, dqy, dqz, dnx, dny, dnz);                                             \
                parked -= 64u;                                                                                                           \
                const bool mv_ = (unsigned)lane < parked;                                                                                \
                const unsigned p_ = mv_ ? q_pos[64 + lane] : 0u, l_ = mv_ ? q_lane[64 + lane] : 0u;                                      \
                if (mv_) { q_pos[lane] = p_; q_lane[lane] = l_; }                                                                        \
            }                                                                                                                            \
        }                                                                                                                                \
    } while (0)
    if (__ballot(wants)) {
        // cells that can hold a member: k_radius_walk's arithmetic
        const int R = (int)fmin(1073741824.0, ceil((double)(a.reach + g.slack[0] + g.slack[1] + g.slack[2]) * (double)g.inv_h));
        const int ccx = grid_cell(g, 0, qx), ccy = grid_cell(g, 1, qy), ccz = grid_cell(g, 2, qz);
        const int x0 = max(ccx - R, 0), x1 = min(ccx + R, Gx - 1);
        const int y0 = max(ccy - R, 0), y1 = min(ccy + R, Gy - 1);
        const int z0 = max(ccz - R, 0), z1 = min(ccz + R, Gz - 1);
        const int big = 0x7fffffff;
        const int ux0 = rad_wave_min(wants ? x0 : big), ux1 = rad_wave_max(wants ? x1 : -1);
        const int uy0 = rad_wave_min(wants ? y0 : big), uy1 = rad_wave_max(wants ? y1 : -1);
        const int uz0 = rad_wave_min(wants ? z0 : big), uz1 = rad_wave_max(wants ? z1 : -1);
        const long long own = rad_wave_max(wants ? (x1 - x0 + 1) * (y1 - y0 + 1) * (z1 - z0 + 1) : 0);
        const long long uni = (long long)(ux1 - ux0 + 1) * (uy1 - uy0 + 1) * (uz1 - uz0 + 1);
        const bool staged = uni <= (long long)kRadUnionFactor * own;
        const unsigned nr = (unsigned)a.n;
        if (staged && lane == 0 && a.n_staged) atomicAdd(a.n_staged, 1u);
        long long t_poll = wall_clock64();
        if (staged) {
            const unsigned t0 = (unsigned)(t - lane);
            bool stop = false;                                          // (wave-uniform)
            for (int cz = uz0; cz <= uz1 && !stop; ++cz) {
                for (int cy = uy0; cy <= uy1 && !stop; ++cy) {
                    const unsigned long long in_row = __ballot(wants && cy >= y0 && cy <= y1 && cz >= z0 && cz <= z1);
                    if (!in_row) continue;
                    const int lo = row_run_lo(Gx, grid_row(Gy, cy, cz), ux0, ux1);
                    const unsigned e = min((unsigned)uniform((int)a.cell_start[lo + (ux1 - ux0 + 1)]), nr), s = min((unsigned)uniform((int)a.cell_start[lo]), e);
                    for (unsigned p = s; p < e && !stop; p += 64u) {
                        // (a tile can cost 64 x 64 pairs: the clock is read per tile, not per slab of cells as where a candidate is ten operations)
                        { const long long t_now = wall_clock64(); if (t_now - t_poll > 20000ll) { t_poll = t_now; stop = __ballot(cancel_seen(a.cancel_word, a.cancel_gen)) != 0ull; } }
                        const bool valid = p + (unsigned)lane < e;
                        const unsigned cp = valid ? p + (unsigned)lane : s;
                        const Pt4<T> c = a.by_row[cp];                                      // one coalesced record per lane
                        const bool cand = valid && a.nrm[cp].idx != 0;
                        if (!__ballot(cand)) continue;
                        for (unsigned long long qq = in_row; qq; qq &= qq - 1ull) {
                            const int j = __builtin_ctzll(qq);
                            const T dx = rad_bcast(qx, j) - c.x, dy = rad_bcast(qy, j) - c.y, dz = rad_bcast(qz, j) - c.z;
                            const T d2 = ((dx * dx) + (dy * dy)) + (dz * dz);
                            const bool member = cand && d2 < a.r2 && cp != t0 + (unsigned)j;      // (a row is no neighbour of itself)
                            FPFH_PARK(member, cp, j);
                        }
                    }
                }
            }
        } else {
            // every lane through its own box, the lanes side by side: one candidate per lane and step
            int cz = z0, cy = y0 - 1; unsigned p = 0, e = 0; bool done = !wants;
            for (;;) {
                { const long long t_now = wall_clock64(); if (t_now - t_poll > 20000ll) { t_poll = t_now; if (__ballot(cancel_seen(a.cancel_word, a.cancel_gen))) break; } }
                while (!done && p >= e) {                              // the next run of records of this lane's box
                    if (++cy > y1) { cy = y0; ++cz; }
                    if (cz > z1) { done = true; break; }
                    const int lo = row_run_lo(Gx, grid_row(Gy, cy, cz), x0, x1);
                    e = min(a.cell_start[lo + (x1 - x0 + 1)], nr); p = min(a.cell_start[lo], e);
                }
                if (!__ballot(!done)) break;
                bool member = false; const unsigned cp = p;
                if (!done) {
                    const Pt4<T> c = a.by_row[p];
                    const T dx = qx - c.x, dy = qy - c.y, dz = qz - c.z;
                    const T d2 = ((dx * dx) + (dy * dy)) + (dz * dz);
                    member = d2 < a.r2 && p != (unsigned)t && a.nrm[p].idx != 0;
                    ++p;
                }
                FPFH_PARK(member, cp, lane);
            }
        }
    }
#undef FPFH_PARK
    if (parked) fpfh_drain(a, q_pos, q_lane, hist, parked, lane, dqx, dqy, dqz, dnx, dny, dnz);
    fpfh_wave_sync();
    // k of every record (its own lane sums one group), then S by record position and the counts by dataset row, 64 x 33 values side by side
    int k = 0;
#pragma unroll
    for (int b = 0; b < 11; ++b) k += hist[lane * kFpfhBins + b];
    const unsigned qrow = (unsigned)q.idx;
    const size_t base = (size_t)(t - lane) * kFpfhBins;
    const int live = min(64, a.n - (t - lane)) * kFpfhBins;
    for (int e0 = 0; e0 < live; e0 += 64) {                             // (the whole wave takes every step: the shuffles read any lane)
        const int e = e0 + lane; const bool in = e < live;
        const int ql = in ? e / kFpfhBins : 0, b = e - ql * kFpfhBins;
        const int kq = __shfl(k, ql, 64); const unsigned row = __shfl(qrow, ql, 64);
        if (in) {
            const int cnt = hist[e];
            a.spfh[base + e] = kq > 0 ? (100.0 * (double)cnt) / (double)kq : 0.0;
            if (a.counts) a.counts[(size_t)row * kFpfhBins + b] = cnt;
        }
    }
}

// One lane per record over its own box: W, then F by dataset row.
template <typename T>
__global__ __launch_bounds__(kBlock) void k_fpfh_walk2(const FpfhArgs<T> a) {
    const int t = blockIdx.x * kBlock + threadIdx.x;
    if (t >= a.n) return;
    const GridParams<T> g = uniform_params(*a.gp);
    const int Gx = g.G[0], Gy = g.G[1], Gz = g.G[2];
    const Pt4<T> q = a.by_row[t];
    const T qx = q.x, qy = q.y, qz = q.z;
    T* const out = a.features + (size_t)q.idx * kFpfhBins;
    if (a.nrm[t].idx == 0) {
#pragma unroll
        for (int b = 0; b < kFpfhBins; ++b) out[b] = (T)0;
        return;
    }
    double W[kFpfhBins];
#pragma unroll
    for (int b = 0; b < kFpfhBins; ++b) W[b] = 0.0;
    const int R = (int)fmin(1073741824.0, ceil((double)(a.reach + g.slack[0] + g.slack[1] + g.slack[2]) * (double)g.inv_h));
    const int ccx = grid_cell(g, 0, qx), ccy = grid_cell(g, 1, qy), ccz = grid_cell(g, 2, qz);
    const int x0 = max(ccx - R, 0), x1 = min(ccx + R, Gx - 1);
    const int y0 = max(ccy - R, 0), y1 = min(ccy + R, Gy - 1);
    const int z0 = max(ccz - R, 0), z1 = min(ccz + R, Gz - 1);
    const unsigned nr = (unsigned)a.n;
    long long t_poll = wall_clock64();
    bool stop = false;
    for (int cz = z0; cz <= z1 && !stop; ++cz) {
        for (int cy = y0; cy <= y1 && !stop; ++cy) {
            const int lo = row_run_lo(Gx, grid_row(Gy, cy, cz), x0, x1);
            const unsigned e = min(a.cell_start[lo + (x1 - x0 + 1)], nr), s = min(a.cell_start[lo], e);
            for (unsigned p = s; p < e && !stop; ++p) {
                // (a member costs 33 divisions: the clock is read every 64 candidates of a run, not once per slab of cells)
                if (((p - s) & 63u) == 0u) { const long long t_now = wall_clock64(); if (t_now - t_poll > 20000ll) { t_poll = t_now; stop = cancel_seen(a.cancel_word, a.cancel_gen); } }
                const Pt4<T> c = a.by_row[p];
                const T dx = qx - c.x, dy = qy - c.y, dz = qz - c.z;
                const T d2 = ((dx * dx) + (dy * dy)) + (dz * dz);
                if (!(d2 < a.r2) || !(d2 > (T)0) || p == (unsigned)t) continue;        // (the S of an invalid row is zero: it adds nothing)
                const double dd = (double)d2;
                const double* const sj = a.spfh + (size_t)p * kFpfhBins;
#pragma unroll
                for (int b = 0; b < kFpfhBins; ++b) W[b] = W[b] + sj[b] / dd;
            }
        }
    }
    const double* const si = a.spfh + (size_t)t * kFpfhBins;
#pragma unroll
    for (int gq = 0; gq < 3; ++gq) {
        double G = 0.0;
#pragma unroll
        for (int b = 0; b < 11; ++b) G = G + W[gq * 11 + b];
#pragma unroll
        for (int b = 0; b < 11; ++b) {
            const double S = si[gq * 11 + b];
            out[gq * 11 + b] = (T)(G == 0.0 ? S : S + (100.0 * W[gq * 11 + b]) / G);
        }
    }
}

}  // namespace pcu
