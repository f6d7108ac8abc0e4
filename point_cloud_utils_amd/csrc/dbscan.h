// csrc/dbscan.h -- cluster_point_cloud_dbscan: density-based clustering of a point cloud. Host side: dbscan_host.h.
//
// The contract, T the input type: the neighbourhood of row i is its row of radius_search(points, points, eps) (radius.h): j is a neighbour of i
// iff d2 = ((dx*dx) + (dy*dy)) + (dz*dz) < r2 in T, no FMA, r2 = T(eps) * T(eps) rounded once on the host; d2 is the same for (i, j) and (j, i),
// so the graph is undirected. i is CORE iff its neighbourhood, itself included, holds at least min_points rows. The clusters are the connected
// components of the core rows joined where d2 < r2, numbered from 0 in the order of their smallest core row. A row that is not core takes the
// label of its nearest core neighbour -- smallest (d2, dataset row) -- or -1 (noise) when it has none.
//
// One walk, three passes (k_dbscan_walk<T, PASS>). It is k_radius_walk's with the queries being the dataset's own records: the records lie
// ascending by row inside each cell (k_cells_by_row), wave w takes records [64 w, 64 w + 64) -- neighbours in the grid's snake order, so there
// are no query keys and no query sort -- and a wave stages the union of its lanes' boxes (lane = candidate, one query broadcast per step) unless
// that union is more than kRadUnionFactor times its largest own box; then every lane walks its own.
//   kDbCore    every record counts its members and stops at min_points; the core flag is written by record position (the later passes read it
//              beside the tile, coalesced) and by dataset row (the result, and the root flags).
//   kDbUnion   core records only: for each core member j with a smaller dataset row, cc_union(parent, i, j) -- the lock-free union-find of
//              components.h as it is, parent indexed by dataset row, so a finished root is the cluster's smallest row whatever the order of the
//              hooks. Every undirected core edge is met from its larger end; an edge whose ends already show one parent is skipped (db_union).
//   kDbBorder  after k_cc_flatten and the scan of the core roots: a core record writes the rank of its root; any other keeps the smallest
//              (d2, row) among its core members (fewer than min_points of them: the minimum is taken by a scalar loop over a ballot) and writes
//              that member's label, or -1.
// The number of launches is fixed; nothing waits for convergence. Every pass polls the cancel word as k_radius_walk does.
#pragma once
#include "pcu_types.h"
#include "grid.h"
#include "radius.h"
#include "components.h"

namespace pcu {

constexpr int kDbCore = 0, kDbUnion = 1, kDbBorder = 2;

template <typename T>
struct DbscanArgs {
    const GridParams<T>* gp; const Pt4<T>* by_row; const unsigned* cell_start; int n;      // the grid; records ascending by row inside a cell
    T r2, reach;                                                                            // membership: d2 < r2; reach >= sqrt(r2), the box arithmetic's
    unsigned min_points;
    unsigned char* core_pos; unsigned char* core_row;                                       // the core flag by record position and by dataset row
    unsigned* parent;                                                                       // union-find over dataset rows (components.h)
    const unsigned* rank; long long* labels;                                                // border pass: inclusive scan of the core roots; the result
    const unsigned* cancel_word; unsigned cancel_gen;
};

__device__ __forceinline__ unsigned db_row(const Pt4<float>& c) { return (unsigned)c.idx; }
__device__ __forceinline__ unsigned db_row(const Pt4<double>& c) { return (unsigned)c.idx; }
// cc_union unless both sides already show one parent: trees only ever merge, so two rows that have had a common ancestor are joined for good.
// On a cluster that is connected already -- nearly every edge of a dense cloud -- this is two independent loads in place of the four
// dependent ones of cc_union's two finds.
__device__ __forceinline__ void db_union(unsigned* parent, unsigned a, unsigned b) {
    if (cc_load(parent + a) != cc_load(parent + b)) cc_union(parent, a, b);
}

// One wave per 64 records in cell order.
template <typename T, int PASS>
__global__ __launch_bounds__(kBlock) void k_dbscan_walk(const DbscanArgs<T> a) {
    const int lane = threadIdx.x & 63;
    const int t = (blockIdx.x * (kBlock / 64) + (threadIdx.x >> 6)) * 64 + lane;
    if (t - lane >= a.n) return;                                        // (the whole wave)
    const bool active = t < a.n;
    const GridParams<T> g = uniform_params(*a.gp);
    const int Gx = g.G[0], Gy = g.G[1], Gz = g.G[2];
    const Pt4<T> q = a.by_row[active ? t : t - lane];
    const T qx = q.x, qy = q.y, qz = q.z;
    const unsigned qrow = db_row(q);
    const bool qcore = PASS != kDbCore && active && a.core_pos[t] != 0;
    const bool wants = active && (PASS == kDbCore || (PASS == kDbUnion ? qcore : !qcore));      // this lane's record is a query of this pass
    unsigned cnt = 0;                                                   // core pass: members so far
    T bd = (T)INFINITY; unsigned br = 0xffffffffu;                      // border pass: the nearest core member so far
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
        long long t_poll = wall_clock64();
        if (staged) {
            for (int cz = uz0; cz <= uz1; ++cz) {
                { const long long t_now = wall_clock64(); if (t_now - t_poll > 20000ll) { t_poll = t_now; if (__ballot(cancel_seen(a.cancel_word, a.cancel_gen))) break; } }
                for (int cy = uy0; cy <= uy1; ++cy) {
                    const unsigned long long in_row = __ballot(wants && cy >= y0 && cy <= y1 && cz >= z0 && cz <= z1 && (PASS != kDbCore || cnt < a.min_points));
                    if (!in_row) continue;
                    const int lo = row_run_lo(Gx, grid_row(Gy, cy, cz), ux0, ux1);
                    const unsigned e = min((unsigned)uniform((int)a.cell_start[lo + (ux1 - ux0 + 1)]), nr), s = min((unsigned)uniform((int)a.cell_start[lo]), e);
                    for (unsigned p = s; p < e; p += 64u) {
                        const bool valid = p + (unsigned)lane < e;
                        const Pt4<T> c = a.by_row[valid ? p + (unsigned)lane : s];             // one coalesced record per lane
                        const unsigned crow = db_row(c);
                        const bool cand = PASS == kDbCore ? valid : (valid && a.core_pos[p + (unsigned)lane] != 0);    // union and border: core candidates only
                        const unsigned long long qs = PASS == kDbCore ? (in_row & __ballot(cnt < a.min_points)) : in_row;
                        if (PASS != kDbCore && !__ballot(cand)) continue;
                        for (unsigned long long qq = qs; qq; qq &= qq - 1ull) {
                            const int j = __builtin_ctzll(qq);
                            const T dx = rad_bcast(qx, j) - c.x, dy = rad_bcast(qy, j) - c.y, dz = rad_bcast(qz, j) - c.z;
                            const T d2 = ((dx * dx) + (dy * dy)) + (dz * dz);
                            const unsigned jrow = PASS == kDbUnion ? rad_bcast(qrow, j) : 0u;
                            const bool member = cand && d2 < a.r2 && (PASS != kDbUnion || crow < jrow);        // union: every edge from its larger end
                            const unsigned long long mm = __ballot(member);
                            if (!mm) continue;
                            if (PASS == kDbCore) { if (lane == j) cnt += (unsigned)__popcll(mm); }
                            if (PASS == kDbUnion) { if (member) db_union(a.parent, jrow, crow); }
                            if (PASS == kDbBorder) {
                                for (unsigned long long m = mm; m; m &= m - 1ull) {            // (a border query has fewer than min_points members in all)
                                    const int k = __builtin_ctzll(m);
                                    const T dm = rad_bcast(d2, k); const unsigned rm = rad_bcast(crow, k);
                                    if (lane == j && (dm < bd || (dm == bd && rm < br))) { bd = dm; br = rm; }
                                }
                            }
                        }
                    }
                }
            }
        } else if (wants) {
            bool go = true;
            for (int cz = z0; cz <= z1 && go; ++cz) {
                { const long long t_now = wall_clock64(); if (t_now - t_poll > 20000ll) { t_poll = t_now; if (cancel_seen(a.cancel_word, a.cancel_gen)) break; } }
                for (int cy = y0; cy <= y1 && go; ++cy) {
                    const int lo = row_run_lo(Gx, grid_row(Gy, cy, cz), x0, x1);
                    const unsigned e = min(a.cell_start[lo + (x1 - x0 + 1)], nr), s = min(a.cell_start[lo], e);
                    for (unsigned p = s; p < e && go; ++p) {
                        const Pt4<T> c = a.by_row[p];
                        const T dx = qx - c.x, dy = qy - c.y, dz = qz - c.z;
                        const T d2 = ((dx * dx) + (dy * dy)) + (dz * dz);
                        if (!(d2 < a.r2)) continue;
                        if (PASS == kDbCore) { ++cnt; go = cnt < a.min_points; continue; }
                        if (a.core_pos[p] == 0) continue;
                        const unsigned crow = db_row(c);
                        if (PASS == kDbUnion) { if (crow < qrow) db_union(a.parent, qrow, crow); }
                        if (PASS == kDbBorder) { if (d2 < bd || (d2 == bd && crow < br)) { bd = d2; br = crow; } }
                    }
                }
            }
        }
    }
    if (!active) return;
    if (PASS == kDbCore) {
        const unsigned char is_core = cnt >= a.min_points ? 1 : 0;
        a.core_pos[t] = is_core;
        a.core_row[qrow] = is_core;
    }
    if (PASS == kDbBorder) {
        const unsigned from = qcore ? qrow : br;                        // (parent is flat by now: parent[x] is x's root, rank[root] its cluster + 1)
        a.labels[qrow] = from != 0xffffffffu ? (long long)a.rank[a.parent[from]] - 1ll : -1ll;
    }
}

// flag[i] = 1 where row i is the root of a cluster: a root of the union-find that is core (a row that is not core was never hooked and is its own root)
__global__ __launch_bounds__(kBlock) void k_dbscan_roots(const unsigned* __restrict__ parent, const unsigned char* __restrict__ core_row, unsigned n, unsigned* __restrict__ flag) {
    const unsigned i = blockIdx.x * kBlock + threadIdx.x;
    if (i < n) flag[i] = (parent[i] == i && core_row[i] != 0) ? 1u : 0u;
}

}  // namespace pcu
