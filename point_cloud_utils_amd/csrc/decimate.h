// csrc/decimate.h -- decimate_triangle_mesh (src/mesh_decimate.cpp:23-66 over igl::decimate): the kernels and the contract (DESIGN.md, row
// f17; restated in numpy: tests/decimate_contract.py). Host side: decimate_host.h.
//
// The reference runs libigl's sequential priority queue, and libigl was not at hand; the operator follows a stated contract, a
// round-synchronous shortest-edge collapse whose result does not depend on any order of execution. State: positions P (v's type), the
// alive faces as int32 triples with their input rows; vertex ids never change during the rounds. While more than max_faces faces are alive:
//   edges     the distinct undirected pairs (lo, hi) of the alive faces in lexicographic order. One face: a boundary edge between boundary
//             vertices. Think of one extra vertex INF and a face (x, y, INF) on every boundary edge; INF is never collapsed or stored.
//   cost      d = double(P[lo]) - double(P[hi]); c = (d0 d0 + d1 d1) + d2 d2 in double, every operation rounded on its own; c rounded to
//             float32; key = bits(c) << 32 | rank. A non-finite c (NaN or infinite positions, float32 overflow) makes the edge invalid.
//   validity  the link condition on the closed mesh, |N(lo) & N(hi)| == 2 with INF a neighbour of every boundary vertex, and no face of hi
//             that does not hold lo becomes, with hi replaced by lo, the vertex set of an existing face, virtual faces included. Normal
//             flips are not tested (igl's shortest-edge heuristic does not test them either).
//   claims    every valid edge writes its key, by minimum, to every real vertex of {lo, hi} | N(lo) | N(hi) and WINS iff it holds them
//             all. Winners touch disjoint sets of faces; the smallest valid key always wins, so a round with a valid edge makes progress.
//   budget    the winners in ascending key order; one is taken iff the winners before it remove fewer than alive - max_faces faces (an
//             interior edge removes 2, a boundary edge 1).
//   apply     P[lo] = (P[lo] + P[hi]) * 0.5 in v's type; faces that hold both ends die, in the others hi becomes lo in place.
// A round without a winner ends the loop. Output: the alive faces in input order, the vertices they list in input order, faces re-indexed.
//
// One round on the device, every launch one thread per item, none waiting on another thread:
//   structure the directed pairs of every alive face (k_ms_pairs of mesh_smooth.h), one stable sort, run heads, scan: the unique runs are
//             the CSR of the neighbours, sorted within a row; a run's length is its edge's number of faces and the ids of the run name the
//             corners opposite the edge. The entries lo -> hi with lo < hi are the edges in lexicographic order, so the entry index serves
//             as the rank: only the order of the keys reaches the output.
//   k_dc_claim  cost, validity and the 64-bit atomicMin on the owner word of every vertex of the claim set
//   k_dc_wins   a valid edge whose key stands in all of them is a winner: flagged, counted, its faces added to the round's total
//   budget    only where the total exceeds what is left to remove (the last round): the winners' keys are compacted, sorted, their face
//             counts scanned in that order and the prefix taken. Elsewhere every winner is taken.
//   k_dc_apply, k_dc_faces_step  the midpoints and the redirections hi -> lo, then the faces; the survivors are flagged, scanned, compacted.
// The owner words hold no state between launches other than the minimum, which is the same whatever order the atomics arrive in.
#pragma once
#include "mesh_smooth.h"
#include "mesh_repair.h"

namespace pcu {

constexpr int kDcTwice = 4, kDcThreeFaces = 8;            // above kMeshBadVertex / kMeshBadFace in the call's flag word
constexpr unsigned long long kDcNoKey = ~0ull;

// Faces of any of the four integer types -> range-checked int32 triples and their rows. A face with an index outside [0, nv) or one that
// lists a vertex twice raises its flag and reads as (0, 0, 0): the call is refused before anything is made of it.
__global__ __launch_bounds__(kBlock) void k_dc_faces_in(const void* __restrict__ f, int kind, unsigned nf, unsigned nv, int* __restrict__ cf, unsigned* __restrict__ rows,
                                                        int* __restrict__ bad) {
    const unsigned i = blockIdx.x * kBlock + threadIdx.x;
    int b = 0;
    if (i < nf) {
        int id[3];
        if (face_in(f, kind, (size_t)i, nv, id)) b = kMeshBadFace;
        else if (id[0] == id[1] || id[1] == id[2] || id[0] == id[2]) { b = kDcTwice; id[0] = id[1] = id[2] = 0; }
        cf[3 * (size_t)i] = id[0]; cf[3 * (size_t)i + 1] = id[1]; cf[3 * (size_t)i + 2] = id[2];
        rows[i] = i;
    }
    const int any = (__ballot(b & kMeshBadFace) ? kMeshBadFace : 0) | (__ballot(b & kDcTwice) ? kDcTwice : 0);
    if (any && (threadIdx.x & 63) == 0) atomicOr(bad, any);
}

// The number of unique entries stands behind the scan of the run heads.
__device__ __forceinline__ unsigned dc_faces_of(const unsigned* __restrict__ head_pos, unsigned e, unsigned ne, unsigned K) {
    return (e + 1u < ne ? head_pos[e + 1u] : K) - head_pos[e];
}
// One thread per entry: an edge of three or more faces raises the flag (the input's; no collapse makes one).
__global__ __launch_bounds__(kBlock) void k_dc_check_edges(const unsigned* __restrict__ head_pos, const unsigned* __restrict__ ne_ptr, unsigned K, int* __restrict__ bad) {
    const unsigned e = blockIdx.x * kBlock + threadIdx.x, ne = *ne_ptr;
    const bool three = e < ne && dc_faces_of(head_pos, e, ne, K) > 2u;
    if (__ballot(three) != 0ull && (threadIdx.x & 63) == 0) atomicOr(bad, kDcThreeFaces);
}

struct DcStructure {                    // one round's adjacency: entries [off[x], off[x + 1]) of vertex x, columns ascending
    const unsigned long long* keys;     // the K sorted directed pairs, row << hb | column
    const unsigned* ids;                // where each stood: 2 * corner + direction; cf[corner] is the vertex opposite the pair's edge
    const unsigned *off, *head_pos;     // head_pos[e]: where the run of entry e starts
    const int* col;
    const unsigned* ne_ptr;             // the number of entries
    const int* cf;                      // the alive faces
    unsigned K; int hb;
};

__device__ __forceinline__ bool dc_row_on_boundary(const DcStructure& S, unsigned a0, unsigned a1, unsigned ne) {
    bool b = false;
    for (unsigned i = a0; i < a1; ++i) b |= dc_faces_of(S.head_pos, i, ne, S.K) == 1u;
    return b;
}
// The validity of edge (lo, hi), lo < hi (the contract's step 4).
__device__ __forceinline__ bool dc_valid(const DcStructure& S, unsigned lo, unsigned hi, unsigned ne) {
    const unsigned a0 = S.off[lo], a1 = S.off[lo + 1u], b0 = S.off[hi], b1 = S.off[hi + 1u];
    unsigned common = 0, ea[2] = {0, 0}, eb[2] = {0, 0};
    for (unsigned i = a0, j = b0; i < a1 && j < b1;) {
        const int x = S.col[i], y = S.col[j];
        if (x < y) ++i;
        else if (y < x) ++j;
        else {
            if (common < 2u) { ea[common] = i; eb[common] = j; }
            ++common; ++i; ++j;
        }
    }
    if (common > 2u) return false;
    const bool both = dc_row_on_boundary(S, a0, a1, ne) && dc_row_on_boundary(S, b0, b1, ne);          // INF is a common neighbour
    if (common + (both ? 1u : 0u) != 2u) return false;
    // A face (hi, x, y) without lo can only meet a face (lo, x, y) where x is a common neighbour: the faces on hi -> x against those on lo -> x.
    for (unsigned k = 0; k < common; ++k) {
        const unsigned na = dc_faces_of(S.head_pos, ea[k], ne, S.K), nb = dc_faces_of(S.head_pos, eb[k], ne, S.K);
        if (na == 1u && nb == 1u) return false;                                                      // (hi, x, INF) onto (lo, x, INF)
        const unsigned pa = S.head_pos[ea[k]], pb = S.head_pos[eb[k]];
        for (unsigned q = 0; q < nb; ++q) {
            const int y = S.cf[S.ids[pb + q] >> 1];
            if (y == (int)lo) continue;
            for (unsigned r = 0; r < na; ++r)
                if (S.cf[S.ids[pa + r] >> 1] == y) return false;
        }
    }
    return true;
}
// The float32 a key carries: every product and sum rounded on its own.
template <typename T>
__device__ __forceinline__ float dc_cost(const T* __restrict__ P, unsigned lo, unsigned hi) {
#pragma clang fp contract(off)
    const double d0 = (double)P[3 * (size_t)lo] - (double)P[3 * (size_t)hi], d1 = (double)P[3 * (size_t)lo + 1] - (double)P[3 * (size_t)hi + 1],
                 d2 = (double)P[3 * (size_t)lo + 2] - (double)P[3 * (size_t)hi + 2];
    const double s01 = d0 * d0 + d1 * d1;
    return (float)(s01 + d2 * d2);
}
// f(x) for every real vertex x of {lo, hi} | N(lo) | N(hi); stops at the first false.
template <typename F>
__device__ __forceinline__ bool dc_claim_set(const DcStructure& S, unsigned lo, unsigned hi, F f) {
    if (!f(lo) || !f(hi)) return false;
    for (unsigned i = S.off[lo], a1 = S.off[lo + 1u]; i < a1; ++i) if (!f((unsigned)S.col[i])) return false;
    for (unsigned i = S.off[hi], b1 = S.off[hi + 1u]; i < b1; ++i) if (!f((unsigned)S.col[i])) return false;
    return true;
}
// One thread per entry lo -> hi. ekey[e] = the key of a valid edge, else kDcNoKey (an entry with lo > hi is its edge's second copy); a
// valid edge lowers the owner words of its claim set to its key.
template <typename T>
__global__ __launch_bounds__(kBlock) void k_dc_claim(DcStructure S, const T* __restrict__ P, unsigned long long* __restrict__ ekey, unsigned long long* owner) {
    const unsigned e = blockIdx.x * kBlock + threadIdx.x, ne = *S.ne_ptr;
    if (e >= ne) return;
    const unsigned lo = (unsigned)(S.keys[S.head_pos[e]] >> S.hb), hi = (unsigned)S.col[e];
    unsigned long long key = kDcNoKey;
    if (lo < hi) {
        const float c = dc_cost<T>(P, lo, hi);
        if (isfinite(c) && dc_valid(S, lo, hi, ne)) key = ((unsigned long long)__float_as_uint(c) << 32) | e;
    }
    ekey[e] = key;
    if (key != kDcNoKey) dc_claim_set(S, lo, hi, [&](unsigned x) { atomicMin(owner + x, key); return true; });
}
// One thread per entry: win[e] = 1 where the edge's key stands in every owner word of its claim set. counts[0] += winners, counts[1] += the
// faces they remove (one add per wave that has any).
__global__ __launch_bounds__(kBlock) void k_dc_wins(DcStructure S, const unsigned long long* __restrict__ ekey, const unsigned long long* __restrict__ owner,
                                                    unsigned* __restrict__ win, unsigned* __restrict__ counts) {
    const unsigned e = blockIdx.x * kBlock + threadIdx.x, ne = *S.ne_ptr;
    unsigned faces = 0;
    if (e < ne) {
        const unsigned long long key = ekey[e];
        if (key != kDcNoKey && dc_claim_set(S, (unsigned)(S.keys[S.head_pos[e]] >> S.hb), (unsigned)S.col[e], [&](unsigned x) { return owner[x] == key; }))
            faces = dc_faces_of(S.head_pos, e, ne, S.K);
        win[e] = faces ? 1u : 0u;
    } else if (e < S.K) {
        win[e] = 0u;
    }
    const unsigned long long any = __ballot(faces != 0u);
    if (any != 0ull) {
        unsigned sum = faces;
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) sum += __shfl_xor(sum, o);
        if ((threadIdx.x & 63) == 0) { atomicAdd(counts, (unsigned)__popcll(any)); atomicAdd(counts + 1, sum); }
    }
}
// The budget, where it binds. scan: the inclusive scan of the win flags over the K entries; the winners' keys in entry order.
__global__ __launch_bounds__(kBlock) void k_dc_winner_keys(const unsigned* __restrict__ win, const unsigned* __restrict__ scan, unsigned K,
                                                           const unsigned long long* __restrict__ ekey, unsigned long long* __restrict__ wkeys) {
    const unsigned e = blockIdx.x * kBlock + threadIdx.x;
    if (e < K && win[e]) wkeys[scan[e] - 1u] = ekey[e];
}
// wkeys sorted: the faces each winner removes, in key order.
__global__ __launch_bounds__(kBlock) void k_dc_winner_faces(DcStructure S, const unsigned long long* __restrict__ wkeys, unsigned nw, unsigned* __restrict__ wfaces) {
    const unsigned i = blockIdx.x * kBlock + threadIdx.x;
    if (i < nw) wfaces[i] = dc_faces_of(S.head_pos, (unsigned)(wkeys[i] & 0xffffffffull), *S.ne_ptr, S.K);
}
// wscan: the inclusive scan of wfaces. A winner is taken iff those before it remove fewer than `need` faces; the others lose their flag.
// counts[2] += the winners taken.
__global__ __launch_bounds__(kBlock) void k_dc_budget(const unsigned long long* __restrict__ wkeys, const unsigned* __restrict__ wfaces, const unsigned* __restrict__ wscan,
                                                      unsigned nw, unsigned need, unsigned* __restrict__ win, unsigned* __restrict__ counts) {
    const unsigned i = blockIdx.x * kBlock + threadIdx.x;
    bool taken = false;
    if (i < nw) {
        taken = wscan[i] - wfaces[i] < need;
        if (!taken) win[(unsigned)(wkeys[i] & 0xffffffffull)] = 0u;
    }
    const unsigned long long any = __ballot(taken);
    if (any != 0ull && (threadIdx.x & 63) == 0) atomicAdd(counts + 2, (unsigned)__popcll(any));
}
// One thread per entry: a taken edge moves lo to the midpoint and redirects hi to lo (to[] is -1 elsewhere). Taken edges share no vertex.
template <typename T>
__global__ __launch_bounds__(kBlock) void k_dc_apply(DcStructure S, const unsigned* __restrict__ win, T* __restrict__ P, int* __restrict__ to) {
#pragma clang fp contract(off)
    const unsigned e = blockIdx.x * kBlock + threadIdx.x;
    if (e >= *S.ne_ptr || !win[e]) return;
    const size_t lo = (size_t)(S.keys[S.head_pos[e]] >> S.hb), hi = (size_t)S.col[e];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const T sum = P[3 * lo + k] + P[3 * hi + k];
        P[3 * lo + k] = sum * (T)0.5;
    }
    to[hi] = (int)lo;
}
// One thread per alive face: hi becomes lo in place; keep[i] = 0 where the face held both ends of a taken edge.
__global__ __launch_bounds__(kBlock) void k_dc_faces_step(int* __restrict__ cf, unsigned m, const int* __restrict__ to, unsigned* __restrict__ keep) {
    const unsigned i = blockIdx.x * kBlock + threadIdx.x;
    if (i >= m) return;
    int x[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        x[k] = cf[3 * (size_t)i + k];
        const int t = to[x[k]];
        if (t >= 0) { x[k] = t; cf[3 * (size_t)i + k] = t; }
    }
    keep[i] = (x[0] != x[1] && x[1] != x[2] && x[0] != x[2]) ? 1u : 0u;
}
// scan: the inclusive scan of keep. The survivors and their rows, in order.
__global__ __launch_bounds__(kBlock) void k_dc_compact(const int* __restrict__ cf, const unsigned* __restrict__ rows, unsigned m, const unsigned* __restrict__ keep,
                                                       const unsigned* __restrict__ scan, int* __restrict__ cf_out, unsigned* __restrict__ rows_out) {
    const unsigned i = blockIdx.x * kBlock + threadIdx.x;
    if (i >= m || !keep[i]) return;
    const size_t r = (size_t)(scan[i] - 1u);
    cf_out[3 * r] = cf[3 * (size_t)i]; cf_out[3 * r + 1] = cf[3 * (size_t)i + 1]; cf_out[3 * r + 2] = cf[3 * (size_t)i + 2];
    rows_out[r] = rows[i];
}
// The faces as returned: re-indexed through map (k_mr_map), with their input rows, in the integer type `kind` names.
__global__ __launch_bounds__(kBlock) void k_dc_faces_out(const int* __restrict__ cf, const unsigned* __restrict__ rows, unsigned m, const int* __restrict__ map, int kind,
                                                         void* __restrict__ out_f, void* __restrict__ out_rows) {
    const unsigned i = blockIdx.x * kBlock + threadIdx.x;
    if (i >= m) return;
#pragma unroll
    for (int k = 0; k < 3; ++k) index_out(out_f, kind, 3 * (size_t)i + k, (unsigned)map[cf[3 * (size_t)i + k]]);
    index_out(out_rows, kind, i, rows[i]);
}

}  // namespace pcu
