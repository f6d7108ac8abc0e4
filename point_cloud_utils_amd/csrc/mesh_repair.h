// csrc/mesh_repair.h -- remove_mesh_vertices, remove_unreferenced_mesh_vertices, deduplicate_mesh_vertices and orient_mesh_faces
// (src/remove_mesh_vertices.cpp:22-73, src/remove_unreferenced_mesh_vertices.cpp:23-37, src/remove_duplicates.cpp:37-81 and :152-176,
// src/orient_mesh_faces.cpp:21-35): the kernels and the four operators' contract. Host side: mesh_repair_host.h.
//
// The reference reaches libigl for two of the four (igl::remove_unreferenced, igl::bfs_orient) and for the rows of the third
// (igl::unique_rows). libigl was not at hand, so each operator follows a stated contract (restated in numpy: tests/mesh_repair_contract.py).
//
// The three vertex calls are the same three moves, one thread per row:
//   map      an int32 map old vertex -> new vertex or -1. From keep flags (the mask, or "some face lists it") through one scan: a kept vertex's
//            new index is the number of kept vertices before it, so the kept vertices stay in input order. For the deduplication the map is
//            svj of deduplicate_point_cloud (voxel.h) and never -1. The "referenced" flags are plain stores of 1u into a zeroed array, one
//            thread per face corner: every racing store writes the same value, and the next launch reads them.
//   rows     the kept vertex rows are copied as they are. No arithmetic touches a coordinate: NaN, infinities and -0.0 pass through.
//   faces    a face is dropped if a corner maps to -1 and, for the deduplication only, if two of its mapped corners are equal. The survivors
//            are flagged, scanned and written with mapped indices in f's integer type, in input order.
// The first launch that reads f checks every index against [0, nv) and raises the flag word; the host reads it with the counts and refuses the
// call before anything is written to the outputs.
//
// orient_mesh_faces. Face i has the directed edges (f[i,0], f[i,1]), (f[i,1], f[i,2]), (f[i,2], f[i,0]); a face that lists a vertex twice takes
// part in no edge. An undirected edge is MANIFOLD when exactly two faces list it. Two faces are in one PATCH when a chain of manifold edges
// joins them (boundary edges and edges of three or more faces join nothing); patches are numbered from 0 in the order of their smallest face.
// Two faces across a manifold edge AGREE when they run along it in opposite directions. In an orientable patch the smallest face keeps its
// row and every other face is kept or reversed, (a, b, c) -> (c, b, a), so that all agree: the result of a breadth-first search from the first
// face of each patch, and unique. A patch with no such assignment (a Moebius band) is returned unchanged and counted.
//   keys     one 64-bit key per face corner, lo << hb | hi of its undirected edge (hb = bits of the largest index); all ones for a face that
//            lists a vertex twice (no edge has lo == hi, so no edge's key has these low bits). One stable sort; the ids carry 3 i + corner.
//   unions   one thread per sorted position; the head of a run of exactly two keys acts. The union-find of components.h, unchanged, over the
//            DOUBLE COVER: element 2 i + o is face i as given (o = 0) or reversed (o = 1). With r = 1 if the two faces run along the edge
//            in the same direction, else 0, the edge unions (2 i, 2 j + r) and (2 i + 1, 2 j + (1 ^ r)). The root of a set is its smallest
//            element, so after the flatten, with m the smallest face of i's patch, parent[2 i] is 2 m or 2 m + 1: the low bit says whether i
//            is reversed, parent[2 i] >> 1 names the patch, and the patch is not orientable exactly when parent[2 m + 1] == 2 m -- then every
//            parent[2 i] of the patch is 2 m and every face keeps its row. The labels are those of a serial run whatever order the hooks
//            happen in. Every access to `parent` in the union launch goes through cc_find / cc_union (components.h: visibility).
//   labels   face i is a root when parent[2 i] == 2 i; the roots are flagged and scanned, and one kernel writes rows and patch numbers.
#pragma once
#include "components.h"

namespace pcu {

constexpr unsigned long long kMrNoEdge = ~0ull;

// ---------------------------------------------------------------------------------------------------- the shared step
// flag[i] = 1 where the mask keeps vertex i
__global__ __launch_bounds__(kBlock) void k_mr_mask_flags(const unsigned char* __restrict__ mask, unsigned nv, unsigned* __restrict__ flag) {
    const unsigned i = blockIdx.x * kBlock + threadIdx.x;
    if (i < nv) flag[i] = mask[i] ? 1u : 0u;
}
// One thread per face corner: ref[f[c]] = 1 (ref is zeroed before). An index outside [0, nv) raises the flag and stores nothing.
__global__ __launch_bounds__(kBlock) void k_mr_referenced(const void* __restrict__ f, int kind, unsigned ncorners, unsigned nv, unsigned* __restrict__ ref,
                                                          int* __restrict__ bad) {
    const unsigned c = blockIdx.x * kBlock + threadIdx.x;
    bool out = false;
    if (c < ncorners) {
        const unsigned long long a = index_in(f, kind, c);
        out = a >= nv;
        if (!out) ref[a] = 1u;
    }
    if (__ballot(out) != 0ull && (threadIdx.x & 63) == 0) atomicOr(bad, kMeshBadFace);
}
// scan: the inclusive scan of the keep flags. map[i] = the number of kept vertices before i, or -1.
__global__ __launch_bounds__(kBlock) void k_mr_map(const unsigned* __restrict__ flag, const unsigned* __restrict__ scan, unsigned nv, int* __restrict__ map) {
    const unsigned i = blockIdx.x * kBlock + threadIdx.x;
    if (i < nv) map[i] = flag[i] ? (int)(scan[i] - 1u) : -1;
}
// out_v[map[i]] = v[i] for the kept rows; corr_v[map[i]] = i and corr_f[i] = map[i] (both optional, in the integer type `kind` names: -1
// wraps for an unsigned one).
template <typename T>
__global__ __launch_bounds__(kBlock) void k_mr_rows(const T* __restrict__ v, const int* __restrict__ map, unsigned nv, T* __restrict__ out_v, int kind,
                                                    void* __restrict__ corr_v, void* __restrict__ corr_f) {
    const unsigned i = blockIdx.x * kBlock + threadIdx.x;
    if (i >= nv) return;
    const int m = map[i];
    if (corr_f) index_out_signed(corr_f, kind, i, m);
    if (m < 0) return;
    out_v[3 * (size_t)m] = v[3 * (size_t)i]; out_v[3 * (size_t)m + 1] = v[3 * (size_t)i + 1]; out_v[3 * (size_t)m + 2] = v[3 * (size_t)i + 2];
    if (corr_v) index_out(corr_v, kind, (size_t)m, i);
}
// One thread per face: keep[i] = 1 where every corner maps to a vertex (and, with `distinct`, to three different ones). A face with an index
// outside [0, nv) raises the flag and is not kept.
__global__ __launch_bounds__(kBlock) void k_mr_face_flags(const void* __restrict__ f, int kind, unsigned nf, unsigned nv, const int* __restrict__ map, int distinct,
                                                          unsigned* __restrict__ keep, int* __restrict__ bad) {
    const unsigned i = blockIdx.x * kBlock + threadIdx.x;
    bool out = false;
    if (i < nf) {
        int id[3];
        out = face_in(f, kind, (size_t)i, nv, id);
        bool k = false;
        if (!out) {
            const int ma = map[id[0]], mb = map[id[1]], mc = map[id[2]];
            k = ma >= 0 && mb >= 0 && mc >= 0 && !(distinct && (ma == mb || mb == mc || ma == mc));
        }
        keep[i] = k ? 1u : 0u;
    }
    if (__ballot(out) != 0ull && (threadIdx.x & 63) == 0) atomicOr(bad, kMeshBadFace);
}
// The kept faces with mapped indices, in input order. keep == nullptr: every face, in its own row. (A call with an index outside [0, nv) is
// refused before this launch; such a face would not be kept, and is passed by where all are.)
__global__ __launch_bounds__(kBlock) void k_mr_faces_out(const void* __restrict__ f, int kind, unsigned nf, unsigned nv, const int* __restrict__ map,
                                                         const unsigned* __restrict__ keep, const unsigned* __restrict__ scan, void* __restrict__ out_f) {
    const unsigned i = blockIdx.x * kBlock + threadIdx.x;
    if (i >= nf || (keep && !keep[i])) return;
    int id[3];
    if (face_in(f, kind, (size_t)i, nv, id)) return;
    const size_t r = keep ? (size_t)(scan[i] - 1u) : (size_t)i;
#pragma unroll
    for (int k = 0; k < 3; ++k) index_out(out_f, kind, 3 * r + k, (unsigned)map[id[k]]);
}

// ---------------------------------------------------------------------------------------------------- orient_mesh_faces
// One thread per face: the three corner keys. A face with an index outside [0, nv) raises the flag; it and a face that lists a vertex twice
// write kMrNoEdge three times.
__global__ __launch_bounds__(kBlock) void k_mr_edge_keys(const void* __restrict__ f, int kind, unsigned nf, unsigned nv, int hb, unsigned long long* __restrict__ keys,
                                                         int* __restrict__ bad) {
    const unsigned i = blockIdx.x * kBlock + threadIdx.x;
    bool out = false;
    if (i < nf) {
        int x[3];
        out = face_in(f, kind, (size_t)i, nv, x);
        const bool none = out || x[0] == x[1] || x[1] == x[2] || x[2] == x[0];
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            const unsigned long long a = (unsigned long long)x[k], b = (unsigned long long)x[(k + 1) % 3];
            keys[3 * (size_t)i + k] = none ? kMrNoEdge : ((a < b ? a : b) << hb) | (a < b ? b : a);
        }
    }
    if (__ballot(out) != 0ull && (threadIdx.x & 63) == 0) atomicOr(bad, kMeshBadFace);
}
// Does corner id (3 i + k) run from the smaller index of its edge to the larger one?
__device__ __forceinline__ bool mr_corner_ascends(const void* __restrict__ f, int kind, unsigned id) {
    const unsigned i = id / 3u, k = id - 3u * i;
    return index_in(f, kind, 3 * (size_t)i + k) < index_in(f, kind, 3 * (size_t)i + (k + 1u) % 3u);
}
// One thread per sorted position: the head of a run of exactly two equal keys, of two different faces, joins them in the double cover.
__global__ __launch_bounds__(kBlock) void k_mr_edge_unions(const unsigned long long* __restrict__ keys, const unsigned* __restrict__ ids, unsigned n,
                                                           const void* __restrict__ f, int kind, unsigned* parent) {
    const unsigned p = blockIdx.x * kBlock + threadIdx.x;
    if (p + 1u >= n) return;
    const unsigned long long key = keys[p];
    if (key == kMrNoEdge || keys[p + 1u] != key) return;
    if (p > 0u && keys[p - 1u] == key) return;
    if (p + 2u < n && keys[p + 2u] == key) return;
    const unsigned ca = ids[p], cb = ids[p + 1u], i = ca / 3u, j = cb / 3u;
    if (i == j) return;
    const unsigned r = mr_corner_ascends(f, kind, ca) == mr_corner_ascends(f, kind, cb) ? 1u : 0u;
    cc_union(parent, 2u * i, 2u * j + r);
    cc_union(parent, 2u * i + 1u, 2u * j + (1u ^ r));
}
// After the flatten of the 2 nf elements: root[i] = 1 where face i is the smallest of its patch; *twisted += the roots whose patch is not
// orientable (one add per wave that has any).
__global__ __launch_bounds__(kBlock) void k_mr_patch_roots(const unsigned* __restrict__ parent, unsigned nf, unsigned* __restrict__ root, unsigned* __restrict__ twisted) {
    const unsigned i = blockIdx.x * kBlock + threadIdx.x;
    bool tw = false;
    if (i < nf) {
        const bool is_root = parent[2 * (size_t)i] == 2u * i;
        root[i] = is_root ? 1u : 0u;
        tw = is_root && parent[2 * (size_t)i + 1] == 2u * i;
    }
    const unsigned long long b = __ballot(tw);
    if (b != 0ull && (threadIdx.x & 63) == 0) atomicAdd(twisted, (unsigned)__popcll(b));
}
// scan: the inclusive scan of the root flags. Row i as given or reversed, and the number of its patch.
__global__ __launch_bounds__(kBlock) void k_mr_orient_out(const void* __restrict__ f, int kind, unsigned nf, const unsigned* __restrict__ parent,
                                                          const unsigned* __restrict__ scan, void* __restrict__ out_f, void* __restrict__ out_c) {
    const unsigned i = blockIdx.x * kBlock + threadIdx.x;
    if (i >= nf) return;
    const unsigned p = parent[2 * (size_t)i], m = p >> 1;
    const bool rev = p & 1u;
    const unsigned a = (unsigned)index_in(f, kind, 3 * (size_t)i), b = (unsigned)index_in(f, kind, 3 * (size_t)i + 1), c = (unsigned)index_in(f, kind, 3 * (size_t)i + 2);
    index_out(out_f, kind, 3 * (size_t)i, rev ? c : a);
    index_out(out_f, kind, 3 * (size_t)i + 1, b);
    index_out(out_f, kind, 3 * (size_t)i + 2, rev ? a : c);
    index_out(out_c, kind, i, m < nf ? scan[m] - 1u : 0u);
}

}  // namespace pcu
