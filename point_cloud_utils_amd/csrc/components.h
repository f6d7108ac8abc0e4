// csrc/components.h -- connected_components and flood_fill_3d (src/connected_components.cpp:11-110, src/flood_fill_3d.cpp:10-75): one
// lock-free union-find, its kernels and the two operators' contract. Host side: components_host.h.
//
// The core. `parent` holds one uint32 per element (vertex, or grid cell). parent[x] <= x at all times and a parent only ever decreases, so
// every value a thread can read from parent[x] -- the current one or a stale one -- is an ancestor of x or x itself. A root is an x with
// parent[x] == x; two trees are joined by hooking the LARGER root under the smaller one with atomicCAS(&parent[hi], hi, lo), so the root of
// a finished tree is the smallest index of its component whatever order the hooks happened in: racing blocks give the labels of a serial
// run. A failed CAS means that another thread has lowered parent[hi] meanwhile; the union goes on from the value the CAS returned. Every
// loop walks strictly downwards in index, so it ends by itself: no thread waits for another wave or workgroup, there is no flag, no ticket
// and no grid-wide barrier.
// Visibility (the chip has eight L2s that are not coherent with each other, and a CU's L1 is never refreshed by another CU's stores): in the
// union launches every write to `parent` is an atomic (the hook, and path halving as an atomicMin) and every read of it is a relaxed
// agent-scope atomic load, which is served past the L1. The parents those launches start from were written by an earlier launch, and what
// they leave is read by later ones (flatten, ranks, labels).
//
// connected_components: two vertices are connected when a face lists both. One thread per face unions (f0, f1) and (f1, f2); after the flatten
// parent[x] is the smallest vertex of x's component, the roots are flagged and scanned, and component r (counted from 0 in the order of the
// smallest vertices: the order the reference's outer loop meets them) is the r-th root. A vertex no face lists is a component of its own.
// The per-component counts are integer atomic adds -- order-independent, so equal inputs give equal bytes -- one per run of equal labels
// within a wave.
//
// flood_fill_3d: cells are numbered x * h * d + y * d + z (z fastest: consecutive lanes read consecutive cells). A cell takes part iff its
// value == the seed's (C++'s ==: -0.0 equals 0.0, a NaN seed equals nothing). Taking part, it is joined with its -z, -y and -x neighbours
// that take part too: the six face neighbours INSIDE the grid (the reference's offset arithmetic makes (x, y, d-1) a neighbour of
// (x, y+1, 0); that is not reproduced). The init launch writes, instead of parent[i] = i, the first lane of the run of consecutive
// participating lanes of the same z row that lane i lies in (a ballot and a leading-zero count: no atomics along z); the union launch joins
// the first lane of a wave with its -z neighbour, and a cell with its -y / -x neighbour unless its -z neighbour takes part and has that
// neighbour too (then that cell's union, or the one it relies on, already covers this one: the two pairs are joined along z). After the
// flatten the cells whose root is the seed's are written as the fill value. Four launches whatever the region's shape or diameter.
#pragma once
#include "pcu_types.h"
#include "grid.h"

namespace pcu {

constexpr long long kCcMaxIndex = 0x7ffffff0ll;         // elements of one parent array: 32-bit indices

// ---------------------------------------------------------------------------------------------------- the core
__device__ __forceinline__ unsigned cc_load(const unsigned* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

// The root of x as far as this thread can see it, with path halving: parent[x] is lowered to its grandparent on the way.
__device__ __forceinline__ unsigned cc_find(unsigned* parent, unsigned x) {
    for (;;) {
        const unsigned p = cc_load(parent + x);
        if (p == x) return x;
        const unsigned g = cc_load(parent + p);
        if (g == p) return p;
        atomicMin(parent + x, g);
        x = g;
    }
}
// The same walk without a write: for launches in which `parent` is not hooked any more.
__device__ __forceinline__ unsigned cc_root(const unsigned* parent, unsigned x) {
    for (;;) {
        const unsigned p = cc_load(parent + x);
        if (p == x) return x;
        x = p;
    }
}
__device__ __forceinline__ void cc_union(unsigned* parent, unsigned a, unsigned b) {
    a = cc_find(parent, a);
    b = cc_find(parent, b);
    while (a != b) {
        const unsigned hi = a > b ? a : b, lo = a > b ? b : a;
        const unsigned seen = atomicCAS(parent + hi, hi, lo);
        if (seen == hi) return;
        a = cc_find(parent, seen);              // hi has a parent by now (seen < hi): go on from there
        b = lo;
    }
}

__global__ __launch_bounds__(kBlock) void k_cc_init(unsigned* __restrict__ parent, unsigned n) {
    const unsigned i = blockIdx.x * kBlock + threadIdx.x;
    if (i < n) parent[i] = i;
}
// parent[x] = root of x, for all x. Another thread of this launch may read parent[x] before or after this store: either value is an
// ancestor of x. flag (optional): 1 for a root.
__global__ __launch_bounds__(kBlock) void k_cc_flatten(unsigned* parent, unsigned n, unsigned* __restrict__ flag) {
    const unsigned i = blockIdx.x * kBlock + threadIdx.x;
    if (i >= n) return;
    const unsigned r = cc_root(parent, i);
    parent[i] = r;
    if (flag) flag[i] = r == i ? 1u : 0u;
}

// ---------------------------------------------------------------------------------------------------- connected_components
// One thread per face: (f0, f1) and (f1, f2); the third edge follows. A face with an index outside [0, nv) raises the flag and joins nothing.
__global__ __launch_bounds__(kBlock) void k_cc_faces(const void* __restrict__ f, int kind, unsigned nf, unsigned nv, unsigned* parent, int* __restrict__ bad) {
    const unsigned i = blockIdx.x * kBlock + threadIdx.x;
    bool out = false;
    if (i < nf) {
        int id[3];
        out = face_in(f, kind, (size_t)i, nv, id);
        if (!out) {
            if (id[0] != id[1]) cc_union(parent, (unsigned)id[0], (unsigned)id[1]);
            if (id[1] != id[2]) cc_union(parent, (unsigned)id[1], (unsigned)id[2]);
        }
    }
    if (__ballot(out) != 0ull && (threadIdx.x & 63) == 0) atomicOr(bad, kMeshBadFace);
}
// cnt[label] += 1 for every active lane, as one add per run of equal labels among consecutive lanes. The active lanes are the wave's first ones.
__device__ __forceinline__ void cc_count(unsigned label, bool active, unsigned* __restrict__ cnt) {
    const int lane = threadIdx.x & 63;
    const unsigned before = __shfl_up(label, 1, 64);
    const bool head = active && (lane == 0 || before != label);
    const unsigned long long heads = __ballot(head), act = __ballot(active);
    if (!head) return;
    const unsigned long long above = heads & ~((2ull << lane) - 1ull);
    const int next = above ? __ffsll((long long)above) - 1 : __popcll(act);
    atomicAdd(cnt + label, (unsigned)(next - lane));
}
// scan: the inclusive scan of the root flags. cv[i] = rank of i's root.
__global__ __launch_bounds__(kBlock) void k_cc_vertex_labels(const unsigned* __restrict__ parent, const unsigned* __restrict__ scan, unsigned nv, int kind,
                                                             void* __restrict__ out_cv, unsigned* __restrict__ cnt) {
    const unsigned i = blockIdx.x * kBlock + threadIdx.x;
    unsigned label = 0;
    if (i < nv) { label = scan[parent[i]] - 1u; index_out(out_cv, kind, i, label); }
    cc_count(label, i < nv, cnt);
}
// cf[i] = cv[f[i, 0]]
__global__ __launch_bounds__(kBlock) void k_cc_face_labels(const void* __restrict__ f, int kind, unsigned nf, unsigned nv, const unsigned* __restrict__ parent,
                                                           const unsigned* __restrict__ scan, void* __restrict__ out_cf, unsigned* __restrict__ cnt) {
    const unsigned i = blockIdx.x * kBlock + threadIdx.x;
    unsigned label = 0;
    if (i < nf) {
        const unsigned long long a = index_in(f, kind, 3 * (size_t)i);
        if (a < nv) label = scan[parent[a]] - 1u;             // (a call with an index outside [0, nv) is refused before this launch)
        index_out(out_cf, kind, i, label);
    }
    cc_count(label, i < nf, cnt);
}
__global__ __launch_bounds__(kBlock) void k_cc_counts_out(const unsigned* __restrict__ cnt_v, const unsigned* __restrict__ cnt_f, unsigned count, int kind,
                                                          void* __restrict__ out_nv, void* __restrict__ out_nf) {
    const unsigned i = blockIdx.x * kBlock + threadIdx.x;
    if (i >= count) return;
    index_out(out_nv, kind, i, cnt_v[i]);
    index_out(out_nf, kind, i, cnt_f[i]);
}

// ---------------------------------------------------------------------------------------------------- flood_fill_3d
// parent[i] = the first lane's cell of the run of participating lanes of one z row that lane i lies in; i itself for a cell that takes no part.
template <typename V>
__global__ __launch_bounds__(kBlock) void k_fill_init(const V* __restrict__ in, unsigned n, unsigned d, unsigned seed, unsigned* __restrict__ parent) {
    const unsigned i = blockIdx.x * kBlock + threadIdx.x;
    const int lane = threadIdx.x & 63;
    const V sv = in[seed];
    const bool part = i < n && in[i] == sv;
    const bool before = __shfl_up((int)part, 1, 64) != 0;
    const bool link = part && before && lane > 0 && i % d != 0u;            // lane - 1 holds the -z neighbour, and it takes part
    const unsigned long long links = __ballot(link);
    const unsigned long long open = ~links & ((2ull << lane) - 1ull);       // the lanes up to this one that start a run (lane 0 always does)
    const int head = 63 - __clzll((long long)open);
    if (i < n) parent[i] = i - (unsigned)(lane - head);                     // (head == lane unless `link`)
}
template <typename V>
__global__ __launch_bounds__(kBlock) void k_fill_union(const V* __restrict__ in, unsigned n, unsigned h, unsigned d, unsigned seed, unsigned* parent) {
    const unsigned i = blockIdx.x * kBlock + threadIdx.x;
    if (i >= n) return;
    const V sv = in[seed];
    if (!(in[i] == sv)) return;
    const unsigned row = i / d, z = i - row * d, hd = h * d;
    const bool pz = z != 0u && in[i - 1u] == sv;
    if (pz && (threadIdx.x & 63) == 0) cc_union(parent, i, i - 1u);         // a run that goes on across the wave's boundary
    if (row % h != 0u && in[i - d] == sv && !(pz && in[i - 1u - d] == sv)) cc_union(parent, i, i - d);
    if (row >= h && in[i - hd] == sv && !(pz && in[i - 1u - hd] == sv)) cc_union(parent, i, i - hd);
}
// out = fill where the cell takes part and its root is the seed's, else in; *count += the cells written as fill. A block walks the grid in
// trips of kFillTrip cells, at most kFillMaxBlocks blocks in all, and every wave adds its total to *count once: one add per wave of a
// launch with one cell per thread is two million adds to one address for a 512^3 grid, and they took 22 of that call's 25 ms.
constexpr int kFillItems = 8, kFillTrip = kBlock * kFillItems;
constexpr unsigned kFillMaxBlocks = 4096;
template <typename V>
__global__ __launch_bounds__(kBlock) void k_fill_write(const V* __restrict__ in, V* __restrict__ out, unsigned n, unsigned seed, const unsigned* __restrict__ parent,
                                                       V fill, unsigned long long* __restrict__ count) {
    const V sv = in[seed];
    const unsigned root = parent[seed];
    unsigned hits = 0;                              // of this wave (the same value in every lane)
    for (unsigned long long base = (unsigned long long)blockIdx.x * kFillTrip; base < n; base += (unsigned long long)gridDim.x * kFillTrip) {
        V x[kFillItems]; unsigned p[kFillItems];
#pragma unroll
        for (int k = 0; k < kFillItems; ++k) {
            const unsigned long long i = base + (unsigned)(k * kBlock) + threadIdx.x;
            if (i < n) x[k] = in[i];
        }
#pragma unroll
        for (int k = 0; k < kFillItems; ++k) {
            const unsigned long long i = base + (unsigned)(k * kBlock) + threadIdx.x;
            p[k] = ~root;
            if (i < n && x[k] == sv) p[k] = parent[i];
        }
#pragma unroll
        for (int k = 0; k < kFillItems; ++k) {
            const unsigned long long i = base + (unsigned)(k * kBlock) + threadIdx.x;
            const bool hit = p[k] == root;
            if (i < n) out[i] = hit ? fill : x[k];
            hits += (unsigned)__popcll(__ballot(hit));
        }
    }
    if (hits != 0u && (threadIdx.x & 63) == 0) atomicAdd(count, (unsigned long long)hits);
}

}  // namespace pcu
