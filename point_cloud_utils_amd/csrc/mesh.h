// csrc/mesh.h -- closest_points_on_mesh: exact point-to-triangle-mesh distance.
//
// Replaces npe_function(closest_points_on_mesh) (src/closest_point_on_mesh.cpp:9-50), which calls igl::point_mesh_squared_distance (libigl's AABB
// tree). libigl's last bits cannot be reproduced, so the operator has a contract of its own that does not depend on the index:
//
//   per face   D2(q, a, b, c) -> (d2, v, w), all in the input type T, separate multiplies and adds, IEEE division:
//                the seven-region closest-point classification (Ericson, Real-Time Collision Detection, 5.1.5) with
//                dot(x, y) = (x0*y0 + x1*y1) + x2*y2, tested in the order vertex A, vertex B, edge AB, vertex C, edge AC, edge BC, interior;
//                an EDGE region is entered only if its denominator is > 0 (a collapsed edge falls through to the next region) and the interior
//                formula with a denominator that is not > 0 gives vertex A: a degenerate face behaves as the segment or point it is and no
//                finite input whose products stay finite gives NaN;
//                u = (1 - v) - w, closest = (u*a + v*b) + w*c, d2 = dot(q - closest, q - closest).
//   per query  the LOWEST face index among the faces of minimal d2 (exact equality), d = sqrt(d2) and bc = (u, v, w) of that face:
//                what a serial loop over all faces with a strict `<` returns.
//
// Index: a linear BVH. Faces are ordered by the 63-bit Morton code of their centroid in the bounding box of the referenced vertices (morton.h,
// radix.h), cut into leaves of kMeshLeaf consecutive faces, and an implicit balanced binary tree is laid over the leaves padded to a power
// of two P: node i has children 2i+1 and 2i+2, leaf j is node P-1+j, padding leaves have the empty box (+inf, -inf). The depth is log2 P <= 25
// whatever the data (thousands of faces with one code are no special case), so the traversal stack has a compile-time size. Boxes are made
// bottom-up, one launch per level: a level reads only what an earlier launch wrote, so no box crosses between workgroups inside a launch.
//
// Pruning that cannot change the result. Let e = eps(T), S = the largest absolute coordinate of a referenced vertex.
//   (1) the computed closest point x~ = (u*a + v*b) + w*c lies within 7 e S of the triangle in every coordinate: three products (e/2 S each), two
//       sums (e/2 * 2S, e/2 * 3S), u + v + w = 1 up to e (two roundings in u), u >= -e (tests/mesh_contract.py states and tests/test_mesh_contract.py
//       checks both). Leaf boxes are padded outward by 16 e S (the rest covers the rounding of the padding itself), so x~ is inside the padded box
//       of its leaf and of every ancestor, and |q - x~| >= D, the true distance from q to that box.
//   (2) the computed d2 = fl(|q - x~|^2) >= D^2 (1 - 3e); the computed box bound lb = fl(D^2) <= D^2 (1 + 3e) (one subtraction, one square, two sums).
//   So a node can hold the winner only if lb (1 - 16e) <= best (the factor 16 is generous against the 6e of (2) and the rounding of the product):
//   a node is skipped only if lb (1 - 16e) > best, and nodes whose bound EQUALS the best are visited, because a face of equal d2 and lower index wins.
#pragma once
#include "pcu_types.h"
#include "grid.h"
#include "morton.h"

namespace pcu {

constexpr int kMeshLeaf = 4;            // faces per leaf
constexpr int kMeshStack = 26;          // >= tree depth + 1 (P <= 2^25 leaves: 2^27 faces)
constexpr int kMeshBlock = 256;

template <typename T>
struct MeshHead {
    typename EncT<T>::type elo[3], ehi[3];      // bounding box of the referenced vertices, order-preserving encoding (atomics)
    int bad;                                    // kMeshBad*
    T lo[3], inv[3];                            // low corner; Morton cells (of 2^21) per unit length, 0 on a flat axis
    T pad;                                      // outward padding of every leaf box: 16 eps S
};
template <typename T>
struct MeshIdx {                                // device pointers of one index
    MeshHead<T>* head = nullptr;
    T* tri = nullptr;                           // (nf, 9): the faces' corners in Morton order (pc_winding.h: (nf, 6), a point and its dipole)
    unsigned* face = nullptr;                   // (nf): face index of every sorted position (pc_winding.h: null)
    T* box = nullptr;                           // (2P - 1, 6): lo[3], hi[3] of every node
    T* ctr = nullptr;                           // (2P - 1, 4): centre and radius of every node's expansion (mesh_winding.h); null unless asked for
    T* mom = nullptr;                           // (2P - 1, 30): its moments; null unless asked for
    int nf = 0, P = 0;                          // elements (faces; pc_winding.h: points) and leaves, padded to a power of two
};

// ---------------------------------------------------------------------------------------------------- build
template <typename T>
__global__ __launch_bounds__(kBlock) void k_mesh_vcheck(const T* __restrict__ v, long long count, int* __restrict__ bad, int bit) {
    const long long i = (long long)blockIdx.x * kBlock + threadIdx.x;
    bool nf = false;
    if (i < count) { const T x = v[i]; nf = !(x - x == (T)0); }
    if (__ballot(nf) != 0ull && (threadIdx.x & 63) == 0) atomicOr(bad, bit);
}
template <typename T>
__global__ void k_mesh_head_init(MeshHead<T>* h) {
    using E = typename EncT<T>::type;
    if (threadIdx.x < 3) { h->elo[threadIdx.x] = ~(E)0; h->ehi[threadIdx.x] = (E)0; }
    if (threadIdx.x == 0) h->bad = 0;
}
// Face indices of any of the four integer types (index_kinds.h) -> the index's own int32 triples, range-checked;
// and the bounding box of the vertices that faces refer to.
template <typename T>
__global__ __launch_bounds__(kBlock) void k_mesh_faces(const void* __restrict__ f, int kind, int nf, int nv, const T* __restrict__ v,
                                                       int* __restrict__ fidx, MeshHead<T>* __restrict__ h) {
    using E = typename EncT<T>::type;
    const int i = blockIdx.x * kBlock + threadIdx.x;
    E lo[3] = {~(E)0, ~(E)0, ~(E)0}, hi[3] = {(E)0, (E)0, (E)0};
    bool bad = false;
    if (i < nf) {
        int id[3];
        bad = face_in(f, kind, (size_t)i, (unsigned)nv, id);
        fidx[3 * (size_t)i] = id[0]; fidx[3 * (size_t)i + 1] = id[1]; fidx[3 * (size_t)i + 2] = id[2];
        if (!bad) {
#pragma unroll
            for (int j = 0; j < 3; ++j)
#pragma unroll
                for (int k = 0; k < 3; ++k) {
                    const E e = enc(v[3 * (size_t)id[j] + k]);
                    lo[k] = e < lo[k] ? e : lo[k]; hi[k] = e > hi[k] ? e : hi[k];
                }
        }
    }
#pragma unroll
    for (int k = 0; k < 3; ++k) {
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            const E a = (E)__shfl_xor(lo[k], o, 64), b = (E)__shfl_xor(hi[k], o, 64);
            lo[k] = a < lo[k] ? a : lo[k]; hi[k] = b > hi[k] ? b : hi[k];
        }
    }
    const bool any_bad = __ballot(bad) != 0ull;
    if ((threadIdx.x & 63) == 0) {
#pragma unroll
        for (int k = 0; k < 3; ++k) { atomicMin(&h->elo[k], lo[k]); atomicMax(&h->ehi[k], hi[k]); }
        if (any_bad) atomicOr(&h->bad, kMeshBadFace);
    }
}
template <typename T>
__global__ void k_mesh_frame(MeshHead<T>* h) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    T S = (T)0;
    for (int k = 0; k < 3; ++k) {
        const T lo = dec(h->elo[k]), hi = dec(h->ehi[k]);
        const T ext = hi - lo;
        h->lo[k] = lo;
        h->inv[k] = (ext > (T)0 && ext < Limits<T>::max_v) ? (T)2097152 / ext : (T)0;
        const T m = fabs(lo) > fabs(hi) ? fabs(lo) : fabs(hi);
        S = m > S ? m : S;
    }
    h->pad = (T)16 * Limits<T>::eps * S;
}
__device__ __forceinline__ unsigned mesh_cell(double t, unsigned top) { return t >= 0.0 ? (t < (double)top ? (unsigned)t : top) : 0u; }     // (NaN -> 0)
template <typename T>
__global__ __launch_bounds__(kBlock) void k_mesh_codes(const T* __restrict__ v, const int* __restrict__ fidx, int nf, const MeshHead<T>* __restrict__ h,
                                                       unsigned long long* __restrict__ keys) {
    const int i = blockIdx.x * kBlock + threadIdx.x;
    if (i >= nf) return;
    const int a = fidx[3 * (size_t)i], b = fidx[3 * (size_t)i + 1], c = fidx[3 * (size_t)i + 2];
    unsigned cell[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const double m = (((double)v[3 * (size_t)a + k] + (double)v[3 * (size_t)b + k]) + (double)v[3 * (size_t)c + k]) / 3.0;
        cell[k] = mesh_cell((m - (double)h->lo[k]) * (double)h->inv[k], 2097151u);
    }
    keys[i] = morton_split21(cell[0]) | morton_split21(cell[1]) << 1 | morton_split21(cell[2]) << 2;
}
template <typename T>
__global__ __launch_bounds__(kBlock) void k_mesh_gather(const T* __restrict__ v, const int* __restrict__ fidx, const unsigned* __restrict__ order, int nf,
                                                        T* __restrict__ tri, unsigned* __restrict__ face) {
    const int s = blockIdx.x * kBlock + threadIdx.x;
    if (s >= nf) return;
    const unsigned id = order[s];
    face[s] = id;
#pragma unroll
    for (int j = 0; j < 3; ++j) {
        const int r = fidx[3 * (size_t)id + j];
#pragma unroll
        for (int k = 0; k < 3; ++k) tri[9 * (size_t)s + 3 * j + k] = v[3 * (size_t)r + k];
    }
}
// leaf j = node P-1+j: the padded box of the sorted faces [kMeshLeaf j, kMeshLeaf (j + 1)); beyond the last face the empty box
template <typename T>
__global__ __launch_bounds__(kBlock) void k_mesh_leaves(const T* __restrict__ tri, int nf, int P, const MeshHead<T>* __restrict__ h, T* __restrict__ box) {
    const int j = blockIdx.x * kBlock + threadIdx.x;
    if (j >= P) return;
    T lo[3] = {(T)INFINITY, (T)INFINITY, (T)INFINITY}, hi[3] = {-(T)INFINITY, -(T)INFINITY, -(T)INFINITY};
    const T pad = h->pad;
    for (int t = 0; t < kMeshLeaf; ++t) {
        const long long s = (long long)kMeshLeaf * j + t;
        if (s >= nf) break;
        for (int c = 0; c < 3; ++c)
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                const T x = tri[9 * (size_t)s + 3 * c + k];
                lo[k] = x - pad < lo[k] ? x - pad : lo[k]; hi[k] = x + pad > hi[k] ? x + pad : hi[k];
            }
    }
    T* o = box + 6 * (size_t)(P - 1 + j);
#pragma unroll
    for (int k = 0; k < 3; ++k) { o[k] = lo[k]; o[3 + k] = hi[k]; }
}
// one level: the m nodes m-1 .. 2m-2 from their children (written by the launch before)
template <typename T>
__global__ __launch_bounds__(kBlock) void k_mesh_refit(T* __restrict__ box, int m) {
    const int i = blockIdx.x * kBlock + threadIdx.x;
    if (i >= m) return;
    const size_t node = (size_t)m - 1 + i;
    const T* l = box + 6 * (2 * node + 1);
    const T* r = l + 6;
    T* o = box + 6 * node;
#pragma unroll
    for (int k = 0; k < 3; ++k) { o[k] = l[k] < r[k] ? l[k] : r[k]; o[3 + k] = l[3 + k] > r[3 + k] ? l[3 + k] : r[3 + k]; }
}

// ---------------------------------------------------------------------------------------------------- queries
template <typename T> __device__ __forceinline__ bool mesh_finite3(const T* p) {
    return (p[0] - p[0] == (T)0) && (p[1] - p[1] == (T)0) && (p[2] - p[2] == (T)0);
}
// 30-bit Morton key of every query in the mesh's frame (clamped to it), so that the lanes of a wave walk the same nodes; non-finite rows are flagged
template <typename T>
__global__ __launch_bounds__(kBlock) void k_mesh_qcodes(const T* __restrict__ p, int np, const MeshHead<T>* __restrict__ h, unsigned long long* __restrict__ keys,
                                                        int* __restrict__ bad) {
    const int i = blockIdx.x * kBlock + threadIdx.x;
    bool nf = false;
    if (i < np) {
        nf = !mesh_finite3(p + 3 * (size_t)i);
        unsigned cell[3];
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            const T x = p[3 * (size_t)i + k];
            cell[k] = mesh_cell(((double)x - (double)h->lo[k]) * (double)h->inv[k] * (1.0 / 2048.0), 1023u);
        }
        keys[i] = morton_split21(cell[0]) | morton_split21(cell[1]) << 1 | morton_split21(cell[2]) << 2;
    }
    if (__ballot(nf) != 0ull && (threadIdx.x & 63) == 0) atomicOr(bad, 1);
}

template <typename T>
__device__ __forceinline__ T mesh_dot(const T x[3], const T y[3]) { return (x[0] * y[0] + x[1] * y[1]) + x[2] * y[2]; }

// D2 of the contract (head of this file). Every test is a positive one, so that a NaN from overflowing products falls through to vertex A.
template <typename T>
__device__ __forceinline__ void mesh_face_d2(const T q[3], const T a[3], const T b[3], const T c[3], T& d2, T& v, T& w) {
    T ab[3], ac[3], ap[3], bp[3], cp[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) { ab[k] = b[k] - a[k]; ac[k] = c[k] - a[k]; ap[k] = q[k] - a[k]; bp[k] = q[k] - b[k]; cp[k] = q[k] - c[k]; }
    const T d1 = mesh_dot(ab, ap), d2_ = mesh_dot(ac, ap), d3 = mesh_dot(ab, bp), d4 = mesh_dot(ac, bp), d5 = mesh_dot(ab, cp), d6 = mesh_dot(ac, cp);
    const T vc = d1 * d4 - d3 * d2_, vb = d5 * d2_ - d1 * d6, va = d3 * d6 - d5 * d4;
    const T e_ab = d1 - d3, e_ac = d2_ - d6, e_b = d4 - d3, e_c = d5 - d6, e_bc = e_b + e_c, den = (va + vb) + vc;
    v = (T)0; w = (T)0;
    if (d1 <= (T)0 && d2_ <= (T)0) { /* vertex A */ }
    else if (d3 >= (T)0 && d4 <= d3) { v = (T)1; }                                                      // vertex B
    else if (vc <= (T)0 && d1 >= (T)0 && d3 <= (T)0 && e_ab > (T)0) { v = d1 / e_ab; }                   // edge AB
    else if (d6 >= (T)0 && d5 <= d6) { w = (T)1; }                                                      // vertex C
    else if (vb <= (T)0 && d2_ >= (T)0 && d6 <= (T)0 && e_ac > (T)0) { w = d2_ / e_ac; }                 // edge AC
    else if (va <= (T)0 && e_b >= (T)0 && e_c >= (T)0 && e_bc > (T)0) { w = e_b / e_bc; v = (T)1 - w; }  // edge BC
    else if (den > (T)0) { v = vb / den; w = vc / den; }                                                // interior
    const T u = ((T)1 - v) - w;
    T r[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) r[k] = q[k] - ((u * a[k] + v * b[k]) + w * c[k]);
    d2 = mesh_dot(r, r);
}

// (1 - 16 eps) times the squared distance from q to a node's box, in T (see "Pruning" at the head of this file); +inf for the empty box
template <typename T>
__device__ __forceinline__ T mesh_bound(const T* __restrict__ bx, const T q[3]) {
    T d[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const T below = bx[k] - q[k], above = q[k] - bx[3 + k];
        const T m = below > above ? below : above;
        d[k] = m > (T)0 ? m : (T)0;
    }
    return mesh_dot(d, d) * ((T)1 - (T)16 * Limits<T>::eps);
}

template <typename T>
struct MeshQuery {
    const T* p; const unsigned* order; int np;
    MeshIdx<T> ix;
    T* out_d; long long* out_fi; T* out_bc;
    const unsigned* cancel_word; unsigned cancel_gen;          // pcu_types.h: cancel_seen
};

// The walk both operators share. One lane per row, rows in key order so that the lanes of a wave walk the same nodes. A Visitor is the lane's
// row and its best so far:
//   node(box, key) -> whether the node can still hold the winner (the operator's "Pruning" rule, against the best of that moment), and the key
//                     that orders two children (the lower one is taken first);
//   kLeaf             the elements of one leaf: sorted positions [kLeaf j, kLeaf (j + 1)) lie below leaf j;
//   element(ix, s)    evaluates the element at sorted position s. The mesh visitors fetch a face there (mesh_face_at) and hand it to their
//                     face(a, b, c, id), which keeps it if it beats the best; `id` points at its face index.
// The child with the lower key is taken first and the other pushed if it passes too: at most one entry per level, so the stack (LDS, one column
// per lane: a runtime-indexed private array would live in scratch memory) holds kMeshStack node ids. A popped node is tested again, against the
// best of that moment. `live` says whether the lane walks at all (the root is not tested here). Returns true if the call was cancelled: the
// caller then returns without writing its row. The leaf loop stays rolled: unrolled, it is a four times larger kernel for the point visitor.
// The element of the three mesh visitors: the face at sorted position s, 9 scalars, and its index.
template <typename T, typename Visitor>
__device__ __forceinline__ void mesh_face_at(Visitor& vis, const MeshIdx<T>& ix, long long s) {
    const T* __restrict__ tr = ix.tri + 9 * (size_t)s;
    const T fa[3] = {tr[0], tr[1], tr[2]}, fb[3] = {tr[3], tr[4], tr[5]}, fc[3] = {tr[6], tr[7], tr[8]};
    vis.face(fa, fb, fc, ix.face + s);
}
template <typename T, typename Visitor>
__device__ __forceinline__ bool mesh_walk(const MeshIdx<T>& ix, Visitor& vis, bool live, const unsigned* cancel_word, unsigned cancel_gen) {
    __shared__ int s_stack[kMeshStack][kMeshBlock];
    const T* __restrict__ box = ix.box;
    const int first_leaf = ix.P - 1, nf = ix.nf;
    int sp = 0, node = 0;
    unsigned steps = 0;
    long long t_poll = wall_clock64();
    while (live) {
        if ((++steps & 63u) == 0u) { const long long t_now = wall_clock64(); if (t_now - t_poll > 20000ll) { t_poll = t_now; if (cancel_seen(cancel_word, cancel_gen)) return true; } }
        bool descend = false;
        if (node >= first_leaf) {
            const long long s0 = (long long)Visitor::kLeaf * (node - first_leaf);
#pragma unroll 1
            for (int t = 0; t < Visitor::kLeaf; ++t) {
                const long long s = s0 + t;
                if (s >= nf) break;
                vis.element(ix, s);
            }
        } else {
            const int c0 = 2 * node + 1;
            T l0, l1;
            const bool v0 = vis.node(box + 6 * (size_t)c0, l0), v1 = vis.node(box + 6 * (size_t)c0 + 6, l1);
            if (v0 && v1) {
                const bool left_first = l0 <= l1;
                s_stack[sp++][threadIdx.x] = left_first ? c0 + 1 : c0;
                node = left_first ? c0 : c0 + 1;
                descend = true;
            } else if (v0 || v1) {
                node = v0 ? c0 : c0 + 1;
                descend = true;
            }
        }
        if (descend) continue;
        live = false;
        while (sp > 0) {
            const int n = s_stack[--sp][threadIdx.x];
            T key;
            if (vis.node(box + 6 * (size_t)n, key)) { node = n; live = true; break; }
        }
    }
    return false;
}

// The best so far of both visitors: the winning value (d2 or t), its face and that face's last two barycentric coordinates
template <typename T>
struct MeshBest { T best = (T)INFINITY, bv = (T)0, bw = (T)0; unsigned bf = 0xffffffffu; };

template <typename T>
struct MeshPointVisitor : MeshBest<T> {         // lexicographic (d2, face); a node whose bound EQUALS the best is visited
    T q[3];
    static constexpr int kLeaf = kMeshLeaf;
    __device__ __forceinline__ void element(const MeshIdx<T>& ix, long long s) { mesh_face_at(*this, ix, s); }
    __device__ __forceinline__ bool node(const T* __restrict__ bx, T& key) const { key = mesh_bound(bx, q); return key <= this->best; }
    __device__ __forceinline__ void face(const T a[3], const T b[3], const T c[3], const unsigned* __restrict__ pid) {
        T d2, v, w;
        mesh_face_d2(q, a, b, c, d2, v, w);
        const unsigned id = *pid;
        if (d2 < this->best || (d2 == this->best && id < this->bf)) { this->best = d2; this->bf = id; this->bv = v; this->bw = w; }
    }
};

// One query per lane (mesh_walk). The root is not box-tested: every finite query has a closest face.
template <typename T>
__global__ __launch_bounds__(kMeshBlock) void k_mesh_closest(const MeshQuery<T> a) {
    const int i = blockIdx.x * kMeshBlock + threadIdx.x;
    if (i >= a.np) return;
    const unsigned row = a.order[i];
    MeshPointVisitor<T> vis;
    vis.q[0] = a.p[3 * (size_t)row]; vis.q[1] = a.p[3 * (size_t)row + 1]; vis.q[2] = a.p[3 * (size_t)row + 2];
    if (mesh_walk(a.ix, vis, mesh_finite3(vis.q), a.cancel_word, a.cancel_gen)) return;     // (a non-finite row is refused by the host after the launch)
    const T u = ((T)1 - vis.bv) - vis.bw;
    a.out_d[row] = sqrt(vis.best);
    a.out_fi[row] = vis.bf == 0xffffffffu ? -1ll : (long long)vis.bf;
    a.out_bc[3 * (size_t)row] = u; a.out_bc[3 * (size_t)row + 1] = vis.bv; a.out_bc[3 * (size_t)row + 2] = vis.bw;
}

// ---------------------------------------------------------------------------------------------------- rays
// ray_mesh_intersection: replaces npe_function(ray_mesh_intersection) (src/ray_mesh_intersection.cpp:107-177, Embree through libigl, always in
// float32). Embree's bits cannot be reproduced, so the operator has a contract of its own that does not depend on the index. All arithmetic in
// T, separate multiplies and adds, IEEE division; S as above.
//   per ray    kz = the dominant axis of d (0 if |d0| >= |d1| and |d0| >= |d2|, else 1 if |d1| >= |d2|, else 2), kx = (kz+1)%3, ky = (kx+1)%3,
//              kx and ky swapped if d[kz] < 0; Sx = d[kx]/d[kz], Sy = d[ky]/d[kz], Sz = 1/d[kz]; inv[k] = 1/d[k];
//              pad = max(16 eps S, 16 eps max_k |o[k]|)
//   per face   HIT(ray, a, b, c) -> (hit, t, b1, b2):
//              1 the watertight test (Woop, Benthin, Wald, JCGT 2013, without its double-precision fallback): A = a - o (B, C alike),
//                Ax = A[kx] - Sx*A[kz], Ay = A[ky] - Sy*A[kz], Az = Sz*A[kz]; U = Cx*By - Cy*Bx, V = Ax*Cy - Ay*Cx, W = Bx*Ay - By*Ax;
//                reject if (U<0 || V<0 || W<0) && (U>0 || V>0 || W>0); det = (U+V)+W, reject if det == 0;
//                t = ((U*Az + V*Bz) + W*Cz)/det, b1 = V/det, b2 = W/det
//              2 the window: accept only if t >= near && t <= far
//              3 the box clip: (t_in, t_out) = BOX(o, inv, min(a,b,c) - pad, max(a,b,c) + pad); accept only if t_in <= t && t <= t_out
//              BOX per axis: t1 = (lo[k]-o[k])*inv[k], t2 = (hi[k]-o[k])*inv[k]; t_in = fmax over k of fmin(t1,t2), t_out = fmin over k of fmax(t1,t2)
//   per ray    the smallest accepted t, the LOWEST face index among equal t; hit: face, bc = ((1-b1)-b2, b1, b2), t; miss: -1, 0, +inf.
// The edge function of a directed edge is the same two products whichever face evaluates it and, without FMA, its exact negation for the
// reversed edge: a ray through a shared edge or vertex cannot slip between two faces.
// Pruning that cannot change the result: rounded subtraction, multiplication, fmin and fmax are monotone, so BOX is monotone in its box. A
// face's clip box lies inside (node box - pad, node box + pad) of every node that holds it (node boxes are the faces' boxes padded by 16 eps S
// already), so a face step 3 accepts at t has t_in(node) <= t <= t_out(node): a node is skipped only if !(t_in <= min(far, best)) ||
// !(t_out >= near) || !(t_in <= t_out), or if it is a padding node (the empty box). A node whose t_in EQUALS the best t is visited.
constexpr int kMeshBadOrigin = 1, kMeshBadDir = 2;

// Sort key of every ray, so that the lanes of a wave walk the same nodes: the 7-bit-per-axis Morton cell of the point where the ray enters the
// mesh's bounding box (the origin if it is inside; a ray that misses the box gets the cell of a clamped point), then 11 bits of direction
// (dominant axis and sign, the other two components over the dominant one in 16 steps each). Results do not depend on it. Non-finite rows
// are flagged. o_stride is 0 (one origin for all rays) or 3.
template <typename T>
__global__ __launch_bounds__(kBlock) void k_mesh_rkeys(const T* __restrict__ o, int o_stride, const T* __restrict__ d, int n, const MeshHead<T>* __restrict__ h,
                                                       unsigned long long* __restrict__ keys, int* __restrict__ bad) {
    const int i = blockIdx.x * kBlock + threadIdx.x;
    bool bad_o = false, bad_d = false;
    if (i < n) {
        const T* po = o + (size_t)o_stride * i;
        const T* pd = d + 3 * (size_t)i;
        bad_o = !mesh_finite3(po); bad_d = !mesh_finite3(pd);
        const double oo[3] = {(double)po[0], (double)po[1], (double)po[2]}, dd[3] = {(double)pd[0], (double)pd[1], (double)pd[2]};
        double t_in = 0.0;
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            const double inv = 1.0 / dd[k];
            const double t1 = ((double)dec(h->elo[k]) - oo[k]) * inv, t2 = ((double)dec(h->ehi[k]) - oo[k]) * inv;
            t_in = fmax(t_in, fmin(t1, t2));
        }
        unsigned cell[3];
#pragma unroll
        for (int k = 0; k < 3; ++k) cell[k] = mesh_cell(((oo[k] + t_in * dd[k]) - (double)h->lo[k]) * (double)h->inv[k] * (1.0 / 16384.0), 127u);
        const double a0 = fabs(dd[0]), a1 = fabs(dd[1]), a2 = fabs(dd[2]);
        const int kz = (a0 >= a1 && a0 >= a2) ? 0 : (a1 >= a2 ? 1 : 2);
        const double dz = kz == 0 ? dd[0] : (kz == 1 ? dd[1] : dd[2]), du = kz == 0 ? dd[1] : (kz == 1 ? dd[2] : dd[0]), dv = kz == 0 ? dd[2] : (kz == 1 ? dd[0] : dd[1]);
        const double s = 8.0 / fabs(dz);
        const unsigned dir = ((unsigned)kz * 2u + (dz < 0.0 ? 1u : 0u)) << 8 | mesh_cell(du * s + 8.0, 15u) << 4 | mesh_cell(dv * s + 8.0, 15u);
        keys[i] = (morton_split21(cell[0]) | morton_split21(cell[1]) << 1 | morton_split21(cell[2]) << 2) << 11 | dir;
    }
    const unsigned long long any_o = __ballot(bad_o), any_d = __ballot(bad_d);
    if ((any_o | any_d) != 0ull && (threadIdx.x & 63) == 0) atomicOr(bad, (any_o ? kMeshBadOrigin : 0) | (any_d ? kMeshBadDir : 0));
}
constexpr int kMeshRayKeyBits = 32;

template <typename T>
struct MeshRay {                                // one ray, its axes already permuted: x, y the sheared axes, z the dominant one
    T o[3], inv[3];                             // origin and slab reciprocals, in the caller's axis order
    T ox, oy, oz, Sx, Sy, Sz, pad, near, far;
    int kx, ky, kz;
};
template <typename T> __device__ __forceinline__ T mesh_pick(const T* p, int k) { return k == 0 ? p[0] : (k == 1 ? p[1] : p[2]); }
// "per ray" of the contract: the ray of origin o and direction d, on a mesh whose leaf boxes are padded by pad_s
template <typename T>
__device__ __forceinline__ void mesh_ray_setup(MeshRay<T>& r, const T* o, const T d[3], T pad_s, T near, T far) {
    r.o[0] = o[0]; r.o[1] = o[1]; r.o[2] = o[2];
    const T a0 = fabs(d[0]), a1 = fabs(d[1]), a2 = fabs(d[2]);
    r.kz = (a0 >= a1 && a0 >= a2) ? 0 : (a1 >= a2 ? 1 : 2);
    r.kx = r.kz == 2 ? 0 : r.kz + 1;
    r.ky = r.kx == 2 ? 0 : r.kx + 1;
    const T dz = mesh_pick(d, r.kz);
    if (dz < (T)0) { const int k = r.kx; r.kx = r.ky; r.ky = k; }
    r.Sx = mesh_pick(d, r.kx) / dz; r.Sy = mesh_pick(d, r.ky) / dz; r.Sz = (T)1 / dz;
    r.ox = mesh_pick(r.o, r.kx); r.oy = mesh_pick(r.o, r.ky); r.oz = mesh_pick(r.o, r.kz);
#pragma unroll
    for (int k = 0; k < 3; ++k) r.inv[k] = (T)1 / d[k];
    T m = fabs(r.o[0]) > fabs(r.o[1]) ? fabs(r.o[0]) : fabs(r.o[1]);
    m = m > fabs(r.o[2]) ? m : fabs(r.o[2]);
    const T pad_o = (T)16 * Limits<T>::eps * m;
    r.pad = pad_s > pad_o ? pad_s : pad_o;
    r.near = near; r.far = far;
}

// BOX of the contract for the box (lo - pad, hi + pad)
template <typename T>
__device__ __forceinline__ void mesh_ray_box(const MeshRay<T>& r, const T lo[3], const T hi[3], T& t_in, T& t_out) {
    T n[3], f[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const T t1 = ((lo[k] - r.pad) - r.o[k]) * r.inv[k], t2 = ((hi[k] + r.pad) - r.o[k]) * r.inv[k];
        n[k] = fmin(t1, t2); f[k] = fmax(t1, t2);
    }
    t_in = fmax(fmax(n[0], n[1]), n[2]); t_out = fmin(fmin(f[0], f[1]), f[2]);
}
// whether a node can hold a face that beats `best` (see "Pruning" above); t_in orders the children
template <typename T>
__device__ __forceinline__ bool mesh_ray_node(const MeshRay<T>& r, const T* __restrict__ bx, T best, T& t_in) {
    const T lo[3] = {bx[0], bx[1], bx[2]}, hi[3] = {bx[3], bx[4], bx[5]};
    T t_out;
    mesh_ray_box(r, lo, hi, t_in, t_out);
    const T lim = r.far < best ? r.far : best;
    return lo[0] <= hi[0] && t_in <= lim && t_out >= r.near && t_in <= t_out;
}
// HIT of the contract
template <typename T>
__device__ __forceinline__ bool mesh_ray_face(const MeshRay<T>& r, const T a[3], const T b[3], const T c[3], T& t, T& b1, T& b2) {
    const T Az_ = mesh_pick(a, r.kz) - r.oz, Bz_ = mesh_pick(b, r.kz) - r.oz, Cz_ = mesh_pick(c, r.kz) - r.oz;
    const T Ax = (mesh_pick(a, r.kx) - r.ox) - r.Sx * Az_, Ay = (mesh_pick(a, r.ky) - r.oy) - r.Sy * Az_;
    const T Bx = (mesh_pick(b, r.kx) - r.ox) - r.Sx * Bz_, By = (mesh_pick(b, r.ky) - r.oy) - r.Sy * Bz_;
    const T Cx = (mesh_pick(c, r.kx) - r.ox) - r.Sx * Cz_, Cy = (mesh_pick(c, r.ky) - r.oy) - r.Sy * Cz_;
    const T U = Cx * By - Cy * Bx, V = Ax * Cy - Ay * Cx, W = Bx * Ay - By * Ax;
    const T z = (T)0;
    if ((U < z || V < z || W < z) && (U > z || V > z || W > z)) return false;
    const T det = (U + V) + W;
    if (det == z) return false;
    const T Az = r.Sz * Az_, Bz = r.Sz * Bz_, Cz = r.Sz * Cz_;
    t = ((U * Az + V * Bz) + W * Cz) / det;
    if (!(t >= r.near && t <= r.far)) return false;
    T lo[3], hi[3], t_in, t_out;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const T m = a[k] < b[k] ? a[k] : b[k], M = a[k] > b[k] ? a[k] : b[k];
        lo[k] = m < c[k] ? m : c[k]; hi[k] = M > c[k] ? M : c[k];
    }
    mesh_ray_box(r, lo, hi, t_in, t_out);
    if (!(t_in <= t && t <= t_out)) return false;
    b1 = V / det; b2 = W / det;
    return true;
}

template <typename T>
struct MeshRays {
    const T* o; int o_stride; const T* d; const unsigned* order; int n;
    MeshIdx<T> ix;
    T near, far;
    long long* out_fi; T* out_bc; T* out_t;
    const unsigned* cancel_word; unsigned cancel_gen;          // pcu_types.h: cancel_seen
};

template <typename T>
struct MeshRayVisitor : MeshBest<T> {           // the smallest accepted t, the lowest face among equal t; a node whose t_in EQUALS the best is visited
    MeshRay<T> r;
    static constexpr int kLeaf = kMeshLeaf;
    __device__ __forceinline__ void element(const MeshIdx<T>& ix, long long s) { mesh_face_at(*this, ix, s); }
    __device__ __forceinline__ bool node(const T* __restrict__ bx, T& key) const { return mesh_ray_node(r, bx, this->best, key); }
    __device__ __forceinline__ void face(const T a[3], const T b[3], const T c[3], const unsigned* __restrict__ pid) {
        T t, b1, b2;
        if (!mesh_ray_face(r, a, b, c, t, b1, b2)) return;
        const unsigned id = *pid;
        if (t < this->best || (t == this->best && id < this->bf && t < (T)INFINITY)) { this->best = t; this->bf = id; this->bv = b1; this->bw = b2; }
    }
};

// One ray per lane (mesh_walk). The root is box-tested before the walk: a ray that misses the mesh's box visits nothing.
template <typename T>
__global__ __launch_bounds__(kMeshBlock) void k_mesh_rays(const MeshRays<T> a) {
    const int i = blockIdx.x * kMeshBlock + threadIdx.x;
    if (i >= a.n) return;
    const unsigned row = a.order[i];
    const T* po = a.o + (size_t)a.o_stride * row;
    const T* pd = a.d + 3 * (size_t)row;
    const T d[3] = {pd[0], pd[1], pd[2]};
    MeshRayVisitor<T> vis;
    mesh_ray_setup(vis.r, po, d, a.ix.head->pad, a.near, a.far);
    T t_in;
    const bool live = mesh_finite3(vis.r.o) && mesh_finite3(d) && vis.node(a.ix.box, t_in);     // (a non-finite row is refused by the host after the launch)
    if (mesh_walk(a.ix, vis, live, a.cancel_word, a.cancel_gen)) return;
    const bool hit = vis.bf != 0xffffffffu;
    a.out_t[row] = hit ? vis.best : (T)INFINITY;
    a.out_fi[row] = hit ? (long long)vis.bf : -1ll;
    a.out_bc[3 * (size_t)row] = hit ? ((T)1 - vis.bv) - vis.bw : (T)0; a.out_bc[3 * (size_t)row + 1] = hit ? vis.bv : (T)0; a.out_bc[3 * (size_t)row + 2] = hit ? vis.bw : (T)0;
}

}  // namespace pcu
