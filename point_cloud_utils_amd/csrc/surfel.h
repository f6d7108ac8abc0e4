// csrc/surfel.h -- ray_surfel_intersection and pointcloud_surfel_geometry.
//
// Replaces src/ray_point_cloud_intersection.cpp ("circle" geometry): every point becomes a fan of `subdivs` triangles, a regular polygon
// inscribed in a disc of radius r perpendicular to the normal, and the reference hands that triangle soup to Embree. Here the fan is never
// materialised for the rays: the tree is over points, and a leaf's points are expanded into their triangles in registers. The operator is
// "the ray contract (f7, mesh.h) applied to a stated fan geometry", bit for bit. All arithmetic in the input type T, separate multiplies and
// adds, IEEE division and square root, dot as in mesh.h, cross(a, b) = (a1*b2 - a2*b1, a2*b0 - a0*b2, a0*b1 - a1*b0).
//
//   table      c_j = cos(6.283185307179586 * j / subdivs), s_j = sin(...) for j in [0, subdivs): computed by the host in double with the C
//              library, rounded to T once and read from a buffer (c_0, s_0, c_1, s_1, ...). No device code calls cos or sin.
//   per point  with p, n, r its position, normal and radius: l = sqrt(dot(n, n)); ni = n / l component by component, or 0 if l == 0;
//              e = (1,0,0) if fabs(fabs(ni[1]) - 1) < (T)1e-5, else (0,1,0); right0 = cross(ni, e), right = right0 / |right0| (0 if that
//              length is 0); up0 = cross(ni, right), up = up0 / |up0| (or 0); A = r * right, B = r * up (three products each).
//              Rim vertex j = (c_j * A + s_j * B) + p per component; the centre vertex is p.
//   geometry   point i owns vertices [i (subdivs + 1), (i + 1)(subdivs + 1)): the rim vertices 0 .. subdivs-1, then the centre; and faces
//              [i subdivs, (i + 1) subdivs): face j = (centre, rim j, rim (j + 1) % subdivs).
//   rays       (pid, t) of a ray = (f_id / subdivs, t) of the f7 contract on that geometry (S = the largest absolute coordinate of a
//              generated vertex); misses give (-1, +inf). Among equal t the lowest pid wins. A zero normal, a normal whose squared length
//              underflows to 0 and r == 0 give a fan without area, which is never hit; a negative r is the same disc.
//
// Index: the linear BVH of mesh.h over points. MeshIdx::tri holds (np, 9) rows (p, A, B) in the order of the 63-bit Morton code of p,
// MeshIdx::face the point's row; a leaf of kSurfelLeaf points has the box of its points' generated vertices, padded by 16 eps S as
// k_mesh_leaves pads; k_mesh_refit, mesh_walk and mesh_ray_node / mesh_ray_face are used as they are, so the pruning argument of f7 holds.
#pragma once
#include "pc_winding.h"

namespace pcu {

// Points per leaf. One surfel is 4 - 11 triangles where a mesh leaf is kMeshLeaf = 4 faces; see DESIGN.md (f11) for what was measured.
constexpr int kSurfelLeaf = 1;
constexpr int kSurfelBadP = 1, kSurfelBadN = 2, kSurfelBadR = 4, kSurfelBadL = 8, kSurfelBadV = 16;     // bits of MeshHead::bad

template <typename T>
__device__ __forceinline__ void surfel_cross(const T a[3], const T b[3], T c[3]) {
    c[0] = a[1] * b[2] - a[2] * b[1]; c[1] = a[2] * b[0] - a[0] * b[2]; c[2] = a[0] * b[1] - a[1] * b[0];
}
template <typename T>
__device__ __forceinline__ void surfel_unit(T x[3]) {
    const T l = sqrt(mesh_dot(x, x));
#pragma unroll
    for (int k = 0; k < 3; ++k) x[k] = l == (T)0 ? (T)0 : x[k] / l;
}
// "per point" of the contract: row i of (p, n, r) -> P, A, B; returns the kSurfelBad* bits of its inputs and of l
template <typename T>
__device__ __forceinline__ int surfel_frame(const T* __restrict__ p, const T* __restrict__ n, const T* __restrict__ r, size_t i, T P[3], T A[3], T B[3]) {
    const T N[3] = {n[3 * i], n[3 * i + 1], n[3 * i + 2]};
    const T R = r[i];
    P[0] = p[3 * i]; P[1] = p[3 * i + 1]; P[2] = p[3 * i + 2];
    const T l = sqrt(mesh_dot(N, N));
    const int bad = (mesh_finite3(P) ? 0 : kSurfelBadP) | (mesh_finite3(N) ? 0 : kSurfelBadN) | (R - R == (T)0 ? 0 : kSurfelBadR) | (l - l == (T)0 ? 0 : kSurfelBadL);
    T ni[3], right[3], up[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) ni[k] = l == (T)0 ? (T)0 : N[k] / l;
    const bool along_y = fabs(fabs(ni[1]) - (T)1) < (T)1e-5;
    const T e[3] = {along_y ? (T)1 : (T)0, along_y ? (T)0 : (T)1, (T)0};
    surfel_cross(ni, e, right);
    surfel_unit(right);
    surfel_cross(ni, right, up);
    surfel_unit(up);
#pragma unroll
    for (int k = 0; k < 3; ++k) { A[k] = R * right[k]; B[k] = R * up[k]; }
    return bad;
}
// rim vertex j of the contract from (c_j, s_j)
template <typename T>
__device__ __forceinline__ void surfel_rim(const T P[3], const T A[3], const T B[3], T c, T s, T v[3]) {
#pragma unroll
    for (int k = 0; k < 3; ++k) v[k] = (c * A[k] + s * B[k]) + P[k];
}
template <typename T>
__device__ __forceinline__ void surfel_rim(const T P[3], const T A[3], const T B[3], const T* __restrict__ cs, T v[3]) { surfel_rim(P, A, B, cs[0], cs[1], v); }
// The table as the walk reads it: through the constant address space, whose loads at a wave-uniform address are scalar ones whatever
// else the kernel does with memory (the table is written before the launch and by no kernel that reads it this way).
template <typename T> using SurfelTable = const T __attribute__((address_space(4)))*;

// ---------------------------------------------------------------------------------------------------- build
// Finiteness of p, n, r, l and of every generated vertex, and the bounding box of all generated vertices (MeshHead as in mesh.h:
// k_mesh_head_init before, k_mesh_frame after).
template <typename T>
__global__ __launch_bounds__(kBlock) void k_surfel_check(const T* __restrict__ p, const T* __restrict__ n, const T* __restrict__ r, int np, int subdivs,
                                                         const T* __restrict__ table, MeshHead<T>* __restrict__ h) {
    using E = typename EncT<T>::type;
    const int i = blockIdx.x * kBlock + threadIdx.x;
    E lo[3] = {~(E)0, ~(E)0, ~(E)0}, hi[3] = {(E)0, (E)0, (E)0};
    int bad = 0;
    if (i < np) {
        T P[3], A[3], B[3];
        bad = surfel_frame(p, n, r, (size_t)i, P, A, B);
        if (!bad) {
#pragma unroll
            for (int k = 0; k < 3; ++k) lo[k] = hi[k] = enc(P[k]);
#pragma unroll 1
            for (int j = 0; j < subdivs; ++j) {
                T v[3];
                surfel_rim(P, A, B, table + 2 * (size_t)j, v);
                if (!mesh_finite3(v)) { bad |= kSurfelBadV; continue; }
#pragma unroll
                for (int k = 0; k < 3; ++k) { const E x = enc(v[k]); lo[k] = x < lo[k] ? x : lo[k]; hi[k] = x > hi[k] ? x : hi[k]; }
            }
        }
    }
#pragma unroll
    for (int k = 0; k < 3; ++k) {
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            const E x = (E)__shfl_xor(lo[k], o, 64), y = (E)__shfl_xor(hi[k], o, 64);
            lo[k] = x < lo[k] ? x : lo[k]; hi[k] = y > hi[k] ? y : hi[k];
        }
    }
    int any = bad;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) any |= __shfl_xor(any, o, 64);
    if ((threadIdx.x & 63) == 0) {
#pragma unroll
        for (int k = 0; k < 3; ++k) { atomicMin(&h->elo[k], lo[k]); atomicMax(&h->ehi[k], hi[k]); }
        if (any) atomicOr(&h->bad, any);
    }
}
// the frame of a cloud without points: the origin (every ray misses the empty root box)
template <typename T>
__global__ void k_surfel_head_empty(MeshHead<T>* h) {
    if (threadIdx.x < 3) { h->elo[threadIdx.x] = enc((T)0); h->ehi[threadIdx.x] = enc((T)0); }
}
// 9 T per sorted point: (p, A, B), by the function the check and the geometry use; and the point's row
template <typename T>
__global__ __launch_bounds__(kBlock) void k_surfel_gather(const T* __restrict__ p, const T* __restrict__ n, const T* __restrict__ r,
                                                          const unsigned* __restrict__ order, int np, T* __restrict__ tri, unsigned* __restrict__ row) {
    const int s = blockIdx.x * kBlock + threadIdx.x;
    if (s >= np) return;
    const unsigned id = order[s];
    T P[3], A[3], B[3];
    (void)surfel_frame(p, n, r, (size_t)id, P, A, B);
    row[s] = id;
    T* o = tri + 9 * (size_t)s;
#pragma unroll
    for (int k = 0; k < 3; ++k) { o[k] = P[k]; o[3 + k] = A[k]; o[6 + k] = B[k]; }
}
// leaf j = node P-1+j: the padded box of the generated vertices of the sorted points [kSurfelLeaf j, kSurfelLeaf (j + 1)); beyond the last
// point the empty box
template <typename T>
__global__ __launch_bounds__(kBlock) void k_surfel_leaves(const T* __restrict__ tri, int np, int P, int subdivs, const T* __restrict__ table,
                                                          const MeshHead<T>* __restrict__ h, T* __restrict__ box) {
    const int j = blockIdx.x * kBlock + threadIdx.x;
    if (j >= P) return;
    T lo[3] = {(T)INFINITY, (T)INFINITY, (T)INFINITY}, hi[3] = {-(T)INFINITY, -(T)INFINITY, -(T)INFINITY};
    const T pad = h->pad;
    for (int t = 0; t < kSurfelLeaf; ++t) {
        const long long s = (long long)kSurfelLeaf * j + t;
        if (s >= np) break;
        const T* e = tri + 9 * (size_t)s;
        const T Pp[3] = {e[0], e[1], e[2]}, A[3] = {e[3], e[4], e[5]}, B[3] = {e[6], e[7], e[8]};
#pragma unroll 1
        for (int c = 0; c <= subdivs; ++c) {
            T v[3] = {Pp[0], Pp[1], Pp[2]};
            if (c < subdivs) surfel_rim(Pp, A, B, table + 2 * (size_t)c, v);
#pragma unroll
            for (int k = 0; k < 3; ++k) { lo[k] = v[k] - pad < lo[k] ? v[k] - pad : lo[k]; hi[k] = v[k] + pad > hi[k] ? v[k] + pad : hi[k]; }
        }
    }
    T* o = box + 6 * (size_t)(P - 1 + j);
#pragma unroll
    for (int k = 0; k < 3; ++k) { o[k] = lo[k]; o[3 + k] = hi[k]; }
}

// ---------------------------------------------------------------------------------------------------- geometry
// One lane per point: its subdivs + 1 vertices and subdivs faces in the reference's layout. `bad` collects the kSurfelBad* bits.
template <typename T>
__global__ __launch_bounds__(kBlock) void k_surfel_geometry(const T* __restrict__ p, const T* __restrict__ n, const T* __restrict__ r, int np, int subdivs,
                                                            const T* __restrict__ table, T* __restrict__ out_v, int* __restrict__ out_f, int* __restrict__ bad_out) {
    const int i = blockIdx.x * kBlock + threadIdx.x;
    int bad = 0;
    if (i < np) {
        T P[3], A[3], B[3];
        bad = surfel_frame(p, n, r, (size_t)i, P, A, B);
        const size_t v0 = (size_t)i * ((size_t)subdivs + 1), f0 = (size_t)i * (size_t)subdivs;
        const int centre = (int)(v0 + (size_t)subdivs);
#pragma unroll 1
        for (int j = 0; j < subdivs; ++j) {
            T v[3];
            surfel_rim(P, A, B, table + 2 * (size_t)j, v);
            if (!mesh_finite3(v)) bad |= kSurfelBadV;
            T* ov = out_v + 3 * (v0 + (size_t)j);
            int* of = out_f + 3 * (f0 + (size_t)j);
            ov[0] = v[0]; ov[1] = v[1]; ov[2] = v[2];
            of[0] = centre; of[1] = (int)(v0 + (size_t)j); of[2] = (int)(v0 + (size_t)(j + 1 == subdivs ? 0 : j + 1));
        }
        T* oc = out_v + 3 * (size_t)centre;
        oc[0] = P[0]; oc[1] = P[1]; oc[2] = P[2];
    }
    int any = bad;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) any |= __shfl_xor(any, o, 64);
    if (any && (threadIdx.x & 63) == 0) atomicOr(bad_out, any);
}

// ---------------------------------------------------------------------------------------------------- rays
template <typename T>
struct SurfelRays : MeshRays<T> { const T* table; int subdivs; };

// The fan visitor of mesh_walk: the node rule of the mesh's rays, leaves of kSurfelLeaf points, HIT of f7 per triangle of the fan. The
// table index is the same for every lane.
template <typename T>
struct SurfelRayVisitor {
    MeshRay<T> r;
    T best = (T)INFINITY; unsigned pid = 0xffffffffu;
    SurfelTable<T> table; int subdivs;
    static constexpr int kLeaf = kSurfelLeaf;
    __device__ __forceinline__ bool node(const T* __restrict__ bx, T& key) const { return mesh_ray_node(r, bx, best, key); }
    __device__ __forceinline__ void element(const MeshIdx<T>& ix, long long s) {
        const T* __restrict__ e = ix.tri + 9 * (size_t)s;
        const T P[3] = {e[0], e[1], e[2]}, A[3] = {e[3], e[4], e[5]}, B[3] = {e[6], e[7], e[8]};
        const unsigned id = ix.face[s];
        T cur[3];
        surfel_rim(P, A, B, table[0], table[1], cur);
#pragma unroll 1
        for (int j = 0; j < subdivs; ++j) {
            const int jn = j + 1 == subdivs ? 0 : j + 1;
            T nxt[3], t, b1, b2;
            surfel_rim(P, A, B, table[2 * (size_t)jn], table[2 * (size_t)jn + 1], nxt);
            if (mesh_ray_face(r, P, cur, nxt, t, b1, b2) && (t < best || (t == best && id < pid && t < (T)INFINITY))) { best = t; pid = id; }
            cur[0] = nxt[0]; cur[1] = nxt[1]; cur[2] = nxt[2];
        }
    }
};

// k_mesh_rays with the fan visitor: one ray per lane, the root box-tested before the walk. Writes (pid, t) and no barycentrics.
template <typename T>
__global__ __launch_bounds__(kMeshBlock) void k_surfel_rays(const SurfelRays<T> a) {
    const int i = blockIdx.x * kMeshBlock + threadIdx.x;
    if (i >= a.n) return;
    const unsigned row = a.order[i];
    const T* po = a.o + (size_t)a.o_stride * row;
    const T* pd = a.d + 3 * (size_t)row;
    const T d[3] = {pd[0], pd[1], pd[2]};
    SurfelRayVisitor<T> vis;
    vis.table = (SurfelTable<T>)a.table; vis.subdivs = a.subdivs;
    mesh_ray_setup(vis.r, po, d, a.ix.head->pad, a.near, a.far);
    T t_in;
    const bool live = mesh_finite3(vis.r.o) && mesh_finite3(d) && vis.node(a.ix.box, t_in);     // (a non-finite row is refused by the host after the launch)
    if (mesh_walk(a.ix, vis, live, a.cancel_word, a.cancel_gen)) return;
    const bool hit = vis.pid != 0xffffffffu;
    a.out_t[row] = hit ? vis.best : (T)INFINITY;
    a.out_fi[row] = hit ? (long long)vis.pid : -1ll;
}

}  // namespace pcu
