// csrc/pc_winding.h -- point_cloud_fast_winding_number and estimate_mesh_face_normals.
//
// Replaces npe_function(point_cloud_fast_winding_number) (src/fast_winding_numbers.cpp:51-67, libigl's Barill et al. 2018 for oriented points)
// and npe_function(estimate_mesh_face_normals) (src/mesh_normals.cpp:65-80). libigl's last bits cannot be reproduced, so the operator has a
// contract of its own. All of it in the input type T, separate multiplies and adds, IEEE division and square root, dot as in mesh.h.
//
//   dipole     D_i = a_i * n_i (three products in T); a may be any finite value (zero, negative), n need not have unit length.
//   exact      W(q) = (1/4pi) sum_i TERM(q, p_i, D_i); with R = p - q, d2 = dot(R, R): TERM = 0 if !(d2 > 0) (a query on a point gets nothing
//              from that point, as in libigl), else d = sqrt(d2), id = 1/d, u = R*id, TERM = (dot(D, u) * id) * id.
//   tree       points in the order of the 63-bit Morton code of their position in the bounding box of all points (a stable sort: ties keep row
//              order), leaves of kPcLeaf consecutive points, the implicit balanced tree of mesh.h over the leaves padded to a power of two P.
//              Boxes are the plain min / max of the points below a node (nothing prunes by box here, so nothing is padded); padding nodes
//              carry r = -1 and contribute nothing.
//   per node   over the points below it, with weight w_i = |D_i|: centre c = sum w_i p_i / sum w_i (the centre of its box if the weight is 0),
//              radius r = the distance from c to the farthest corner of its box, and with x = p_i - c the moments
//                M0 = sum D_i,   M1_ij = sum x_i D_j,   M2_ijk = sum x_i x_j D_k        (the 3 + 9 + 18 layout of mesh_winding.h).
//              Leaves accumulate in double about the centre as stored (rounded to T) and store in T; inner nodes move their children's
//              moments with k_mesh_mrefit as it is ("area" read as weight).
//   per query  as mesh_wind_query does it: the root is tested before the walk, a node with d > beta r adds mesh_wind_far, any other inner
//              node is opened, left child first, any other leaf adds TERM of its points in sorted order; w = acc / 4pi.
// No floating-point atomics and a traversal order that depends on query and tree alone: equal arguments give equal bits.
//
// estimate_mesh_face_normals, per face (a, b, c) in T without FMA: e1 = b - a, e2 = c - a,
//   N = (e1[1]*e2[2] - e1[2]*e2[1], e1[2]*e2[0] - e1[0]*e2[2], e1[0]*e2[1] - e1[1]*e2[0]), r = sqrt(dot(N, N)),
//   the row is N / r component by component, or (0, 0, 0) if r == 0 (the reference passes a zero background vector). A face whose cross
//   product underflows to zero gets a zero normal; a non-finite r is refused.
#pragma once
#include "mesh_winding.h"

namespace pcu {

// Points per leaf. Chosen on the CPU model of the contract (tests/pc_winding_contract.py: LEAF), where it roughly balances one expansion
// (34 loads) against 8 dipoles (48 loads); it has not been timed on the GPU. The model holds the same constant.
constexpr int kPcLeaf = 8;
constexpr int kPcBadP = 1, kPcBadN = 2, kPcBadA = 4, kPcBadD = 8;      // bits of MeshHead::bad
constexpr int kMeshBadNormal = 4;                                       // (next to kMeshBadVertex, kMeshBadFace)

// ---------------------------------------------------------------------------------------------------- build
// Finiteness of p, n and a, and the bounding box of all points (MeshHead as in mesh.h: k_mesh_head_init before, k_mesh_frame after).
template <typename T>
__global__ __launch_bounds__(kBlock) void k_pc_check(const T* __restrict__ p, const T* __restrict__ n, const T* __restrict__ a, int np,
                                                     MeshHead<T>* __restrict__ h) {
    using E = typename EncT<T>::type;
    const int i = blockIdx.x * kBlock + threadIdx.x;
    E lo[3] = {~(E)0, ~(E)0, ~(E)0}, hi[3] = {(E)0, (E)0, (E)0};
    bool bp = false, bn = false, ba = false;
    if (i < np) {
        bp = !mesh_finite3(p + 3 * (size_t)i); bn = !mesh_finite3(n + 3 * (size_t)i);
        const T w = a[i];
        ba = !(w - w == (T)0);
        if (!bp) {
#pragma unroll
            for (int k = 0; k < 3; ++k) { lo[k] = hi[k] = enc(p[3 * (size_t)i + k]); }
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
    const unsigned long long any_p = __ballot(bp), any_n = __ballot(bn), any_a = __ballot(ba);
    if ((threadIdx.x & 63) == 0) {
#pragma unroll
        for (int k = 0; k < 3; ++k) { atomicMin(&h->elo[k], lo[k]); atomicMax(&h->ehi[k], hi[k]); }
        if ((any_p | any_n | any_a) != 0ull) atomicOr(&h->bad, (any_p ? kPcBadP : 0) | (any_n ? kPcBadN : 0) | (any_a ? kPcBadA : 0));
    }
}
// k_mesh_codes for points: the centroid is the point itself
template <typename T>
__global__ __launch_bounds__(kBlock) void k_pc_codes(const T* __restrict__ p, int np, const MeshHead<T>* __restrict__ h, unsigned long long* __restrict__ keys) {
    const int i = blockIdx.x * kBlock + threadIdx.x;
    if (i >= np) return;
    unsigned cell[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) cell[k] = mesh_cell(((double)p[3 * (size_t)i + k] - (double)h->lo[k]) * (double)h->inv[k], 2097151u);
    keys[i] = morton_split21(cell[0]) | morton_split21(cell[1]) << 1 | morton_split21(cell[2]) << 2;
}
// 6 T per sorted point: the position, then D = a * n. A non-finite D (the product overflows) is flagged.
template <typename T>
__global__ __launch_bounds__(kBlock) void k_pc_gather(const T* __restrict__ p, const T* __restrict__ n, const T* __restrict__ a,
                                                      const unsigned* __restrict__ order, int np, T* __restrict__ pd, int* __restrict__ bad) {
    const int s = blockIdx.x * kBlock + threadIdx.x;
    bool nf = false;
    if (s < np) {
        const unsigned id = order[s];
        const T w = a[id];
        T D[3];
#pragma unroll
        for (int k = 0; k < 3; ++k) { pd[6 * (size_t)s + k] = p[3 * (size_t)id + k]; D[k] = w * n[3 * (size_t)id + k]; pd[6 * (size_t)s + 3 + k] = D[k]; }
        nf = !mesh_finite3(D);
    }
    if (__ballot(nf) != 0ull && (threadIdx.x & 63) == 0) atomicOr(bad, kPcBadD);
}
// leaf j = node P-1+j: the box of the sorted points [kPcLeaf j, kPcLeaf (j + 1)); beyond the last point the empty box
template <typename T>
__global__ __launch_bounds__(kBlock) void k_pc_leaves(const T* __restrict__ pd, int np, int P, T* __restrict__ box) {
    const int j = blockIdx.x * kBlock + threadIdx.x;
    if (j >= P) return;
    T lo[3] = {(T)INFINITY, (T)INFINITY, (T)INFINITY}, hi[3] = {-(T)INFINITY, -(T)INFINITY, -(T)INFINITY};
    for (int t = 0; t < kPcLeaf; ++t) {
        const long long s = (long long)kPcLeaf * j + t;
        if (s >= np) break;
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            const T x = pd[6 * (size_t)s + k];
            lo[k] = x < lo[k] ? x : lo[k]; hi[k] = x > hi[k] ? x : hi[k];
        }
    }
    T* o = box + 6 * (size_t)(P - 1 + j);
#pragma unroll
    for (int k = 0; k < 3; ++k) { o[k] = lo[k]; o[3 + k] = hi[k]; }
}
// The analogue of k_mesh_mleaves: leaf j from its sorted points and its box. `weight` is what k_mesh_mrefit reads as area.
template <typename T>
__global__ __launch_bounds__(kBlock) void k_pc_mleaves(const T* __restrict__ pd, int np, int P, const T* __restrict__ box, T* __restrict__ ctr,
                                                       T* __restrict__ mom, double* __restrict__ weight) {
    const int j = blockIdx.x * kBlock + threadIdx.x;
    if (j >= P) return;
    const size_t node = (size_t)P - 1 + j;
    const long long s0 = (long long)kPcLeaf * j;
    if (s0 >= np) { mesh_mom_padding(node, ctr, mom, weight); return; }
    const int count = np - s0 < kPcLeaf ? (int)(np - s0) : kPcLeaf;
    double W = 0.0, sum[3] = {0.0, 0.0, 0.0};
    for (int t = 0; t < count; ++t) {
        const T* e = pd + 6 * (size_t)(s0 + t);
        const double D[3] = {(double)e[3], (double)e[4], (double)e[5]};
        const double w = sqrt((D[0] * D[0] + D[1] * D[1]) + D[2] * D[2]);
        W += w;
#pragma unroll
        for (int k = 0; k < 3; ++k) sum[k] += w * (double)e[k];
    }
    T pT[3]; double p[3];
    mesh_mom_centre(box + 6 * node, sum, W, pT, p);
    double M[30];
#pragma unroll
    for (int e = 0; e < 30; ++e) M[e] = 0.0;
    for (int t = 0; t < count; ++t) {
        const T* e = pd + 6 * (size_t)(s0 + t);
        double x[3], D[3];
#pragma unroll
        for (int k = 0; k < 3; ++k) { x[k] = (double)e[k] - p[k]; D[k] = (double)e[3 + k]; }
#pragma unroll
        for (int k = 0; k < 3; ++k) M[k] += D[k];
#pragma unroll
        for (int i = 0; i < 3; ++i)
#pragma unroll
            for (int k = 0; k < 3; ++k) M[3 + 3 * i + k] += x[i] * D[k];
#pragma unroll
        for (int i = 0; i < 3; ++i)
#pragma unroll
            for (int jj = i; jj < 3; ++jj)
#pragma unroll
                for (int k = 0; k < 3; ++k) M[12 + 3 * mesh_pair(i, jj) + k] += (x[i] * x[jj]) * D[k];
    }
    mesh_mom_store(node, box + 6 * node, pT, p, M, W, ctr, mom, weight);
}

// ---------------------------------------------------------------------------------------------------- queries
// The dipole visitor of mesh_walk: the node rule of the mesh's winding number, leaves of kPcLeaf points, TERM of the contract per point.
template <typename T>
struct PcWindVisitor : MeshWindNodes<T> {
    static constexpr int kLeaf = kPcLeaf;
    __device__ __forceinline__ void element(const MeshIdx<T>& ix, long long s) {
        const T* __restrict__ e = ix.tri + 6 * (size_t)s;
        const T R[3] = {e[0] - this->q[0], e[1] - this->q[1], e[2] - this->q[2]};
        const T d2 = mesh_dot(R, R);
        if (!(d2 > (T)0)) return;
        const T id = (T)1 / sqrt(d2);
        const T u[3] = {R[0] * id, R[1] * id, R[2] * id};
        this->acc += (mesh_dot(e + 3, u) * id) * id;
    }
};

// One query per lane, rows in the order of k_mesh_qcodes (in the cloud's frame): the lanes of a wave read the same nodes' moments.
template <typename T>
__global__ __launch_bounds__(kMeshBlock) void k_pc_winding(const MeshSigned<T> a) {
    const int i = blockIdx.x * kMeshBlock + threadIdx.x;
    if (i >= a.np) return;
    const unsigned row = a.order[i];
    const T q[3] = {a.p[3 * (size_t)row], a.p[3 * (size_t)row + 1], a.p[3 * (size_t)row + 2]};
    T w;
    if (mesh_wind_query<T, PcWindVisitor<T>>(a, q, mesh_finite3(q), w)) return;     // (a non-finite row is refused by the host after the launch)
    a.out_val[row] = w;
}

// ---------------------------------------------------------------------------------------------------- face normals
// One lane per face, through the range-checked int32 triples of k_mesh_faces. A non-finite length is flagged.
template <typename T>
__global__ __launch_bounds__(kBlock) void k_mesh_fnormals(const T* __restrict__ v, const int* __restrict__ fidx, int nf, T* __restrict__ out, int* __restrict__ bad) {
    const int t = blockIdx.x * kBlock + threadIdx.x;
    bool nfin = false;
    if (t < nf) {
        const T* a = v + 3 * (size_t)fidx[3 * (size_t)t];
        const T* b = v + 3 * (size_t)fidx[3 * (size_t)t + 1];
        const T* c = v + 3 * (size_t)fidx[3 * (size_t)t + 2];
        const T e1[3] = {b[0] - a[0], b[1] - a[1], b[2] - a[2]}, e2[3] = {c[0] - a[0], c[1] - a[1], c[2] - a[2]};
        const T N[3] = {e1[1] * e2[2] - e1[2] * e2[1], e1[2] * e2[0] - e1[0] * e2[2], e1[0] * e2[1] - e1[1] * e2[0]};
        const T r = sqrt(mesh_dot(N, N));
        nfin = !(r - r == (T)0);
        const bool zero = r == (T)0;
#pragma unroll
        for (int k = 0; k < 3; ++k) out[3 * (size_t)t + k] = zero ? (T)0 : N[k] / r;
    }
    if (__ballot(nfin) != 0ull && (threadIdx.x & 63) == 0) atomicOr(bad, kMeshBadNormal);
}

}  // namespace pcu
