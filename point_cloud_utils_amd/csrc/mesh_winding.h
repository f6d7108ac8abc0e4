// csrc/mesh_winding.h -- triangle_soup_fast_winding_number and signed_distance_to_mesh over the linear BVH of mesh.h.
//
// Replaces npe_function(triangle_soup_fast_winding_number) (src/fast_winding_numbers.cpp:20-34) and npe_function(signed_distance_to_mesh)
// (src/signed_distance.cpp:22-56), which call libigl. libigl's last bits cannot be reproduced, so the operators have a contract of their own.
//
//   exact      W(q) = (1/4pi) sum over faces of OMEGA(q, a, b, c), the signed solid angle by Van Oosterom and Strackee:
//                A = a - q, B = b - q, C = c - q, OMEGA = 2 atan2(A.(BxC), |A||B||C| + (A.B)|C| + (B.C)|A| + (C.A)|B|), atan2(0, 0) = 0.
//              atan2 is this file's own (mesh_atan2: one division and an odd polynomial, no fused multiply-add; a few eps of absolute error),
//              so that the kernels hold the library's rule "fused operations only inside divisions and square roots".
//   per node   of the tree of mesh.h, over the faces t below it, with N_t = (b-a)x(c-a)/2, A_t = |N_t|, g_t = (a+b+c)/3:
//                centre p = sum A_t g_t / sum A_t (the centre of its box if the area is 0), radius r = the distance from p to the farthest
//                corner of its padded box (>= the distance to any vertex below), and the moments about p
//                  M0 = sum N_t,   M1_ij = sum (g_t - p)_i N_t,j,   M2_ijk = sum Q_t,ij N_t,k,
//                  Q_t = (xa xa' + xb xb' + xc xc' + (xa+xb+xc)(xa+xb+xc)')/12, x = vertex - p (the face's exact second area moment over its area).
//                M2 is symmetric in ij: 3 + 9 + 18 = 30 values, stored as M0[k], M1[3i+j], M2[3 pair + k] with pair = 00, 01, 02, 11, 12, 22.
//                Padding nodes (the empty box) carry r = -1 and contribute nothing.
//   per query  walk from the root, left child first. With R = p - q, d = |R|: a node with d > beta r contributes
//                M0.R/d^3 + sum_ij M1_ij (delta_ij/d^3 - 3 R_i R_j/d^5) + 1/2 sum_ijk M2_ijk (-3(delta_ij R_k + delta_ik R_j + delta_jk R_i)/d^5 + 15 R_i R_j R_k/d^7),
//                evaluated through u = R/d and 1/d by Horner's rule, so that no power of d is formed on its own; any other inner node is opened;
//                any other leaf contributes sum OMEGA of its faces. w = (the sum of all contributions in walk order) / 4pi.
//                This is the three-term expansion of Barill et al. (SIGGRAPH 2018); beta = 2 is libigl's default, beta = +inf opens everything.
// All of it in the input type T, separate multiplies and adds; the moments are accumulated in double and stored in T. No floating-point
// atomics and a traversal order that depends on query and tree alone: equal arguments give equal bits.
//
// signed_distance_to_mesh: (d, fi, bc) of closest_points_on_mesh (mesh.h) bit for bit; s = -d if |w| > 1/2, else +d; then
// s = min(max(s, lower), upper) with the bounds rounded to float first (the reference declares them float) and then cast to T.
#pragma once
#include "mesh.h"

namespace pcu {

// ---------------------------------------------------------------------------------------------------- moment build
__device__ __forceinline__ int mesh_pair(int i, int j) { return i == 0 ? j : (i == 1 ? 2 + j : 5); }      // i <= j -> 0..5

// radius of a node: from p to the farthest corner of its box
template <typename T>
__device__ __forceinline__ double mesh_mom_radius(const T* __restrict__ bx, const double p[3]) {
    double s = 0.0;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const double lo = fabs(p[k] - (double)bx[k]), hi = fabs((double)bx[3 + k] - p[k]);
        const double m = lo > hi ? lo : hi;
        s += m * m;
    }
    return sqrt(s);
}
template <typename T>
__device__ __forceinline__ void mesh_mom_padding(size_t node, T* __restrict__ ctr, T* __restrict__ mom, double* __restrict__ area) {
    ctr[4 * node] = (T)0; ctr[4 * node + 1] = (T)0; ctr[4 * node + 2] = (T)0; ctr[4 * node + 3] = (T)-1;
    for (int e = 0; e < 30; ++e) mom[30 * node + e] = (T)0;
    area[node] = 0.0;
}
// The centre of a node as it is stored (rounded to T: the moments are taken about the stored point): the area-weighted mean `sum / A`, or the
// centre of the box for a node without area.
template <typename T>
__device__ __forceinline__ void mesh_mom_centre(const T* __restrict__ bx, const double sum[3], double A, T pT[3], double p[3]) {
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        pT[k] = (T)(A > 0.0 ? sum[k] / A : 0.5 * (double)bx[k] + 0.5 * (double)bx[3 + k]);
        p[k] = (double)pT[k];
    }
}
template <typename T>
__device__ __forceinline__ void mesh_mom_store(size_t node, const T* __restrict__ bx, const T pT[3], const double p[3], const double M[30], double A,
                                               T* __restrict__ ctr, T* __restrict__ mom, double* __restrict__ area) {
    ctr[4 * node] = pT[0]; ctr[4 * node + 1] = pT[1]; ctr[4 * node + 2] = pT[2]; ctr[4 * node + 3] = (T)mesh_mom_radius(bx, p);
#pragma unroll
    for (int e = 0; e < 30; ++e) mom[30 * node + e] = (T)M[e];
    area[node] = A;
}

// leaf j = node P-1+j, from the sorted faces [kMeshLeaf j, kMeshLeaf (j + 1)) and its box
template <typename T>
__global__ __launch_bounds__(kBlock) void k_mesh_mleaves(const T* __restrict__ tri, int nf, int P, const T* __restrict__ box, T* __restrict__ ctr,
                                                         T* __restrict__ mom, double* __restrict__ area) {
    const int j = blockIdx.x * kBlock + threadIdx.x;
    if (j >= P) return;
    const size_t node = (size_t)P - 1 + j;
    const long long s0 = (long long)kMeshLeaf * j;
    if (s0 >= nf) { mesh_mom_padding(node, ctr, mom, area); return; }
    const int count = nf - s0 < kMeshLeaf ? (int)(nf - s0) : kMeshLeaf;
    double A = 0.0, sum[3] = {0.0, 0.0, 0.0};
    for (int t = 0; t < count; ++t) {
        const T* tr = tri + 9 * (size_t)(s0 + t);
        double a[3], e1[3], e2[3], g[3];
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            a[k] = (double)tr[k]; e1[k] = (double)tr[3 + k] - a[k]; e2[k] = (double)tr[6 + k] - a[k];
            g[k] = ((a[k] + (double)tr[3 + k]) + (double)tr[6 + k]) / 3.0;
        }
        const double N[3] = {0.5 * (e1[1] * e2[2] - e1[2] * e2[1]), 0.5 * (e1[2] * e2[0] - e1[0] * e2[2]), 0.5 * (e1[0] * e2[1] - e1[1] * e2[0])};
        const double At = sqrt((N[0] * N[0] + N[1] * N[1]) + N[2] * N[2]);
        A += At;
#pragma unroll
        for (int k = 0; k < 3; ++k) sum[k] += At * g[k];
    }
    T pT[3]; double p[3];
    mesh_mom_centre(box + 6 * node, sum, A, pT, p);
    double M[30];
#pragma unroll
    for (int e = 0; e < 30; ++e) M[e] = 0.0;
    for (int t = 0; t < count; ++t) {
        const T* tr = tri + 9 * (size_t)(s0 + t);
        double x[3][3], sx[3], e1[3], e2[3];
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            x[0][k] = (double)tr[k] - p[k]; x[1][k] = (double)tr[3 + k] - p[k]; x[2][k] = (double)tr[6 + k] - p[k];
            sx[k] = (x[0][k] + x[1][k]) + x[2][k];
            e1[k] = x[1][k] - x[0][k]; e2[k] = x[2][k] - x[0][k];
        }
        const double N[3] = {0.5 * (e1[1] * e2[2] - e1[2] * e2[1]), 0.5 * (e1[2] * e2[0] - e1[0] * e2[2]), 0.5 * (e1[0] * e2[1] - e1[1] * e2[0])};
#pragma unroll
        for (int k = 0; k < 3; ++k) M[k] += N[k];
#pragma unroll
        for (int i = 0; i < 3; ++i)
#pragma unroll
            for (int k = 0; k < 3; ++k) M[3 + 3 * i + k] += (sx[i] / 3.0) * N[k];
#pragma unroll
        for (int i = 0; i < 3; ++i)
#pragma unroll
            for (int jj = i; jj < 3; ++jj) {
                const double Q = (((x[0][i] * x[0][jj] + x[1][i] * x[1][jj]) + x[2][i] * x[2][jj]) + sx[i] * sx[jj]) / 12.0;
#pragma unroll
                for (int k = 0; k < 3; ++k) M[12 + 3 * mesh_pair(i, jj) + k] += Q * N[k];
            }
    }
    mesh_mom_store(node, box + 6 * node, pT, p, M, A, ctr, mom, area);
}

// one level: the m nodes m-1 .. 2m-2 from their children (written by the launch before). With delta = p_child - p_parent a child's moments move to
// the parent's centre by M0' = M0, M1'_ij = M1_ij + delta_i M0_j, M2'_ijk = M2_ijk + delta_i M1_jk + delta_j M1_ik + delta_i delta_j M0_k.
template <typename T>
__global__ __launch_bounds__(kBlock) void k_mesh_mrefit(const T* __restrict__ box, T* ctr, T* mom, double* area, int m) {
    const int i0 = blockIdx.x * kBlock + threadIdx.x;
    if (i0 >= m) return;
    const size_t node = (size_t)m - 1 + i0, c0 = 2 * node + 1;
    const bool has[2] = {ctr[4 * c0 + 3] >= (T)0, ctr[4 * c0 + 7] >= (T)0};
    if (!has[0] && !has[1]) { mesh_mom_padding(node, ctr, mom, area); return; }
    double A = 0.0, sum[3] = {0.0, 0.0, 0.0};
    for (int c = 0; c < 2; ++c) {
        if (!has[c]) continue;
        const double Ac = area[c0 + c];
        A += Ac;
#pragma unroll
        for (int k = 0; k < 3; ++k) sum[k] += Ac * (double)ctr[4 * (c0 + c) + k];
    }
    T pT[3]; double p[3];
    mesh_mom_centre(box + 6 * node, sum, A, pT, p);
    double M[30];
#pragma unroll
    for (int e = 0; e < 30; ++e) M[e] = 0.0;
    for (int c = 0; c < 2; ++c) {
        if (!has[c]) continue;
        const T* mc = mom + 30 * (c0 + c);
        double dl[3], M0[3], M1[3][3];
#pragma unroll
        for (int k = 0; k < 3; ++k) { dl[k] = (double)ctr[4 * (c0 + c) + k] - p[k]; M0[k] = (double)mc[k]; }
#pragma unroll
        for (int i = 0; i < 3; ++i)
#pragma unroll
            for (int k = 0; k < 3; ++k) M1[i][k] = (double)mc[3 + 3 * i + k];
#pragma unroll
        for (int k = 0; k < 3; ++k) M[k] += M0[k];
#pragma unroll
        for (int i = 0; i < 3; ++i)
#pragma unroll
            for (int k = 0; k < 3; ++k) M[3 + 3 * i + k] += M1[i][k] + dl[i] * M0[k];
#pragma unroll
        for (int i = 0; i < 3; ++i)
#pragma unroll
            for (int j = i; j < 3; ++j)
#pragma unroll
                for (int k = 0; k < 3; ++k) {
                    const int e = 12 + 3 * mesh_pair(i, j) + k;
                    M[e] += (((double)mc[e] + dl[i] * M1[j][k]) + dl[j] * M1[i][k]) + (dl[i] * dl[j]) * M0[k];
                }
    }
    mesh_mom_store(node, box + 6 * node, pT, p, M, A, ctr, mom, area);
}

// ---------------------------------------------------------------------------------------------------- queries
// atan2(y, x) in T without library code: with m = min(|x|, |y|), M = max(|x|, |y|) the ratio m/M is reduced about c = 0 (m < 0.2 M),
// c = 53/128 (m < 0.67 M) or c = 1 by atan(m/M) = atan(c) + atan(t), t = (m - cM)/(M + cm), |t| <= 0.2004; atan(t) is its Taylor polynomial
// up to t^11 (float: the first term left out is below 1e-8 t) or t^23 (double: 2e-17 t) by Horner's rule in t^2; then the octant is undone
// (pi/2 - r if |y| > |x|, pi - r if x < 0, the sign of y). atan2(+-0, +-0) = +-0. Every step rounds on its own: a few eps in all.
template <typename T> struct AtanPoly;
template <> struct AtanPoly<float> { static constexpr int n = 6; };
template <> struct AtanPoly<double> { static constexpr int n = 12; };
template <typename T>
__device__ __forceinline__ T mesh_atan2(T y, T x) {
    const T ay = fabs(y), ax = fabs(x);
    const T mx = ax > ay ? ax : ay, mn = ax > ay ? ay : ax;
    if (!(mx > (T)0)) return y;                                                // (0, 0): the zero of y; a NaN stays one
    T c = (T)1, at = (T)0.78539816339744830962;
    if (mn < (T)0.2 * mx) { c = (T)0; at = (T)0; }
    else if (mn < (T)0.67 * mx) { c = (T)0.4140625; at = (T)0.39257013501182859517; }
    const T t = (mn - c * mx) / (mx + c * mn), z = t * t;
    T p = (T)1 / (T)(2 * AtanPoly<T>::n - 1);
    if ((AtanPoly<T>::n & 1) == 0) p = -p;
#pragma unroll
    for (int k = AtanPoly<T>::n - 2; k >= 0; --k) p = p * z + ((k & 1) ? -(T)1 : (T)1) / (T)(2 * k + 1);      // (constants: folded at compile time)
    T r = at + t * p;
    if (ay > ax) r = (T)1.57079632679489661923 - r;
    if (x < (T)0) r = (T)3.14159265358979323846 - r;
    return y < (T)0 ? -r : r;
}

// OMEGA of the contract (a query on a vertex: det and den are zeros, and mesh_atan2 gives 0).
template <typename T>
__device__ __forceinline__ T mesh_wind_face(const T q[3], const T a[3], const T b[3], const T c[3]) {
    T A[3], B[3], C[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) { A[k] = a[k] - q[k]; B[k] = b[k] - q[k]; C[k] = c[k] - q[k]; }
    const T la = sqrt(mesh_dot(A, A)), lb = sqrt(mesh_dot(B, B)), lc = sqrt(mesh_dot(C, C));
    const T bxc[3] = {B[1] * C[2] - B[2] * C[1], B[2] * C[0] - B[0] * C[2], B[0] * C[1] - B[1] * C[0]};
    const T det = mesh_dot(A, bxc);
    const T den = (((la * lb) * lc + mesh_dot(A, B) * lc) + mesh_dot(B, C) * la) + mesh_dot(C, A) * lb;
    return (T)2 * mesh_atan2(det, den);
}

// The expansion of the contract about a node's centre, times 4pi: R = centre - q, d = |R| > 0, m the node's 30 moments.
template <typename T>
__device__ __forceinline__ T mesh_wind_far(const T* __restrict__ m, const T R[3], T d) {
    const T id = (T)1 / d;
    const T u[3] = {R[0] * id, R[1] * id, R[2] * id};
    const T t0 = mesh_dot(m, u);
    const T row[3] = {mesh_dot(m + 3, u), mesh_dot(m + 6, u), mesh_dot(m + 9, u)};
    const T t1 = ((m[3] + m[7]) + m[11]) - (T)3 * mesh_dot(u, row);
    const T* __restrict__ m2 = m + 12;
    T tr[3], S[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        tr[k] = (m2[k] + m2[9 + k]) + m2[15 + k];
        const T diag = ((u[0] * u[0]) * m2[k] + (u[1] * u[1]) * m2[9 + k]) + (u[2] * u[2]) * m2[15 + k];
        const T off = ((u[0] * u[1]) * m2[3 + k] + (u[0] * u[2]) * m2[6 + k]) + (u[1] * u[2]) * m2[12 + k];
        S[k] = diag + (T)2 * off;
    }
    const T cj[3] = {(m2[0] + m2[4]) + m2[8], (m2[3] + m2[10]) + m2[14], (m2[6] + m2[13]) + m2[17]};      // sum_j M2_ijj
    const T t2 = (T)15 * mesh_dot(S, u) - (T)3 * (mesh_dot(tr, u) + (T)2 * mesh_dot(cj, u));
    return ((((T)0.5 * t2) * id + t1) * id + t0) * id * id;
}

// The winding visitor of mesh_walk. node() recovers the node number from the box pointer; a far node adds its expansion and is not entered, a
// padding node is not entered, anything else is (with a constant key: the left child goes first). mesh_walk tests a pushed node again when it
// pops it. That adds nothing twice: the test is a pure function of query and node, only nodes that pass (are to be opened) are pushed, and a
// node that passes adds nothing.
template <typename T>
struct MeshWindNodes {                          // the node rule and the sum, shared with the dipole tree of pc_winding.h
    T q[3], beta, acc = (T)0;
    const T* box0; const T* ctr; const T* mom;
    __device__ __forceinline__ bool node(const T* __restrict__ bx, T& key) {
        key = (T)0;
        const size_t n = (size_t)(bx - box0) / 6;
        const T* __restrict__ c = ctr + 4 * n;
        const T r = c[3];
        if (r < (T)0) return false;
        const T R[3] = {c[0] - q[0], c[1] - q[1], c[2] - q[2]};
        const T d = sqrt(mesh_dot(R, R));
        if (!(d > beta * r)) return true;
        acc += mesh_wind_far(mom + 30 * n, R, d);
        return false;
    }
};
template <typename T>
struct MeshWindVisitor : MeshWindNodes<T> {
    static constexpr int kLeaf = kMeshLeaf;
    __device__ __forceinline__ void element(const MeshIdx<T>& ix, long long s) { mesh_face_at(*this, ix, s); }
    __device__ __forceinline__ void face(const T a[3], const T b[3], const T c[3], const unsigned* __restrict__) { this->acc += mesh_wind_face(this->q, a, b, c); }
};

template <typename T>
struct MeshSigned {                             // the rows of both operators; the winding number alone leaves out_fi, out_bc and the bounds unused
    const T* p; const unsigned* order; int np;
    MeshIdx<T> ix;
    T beta, lower, upper;
    T* out_val; long long* out_fi; T* out_bc;
    const unsigned* cancel_word; unsigned cancel_gen;          // pcu_types.h: cancel_seen
};

// w of one query (the root is tested before the walk: it may be far as a whole). Returns true if the call was cancelled.
template <typename T, typename Visitor = MeshWindVisitor<T>>
__device__ __forceinline__ bool mesh_wind_query(const MeshSigned<T>& a, const T q[3], bool finite, T& w) {
    Visitor vis;
    vis.q[0] = q[0]; vis.q[1] = q[1]; vis.q[2] = q[2]; vis.beta = a.beta;
    vis.box0 = a.ix.box; vis.ctr = a.ix.ctr; vis.mom = a.ix.mom;
    T key;
    const bool live = finite && vis.node(a.ix.box, key);
    if (mesh_walk(a.ix, vis, live, a.cancel_word, a.cancel_gen)) return true;
    w = vis.acc / (T)12.566370614359172;
    return false;
}

// One query per lane, rows in the order of k_mesh_qcodes: the lanes of a wave read the same nodes' moments.
template <typename T>
__global__ __launch_bounds__(kMeshBlock) void k_mesh_winding(const MeshSigned<T> a) {
    const int i = blockIdx.x * kMeshBlock + threadIdx.x;
    if (i >= a.np) return;
    const unsigned row = a.order[i];
    const T q[3] = {a.p[3 * (size_t)row], a.p[3 * (size_t)row + 1], a.p[3 * (size_t)row + 2]};
    T w;
    if (mesh_wind_query(a, q, mesh_finite3(q), w)) return;     // (a non-finite row is refused by the host after the launch)
    a.out_val[row] = w;
}

// signed_distance_to_mesh in one launch: the point walk of k_mesh_closest, then the winding walk, in the same lane. The two inlined copies of
// mesh_walk have a stack each: 2 x 26,624 B of LDS, so 3 blocks (12 waves) per CU where the single-walk kernels get 6.
template <typename T>
__global__ __launch_bounds__(kMeshBlock) void k_mesh_sdf(const MeshSigned<T> a) {
    const int i = blockIdx.x * kMeshBlock + threadIdx.x;
    if (i >= a.np) return;
    const unsigned row = a.order[i];
    MeshPointVisitor<T> vis;
    vis.q[0] = a.p[3 * (size_t)row]; vis.q[1] = a.p[3 * (size_t)row + 1]; vis.q[2] = a.p[3 * (size_t)row + 2];
    const bool finite = mesh_finite3(vis.q);
    if (mesh_walk(a.ix, vis, finite, a.cancel_word, a.cancel_gen)) return;
    T w;
    if (mesh_wind_query(a, vis.q, finite, w)) return;
    const T d = sqrt(vis.best);
    T s = fabs(w) > (T)0.5 ? -d : d;
    s = s > a.lower ? s : a.lower;
    s = s < a.upper ? s : a.upper;
    const T u = ((T)1 - vis.bv) - vis.bw;
    a.out_val[row] = s;
    a.out_fi[row] = vis.bf == 0xffffffffu ? -1ll : (long long)vis.bf;
    a.out_bc[3 * (size_t)row] = u; a.out_bc[3 * (size_t)row + 1] = vis.bv; a.out_bc[3 * (size_t)row + 2] = vis.bw;
}

}  // namespace pcu
