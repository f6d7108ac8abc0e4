// csrc/mesh_smooth.h -- adjacency_list / mesh_vertex_adjacency, estimate_mesh_vertex_normals and laplacian_smooth_mesh.
//
// The reference reaches libigl for all three (src/adjacency_list.cpp, src/mesh_normals.cpp:24-50, src/smooth.cpp:24-79). libigl was not at
// hand, so each operator follows a stated contract (restated in numpy: tests/mesh_smooth_contract.py).
//
//   structure  Corner (t, c) of face t has the id 3t + c. The INCIDENCE of vertex i is its corners ascending by id: one stable sort of the
//              3 #f keys `vertex`. The ADJACENCY of i is the set of j != i that share a face with i, each once, ascending: the six directed
//              pairs of every face as keys row << hb | col (hb = bits of nv - 1), one stable sort, run heads that are no self pairs, one scan.
//              Pair 2 (3t + c) + d belongs to corner (t, c), whose opposite edge is (j, k) = (f[t][c+1], f[t][c+2]): d = 0 is j -> k, d = 1
//              is k -> j. The sort is stable, so the duplicates of one directed pair stay ascending by corner id.
//   normals    per face N = (b - a) x (c - a) and N / sqrt(dot(N, N)) as estimate_mesh_face_normals computes them (pc_winding.h); the corner
//              (t, c) adds to its vertex the unit normal (uniform), N (area) or the unit normal times atan2(|e1 x e2|, e1 . e2) (angle; e1, e2
//              the edges that leave the corner); a vertex's sum starts at 0 and takes its corners in incidence order, component by component;
//              the row is s / sqrt((s0 s0 + s1 s1) + s2 s2), or zero where that length is zero.
//   smoothing  w(t, c) = (0.5 (e1 . e2)) / |e1 x e2| of the INPUT v, 0 where |e1 x e2| == 0, goes to L[j,k] and L[k,j]; the duplicates of a
//              directed pair are added in sorted order, L[i,i] = -(the row's entries added by ascending column). Per iteration M = I or
//              M_ii = (sum of |N| over the incidence of i, of the current u) / 6; (M - h L) u' = M u by Jacobi-preconditioned conjugate
//              gradients from x0 = u, the three columns on their own; a vertex with M_ii == 0 keeps its position (its row and column leave
//              the system). A column stops when r.r <= (64 eps)^2 b.b. With cotangent weights u' <- (u' - c) / sqrt(A) + c follows for the
//              vertices with M_ii != 0: A = 0.5 sum |N|, c = (sum |N| (a + b + c) / 3) / sum |N| over the faces of u'.
// No floating-point atomics: rows are gathered through the CSR by one lane each, dot products are folded per block by a fixed tree and then
// by one block over the per-block values in a fixed order. alpha, beta and the stop flags stay on the device (MsCg): every step of a column
// that has stopped is a no-op, so how often the host looks cannot change a byte.
//
// A row per lane, not per wave: a triangle mesh has about six entries per row, so a wave per row would idle nine lanes in ten and would need
// a fixed cross-lane fold to keep the ascending-column order that a single lane has by construction. The price is the rare long row (the
// apex of a fan), which one lane walks alone. Not timed against the alternative.
#pragma once
#include "pc_winding.h"

namespace pcu {

constexpr int kMsFoldMax = 9;                   // columns one fold carries at most
constexpr int kMsCgDone = 1, kMsCgBreakdown = 2;

template <typename T>
struct MsCg {                                   // the solver's scalars, on the device
    T rz[3], bb[3], alpha[3], beta[3];
    int done[3];
    int flag;                                   // kMsCgDone: every column has stopped; kMsCgBreakdown: p.Ap <= 0 (or NaN) met
    int iters;                                  // iterations in which some column was still running, over all solves of the call
};

// ---------------------------------------------------------------------------------------------------- folds
// The block's sum of NC values per lane: xor tree inside a wave, then the waves in order. Every lane of the block must call it.
template <typename T, int NC>
__device__ __forceinline__ void ms_block_fold(T (&v)[NC], T* __restrict__ out) {
    __shared__ T s_w[kBlock / 64][NC];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int k = 0; k < NC; ++k) {
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) v[k] = v[k] + __shfl_xor(v[k], o, 64);
    }
    if (lane == 0) {
#pragma unroll
        for (int k = 0; k < NC; ++k) s_w[wave][k] = v[k];
    }
    __syncthreads();
    if (threadIdx.x == 0) {
#pragma unroll
        for (int k = 0; k < NC; ++k) {
            T a = s_w[0][k];
#pragma unroll
            for (int w = 1; w < kBlock / 64; ++w) a = a + s_w[w][k];
            out[k] = a;
        }
    }
}
// Second stage, one block: lane t adds the per-block values t, t + 256, ... in that order, then the block folds. Lane 0 holds the totals.
template <typename T, int NC>
__device__ __forceinline__ void ms_fold_parts(const T* __restrict__ part, int nb, T* __restrict__ total) {
    T a[NC];
#pragma unroll
    for (int k = 0; k < NC; ++k) a[k] = (T)0;
    for (int b = threadIdx.x; b < nb; b += kBlock) {
#pragma unroll
        for (int k = 0; k < NC; ++k) a[k] = a[k] + part[(size_t)b * NC + k];
    }
    ms_block_fold<T, NC>(a, total);
}

// ---------------------------------------------------------------------------------------------------- structure
// Faces of any of the four integer types -> range-checked int32 triples (a refused face reads as (0, 0, 0)) and the 3 nf corner keys.
__global__ __launch_bounds__(kBlock) void k_ms_corners(const void* __restrict__ f, int kind, int nf, int nv, int* __restrict__ fidx,
                                                       unsigned long long* __restrict__ ck, int* __restrict__ bad) {
    const int t = blockIdx.x * kBlock + threadIdx.x;
    bool b = false;
    if (t < nf) {
        int id[3];
        b = face_in(f, kind, (size_t)t, (unsigned)nv, id);
#pragma unroll
        for (int j = 0; j < 3; ++j) { fidx[3 * (size_t)t + j] = id[j]; ck[3 * (size_t)t + j] = (unsigned long long)id[j]; }
    }
    if (__ballot(b) != 0ull && (threadIdx.x & 63) == 0) atomicOr(bad, kMeshBadFace);
}
// One lane per corner: the two directed pairs of its opposite edge.
__global__ __launch_bounds__(kBlock) void k_ms_pairs(const int* __restrict__ fidx, int ncorners, int hb, unsigned long long* __restrict__ pk) {
    const int c = blockIdx.x * kBlock + threadIdx.x;
    if (c >= ncorners) return;
    const int t = c / 3, cc = c - 3 * t;
    const unsigned long long j = (unsigned long long)fidx[3 * (size_t)t + (cc + 1) % 3], k = (unsigned long long)fidx[3 * (size_t)t + (cc + 2) % 3];
    pk[2 * (size_t)c] = (j << hb) | k;
    pk[2 * (size_t)c + 1] = (k << hb) | j;
}
// pos[i] = the number of sorted keys whose row (key >> shift) is below i, for i in [0, nv]: a binary search per row.
__global__ __launch_bounds__(kBlock) void k_ms_row_starts(const unsigned long long* __restrict__ keys, int n, int shift, int nv, unsigned* __restrict__ pos) {
    const int i = blockIdx.x * kBlock + threadIdx.x;
    if (i > nv) return;
    int lo = 0, hi = n;
    while (lo < hi) {
        const int mid = lo + (hi - lo) / 2;
        if ((keys[mid] >> shift) < (unsigned long long)i) lo = mid + 1; else hi = mid;
    }
    pos[i] = (unsigned)lo;
}
// The head of every run of equal directed pairs that is no self pair i -> i.
__global__ __launch_bounds__(kBlock) void k_ms_pair_heads(const unsigned long long* __restrict__ keys, int n, int hb, unsigned* __restrict__ flag) {
    const int j = blockIdx.x * kBlock + threadIdx.x;
    if (j >= n) return;
    const unsigned long long k = keys[j], mask = (1ull << hb) - 1ull;
    flag[j] = ((j == 0 || k != keys[j - 1]) && (k >> hb) != (k & mask)) ? 1u : 0u;
}
// Unique entry scan[j] - 1 of head j: where its run starts and its column.
__global__ __launch_bounds__(kBlock) void k_ms_entries(const unsigned long long* __restrict__ keys, const unsigned* __restrict__ flag, const unsigned* __restrict__ scan,
                                                       int n, int hb, unsigned* __restrict__ head_pos, int* __restrict__ col) {
    const int j = blockIdx.x * kBlock + threadIdx.x;
    if (j >= n || !flag[j]) return;
    const unsigned e = scan[j] - 1u;
    head_pos[e] = (unsigned)j;
    col[e] = (int)(keys[j] & ((1ull << hb) - 1ull));
}
// off[i] = unique entries in rows below i, i in [0, nv]
__global__ __launch_bounds__(kBlock) void k_ms_offsets(const unsigned* __restrict__ pos, const unsigned* __restrict__ scan, int nv, unsigned* __restrict__ off) {
    const int i = blockIdx.x * kBlock + threadIdx.x;
    if (i > nv) return;
    const unsigned p = pos[i];
    off[i] = p == 0u ? 0u : scan[p - 1u];
}
// The CSR as the ABI returns it: int64 offsets, neighbours in the faces' integer type.
__global__ __launch_bounds__(kBlock) void k_ms_adj_out(const unsigned* __restrict__ off, int nv, const int* __restrict__ col, unsigned ne, int kind,
                                                       long long* __restrict__ out_off, void* __restrict__ out_nb) {
    const unsigned i = blockIdx.x * kBlock + threadIdx.x;
    if (i <= (unsigned)nv) out_off[i] = (long long)off[i];
    if (i < ne) index_out_signed(out_nb, kind, i, col[i]);
}

// ---------------------------------------------------------------------------------------------------- geometry
template <typename T>
__device__ __forceinline__ void ms_cross(const T e1[3], const T e2[3], T N[3]) {
    N[0] = e1[1] * e2[2] - e1[2] * e2[1]; N[1] = e1[2] * e2[0] - e1[0] * e2[2]; N[2] = e1[0] * e2[1] - e1[1] * e2[0];
}
// N = (b - a) x (c - a) of face t and its length
template <typename T>
__device__ __forceinline__ T ms_face_normal(const T* __restrict__ v, const int* __restrict__ fidx, int t, T N[3]) {
    const T* a = v + 3 * (size_t)fidx[3 * (size_t)t];
    const T* b = v + 3 * (size_t)fidx[3 * (size_t)t + 1];
    const T* c = v + 3 * (size_t)fidx[3 * (size_t)t + 2];
    const T e1[3] = {b[0] - a[0], b[1] - a[1], b[2] - a[2]}, e2[3] = {c[0] - a[0], c[1] - a[1], c[2] - a[2]};
    ms_cross(e1, e2, N);
    return sqrt(mesh_dot(N, N));
}
// |e1 x e2| and e1 . e2 of the edges that leave corner cc of face t
template <typename T>
__device__ __forceinline__ void ms_corner(const T* __restrict__ v, const int* __restrict__ fidx, int t, int cc, T& len, T& dot) {
    const T* p = v + 3 * (size_t)fidx[3 * (size_t)t + cc];
    const T* q = v + 3 * (size_t)fidx[3 * (size_t)t + (cc + 1) % 3];
    const T* r = v + 3 * (size_t)fidx[3 * (size_t)t + (cc + 2) % 3];
    const T e1[3] = {q[0] - p[0], q[1] - p[1], q[2] - p[2]}, e2[3] = {r[0] - p[0], r[1] - p[1], r[2] - p[2]};
    T X[3];
    ms_cross(e1, e2, X);
    len = sqrt(mesh_dot(X, X));
    dot = mesh_dot(e1, e2);
}

// ---------------------------------------------------------------------------------------------------- vertex normals
// mode 0: the unit normal per face, 1: N itself, 2: the unit normal and the three corner angles
template <typename T>
__global__ __launch_bounds__(kBlock) void k_ms_face_vec(const T* __restrict__ v, const int* __restrict__ fidx, int nf, int mode, T* __restrict__ fn, T* __restrict__ ang) {
    const int t = blockIdx.x * kBlock + threadIdx.x;
    if (t >= nf) return;
    T N[3];
    const T r = ms_face_normal(v, fidx, t, N);
    const bool zero = r == (T)0;
#pragma unroll
    for (int k = 0; k < 3; ++k) fn[3 * (size_t)t + k] = mode == 1 ? N[k] : (zero ? (T)0 : N[k] / r);
    if (mode == 2) {
#pragma unroll
        for (int cc = 0; cc < 3; ++cc) {
            T len, dot;
            ms_corner(v, fidx, t, cc, len, dot);
            ang[3 * (size_t)t + cc] = atan2(len, dot);
        }
    }
}
// One lane per vertex: its corners' contributions in incidence order, then the division by the length. A non-finite length is flagged.
// `bad` holds the finished vertex and face checks of the launches before: with one of them raised the call will be refused, and nothing is
// written to out (the caller's own memory when the call's pointers are device memory).
template <typename T>
__global__ __launch_bounds__(kBlock) void k_ms_vnormals(const unsigned* __restrict__ inc_pos, const unsigned* __restrict__ inc_ids, const T* __restrict__ fn,
                                                        const T* __restrict__ ang, int mode, int nv, T* __restrict__ out, int* __restrict__ bad) {
    const int i = blockIdx.x * kBlock + threadIdx.x;
    bool nfin = false;
    const bool refused = (__atomic_load_n(bad, __ATOMIC_RELAXED) & (kMeshBadVertex | kMeshBadFace)) != 0;
    if (i < nv) {
        T s[3] = {(T)0, (T)0, (T)0};
        const unsigned end = inc_pos[i + 1];
        for (unsigned j = inc_pos[i]; j < end; ++j) {
            const unsigned c = inc_ids[j], t = c / 3u;
            if (mode == 2) {
                const T a = ang[c];
#pragma unroll
                for (int k = 0; k < 3; ++k) s[k] = s[k] + fn[3 * (size_t)t + k] * a;
            } else {
#pragma unroll
                for (int k = 0; k < 3; ++k) s[k] = s[k] + fn[3 * (size_t)t + k];
            }
        }
        const T r = sqrt(mesh_dot(s, s));
        nfin = !(r - r == (T)0);
        const bool zero = r == (T)0;
#pragma unroll
        for (int k = 0; k < 3; ++k) if (!refused) out[3 * (size_t)i + k] = zero ? (T)0 : s[k] / r;
    }
    if (__ballot(nfin) != 0ull && (threadIdx.x & 63) == 0) atomicOr(bad, kMeshBadNormal);
}

// ---------------------------------------------------------------------------------------------------- the cotangent matrix
template <typename T>
__global__ __launch_bounds__(kBlock) void k_ms_corner_w(const T* __restrict__ v, const int* __restrict__ fidx, int ncorners, T* __restrict__ w) {
    const int c = blockIdx.x * kBlock + threadIdx.x;
    if (c >= ncorners) return;
    const int t = c / 3;
    T len, dot;
    ms_corner(v, fidx, t, c - 3 * t, len, dot);
    w[c] = len == (T)0 ? (T)0 : ((T)0.5 * dot) / len;
}
// One lane per unique entry: the weights of its run of duplicates, in sorted order.
template <typename T>
__global__ __launch_bounds__(kBlock) void k_ms_run_sums(const unsigned long long* __restrict__ keys, const unsigned* __restrict__ ids, int n,
                                                        const unsigned* __restrict__ head_pos, unsigned ne, const T* __restrict__ w, T* __restrict__ val) {
    const unsigned e = blockIdx.x * kBlock + threadIdx.x;
    if (e >= ne) return;
    unsigned j = head_pos[e];
    const unsigned long long k = keys[j];
    T a = (T)0;
    for (; j < (unsigned)n && keys[j] == k; ++j) a = a + w[ids[j] >> 1];
    val[e] = a;
}
template <typename T>
__global__ __launch_bounds__(kBlock) void k_ms_diag(const unsigned* __restrict__ off, const T* __restrict__ val, int nv, T* __restrict__ diag) {
    const int i = blockIdx.x * kBlock + threadIdx.x;
    if (i >= nv) return;
    T a = (T)0;
    const unsigned end = off[i + 1];
    for (unsigned e = off[i]; e < end; ++e) a = a + val[e];
    diag[i] = -a;
}

// ---------------------------------------------------------------------------------------------------- mass, area, rescale
template <typename T>
__global__ __launch_bounds__(kBlock) void k_ms_fill(T* __restrict__ x, int n, T value) {
    const int i = blockIdx.x * kBlock + threadIdx.x;
    if (i < n) x[i] = value;
}
template <typename T>
__global__ __launch_bounds__(kBlock) void k_ms_face_len(const T* __restrict__ u, const int* __restrict__ fidx, int nf, T* __restrict__ len) {
    const int t = blockIdx.x * kBlock + threadIdx.x;
    if (t >= nf) return;
    T N[3];
    len[t] = ms_face_normal(u, fidx, t, N);
}
template <typename T>
__global__ __launch_bounds__(kBlock) void k_ms_mass(const unsigned* __restrict__ inc_pos, const unsigned* __restrict__ inc_ids, const T* __restrict__ len, int nv,
                                                    T* __restrict__ M) {
    const int i = blockIdx.x * kBlock + threadIdx.x;
    if (i >= nv) return;
    T a = (T)0;
    const unsigned end = inc_pos[i + 1];
    for (unsigned j = inc_pos[i]; j < end; ++j) a = a + len[inc_ids[j] / 3u];
    M[i] = a / (T)6;
}
// per block: sum |N|, sum |N| (a + b + c) / 3
template <typename T>
__global__ __launch_bounds__(kBlock) void k_ms_area_parts(const T* __restrict__ u, const int* __restrict__ fidx, int nf, T* __restrict__ part) {
    const int t = blockIdx.x * kBlock + threadIdx.x;
    T a[4] = {(T)0, (T)0, (T)0, (T)0};
    if (t < nf) {
        T N[3];
        const T r = ms_face_normal(u, fidx, t, N);
        const T* p = u + 3 * (size_t)fidx[3 * (size_t)t];
        const T* q = u + 3 * (size_t)fidx[3 * (size_t)t + 1];
        const T* s = u + 3 * (size_t)fidx[3 * (size_t)t + 2];
        a[0] = r;
#pragma unroll
        for (int k = 0; k < 3; ++k) a[k + 1] = r * (((p[k] + q[k]) + s[k]) / (T)3);
    }
    ms_block_fold<T, 4>(a, part + 4 * (size_t)blockIdx.x);
}
// ac = (A, c0, c1, c2)
template <typename T>
__global__ __launch_bounds__(kBlock) void k_ms_area_fold(const T* __restrict__ part, int nb, T* __restrict__ ac) {
    __shared__ T s_t[4];
    ms_fold_parts<T, 4>(part, nb, s_t);
    if (threadIdx.x == 0) {
        ac[0] = (T)0.5 * s_t[0];
#pragma unroll
        for (int k = 0; k < 3; ++k) ac[k + 1] = s_t[k + 1] / s_t[0];
    }
}
template <typename T>
__global__ __launch_bounds__(kBlock) void k_ms_rescale(T* __restrict__ u, const T* __restrict__ M, int nv, const T* __restrict__ ac) {
    const int i = blockIdx.x * kBlock + threadIdx.x;
    if (i >= nv || M[i] == (T)0) return;
    const T s = sqrt(ac[0]);
#pragma unroll
    for (int k = 0; k < 3; ++k) u[3 * (size_t)i + k] = (u[3 * (size_t)i + k] - ac[k + 1]) / s + ac[k + 1];
}

// ---------------------------------------------------------------------------------------------------- conjugate gradients
// (A x)_i = D_i x_i - h * (sum over the row's entries, ascending column, of val x_col), D_i = M_i - h diag_i.
template <typename T>
__device__ __forceinline__ void ms_row(const unsigned* __restrict__ off, const int* __restrict__ col, const T* __restrict__ val, const T* __restrict__ x, int i, T D, T h,
                                       T y[3]) {
    T a[3] = {(T)0, (T)0, (T)0};
    const unsigned end = off[i + 1];
    for (unsigned e = off[i]; e < end; ++e) {
        const T w = val[e];
        const T* xc = x + 3 * (size_t)col[e];
#pragma unroll
        for (int k = 0; k < 3; ++k) a[k] = a[k] + w * xc[k];
    }
#pragma unroll
    for (int k = 0; k < 3; ++k) y[k] = D * x[3 * (size_t)i + k] - h * a[k];
}
// x = u in place; b = M u, D, r = b - A x (0 in the row of a vertex with M == 0), z = r / D, p = z; per block r.z, r.r, b.b
template <typename T>
__global__ __launch_bounds__(kBlock) void k_ms_cg_init(const unsigned* __restrict__ off, const int* __restrict__ col, const T* __restrict__ val, const T* __restrict__ diag,
                                                       const T* __restrict__ M, T h, const T* __restrict__ x, int nv, T* __restrict__ b, T* __restrict__ D,
                                                       T* __restrict__ r, T* __restrict__ z, T* __restrict__ p, T* __restrict__ part) {
    const int i = blockIdx.x * kBlock + threadIdx.x;
    T a[9];
#pragma unroll
    for (int k = 0; k < 9; ++k) a[k] = (T)0;
    if (i < nv) {
        const T m = M[i], d = m - h * diag[i];
        D[i] = d;
        T y[3];
        ms_row(off, col, val, x, i, d, h, y);
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            const T bk = m * x[3 * (size_t)i + k];
            const T rk = m == (T)0 ? (T)0 : bk - y[k];
            const T zk = m == (T)0 ? (T)0 : rk / d;
            b[3 * (size_t)i + k] = bk; r[3 * (size_t)i + k] = rk; z[3 * (size_t)i + k] = zk; p[3 * (size_t)i + k] = zk;
            a[k] = rk * zk; a[3 + k] = rk * rk; a[6 + k] = bk * bk;
        }
    }
    ms_block_fold<T, 9>(a, part + 9 * (size_t)blockIdx.x);
}
template <typename T>
__global__ __launch_bounds__(kBlock) void k_ms_cg_fold_init(const T* __restrict__ part, int nb, MsCg<T>* __restrict__ st) {
    __shared__ T s_t[9];
    ms_fold_parts<T, 9>(part, nb, s_t);
    if (threadIdx.x == 0) {
        const T tol = (T)64 * Limits<T>::eps, tol2 = tol * tol;
        int all = 1;
        for (int k = 0; k < 3; ++k) {
            st->rz[k] = s_t[k]; st->bb[k] = s_t[6 + k]; st->alpha[k] = (T)0; st->beta[k] = (T)0;
            const int d = s_t[3 + k] <= tol2 * s_t[6 + k] ? 1 : 0;
            st->done[k] = d; all &= d;
        }
        st->flag = all ? kMsCgDone : 0;
    }
}
// Ap and per block p.Ap; the row of a vertex with M == 0 gives 0
template <typename T>
__global__ __launch_bounds__(kBlock) void k_ms_cg_spmv(const unsigned* __restrict__ off, const int* __restrict__ col, const T* __restrict__ val, const T* __restrict__ D,
                                                       const T* __restrict__ M, T h, const T* __restrict__ p, int nv, T* __restrict__ Ap, T* __restrict__ part,
                                                       const MsCg<T>* __restrict__ st) {
    if (st->flag) return;                       // (uniform over the grid: every column has stopped)
    const int i = blockIdx.x * kBlock + threadIdx.x;
    T a[3] = {(T)0, (T)0, (T)0};
    if (i < nv) {
        T y[3] = {(T)0, (T)0, (T)0};
        if (M[i] != (T)0) ms_row(off, col, val, p, i, D[i], h, y);
#pragma unroll
        for (int k = 0; k < 3; ++k) { Ap[3 * (size_t)i + k] = y[k]; a[k] = p[3 * (size_t)i + k] * y[k]; }
    }
    ms_block_fold<T, 3>(a, part + 3 * (size_t)blockIdx.x);
}
template <typename T>
__global__ __launch_bounds__(kBlock) void k_ms_cg_fold_a(const T* __restrict__ part, int nb, MsCg<T>* __restrict__ st) {
    if (st->flag) return;
    __shared__ T s_t[3];
    ms_fold_parts<T, 3>(part, nb, s_t);
    if (threadIdx.x == 0) {
        bool broke = false;
        for (int k = 0; k < 3; ++k) {
            if (st->done[k]) continue;
            if (!(s_t[k] > (T)0)) broke = true; else st->alpha[k] = st->rz[k] / s_t[k];
        }
        if (broke) { st->done[0] = st->done[1] = st->done[2] = 1; st->flag = kMsCgBreakdown; }
        else st->iters = st->iters + 1;
    }
}
// x += alpha p, r -= alpha Ap, z = r / D; per block r.z and r.r
template <typename T>
__global__ __launch_bounds__(kBlock) void k_ms_cg_update(const T* __restrict__ D, const T* __restrict__ M, const T* __restrict__ p, const T* __restrict__ Ap, int nv,
                                                         T* __restrict__ x, T* __restrict__ r, T* __restrict__ z, T* __restrict__ part, const MsCg<T>* __restrict__ st) {
    if (st->flag) return;
    const int i = blockIdx.x * kBlock + threadIdx.x;
    T a[6] = {(T)0, (T)0, (T)0, (T)0, (T)0, (T)0};
    if (i < nv && M[i] != (T)0) {
        const T d = D[i];
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            if (st->done[k]) continue;
            const size_t q = 3 * (size_t)i + k;
            const T al = st->alpha[k];
            x[q] = x[q] + al * p[q];
            const T rk = r[q] - al * Ap[q], zk = rk / d;
            r[q] = rk; z[q] = zk;
            a[k] = rk * zk; a[3 + k] = rk * rk;
        }
    }
    ms_block_fold<T, 6>(a, part + 6 * (size_t)blockIdx.x);
}
template <typename T>
__global__ __launch_bounds__(kBlock) void k_ms_cg_fold_b(const T* __restrict__ part, int nb, MsCg<T>* __restrict__ st) {
    if (st->flag) return;
    __shared__ T s_t[6];
    ms_fold_parts<T, 6>(part, nb, s_t);
    if (threadIdx.x == 0) {
        const T tol = (T)64 * Limits<T>::eps, tol2 = tol * tol;
        int all = 1;
        for (int k = 0; k < 3; ++k) {
            if (!st->done[k]) {
                st->beta[k] = s_t[k] / st->rz[k];
                st->rz[k] = s_t[k];
                if (s_t[3 + k] <= tol2 * st->bb[k]) st->done[k] = 1;
            }
            all &= st->done[k];
        }
        if (all) st->flag = kMsCgDone;
    }
}
// p = z + beta p
template <typename T>
__global__ __launch_bounds__(kBlock) void k_ms_cg_direction(const T* __restrict__ z, int nv, T* __restrict__ p, const MsCg<T>* __restrict__ st) {
    if (st->flag) return;
    const int i = blockIdx.x * kBlock + threadIdx.x;
    if (i >= nv) return;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        if (st->done[k]) continue;
        const size_t q = 3 * (size_t)i + k;
        p[q] = z[q] + st->beta[k] * p[q];
    }
}

}  // namespace pcu
