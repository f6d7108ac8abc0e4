// csrc/pc_winding_host.h -- host orchestration of point_cloud_fast_winding_number and estimate_mesh_face_normals (kernels and contract:
// pc_winding.h). The dipole tree is a MeshIdx whose elements are points: its handle, its create and its calls go through the frames of
// mesh_host.h (TreeIndex, tree_index_create, tree_call), the rows through mesh_run like the mesh operators'. Included by pcu_hip.hip after
// mesh_host.h and mesh_sample_host.h.
#pragma once

// An oriented point cloud kept on the GPU as its dipole tree (pcu_hip_pc_winding_index_*): the TreeIndex of mesh_host.h over points.
struct pcu_hip_pc_winding_index : TreeIndex {};
// head, 6 T per point, and per node its box, centre and radius, moments (40 T per node: about 10 per point)
template <typename T>
static size_t pc_index_bytes(int64_t np) {
    const size_t N = (size_t)np, P = (size_t)leaves_pow2(np, kPcLeaf);
    return align_up(sizeof(MeshHead<T>), 256) + align_up(N * 6 * sizeof(T), 256) + align_up(2 * P * 6 * sizeof(T), 256) + align_up(2 * P * 4 * sizeof(T), 256) +
           align_up(2 * P * 30 * sizeof(T), 256) + 1024;
}
// the sort, the nodes' weights and, for host arrays, p, n and a staged
template <typename T>
static size_t pc_build_bytes(int64_t np, bool on_dev) {
    size_t b = sort_bytes((size_t)np) + align_up(2 * (size_t)leaves_pow2(np, kPcLeaf) * sizeof(double), 256) + 4096;
    if (!on_dev) b += 2 * align_up((size_t)np * 3 * sizeof(T), 256) + align_up((size_t)np * sizeof(T), 256);
    return b;
}
static int pc_zero_rows() {     // validate_point_cloud(..., allow_0=false) (src/common/common.h:58-66)
    return fail(PCU_HIP_ERR_INVALID, "Invalid input point cloud with zero points: points must have shape (n, 3) (n > 0). Got points.shape =(0, 3).");
}
static int pc_validate_rows(int64_t n) {
    if (n <= 0) return pc_zero_rows();
    return n > kMeshMaxRows ? mesh_row_limit() : 0;
}

// Enqueues the build on s and waits once (the validity flags). `ari` gives the buffers of the index, `ar` the temporaries.
template <typename T>
static int pc_build(Arena& ari, Arena& ar, hipStream_t s, const T* p, const T* n, const T* a, int64_t np, bool on_dev, MeshIdx<T>& M) {
    const T *dp = nullptr, *dn = nullptr, *da = nullptr;
    if (stage_in(ar, p, np, on_dev, s, &dp) || stage_in(ar, n, np, on_dev, s, &dn) || stage_any(ar, a, (size_t)np, on_dev, s, &da)) return -1;
    M.nf = (int)np; M.P = leaves_pow2(np, kPcLeaf);
    double* weight = nullptr;
    unsigned long long *ka = nullptr, *kb = nullptr; unsigned *ia = nullptr, *ib = nullptr;
    if (aalloc(ari, &M.head, 1) || aalloc(ari, &M.tri, (size_t)np * 6) || aalloc(ari, &M.box, (size_t)M.P * 12) || aalloc(ari, &M.ctr, (size_t)M.P * 8) ||
        aalloc(ari, &M.mom, (size_t)M.P * 60) || aalloc(ar, &weight, (size_t)M.P * 2) ||
        aalloc(ar, &ka, (size_t)np) || aalloc(ar, &kb, (size_t)np) || aalloc(ar, &ia, (size_t)np) || aalloc(ar, &ib, (size_t)np)) return -1;
    const unsigned nbp = blocks_for((size_t)np), nbl = blocks_for((size_t)M.P);
    int* d_bad = mesh_head_flag(M.head);
    hipLaunchKernelGGL(k_mesh_head_init<T>, dim3(1), dim3(64), 0, s, M.head);
    hipLaunchKernelGGL(k_pc_check<T>, dim3(nbp), dim3(kBlock), 0, s, dp, dn, da, (int)np, M.head);
    hipLaunchKernelGGL(k_mesh_frame<T>, dim3(1), dim3(64), 0, s, M.head);
    hipLaunchKernelGGL(k_pc_codes<T>, dim3(nbp), dim3(kBlock), 0, s, dp, (int)np, (const MeshHead<T>*)M.head, ka);
    HIP_TRY(hipGetLastError());
    if (own_radix_sort(ar, s, &ka, &kb, &ia, &ib, /*ids_identity=*/true, (int)np, 63)) return -1;
    hipLaunchKernelGGL(k_pc_gather<T>, dim3(nbp), dim3(kBlock), 0, s, dp, dn, da, (const unsigned*)ia, (int)np, M.tri, d_bad);
    hipLaunchKernelGGL(k_pc_leaves<T>, dim3(nbl), dim3(kBlock), 0, s, (const T*)M.tri, (int)np, M.P, M.box);
    for (int m = M.P / 2; m >= 1; m /= 2) hipLaunchKernelGGL(k_mesh_refit<T>, dim3(blocks_for((size_t)m)), dim3(kBlock), 0, s, M.box, m);
    hipLaunchKernelGGL(k_pc_mleaves<T>, dim3(nbl), dim3(kBlock), 0, s, (const T*)M.tri, (int)np, M.P, (const T*)M.box, M.ctr, M.mom, weight);
    for (int m = M.P / 2; m >= 1; m /= 2)
        hipLaunchKernelGGL(k_mesh_mrefit<T>, dim3(blocks_for((size_t)m)), dim3(kBlock), 0, s, (const T*)M.box, M.ctr, M.mom, weight, m);
    HIP_TRY(hipGetLastError());
    int bad = 0;
    if (flag_fetch(s, d_bad, &bad)) return -1;
    HIP_WAIT(s);
    if (bad & kPcBadP) return fail(PCU_HIP_ERR_INVALID, "p must not contain NaN or infinite coordinates");
    if (bad & kPcBadN) return fail(PCU_HIP_ERR_INVALID, "n must not contain NaN or infinite coordinates");
    if (bad & kPcBadA) return fail(PCU_HIP_ERR_INVALID, "a must not contain NaN or infinite values");
    if (bad & kPcBadD) return fail(PCU_HIP_ERR_INVALID, "a * n overflows the scalar type of p");
    return 0;
}

static int pc_beta_check(double beta) {
    return beta > 0.0 ? 0 : fail(PCU_HIP_ERR_INVALID, "beta must be greater than 0 (finite, or +inf for the plain sum over all points)");
}
template <typename T>
struct PcWindingOp : MeshPointsOp<T> {          // point_cloud_fast_winding_number (src/fast_winding_numbers.cpp:51-67): one T per row
    double beta;
    using Params = MeshSigned<T>;
    static constexpr int kRows3 = 1;
    static constexpr bool kMoments = true, kFaces = false;
    int validate(int64_t n) const { if (int rc = pc_beta_check(beta)) return rc; return pc_validate_rows(n); }
    void walk(hipStream_t s, MeshSigned<T> a, T* val, int64_t n) const {
        a.p = this->p; a.np = (int)n; a.beta = (T)beta; a.out_val = val;
        hipLaunchKernelGGL(k_pc_winding<T>, dim3((unsigned)((n + kMeshBlock - 1) / kMeshBlock)), dim3(kMeshBlock), 0, s, a);
    }
    static int message(int) { return fail(PCU_HIP_ERR_INVALID, "q must not contain NaN or infinite coordinates"); }
};

// One call, the cloud given (`pc`) or its index (`ix`).
template <typename T> struct PcGiven { const T* p; const T* n; const T* a; int64_t np; };
template <typename T>
static int pc_call(pcu_hip_ctx* c, const PcGiven<T>* pc, const pcu_hip_pc_winding_index* ix, const T* q, int64_t nq, double beta, T* out_w, unsigned flags,
                   void* stream, pcu_hip_stats* st) {
    if (int rc = tree_index_check<T>(c, ix, pc != nullptr, "point cloud winding index", st)) return rc;
    PcWindingOp<T> op{{q}, beta};
    if (pc) { if (int rc = pc_validate_rows(pc->np)) return rc; }
    if (int rc = op.validate(nq)) return rc;
    const size_t given = pc ? pc_index_bytes<T>(pc->np) + pc_build_bytes<T>(pc->np, flags & PCU_HIP_PTRS_ON_DEVICE) : 0;
    return tree_call<T>(c, flags, stream, st, pc ? nullptr : ix, given, [&](Arena& ar, hipStream_t s, bool on_dev, MeshIdx<T>& built, PcWindingOp<T>&) {
        return pc_build<T>(ar, ar, s, pc->p, pc->n, pc->a, pc->np, on_dev, built);
    }, op, nq, out_w, nullptr, nullptr);
}

template <typename T>
static int pc_index_create_impl(pcu_hip_ctx* c, const T* p, const T* n, const T* a, int64_t np, unsigned flags, void* stream, pcu_hip_pc_winding_index** out) {
    if (int rc = index_out_begin(c, out)) return rc;
    if (int rc = pc_validate_rows(np)) return rc;
    const bool on_dev = flags & PCU_HIP_PTRS_ON_DEVICE;
    return tree_index_create<T>(c, flags, stream, np, pc_index_bytes<T>(np), pc_build_bytes<T>(np, on_dev), "point cloud winding index", out,
                                [&](Arena& ari, Arena& ar, hipStream_t s, pcu_hip_pc_winding_index& h) {
        return pc_build<T>(ari, ar, s, p, n, a, np, on_dev, tree_idx<T>(&h));
    });
}

// estimate_mesh_face_normals (src/mesh_normals.cpp:65-80)
template <typename T>
static int mesh_face_normals_impl(pcu_hip_ctx* c, const MeshGiven<T>& m, T* out_n, unsigned flags, void* stream, pcu_hip_stats* st) {
    if (!c) return fail(PCU_HIP_ERR_INVALID, "null context");
    if (int rc = mesh_validate(m.nv, m.nf, 0, m.f_kind)) return rc;
    const bool on_dev = flags & PCU_HIP_PTRS_ON_DEVICE;
    return op_run(c, flags, stream, st, ms_mesh_bytes(m, on_dev) + (on_dev ? 0 : align_up((size_t)m.nf * 3 * sizeof(T), 256)), [&](OpFrame& fr) -> int {
        auto& [c, s, on_dev, ar, tm] = fr;
        MsMesh<T> M; MsSeen<T> seen;
        if (ms_mesh_stage<T>(ar, s, m, on_dev, M)) return -1;
        T* d_n = nullptr;
        if (out_room(ar, on_dev, out_n, (size_t)m.nf * 3, &d_n)) return -1;
        hipLaunchKernelGGL(k_mesh_fnormals<T>, dim3(blocks_for((size_t)m.nf)), dim3(kBlock), 0, s, M.v, (const int*)M.fidx, (int)m.nf, d_n, mesh_head_flag(M.head));
        HIP_TRY(hipGetLastError());
        if (ms_mesh_readback(s, M, false, &seen) || out_give(s, on_dev, out_n, d_n, (size_t)m.nf * 3)) return -1;
        HIP_WAIT(s);
        if (int rc = ms_mesh_refuse(seen, m.nv, false)) return rc;
        if (seen.bad & kMeshBadNormal) return fail(PCU_HIP_ERR_INVALID, "face normals overflow the scalar type of v");
        if (st) { st->n_queries = m.nf; st->n_passes = 1; }
        return 0;
    });
}
