// csrc/pc_winding_host.h -- host orchestration of point_cloud_fast_winding_number and estimate_mesh_face_normals (kernels and contract:
// pc_winding.h). The dipole tree is a MeshIdx whose elements are points: the rows go through mesh_run like the mesh operators'. Included by
// pcu_hip.hip after mesh_host.h and mesh_sample_host.h.
#pragma once

// An oriented point cloud kept on the GPU as its dipole tree (pcu_hip_pc_winding_index_*): one block owned by the object.
struct pcu_hip_pc_winding_index {
    int elem_size = 0;            // 4: float, 8: double
    int device = 0;
    int64_t np = 0;
    void* mem = nullptr;
    MeshIdx<float> m32; MeshIdx<double> m64;
};
template <typename T> static const MeshIdx<T>& pc_idx(const pcu_hip_pc_winding_index* p);
template <> const MeshIdx<float>& pc_idx<float>(const pcu_hip_pc_winding_index* p) { return p->m32; }
template <> const MeshIdx<double>& pc_idx<double>(const pcu_hip_pc_winding_index* p) { return p->m64; }
static void pc_index_free(pcu_hip_pc_winding_index* p) {
    if (!p) return;
    if (p->mem) (void)hipFree(p->mem);
    delete p;
}
static int pc_leaves_pow2(int64_t np) {
    const int64_t leaves = (np + kPcLeaf - 1) / kPcLeaf;
    int P = 1;
    while (P < leaves) P <<= 1;
    return P;
}
// head, 6 T per point, and per node its box, centre and radius, moments (40 T per node: about 10 per point)
template <typename T>
static size_t pc_index_bytes(int64_t np) {
    const size_t N = (size_t)np, P = (size_t)pc_leaves_pow2(np);
    return align_up(sizeof(MeshHead<T>), 256) + align_up(N * 6 * sizeof(T), 256) + align_up(2 * P * 6 * sizeof(T), 256) + align_up(2 * P * 4 * sizeof(T), 256) +
           align_up(2 * P * 30 * sizeof(T), 256) + 1024;
}
// the sort, the nodes' weights and, for host arrays, p, n and a staged
template <typename T>
static size_t pc_build_bytes(int64_t np, bool on_dev) {
    size_t b = sort_bytes((size_t)np) + align_up(2 * (size_t)pc_leaves_pow2(np) * sizeof(double), 256) + 4096;
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
    M.nf = (int)np; M.P = pc_leaves_pow2(np);
    double* weight = nullptr;
    unsigned long long *ka = nullptr, *kb = nullptr; unsigned *ia = nullptr, *ib = nullptr;
    if (aalloc(ari, &M.head, 1) || aalloc(ari, &M.tri, (size_t)np * 6) || aalloc(ari, &M.box, (size_t)M.P * 12) || aalloc(ari, &M.ctr, (size_t)M.P * 8) ||
        aalloc(ari, &M.mom, (size_t)M.P * 60) || aalloc(ar, &weight, (size_t)M.P * 2) ||
        aalloc(ar, &ka, (size_t)np) || aalloc(ar, &kb, (size_t)np) || aalloc(ar, &ia, (size_t)np) || aalloc(ar, &ib, (size_t)np)) return -1;
    const int nbp = (int)((np + kBlock - 1) / kBlock), nbl = (M.P + kBlock - 1) / kBlock;
    int* d_bad = reinterpret_cast<int*>(reinterpret_cast<char*>(M.head) + offsetof(MeshHead<T>, bad));
    hipLaunchKernelGGL(k_mesh_head_init<T>, dim3(1), dim3(64), 0, s, M.head);
    hipLaunchKernelGGL(k_pc_check<T>, dim3(nbp), dim3(kBlock), 0, s, dp, dn, da, (int)np, M.head);
    hipLaunchKernelGGL(k_mesh_frame<T>, dim3(1), dim3(64), 0, s, M.head);
    hipLaunchKernelGGL(k_pc_codes<T>, dim3(nbp), dim3(kBlock), 0, s, dp, (int)np, (const MeshHead<T>*)M.head, ka);
    HIP_TRY(hipGetLastError());
    if (own_radix_sort(ar, s, &ka, &kb, &ia, &ib, /*ids_identity=*/true, (int)np, 63)) return -1;
    hipLaunchKernelGGL(k_pc_gather<T>, dim3(nbp), dim3(kBlock), 0, s, dp, dn, da, (const unsigned*)ia, (int)np, M.tri, d_bad);
    hipLaunchKernelGGL(k_pc_leaves<T>, dim3(nbl), dim3(kBlock), 0, s, (const T*)M.tri, (int)np, M.P, M.box);
    for (int m = M.P / 2; m >= 1; m /= 2) hipLaunchKernelGGL(k_mesh_refit<T>, dim3((m + kBlock - 1) / kBlock), dim3(kBlock), 0, s, M.box, m);
    hipLaunchKernelGGL(k_pc_mleaves<T>, dim3(nbl), dim3(kBlock), 0, s, (const T*)M.tri, (int)np, M.P, (const T*)M.box, M.ctr, M.mom, weight);
    for (int m = M.P / 2; m >= 1; m /= 2)
        hipLaunchKernelGGL(k_mesh_mrefit<T>, dim3((m + kBlock - 1) / kBlock), dim3(kBlock), 0, s, (const T*)M.box, M.ctr, M.mom, weight, m);
    HIP_TRY(hipGetLastError());
    int bad = 0;
    HIP_TRY(hipMemcpyAsync(&bad, d_bad, sizeof(int), hipMemcpyDeviceToHost, s));
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

// One call. Cloud given (`pc`): tree, rows and temporaries in the call's arena; index given (`ix`): rows and temporaries.
template <typename T> struct PcGiven { const T* p; const T* n; const T* a; int64_t np; };
template <typename T>
static int pc_call(pcu_hip_ctx* c, const PcGiven<T>* pc, const pcu_hip_pc_winding_index* ix, const T* q, int64_t nq, double beta, T* out_w, unsigned flags,
                   void* stream, pcu_hip_stats* st) {
    if (pc ? !c : (!c || !ix)) return fail(PCU_HIP_ERR_INVALID, pc ? "null context" : "null context / point cloud winding index");
    if (st) memset(st, 0, sizeof *st);
    if (!pc) {
        if (ix->elem_size != (int)sizeof(T)) return fail(PCU_HIP_ERR_INVALID, "the point cloud winding index was built for the other scalar type");
        if (ix->device != c->device) return fail(PCU_HIP_ERR_INVALID, "the point cloud winding index lives on another device than the context");
    }
    PcWindingOp<T> op{{q}, beta};
    if (pc) { if (int rc = pc_validate_rows(pc->np)) return rc; }
    if (int rc = op.validate(nq)) return rc;
    const bool on_dev = flags & PCU_HIP_PTRS_ON_DEVICE;
    size_t bytes = mesh_run_bytes<T>(nq, 1, on_dev);
    if (pc) bytes += pc_index_bytes<T>(pc->np) + pc_build_bytes<T>(pc->np, on_dev);
    return op_run(c, flags, stream, st, bytes, [&](OpFrame& fr) -> int {
        auto& [c, s, on_dev, ar, tm] = fr;
        MeshIdx<T> built;
        if (pc) { tm.mark(0); if (int rc = pc_build<T>(ar, ar, s, pc->p, pc->n, pc->a, pc->np, on_dev, built)) return rc; }
        if (int rc = mesh_run<T>(ar, s, pc ? built : pc_idx<T>(ix), op, nq, on_dev, out_w, nullptr, nullptr, tm)) return rc;
        mesh_stats(st, tm, nq, pc != nullptr);
        return 0;
    });
}

template <typename T>
static int pc_index_create_impl(pcu_hip_ctx* c, const T* p, const T* n, const T* a, int64_t np, unsigned flags, void* stream, pcu_hip_pc_winding_index** out) {
    if (!c || !out) return fail(PCU_HIP_ERR_INVALID, "null context / output");
    *out = nullptr;
    if (int rc = pc_validate_rows(np)) return rc;
    const bool on_dev = flags & PCU_HIP_PTRS_ON_DEVICE;
    hipStream_t s = pick_stream(c, flags, stream);
    pcu_hip_pc_winding_index* h = new pcu_hip_pc_winding_index();
    h->elem_size = (int)sizeof(T); h->device = c->device; h->np = np;
    const size_t bytes = pc_index_bytes<T>(np);
    if (hipMalloc(&h->mem, bytes) != hipSuccess) { h->mem = nullptr; pc_index_free(h); return fail(PCU_HIP_ERR_RUNTIME, "out of device memory for the point cloud winding index"); }
    if (ctx_begin(c, pc_build_bytes<T>(np, on_dev))) { pc_index_free(h); return PCU_HIP_ERR_RUNTIME; }
    ArenaState blk;                                 // a bump allocator over the index's own block
    blk.base = static_cast<char*>(h->mem); blk.cap = bytes;
    Arena ari{&blk}, ar{c};
    int rc = pc_build<T>(ari, ar, s, p, n, a, np, on_dev, const_cast<MeshIdx<T>&>(pc_idx<T>(h)));
    if (!rc) rc = wait_stream(s);                   // (the temporaries go back to the context with this call)
    rc = attempt_exit(c, index_block_exit(blk, rc, "point cloud winding index"));
    if (rc) { (void)hipStreamSynchronize(s); pc_index_free(h); return rc; }
    *out = h;
    return 0;
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
        T* d_n = out_n;
        if (!on_dev && aalloc(ar, &d_n, (size_t)m.nf * 3)) return -1;
        int* d_bad = reinterpret_cast<int*>(reinterpret_cast<char*>(M.head) + offsetof(MeshHead<T>, bad));
        hipLaunchKernelGGL(k_mesh_fnormals<T>, dim3((unsigned)((m.nf + kBlock - 1) / kBlock)), dim3(kBlock), 0, s, M.v, (const int*)M.fidx, (int)m.nf, d_n, d_bad);
        HIP_TRY(hipGetLastError());
        if (ms_mesh_readback(s, M, false, &seen)) return -1;
        if (!on_dev) HIP_TRY(hipMemcpyAsync(out_n, d_n, (size_t)m.nf * 3 * sizeof(T), hipMemcpyDeviceToHost, s));
        HIP_WAIT(s);
        if (int rc = ms_mesh_refuse(seen, m.nv, false)) return rc;
        if (seen.bad & kMeshBadNormal) return fail(PCU_HIP_ERR_INVALID, "face normals overflow the scalar type of v");
        if (st) { st->n_queries = m.nf; st->n_passes = 1; }
        return 0;
    });
}
