// csrc/mesh_smooth_host.h -- host orchestration of mesh_vertex_adjacency / adjacency_list, estimate_mesh_vertex_normals and
// laplacian_smooth_mesh (kernels and contract: mesh_smooth.h). Included by pcu_hip.hip after the operator frame and the parking functions,
// voxel_host.h (sort_bytes, scan_bytes, sort_keys, rank_flags) and mesh_host.h (mesh_validate, MeshGiven).
#pragma once

constexpr int kMsCgMaxIters = 4096;             // a chosen cap that nobody has timed
constexpr int kMsCgPoll = 8;                    // the host reads the solver's flag word every so many iterations

// faces and incidence
static size_t ms_incidence_bytes(size_t nv, size_t nf) { return align_up(nf * 12, 256) + sort_bytes(3 * nf) + align_up((nv + 1) * 4, 256) + 4096; }
// the pair sort and the CSR (with room for every pair to be an entry)
static size_t ms_adjacency_bytes(size_t nv, size_t nf) {
    return sort_bytes(6 * nf) + 4 * align_up(6 * nf * 4, 256) + scan_bytes(6 * nf) + 2 * align_up((nv + 1) * 4, 256) + 4096;
}

struct MsStructure {
    int* fidx = nullptr;                                    // (nf, 3) range-checked faces
    int* d_bad = nullptr;                                   // kMeshBad*
    unsigned long long* ckeys = nullptr;                    // the corner keys, sorted by ms_incidence
    unsigned *inc_pos = nullptr, *inc_ids = nullptr;        // incidence: corners inc_ids[inc_pos[i] .. inc_pos[i + 1]) of vertex i
    unsigned long long* pkeys = nullptr; unsigned* pids = nullptr; int K = 0;      // the sorted directed pairs and their positions before the sort
    unsigned *off = nullptr, *head_pos = nullptr; int* col = nullptr; unsigned ne = 0;     // CSR of the unique entries; where each entry's run starts
    int hb = 0;
};

// Stages f, checks its range and writes the corner keys. No wait.
static int ms_faces(Arena& ar, hipStream_t s, const void* f, int64_t nf, int f_kind, int64_t nv, bool on_dev, MsStructure& S) {
    const char* d_f = nullptr;
    if (stage_faces(ar, f, (size_t)nf, f_kind, on_dev, s, &d_f)) return -1;
    if (aalloc(ar, &S.fidx, (size_t)nf * 3) || aalloc(ar, &S.ckeys, (size_t)nf * 3) || flag_word(ar, s, &S.d_bad)) return -1;
    S.hb = bits_of((unsigned long long)(nv - 1));
    hipLaunchKernelGGL(k_ms_corners, dim3(blocks_for((size_t)nf)), dim3(kBlock), 0, s, (const void*)d_f, f_kind, (int)nf, (int)nv, S.fidx, S.ckeys, S.d_bad);
    HIP_TRY(hipGetLastError());
    return 0;
}
// The incidence: one stable sort of the corner keys, one binary search per vertex. No wait.
static int ms_incidence(Arena& ar, hipStream_t s, int64_t nf, int64_t nv, MsStructure& S) {
    const int C = (int)(3 * nf);
    SortedRuns r; r.keys = S.ckeys;
    if (aalloc(ar, &S.inc_pos, (size_t)nv + 1) || sort_keys(ar, s, r, C, std::max(S.hb, 1))) return -1;
    S.ckeys = r.keys; S.inc_ids = r.ids;
    hipLaunchKernelGGL(k_ms_row_starts, dim3(blocks_for((size_t)nv + 1)), dim3(kBlock), 0, s, (const unsigned long long*)S.ckeys, C, 0, (int)nv, S.inc_pos);
    HIP_TRY(hipGetLastError());
    return 0;
}
// The adjacency as CSR. One wait: the flag word and the number of unique entries; a refused mesh returns its error here.
static int ms_adjacency(Arena& ar, hipStream_t s, int64_t nf, int64_t nv, MsStructure& S) {
    const int K = (int)(6 * nf);
    S.K = K;
    SortedRuns r; unsigned* pos = nullptr;
    if (aalloc(ar, &r.keys, (size_t)K) || aalloc(ar, &pos, (size_t)nv + 1) || aalloc(ar, &S.off, (size_t)nv + 1)) return -1;
    hipLaunchKernelGGL(k_ms_pairs, dim3(blocks_for((size_t)K / 2)), dim3(kBlock), 0, s, (const int*)S.fidx, K / 2, S.hb, r.keys);
    if (sort_keys(ar, s, r, K, std::max(2 * S.hb, 1))) return -1;
    S.pkeys = r.keys; S.pids = r.ids;
    if (rank_flags(ar, s, r, K, [&](unsigned* flag) {
            hipLaunchKernelGGL(k_ms_pair_heads, dim3(blocks_for((size_t)K)), dim3(kBlock), 0, s, (const unsigned long long*)S.pkeys, K, S.hb, flag);
        })) return -1;
    unsigned *flag = r.flag, *scan = r.scan;
    hipLaunchKernelGGL(k_ms_row_starts, dim3(blocks_for((size_t)nv + 1)), dim3(kBlock), 0, s, (const unsigned long long*)S.pkeys, K, S.hb, (int)nv, pos);
    hipLaunchKernelGGL(k_ms_offsets, dim3(blocks_for((size_t)nv + 1)), dim3(kBlock), 0, s, (const unsigned*)pos, (const unsigned*)scan, (int)nv, S.off);
    HIP_TRY(hipGetLastError());
    int bad = 0; unsigned ne = 0;
    if (read_flag_and_last(s, S.d_bad, scan, (size_t)K, &bad, &ne)) return -1;
    HIP_WAIT(s);
    if (bad) return mesh_refusal(bad, nv);
    S.ne = ne;
    if (aalloc(ar, &S.head_pos, (size_t)ne) || aalloc(ar, &S.col, (size_t)ne)) return -1;
    if (ne > 0) {
        hipLaunchKernelGGL(k_ms_entries, dim3(blocks_for((size_t)K)), dim3(kBlock), 0, s, (const unsigned long long*)S.pkeys, (const unsigned*)flag, (const unsigned*)scan, K, S.hb,
                           S.head_pos, S.col);
        HIP_TRY(hipGetLastError());
    }
    return 0;
}

// mesh_vertex_adjacency. The CSR is parked for pcu_hip_mesh_adjacency_take: (nv + 1) int64 offsets, then *out_count
// neighbours in the faces' integer type.
static int mesh_adjacency_impl(pcu_hip_ctx* c, const void* f, int64_t nf, int f_kind, int64_t nv, int64_t* out_count, unsigned flags, void* stream, pcu_hip_stats* st) {
    if (!c || !out_count) return fail(PCU_HIP_ERR_INVALID, "null context / out_count");
    *out_count = 0;
    c->parked = ParkedResult();
    if (int rc = mesh_validate(nv, nf, 0, f_kind)) return rc;
    if (!f) return fail(PCU_HIP_ERR_INVALID, "null f");
    const bool on_dev = flags & PCU_HIP_PTRS_ON_DEVICE;
    const size_t NV = (size_t)nv, NF = (size_t)nf, kb = (size_t)int_kind_bytes(f_kind);
    const size_t bytes = (on_dev ? 0 : align_up(NF * 3 * kb, 256)) + align_up(NF * 12, 256) + align_up(NF * 24, 256) + ms_adjacency_bytes(NV, NF) + 8192;
    return op_run(c, flags, stream, st, bytes, [&](OpFrame& fr) -> int {
        auto& [c, s, on_dev, ar, tm] = fr;      // marks 0-1: faces, keys, sort, heads, scan, offsets and the wait, 1-2: entries and the parked copy
        MsStructure S;
        tm.mark(0);
        if (ms_faces(ar, s, f, nf, f_kind, nv, on_dev, S)) return -1;
        if (int rc = ms_adjacency(ar, s, nf, nv, S)) return rc;
        tm.mark(1);
        char* seg[kParkSegs];
        if (park_reserve(c, {(NV + 1) * 8, (size_t)S.ne * kb}, seg)) return -1;
        hipLaunchKernelGGL(k_ms_adj_out, dim3(blocks_for(std::max(NV + 1, (size_t)S.ne))), dim3(kBlock), 0, s, (const unsigned*)S.off, (int)nv, (const int*)S.col, S.ne, f_kind,
                           reinterpret_cast<long long*>(seg[0]), (void*)seg[1]);
        HIP_TRY(hipGetLastError());
        tm.mark(2);
        HIP_WAIT(s);
        park_commit(c, Parked::Adjacency, nv, (int64_t)S.ne);
        *out_count = (int64_t)S.ne;
        if (st) { st->n_queries = nf; st->n_escalated = (int64_t)S.ne; st->n_passes = 1; st->ms_index = tm.span(0, 1); st->ms_search = tm.span(1, 2); st->ms_total = tm.span(0, 2); }
        return 0;
    });
}
// The result of this context's last pcu_hip_mesh_adjacency. Once.
static int mesh_adjacency_take_impl(pcu_hip_ctx* c, int64_t nv, int64_t count, int64_t* out_offsets, void* out_neighbours, unsigned flags, void* stream) {
    if (!c || !out_offsets || (!out_neighbours && count > 0)) return fail(PCU_HIP_ERR_INVALID, "null context / out_offsets / out_neighbours");
    return park_take(c, Parked::Adjacency, nv, count, {out_offsets, out_neighbours}, flags, stream,
                     "pcu_hip_mesh_adjacency_take: this context holds no adjacency of %lld vertices and %lld entries");
}

// estimate_mesh_vertex_normals (src/mesh_normals.cpp:24-50). weighting: 0 uniform, 1 area, 2 angle.
template <typename T>
static int mesh_vertex_normals_impl(pcu_hip_ctx* c, const MeshGiven<T>& m, int weighting, T* out_n, unsigned flags, void* stream, pcu_hip_stats* st) {
    if (!c) return fail(PCU_HIP_ERR_INVALID, "null context");
    if (int rc = mesh_validate(m.nv, m.nf, 0, m.f_kind)) return rc;
    if (weighting < 0 || weighting > 2) return fail(PCU_HIP_ERR_INVALID, "weighting must be 0 (uniform), 1 (area) or 2 (angle)");
    if (!m.v || !m.f || !out_n) return fail(PCU_HIP_ERR_INVALID, "null v / f / out_n");
    const bool on_dev = flags & PCU_HIP_PTRS_ON_DEVICE;
    const size_t NV = (size_t)m.nv, NF = (size_t)m.nf;
    size_t bytes = ms_incidence_bytes(NV, NF) + align_up(NF * 24, 256) + 2 * align_up(NF * 3 * sizeof(T), 256) + 8192;
    if (!on_dev) bytes += 2 * align_up(NV * 3 * sizeof(T), 256) + align_up(NF * 3 * int_kind_bytes(m.f_kind), 256);
    return op_run(c, flags, stream, st, bytes, [&](OpFrame& fr) -> int {
        auto& [c, s, on_dev, ar, tm] = fr;      // marks 0-1: checks and incidence, 1-2: per-face vectors and the gather
        MsStructure S;
        const T* dv = nullptr;
        tm.mark(0);
        if (stage_in(ar, m.v, m.nv, on_dev, s, &dv) || ms_faces(ar, s, m.f, m.nf, m.f_kind, m.nv, on_dev, S)) return -1;
        hipLaunchKernelGGL(k_mesh_vcheck<T>, dim3(blocks_for(NV * 3)), dim3(kBlock), 0, s, dv, (long long)NV * 3, S.d_bad, kMeshBadVertex);
        if (ms_incidence(ar, s, m.nf, m.nv, S)) return -1;
        tm.mark(1);
        T *fn = nullptr, *ang = nullptr, *d_n = nullptr;
        if (aalloc(ar, &fn, NF * 3) || (weighting == 2 && aalloc(ar, &ang, NF * 3)) || out_room(ar, on_dev, out_n, NV * 3, &d_n)) return -1;
        hipLaunchKernelGGL(k_ms_face_vec<T>, dim3(blocks_for(NF)), dim3(kBlock), 0, s, dv, (const int*)S.fidx, (int)m.nf, weighting, fn, ang);
        hipLaunchKernelGGL(k_ms_vnormals<T>, dim3(blocks_for(NV)), dim3(kBlock), 0, s, (const unsigned*)S.inc_pos, (const unsigned*)S.inc_ids, (const T*)fn, (const T*)ang,
                           weighting, (int)m.nv, d_n, S.d_bad);
        HIP_TRY(hipGetLastError());
        tm.mark(2);
        int bad = 0;
        if (flag_fetch(s, S.d_bad, &bad) || out_give(s, on_dev, out_n, d_n, NV * 3)) return -1;
        HIP_WAIT(s);
        if (int rc = mesh_refusal(bad, m.nv)) return rc;
        if (bad & kMeshBadNormal) return fail(PCU_HIP_ERR_INVALID, "vertex normals overflow the scalar type of v");
        if (st) { st->n_queries = m.nv; st->n_passes = 1; st->ms_index = tm.span(0, 1); st->ms_search = tm.span(1, 2); st->ms_total = tm.span(0, 2); }
        return 0;
    });
}

// One solve of (M - h L) x = M x in place, enqueued in pieces: the host looks at the flag word every kMsCgPoll iterations.
template <typename T>
struct MsSolve {
    const unsigned* off; const int* col; const T *val, *diag; T *M, *b, *D, *r, *z, *p, *Ap, *part; MsCg<T>* cg; int nv; T h;
};
template <typename T>
static int ms_solve(hipStream_t s, const MsSolve<T>& q, T* x) {
    const unsigned nb = blocks_for((size_t)q.nv);
    hipLaunchKernelGGL(k_ms_cg_init<T>, dim3(nb), dim3(kBlock), 0, s, q.off, q.col, q.val, q.diag, (const T*)q.M, q.h, (const T*)x, q.nv, q.b, q.D, q.r, q.z, q.p, q.part);
    hipLaunchKernelGGL(k_ms_cg_fold_init<T>, dim3(1), dim3(kBlock), 0, s, (const T*)q.part, (int)nb, q.cg);
    int seen[2] = {0, 0};           // flag, iters
    for (int it = 0; it <= kMsCgMaxIters; ++it) {
        if (it % kMsCgPoll == 0 || it == kMsCgMaxIters) {
            HIP_TRY(hipGetLastError());
            HIP_TRY(hipMemcpyAsync(seen, &q.cg->flag, 2 * sizeof(int), hipMemcpyDeviceToHost, s));
            HIP_WAIT(s);
            if (seen[0] || it == kMsCgMaxIters) break;
        }
        hipLaunchKernelGGL(k_ms_cg_spmv<T>, dim3(nb), dim3(kBlock), 0, s, q.off, q.col, q.val, (const T*)q.D, (const T*)q.M, q.h, (const T*)q.p, q.nv, q.Ap, q.part,
                           (const MsCg<T>*)q.cg);
        hipLaunchKernelGGL(k_ms_cg_fold_a<T>, dim3(1), dim3(kBlock), 0, s, (const T*)q.part, (int)nb, q.cg);
        hipLaunchKernelGGL(k_ms_cg_update<T>, dim3(nb), dim3(kBlock), 0, s, (const T*)q.D, (const T*)q.M, (const T*)q.p, (const T*)q.Ap, q.nv, x, q.r, q.z, q.part,
                           (const MsCg<T>*)q.cg);
        hipLaunchKernelGGL(k_ms_cg_fold_b<T>, dim3(1), dim3(kBlock), 0, s, (const T*)q.part, (int)nb, q.cg);
        hipLaunchKernelGGL(k_ms_cg_direction<T>, dim3(nb), dim3(kBlock), 0, s, (const T*)q.z, q.nv, q.p, (const MsCg<T>*)q.cg);
    }
    if (seen[0] & kMsCgBreakdown) return fail(PCU_HIP_ERR_RUNTIME, "laplacian_smooth_mesh: the conjugate-gradient solve met p.Ap <= 0 (the system is not positive definite in this arithmetic)");
    if (!(seen[0] & kMsCgDone)) return fail(PCU_HIP_ERR_RUNTIME, "laplacian_smooth_mesh: the conjugate-gradient solve has not converged after %d iterations", kMsCgMaxIters);
    return 0;
}

// laplacian_smooth_mesh (src/smooth.cpp:24-79)
template <typename T>
static int laplacian_smooth_impl(pcu_hip_ctx* c, const MeshGiven<T>& m, int num_iters, double step_size, int use_cotan, T* out, unsigned flags, void* stream,
                                 pcu_hip_stats* st) {
    if (!c) return fail(PCU_HIP_ERR_INVALID, "null context");
    if (int rc = mesh_validate(m.nv, m.nf, 0, m.f_kind)) return rc;
    if (m.f_kind != 0 && m.f_kind != 1) return fail(PCU_HIP_ERR_INVALID, "f_kind must be PCU_HIP_FACE_INT32 or PCU_HIP_FACE_INT64");
    if (num_iters < 0) return fail(PCU_HIP_ERR_INVALID, "Invalid value for argument num_iters in smooth_mesh_laplacian. Must be a positive integer or 0.");
    if (!(step_size >= 0.0) || !std::isfinite(step_size)) return fail(PCU_HIP_ERR_INVALID, "step_size must be finite and not negative");
    if (!m.v || !m.f || !out) return fail(PCU_HIP_ERR_INVALID, "null v / f / out");
    const bool on_dev = flags & PCU_HIP_PTRS_ON_DEVICE;
    const size_t NV = (size_t)m.nv, NF = (size_t)m.nf, nb = blocks_for(NV), nbf = blocks_for(NF);
    size_t bytes = ms_incidence_bytes(NV, NF) + align_up(NF * 24, 256) + ms_adjacency_bytes(NV, NF) + align_up(NF * 3 * sizeof(T), 256) + align_up(NF * 6 * sizeof(T), 256) +
                   align_up(NF * sizeof(T), 256) + 7 * align_up(NV * 3 * sizeof(T), 256) + 3 * align_up(NV * sizeof(T), 256) +
                   align_up(std::max(nb * kMsFoldMax, nbf * 4) * sizeof(T), 256) + 16384;
    if (!on_dev) bytes += align_up(NV * 3 * sizeof(T), 256) + align_up(NF * 3 * int_kind_bytes(m.f_kind), 256);
    return op_run(c, flags, stream, st, bytes, [&](OpFrame& fr) -> int {
        auto& [c, s, on_dev, ar, tm] = fr;      // marks 0-1: checks, incidence and adjacency, 1-2: the cotangent matrix, 2-3: the iterations
        MsStructure S;
        const T* dv = nullptr;
        tm.mark(0);
        if (stage_in(ar, m.v, m.nv, on_dev, s, &dv) || ms_faces(ar, s, m.f, m.nf, m.f_kind, m.nv, on_dev, S)) return -1;
        hipLaunchKernelGGL(k_mesh_vcheck<T>, dim3(blocks_for(NV * 3)), dim3(kBlock), 0, s, dv, (long long)NV * 3, S.d_bad, kMeshBadVertex);
        if (ms_incidence(ar, s, m.nf, m.nv, S)) return -1;
        if (int rc = ms_adjacency(ar, s, m.nf, m.nv, S)) return rc;
        tm.mark(1);
        T* u = nullptr;
        if (out_room(ar, on_dev, out, NV * 3, &u)) return -1;
        if (u != dv) HIP_TRY(hipMemcpyAsync(u, dv, NV * 3 * sizeof(T), hipMemcpyDeviceToDevice, s));
        int iters = 0;
        if (num_iters > 0) {
            T *w = nullptr, *val = nullptr, *diag = nullptr, *len = nullptr, *ac = nullptr;
            MsSolve<T> q;
            if (aalloc(ar, &w, NF * 3) || aalloc(ar, &val, (size_t)S.ne) || aalloc(ar, &diag, NV) || aalloc(ar, &q.M, NV) || aalloc(ar, &q.D, NV) || aalloc(ar, &q.b, NV * 3) ||
                aalloc(ar, &q.r, NV * 3) || aalloc(ar, &q.z, NV * 3) || aalloc(ar, &q.p, NV * 3) || aalloc(ar, &q.Ap, NV * 3) ||
                aalloc(ar, &q.part, std::max(nb * kMsFoldMax, nbf * 4)) || aalloc(ar, &q.cg, 1) || (use_cotan && (aalloc(ar, &len, NF) || aalloc(ar, &ac, 4)))) return -1;
            HIP_TRY(hipMemsetAsync(q.cg, 0, sizeof(MsCg<T>), s));
            hipLaunchKernelGGL(k_ms_corner_w<T>, dim3(blocks_for(NF * 3)), dim3(kBlock), 0, s, dv, (const int*)S.fidx, (int)(3 * m.nf), w);
            if (S.ne > 0)
                hipLaunchKernelGGL(k_ms_run_sums<T>, dim3(blocks_for((size_t)S.ne)), dim3(kBlock), 0, s, (const unsigned long long*)S.pkeys, (const unsigned*)S.pids, S.K,
                                   (const unsigned*)S.head_pos, S.ne, (const T*)w, val);
            hipLaunchKernelGGL(k_ms_diag<T>, dim3((unsigned)nb), dim3(kBlock), 0, s, (const unsigned*)S.off, (const T*)val, (int)m.nv, diag);
            if (!use_cotan) hipLaunchKernelGGL(k_ms_fill<T>, dim3((unsigned)nb), dim3(kBlock), 0, s, q.M, (int)m.nv, (T)1);
            HIP_TRY(hipGetLastError());
            tm.mark(2);
            q.off = S.off; q.col = S.col; q.val = val; q.diag = diag; q.nv = (int)m.nv;
            q.h = (T)(use_cotan ? step_size * 1e-3 : step_size);
            for (int iter = 0; iter < num_iters; ++iter) {
                if (use_cotan) {
                    hipLaunchKernelGGL(k_ms_face_len<T>, dim3((unsigned)nbf), dim3(kBlock), 0, s, (const T*)u, (const int*)S.fidx, (int)m.nf, len);
                    hipLaunchKernelGGL(k_ms_mass<T>, dim3((unsigned)nb), dim3(kBlock), 0, s, (const unsigned*)S.inc_pos, (const unsigned*)S.inc_ids, (const T*)len, (int)m.nv, q.M);
                }
                if (int rc = ms_solve<T>(s, q, u)) return rc;
                if (use_cotan) {
                    hipLaunchKernelGGL(k_ms_area_parts<T>, dim3((unsigned)nbf), dim3(kBlock), 0, s, (const T*)u, (const int*)S.fidx, (int)m.nf, q.part);
                    hipLaunchKernelGGL(k_ms_area_fold<T>, dim3(1), dim3(kBlock), 0, s, (const T*)q.part, (int)nbf, ac);
                    hipLaunchKernelGGL(k_ms_rescale<T>, dim3((unsigned)nb), dim3(kBlock), 0, s, u, (const T*)q.M, (int)m.nv, (const T*)ac);
                    HIP_TRY(hipGetLastError());
                }
            }
            HIP_TRY(hipMemcpyAsync(&iters, &q.cg->iters, sizeof(int), hipMemcpyDeviceToHost, s));
        } else {
            tm.mark(2);
        }
        tm.mark(3);
        if (out_give(s, on_dev, out, u, NV * 3)) return -1;
        HIP_WAIT(s);
        if (st) {
            st->n_queries = m.nv; st->n_escalated = (int64_t)S.ne; st->n_passes = iters;
            st->ms_index = tm.span(0, 1); st->ms_search = tm.span(1, 2); st->ms_kernel_search = tm.span(2, 3); st->ms_total = tm.span(0, 3);
        }
        return 0;
    });
}
