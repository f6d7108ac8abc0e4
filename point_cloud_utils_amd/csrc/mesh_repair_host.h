// csrc/mesh_repair_host.h -- host orchestration of remove_mesh_vertices, remove_unreferenced_mesh_vertices, deduplicate_mesh_vertices and
// orient_mesh_faces (kernels and contract: mesh_repair.h). Included by pcu_hip.hip after the operator frame (stage_faces, out_room / out_give,
// flag_word, mesh_refusal), voxel_host.h (dedup_device, sort_keys, rank_flags, scan_bytes, read_flag_and_last) and mesh_host.h (mesh_validate, MeshGiven).
// Every output's size depends on the data: the caller gives room for the upper bound (#v rows, #f rows), the counts come back through
// int64_t*, and nothing is written to an output before the face indices have passed their range check.
#pragma once

// flags and their scan (n * 8 + 4), the scan's tile sums
static size_t mr_rank_bytes(size_t n) { return 2 * align_up((n + 1) * 4, 256) + scan_bytes(n) + 512; }
// what a call with host pointers stages: v, f and the outputs of the same sizes
template <typename T>
static size_t mr_staged_bytes(size_t nv, size_t nf, size_t kb) { return 2 * (align_up(nv * 3 * sizeof(T), 256) + align_up(nf * 3 * kb, 256)); }
static void mr_stats(pcu_hip_stats* st, Timer& tm, int64_t nf, int64_t escalated) {
    if (!st) return;
    st->n_queries = nf; st->n_escalated = escalated; st->n_passes = 1;
    st->ms_index = tm.span(0, 1); st->ms_search = tm.span(2, 3); st->ms_total = tm.span(0, 3);
}

// The flag-and-scan steps (rank_flags of voxel_host.h with this file's kernels). No wait in any.
static int mr_rank_mask(Arena& ar, hipStream_t s, SortedRuns& r, const unsigned char* d_mask, unsigned nv) {
    return rank_flags(ar, s, r, (int)nv, [&](unsigned* flag) { hipLaunchKernelGGL(k_mr_mask_flags, dim3(blocks_for(nv)), dim3(kBlock), 0, s, d_mask, nv, flag); });
}
static int mr_rank_referenced(Arena& ar, hipStream_t s, SortedRuns& r, const void* d_f, int f_kind, unsigned nf, unsigned nv, int* d_bad) {
    return rank_flags(ar, s, r, (int)nv, [&](unsigned* ref) {
        (void)hipMemsetAsync(ref, 0, (size_t)nv * 4, s);
        hipLaunchKernelGGL(k_mr_referenced, dim3(blocks_for((size_t)nf * 3)), dim3(kBlock), 0, s, d_f, f_kind, 3u * nf, nv, ref, d_bad);
    });
}
static int mr_rank_faces(Arena& ar, hipStream_t s, SortedRuns& r, const void* d_f, int f_kind, unsigned nf, unsigned nv, const int* map, int distinct, int* d_bad) {
    return rank_flags(ar, s, r, (int)nf, [&](unsigned* keep) {
        hipLaunchKernelGGL(k_mr_face_flags, dim3(blocks_for(nf)), dim3(kBlock), 0, s, d_f, f_kind, nf, nv, map, distinct, keep, d_bad);
    });
}
static int mr_rank_roots(Arena& ar, hipStream_t s, SortedRuns& r, const unsigned* parent, unsigned nf, unsigned* d_tw) {
    return rank_flags(ar, s, r, (int)nf, [&](unsigned* root) { hipLaunchKernelGGL(k_mr_patch_roots, dim3(blocks_for(nf)), dim3(kBlock), 0, s, parent, nf, root, d_tw); });
}

// remove_mesh_vertices (src/remove_mesh_vertices.cpp:22-73). mask: nv bytes, non-zero keeps. out_v (nv,3) and out_f (nf,3) are sized for the
// worst case; *out_nv and *out_nf rows are written. One wait for the flag word and the two counts.
template <typename T>
static int remove_mesh_vertices_impl(pcu_hip_ctx* c, const MeshGiven<T>& m, const unsigned char* mask, T* out_v, void* out_f, int64_t* out_nv, int64_t* out_nf,
                                     unsigned flags, void* stream, pcu_hip_stats* st) {
    if (!c || !out_nv || !out_nf) return fail(PCU_HIP_ERR_INVALID, "null context / out_nv / out_nf");
    *out_nv = *out_nf = 0;
    if (int rc = mesh_validate(m.nv, m.nf, 0, m.f_kind)) return rc;
    if (!m.v || !m.f || !mask || !out_v || !out_f) return fail(PCU_HIP_ERR_INVALID, "null v / f / mask / out_v / out_f");
    const bool on_dev = flags & PCU_HIP_PTRS_ON_DEVICE;
    const size_t NV = (size_t)m.nv, NF = (size_t)m.nf, kb = (size_t)int_kind_bytes(m.f_kind);
    const size_t bytes = align_up(NV * 4, 256) + mr_rank_bytes(NV) + mr_rank_bytes(NF) + (on_dev ? 0 : mr_staged_bytes<T>(NV, NF, kb) + align_up(NV, 256)) + 8192;
    return op_run(c, flags, stream, st, bytes, [&](OpFrame& fr) -> int {
        auto& [c, s, on_dev, ar, tm] = fr;      // marks 0-1: flags, scans, map and the wait, 2-3: rows and faces
        const T* dv = nullptr; const char* d_f = nullptr; const unsigned char* d_mask = nullptr;
        if (stage_in(ar, m.v, m.nv, on_dev, s, &dv) || stage_faces(ar, m.f, NF, m.f_kind, on_dev, s, &d_f) || stage_any(ar, mask, NV, on_dev, s, &d_mask)) return -1;
        int *map = nullptr, *d_bad = nullptr;
        if (aalloc(ar, &map, NV) || flag_word(ar, s, &d_bad)) return -1;
        const unsigned unv = (unsigned)m.nv, unf = (unsigned)m.nf;
        tm.mark(0);
        SortedRuns vs, fs;
        if (mr_rank_mask(ar, s, vs, d_mask, unv)) return -1;
        hipLaunchKernelGGL(k_mr_map, dim3(blocks_for(NV)), dim3(kBlock), 0, s, (const unsigned*)vs.flag, (const unsigned*)vs.scan, unv, map);
        if (mr_rank_faces(ar, s, fs, d_f, m.f_kind, unf, unv, map, 0, d_bad)) return -1;
        int bad = 0; unsigned kept_v = 0, kept_f = 0;
        if (read_flag_and_last(s, d_bad, (const unsigned*)fs.scan, NF, &bad, &kept_f)) return -1;
        HIP_TRY(hipMemcpyAsync(&kept_v, vs.scan + (NV - 1), 4, hipMemcpyDeviceToHost, s));
        HIP_WAIT(s);
        tm.mark(1);
        if (bad) return mesh_refusal(bad, m.nv);
        if (kept_v > unv || kept_f > unf) return fail(PCU_HIP_ERR_RUNTIME, "internal: %u of %lld vertices, %u of %lld faces kept", kept_v, (long long)m.nv, kept_f, (long long)m.nf);
        T* d_ov = nullptr; char *const h_of = static_cast<char*>(out_f), *d_of = nullptr;
        if (out_room(ar, on_dev, out_v, (size_t)kept_v * 3, &d_ov) || out_room(ar, on_dev, h_of, (size_t)kept_f * 3 * kb, &d_of)) return -1;
        tm.mark(2);
        hipLaunchKernelGGL(k_mr_rows<T>, dim3(blocks_for(NV)), dim3(kBlock), 0, s, dv, (const int*)map, unv, d_ov, m.f_kind, (void*)nullptr, (void*)nullptr);
        hipLaunchKernelGGL(k_mr_faces_out, dim3(blocks_for(NF)), dim3(kBlock), 0, s, (const void*)d_f, m.f_kind, unf, unv, (const int*)map, (const unsigned*)fs.flag,
                           (const unsigned*)fs.scan, (void*)d_of);
        HIP_TRY(hipGetLastError());
        tm.mark(3);
        if (out_give(s, on_dev, out_v, d_ov, (size_t)kept_v * 3) || out_give(s, on_dev, h_of, d_of, (size_t)kept_f * 3 * kb)) return -1;
        HIP_WAIT(s);
        *out_nv = (int64_t)kept_v; *out_nf = (int64_t)kept_f;
        mr_stats(st, tm, m.nf, m.nf - (int64_t)kept_f);
        return 0;
    });
}

// remove_unreferenced_mesh_vertices (src/remove_unreferenced_mesh_vertices.cpp:23-37). out_v (nv,3) and out_corr_v (nv) are sized for the worst
// case, *out_nv rows are written; out_f (nf,3) and out_corr_f (nv) are written whole. The three integer outputs are of f's type.
template <typename T>
static int remove_unreferenced_impl(pcu_hip_ctx* c, const MeshGiven<T>& m, T* out_v, void* out_f, void* out_corr_v, void* out_corr_f, int64_t* out_nv,
                                    unsigned flags, void* stream, pcu_hip_stats* st) {
    if (!c || !out_nv) return fail(PCU_HIP_ERR_INVALID, "null context / out_nv");
    *out_nv = 0;
    if (int rc = mesh_validate(m.nv, m.nf, 0, m.f_kind)) return rc;
    if (!m.v || !m.f || !out_v || !out_f || !out_corr_v || !out_corr_f) return fail(PCU_HIP_ERR_INVALID, "null v / f / out_v / out_f / out_corr_v / out_corr_f");
    const bool on_dev = flags & PCU_HIP_PTRS_ON_DEVICE;
    const size_t NV = (size_t)m.nv, NF = (size_t)m.nf, kb = (size_t)int_kind_bytes(m.f_kind);
    const size_t bytes = align_up(NV * 4, 256) + mr_rank_bytes(NV) + (on_dev ? 0 : mr_staged_bytes<T>(NV, NF, kb) + 2 * align_up(NV * kb, 256)) + 8192;
    return op_run(c, flags, stream, st, bytes, [&](OpFrame& fr) -> int {
        auto& [c, s, on_dev, ar, tm] = fr;      // marks 0-1: referenced flags, scan, map and the wait, 2-3: rows and faces
        const T* dv = nullptr; const char* d_f = nullptr;
        if (stage_in(ar, m.v, m.nv, on_dev, s, &dv) || stage_faces(ar, m.f, NF, m.f_kind, on_dev, s, &d_f)) return -1;
        int *map = nullptr, *d_bad = nullptr;
        if (aalloc(ar, &map, NV) || flag_word(ar, s, &d_bad)) return -1;
        const unsigned unv = (unsigned)m.nv, unf = (unsigned)m.nf;
        tm.mark(0);
        SortedRuns vs;
        if (mr_rank_referenced(ar, s, vs, d_f, m.f_kind, unf, unv, d_bad)) return -1;
        hipLaunchKernelGGL(k_mr_map, dim3(blocks_for(NV)), dim3(kBlock), 0, s, (const unsigned*)vs.flag, (const unsigned*)vs.scan, unv, map);
        int bad = 0; unsigned kept_v = 0;
        if (read_flag_and_last(s, d_bad, (const unsigned*)vs.scan, NV, &bad, &kept_v)) return -1;
        HIP_WAIT(s);
        tm.mark(1);
        if (bad) return mesh_refusal(bad, m.nv);
        if (kept_v == 0 || kept_v > unv) return fail(PCU_HIP_ERR_RUNTIME, "internal: %u of %lld vertices referenced", kept_v, (long long)m.nv);
        T* d_ov = nullptr; char *const h_of = static_cast<char*>(out_f), *const h_cv = static_cast<char*>(out_corr_v), *const h_cf = static_cast<char*>(out_corr_f);
        char *d_of = nullptr, *d_cv = nullptr, *d_cf = nullptr;
        if (out_room(ar, on_dev, out_v, (size_t)kept_v * 3, &d_ov) || out_room(ar, on_dev, h_of, NF * 3 * kb, &d_of) || out_room(ar, on_dev, h_cv, (size_t)kept_v * kb, &d_cv) ||
            out_room(ar, on_dev, h_cf, NV * kb, &d_cf)) return -1;
        tm.mark(2);
        hipLaunchKernelGGL(k_mr_rows<T>, dim3(blocks_for(NV)), dim3(kBlock), 0, s, dv, (const int*)map, unv, d_ov, m.f_kind, (void*)d_cv, (void*)d_cf);
        hipLaunchKernelGGL(k_mr_faces_out, dim3(blocks_for(NF)), dim3(kBlock), 0, s, (const void*)d_f, m.f_kind, unf, unv, (const int*)map, (const unsigned*)nullptr,
                           (const unsigned*)nullptr, (void*)d_of);
        HIP_TRY(hipGetLastError());
        tm.mark(3);
        if (out_give(s, on_dev, out_v, d_ov, (size_t)kept_v * 3) || out_give(s, on_dev, h_of, d_of, NF * 3 * kb) || out_give(s, on_dev, h_cv, d_cv, (size_t)kept_v * kb) ||
            out_give(s, on_dev, h_cf, d_cf, NV * kb)) return -1;
        HIP_WAIT(s);
        *out_nv = (int64_t)kept_v;
        mr_stats(st, tm, m.nf, 0);
        return 0;
    });
}

// deduplicate_mesh_vertices (src/remove_duplicates.cpp:37-81, :152-176). out_v (nv,3), out_svi (nv) and out_f (nf,3) are sized for the worst
// case, *out_nv and *out_nf rows are written; out_svj (nv) is written whole. The vertex side is dedup_device's (voxel_host.h) into the
// workspace, so that svj stays on the device and a refused call has written nothing.
template <typename T>
static int dedup_mesh_impl(pcu_hip_ctx* c, const MeshGiven<T>& m, double epsilon, T* out_v, void* out_f, int32_t* out_svi, int32_t* out_svj, int64_t* out_nv,
                           int64_t* out_nf, unsigned flags, void* stream, pcu_hip_stats* st) {
    if (!c || !out_nv || !out_nf) return fail(PCU_HIP_ERR_INVALID, "null context / out_nv / out_nf");
    *out_nv = *out_nf = 0;
    if (int rc = mesh_validate(m.nv, m.nf, 0, m.f_kind)) return rc;
    if (!m.v || !m.f || !out_v || !out_f || !out_svi || !out_svj) return fail(PCU_HIP_ERR_INVALID, "null v / f / out_v / out_f / out_svi / out_svj");
    const bool on_dev = flags & PCU_HIP_PTRS_ON_DEVICE;
    const size_t NV = (size_t)m.nv, NF = (size_t)m.nf, kb = (size_t)int_kind_bytes(m.f_kind);
    const size_t bytes = dedup_bytes<T>(NV) + align_up(NV * 3 * sizeof(T), 256) + 2 * align_up(NV * 4, 256) + mr_rank_bytes(NF) +
                         (on_dev ? 0 : mr_staged_bytes<T>(NV, NF, kb)) + 8192;
    return op_run(c, flags, stream, st, bytes, [&](OpFrame& fr) -> int {
        auto& [c, s, on_dev, ar, tm] = fr;      // marks 0-1: the vertices' keys, sort and runs, the face flags, their scan and the wait, 2-3: faces and copies
        const T* dv = nullptr; const char* d_f = nullptr;
        if (stage_in(ar, m.v, m.nv, on_dev, s, &dv) || stage_faces(ar, m.f, NF, m.f_kind, on_dev, s, &d_f)) return -1;
        T* t_v = nullptr; int *t_svi = nullptr, *t_svj = nullptr, *d_bad = nullptr;
        if (aalloc(ar, &t_v, NV * 3) || aalloc(ar, &t_svi, NV) || aalloc(ar, &t_svj, NV) || flag_word(ar, s, &d_bad)) return -1;
        const unsigned unv = (unsigned)m.nv, unf = (unsigned)m.nf;
        tm.mark(0);
        const unsigned* n_out_dev = nullptr;
        if (dedup_device<T>(ar, s, dv, (int)m.nv, epsilon, t_v, t_svi, t_svj, &n_out_dev)) return -1;
        SortedRuns fs;
        if (mr_rank_faces(ar, s, fs, d_f, m.f_kind, unf, unv, t_svj, 1, d_bad)) return -1;
        int bad = 0; unsigned kept_v = 0, kept_f = 0;
        if (read_flag_and_last(s, d_bad, (const unsigned*)fs.scan, NF, &bad, &kept_f)) return -1;
        HIP_TRY(hipMemcpyAsync(&kept_v, n_out_dev, 4, hipMemcpyDeviceToHost, s));
        HIP_WAIT(s);
        tm.mark(1);
        if (bad) return mesh_refusal(bad, m.nv);
        if (kept_v == 0 || kept_v > unv || kept_f > unf) return fail(PCU_HIP_ERR_RUNTIME, "internal: %u of %lld vertices, %u of %lld faces kept", kept_v, (long long)m.nv, kept_f, (long long)m.nf);
        char *const h_of = static_cast<char*>(out_f), *d_of = nullptr;
        if (out_room(ar, on_dev, h_of, (size_t)kept_f * 3 * kb, &d_of)) return -1;
        tm.mark(2);
        hipLaunchKernelGGL(k_mr_faces_out, dim3(blocks_for(NF)), dim3(kBlock), 0, s, (const void*)d_f, m.f_kind, unf, unv, (const int*)t_svj, (const unsigned*)fs.flag,
                           (const unsigned*)fs.scan, (void*)d_of);
        HIP_TRY(hipGetLastError());
        if (out_give(s, on_dev, out_v, t_v, (size_t)kept_v * 3) || out_give(s, on_dev, out_svi, t_svi, (size_t)kept_v) || out_give(s, on_dev, out_svj, t_svj, NV)) return -1;
        tm.mark(3);
        if (out_give(s, on_dev, h_of, d_of, (size_t)kept_f * 3 * kb)) return -1;
        HIP_WAIT(s);
        *out_nv = (int64_t)kept_v; *out_nf = (int64_t)kept_f;
        mr_stats(st, tm, m.nf, m.nf - (int64_t)kept_f);
        return 0;
    });
}

// orient_mesh_faces (src/orient_mesh_faces.cpp:21-35). f (nf,3) of indices in [0, nv); out_f (nf,3) and out_c (nf) in f's integer type;
// *out_patches = the number of patches. stats: n_escalated = the patches that are not orientable (their faces are returned unchanged).
static int orient_mesh_faces_impl(pcu_hip_ctx* c, const void* f, int64_t nf, int f_kind, int64_t nv, void* out_f, void* out_c, int64_t* out_patches,
                                  unsigned flags, void* stream, pcu_hip_stats* st) {
    if (!c || !out_patches) return fail(PCU_HIP_ERR_INVALID, "null context / out_patches");
    *out_patches = 0;
    if (nf <= 0) return fail(PCU_HIP_ERR_INVALID, "Invalid input faces with zero elements: f must have shape (n, 3) where n > 0. Got f.shape =(%lld, 3).", (long long)nf);
    if (int rc = int_kind_check(f_kind)) return rc;
    if (nf > kMeshMaxRows) return mesh_row_limit();
    if (nv <= 0 || nv > kCcMaxIndex) return fail(PCU_HIP_ERR_INVALID, "nv must be in [1, 2^31-16]");
    if (!f || !out_f || !out_c) return fail(PCU_HIP_ERR_INVALID, "null f / out_f / out_c");
    const bool on_dev = flags & PCU_HIP_PTRS_ON_DEVICE;
    const size_t NF = (size_t)nf, kb = (size_t)int_kind_bytes(f_kind);
    const size_t bytes = sort_bytes(3 * NF) + align_up(2 * NF * 4, 256) + mr_rank_bytes(NF) + (on_dev ? 0 : 2 * align_up(NF * 3 * kb, 256) + align_up(NF * kb, 256)) + 8192;
    return op_run(c, flags, stream, st, bytes, [&](OpFrame& fr) -> int {
        auto& [c, s, on_dev, ar, tm] = fr;      // marks 0-1: keys, sort and unions, 1-2: flatten, roots and their ranks, 3-4: rows and labels
        const char* d_f = nullptr;
        if (stage_faces(ar, f, NF, f_kind, on_dev, s, &d_f)) return -1;
        SortedRuns es, ps;
        unsigned *parent = nullptr, *d_tw = nullptr; int* d_bad = nullptr;
        if (aalloc(ar, &es.keys, 3 * NF) || aalloc(ar, &parent, 2 * NF) || aalloc(ar, &d_tw, 1) || flag_word(ar, s, &d_bad)) return -1;
        const unsigned unf = (unsigned)nf, unv = (unsigned)nv;
        const int hb = std::max(bits_of((unsigned long long)(nv - 1)), 1);
        HIP_TRY(hipMemsetAsync(d_tw, 0, sizeof(unsigned), s));
        tm.mark(0);
        hipLaunchKernelGGL(k_mr_edge_keys, dim3(blocks_for(NF)), dim3(kBlock), 0, s, (const void*)d_f, f_kind, unf, unv, hb, es.keys, d_bad);
        if (sort_keys(ar, s, es, (int)(3 * nf), 2 * hb)) return -1;
        hipLaunchKernelGGL(k_cc_init, dim3(blocks_for(2 * NF)), dim3(kBlock), 0, s, parent, 2u * unf);
        hipLaunchKernelGGL(k_mr_edge_unions, dim3(blocks_for(3 * NF)), dim3(kBlock), 0, s, (const unsigned long long*)es.keys, (const unsigned*)es.ids, 3u * unf, (const void*)d_f,
                           f_kind, parent);
        tm.mark(1);
        hipLaunchKernelGGL(k_cc_flatten, dim3(blocks_for(2 * NF)), dim3(kBlock), 0, s, parent, 2u * unf, (unsigned*)nullptr);
        if (mr_rank_roots(ar, s, ps, parent, unf, d_tw)) return -1;
        tm.mark(2);
        int bad = 0; unsigned count = 0, twisted = 0;
        if (read_flag_and_last(s, d_bad, (const unsigned*)ps.scan, NF, &bad, &count)) return -1;
        HIP_TRY(hipMemcpyAsync(&twisted, d_tw, 4, hipMemcpyDeviceToHost, s));
        HIP_WAIT(s);
        if (bad) return mesh_refusal(bad, nv);
        if (count == 0 || count > unf || twisted > count) return fail(PCU_HIP_ERR_RUNTIME, "internal: %u patches (%u not orientable) of %lld faces", count, twisted, (long long)nf);
        char *const h_of = static_cast<char*>(out_f), *const h_oc = static_cast<char*>(out_c), *d_of = nullptr, *d_oc = nullptr;
        if (out_room(ar, on_dev, h_of, NF * 3 * kb, &d_of) || out_room(ar, on_dev, h_oc, NF * kb, &d_oc)) return -1;
        tm.mark(3);
        hipLaunchKernelGGL(k_mr_orient_out, dim3(blocks_for(NF)), dim3(kBlock), 0, s, (const void*)d_f, f_kind, unf, (const unsigned*)parent, (const unsigned*)ps.scan,
                           (void*)d_of, (void*)d_oc);
        HIP_TRY(hipGetLastError());
        tm.mark(4);
        if (out_give(s, on_dev, h_of, d_of, NF * 3 * kb) || out_give(s, on_dev, h_oc, d_oc, NF * kb)) return -1;
        HIP_WAIT(s);
        *out_patches = (int64_t)count;
        if (st) {
            st->n_queries = nf; st->n_escalated = (int64_t)twisted; st->n_passes = 1;
            st->ms_index = tm.span(0, 1); st->ms_search = tm.span(1, 2); st->ms_tie = tm.span(3, 4); st->ms_total = tm.span(0, 4);
        }
        return 0;
    });
}
