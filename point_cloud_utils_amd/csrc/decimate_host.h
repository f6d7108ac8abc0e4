// csrc/decimate_host.h -- host orchestration of decimate_triangle_mesh (kernels and contract: decimate.h). Included by pcu_hip.hip after the
// operator frame (stage_faces, flag_word, mesh_refusal) and the parking functions, voxel_host.h (sort_bytes, scan_bytes, sort_keys, rank_flags,
// own_inclusive_scan), mesh_host.h (mesh_validate, MeshGiven) and mesh_repair_host.h (mr_rank_bytes, mr_rank_referenced).
// Everything runs on the caller's stream out of the call's arena: the buffers that live through the call are taken first, and every round
// starts its own at the same mark. The host waits once per round, for the flag word, the number of winners and the faces they remove.
#pragma once

constexpr int kDcCounts = 4;                    // winners, the faces they remove, winners taken by a binding budget, spare

// one round's temporaries over K = 6 * (alive faces) directed pairs
static size_t dc_round_bytes(size_t nv, size_t K) {
    return sort_bytes(K) + mr_rank_bytes(K) + 2 * align_up((nv + 1) * 4, 256) + 2 * align_up(K * 4, 256) + align_up(K * 8, 256) +          // structure, keys
           mr_rank_bytes(K) + sort_bytes(K / 2 + 1) + 2 * align_up((K / 2 + 2) * 4, 256) + scan_bytes(K / 2 + 1) +                          // budget
           mr_rank_bytes(K / 6 + 1) + 16384;                                                                                               // faces
}

// The sorted pairs of the m alive faces and their CSR. No wait.
static int dc_structure(Arena& ar, hipStream_t s, const int* cf, unsigned m, unsigned nv, int hb, DcStructure& S) {
    const int K = (int)(6 * m);
    SortedRuns r; unsigned *pos = nullptr, *off = nullptr, *head_pos = nullptr; int* col = nullptr;
    if (aalloc(ar, &r.keys, (size_t)K) || aalloc(ar, &pos, (size_t)nv + 1) || aalloc(ar, &off, (size_t)nv + 1) || aalloc(ar, &head_pos, (size_t)K) || aalloc(ar, &col, (size_t)K)) return -1;
    hipLaunchKernelGGL(k_ms_pairs, dim3(blocks_for((size_t)K / 2)), dim3(kBlock), 0, s, cf, K / 2, hb, r.keys);
    if (sort_keys(ar, s, r, K, 2 * hb)) return -1;
    const unsigned long long* keys = r.keys;
    if (rank_flags(ar, s, r, K, [&](unsigned* flag) { hipLaunchKernelGGL(k_ms_pair_heads, dim3(blocks_for((size_t)K)), dim3(kBlock), 0, s, keys, K, hb, flag); })) return -1;
    hipLaunchKernelGGL(k_ms_row_starts, dim3(blocks_for((size_t)nv + 1)), dim3(kBlock), 0, s, keys, K, hb, (int)nv, pos);
    hipLaunchKernelGGL(k_ms_offsets, dim3(blocks_for((size_t)nv + 1)), dim3(kBlock), 0, s, (const unsigned*)pos, (const unsigned*)r.scan, (int)nv, off);
    hipLaunchKernelGGL(k_ms_entries, dim3(blocks_for((size_t)K)), dim3(kBlock), 0, s, keys, (const unsigned*)r.flag, (const unsigned*)r.scan, K, hb, head_pos, col);
    HIP_TRY(hipGetLastError());
    S = DcStructure{keys, r.ids, off, head_pos, col, r.scan + (K - 1), cf, (unsigned)K, hb};
    return 0;
}

// hi becomes lo in the m alive faces; the survivors flagged and ranked. No wait.
static int dc_rank_alive(Arena& ar, hipStream_t s, SortedRuns& r, int* cf, unsigned m, const int* to) {
    return rank_flags(ar, s, r, (int)m, [&](unsigned* keep) { hipLaunchKernelGGL(k_dc_faces_step, dim3(blocks_for((size_t)m)), dim3(kBlock), 0, s, cf, m, to, keep); });
}

// The budget where it binds: of the nw winners flagged in `win`, those stay that the contract takes. No wait.
static int dc_budget(Arena& ar, hipStream_t s, const DcStructure& S, const unsigned long long* ekey, unsigned* win, unsigned nw, unsigned need, unsigned* counts) {
    SortedRuns r; unsigned *scan = nullptr, *wfaces = nullptr, *wscan = nullptr;
    if (aalloc(ar, &scan, (size_t)S.K + 1) || aalloc(ar, &r.keys, (size_t)nw) || aalloc(ar, &wfaces, (size_t)nw) || aalloc(ar, &wscan, (size_t)nw + 1)) return -1;
    if (own_inclusive_scan(ar, s, (const unsigned*)win, scan, (size_t)S.K)) return -1;
    hipLaunchKernelGGL(k_dc_winner_keys, dim3(blocks_for((size_t)S.K)), dim3(kBlock), 0, s, (const unsigned*)win, (const unsigned*)scan, S.K, ekey, r.keys);
    if (sort_keys(ar, s, r, (int)nw, 64)) return -1;
    hipLaunchKernelGGL(k_dc_winner_faces, dim3(blocks_for((size_t)nw)), dim3(kBlock), 0, s, S, (const unsigned long long*)r.keys, nw, wfaces);
    if (own_inclusive_scan(ar, s, (const unsigned*)wfaces, wscan, (size_t)nw)) return -1;
    hipLaunchKernelGGL(k_dc_budget, dim3(blocks_for((size_t)nw)), dim3(kBlock), 0, s, (const unsigned long long*)r.keys, (const unsigned*)wfaces, (const unsigned*)wscan, nw, need, win, counts);
    HIP_TRY(hipGetLastError());
    return 0;
}

// decimate_triangle_mesh (src/mesh_decimate.cpp:23-66). The result is parked for pcu_hip_decimate_triangle_mesh_take: *out_nv vertices and
// *out_nf faces. stats: n_queries = #f, n_passes = the rounds that collapsed an edge, n_escalated = the collapses.
template <typename T>
static int decimate_impl(pcu_hip_ctx* c, const MeshGiven<T>& m, int64_t max_faces, int64_t* out_nv, int64_t* out_nf, unsigned flags, void* stream, pcu_hip_stats* st) {
    if (!c || !out_nv || !out_nf) return fail(PCU_HIP_ERR_INVALID, "null context / out_nv / out_nf");
    *out_nv = *out_nf = 0;
    c->parked = ParkedResult();
    if (int rc = mesh_validate(m.nv, m.nf, 0, m.f_kind)) return rc;
    if (max_faces <= 0) return fail(PCU_HIP_ERR_INVALID, "max_faces must be greater than 0, got %lld.", (long long)max_faces);
    if (max_faces > m.nf)
        return fail(PCU_HIP_ERR_INVALID, "max_faces must be less than or equal to the number of input faces (%lld), got %lld.", (long long)m.nf, (long long)max_faces);
    if (!m.v || !m.f) return fail(PCU_HIP_ERR_INVALID, "null v / f");
    const bool on_dev = flags & PCU_HIP_PTRS_ON_DEVICE;
    const size_t NV = (size_t)m.nv, NF = (size_t)m.nf, kb = (size_t)int_kind_bytes(m.f_kind);
    const size_t bytes = align_up(NV * 3 * sizeof(T), 256) + 2 * align_up(NF * 12, 256) + 2 * align_up(NF * 4, 256) + align_up(NV * 8, 256) + 2 * align_up(NV * 4, 256) +
                         dc_round_bytes(NV, 6 * NF) + mr_rank_bytes(NV) + (on_dev ? 0 : align_up(NV * 3 * sizeof(T), 256) + align_up(NF * 3 * kb, 256)) + 16384;
    return op_run(c, flags, stream, st, bytes, [&](OpFrame& fr) -> int {
        auto& [c, s, on_dev, ar, tm] = fr;      // marks 0-1: a round's structure, 1-2: cost, validity, claims and wins, 3-4: budget, apply and compaction, 5-6: the call
        const T* dv = nullptr; const char* d_f = nullptr;
        if (stage_in(ar, m.v, m.nv, on_dev, s, &dv) || stage_faces(ar, m.f, NF, m.f_kind, on_dev, s, &d_f)) return -1;
        T* P = nullptr; int *cf = nullptr, *cf_alt = nullptr, *to = nullptr, *d_bad = nullptr; unsigned *rows = nullptr, *rows_alt = nullptr, *counts = nullptr;
        unsigned long long* owner = nullptr;
        tm.mark(5);
        if (aalloc(ar, &P, NV * 3) || aalloc(ar, &cf, NF * 3) || aalloc(ar, &cf_alt, NF * 3) || aalloc(ar, &rows, NF) || aalloc(ar, &rows_alt, NF) ||
            aalloc(ar, &owner, NV) || aalloc(ar, &to, NV) || flag_word(ar, s, &d_bad, 1 + kDcCounts)) return -1;
        counts = reinterpret_cast<unsigned*>(d_bad + 1);
        const unsigned unv = (unsigned)m.nv, unf = (unsigned)m.nf;
        const int hb = std::max(bits_of((unsigned long long)(m.nv - 1)), 1);
        HIP_TRY(hipMemcpyAsync(P, dv, NV * 3 * sizeof(T), hipMemcpyDeviceToDevice, s));
        hipLaunchKernelGGL(k_dc_faces_in, dim3(blocks_for(NF)), dim3(kBlock), 0, s, (const void*)d_f, m.f_kind, unf, unv, cf, rows, d_bad);
        const size_t mark = ar.a->off;
        unsigned alive = unf;
        int64_t rounds = 0, collapses = 0;
        float ms_structure = 0, ms_select = 0, ms_apply = 0;
        bool apply_untimed = false;             // marks 3-4 of the last round stand and no wait has come since
        for (bool first = true;; first = false) {
            if (!first && alive <= (unsigned)max_faces) break;
            ar.a->off = mark;
            DcStructure S;
            tm.mark(0);
            if (dc_structure(ar, s, cf, alive, unv, hb, S)) return -1;
            tm.mark(1);
            if (first) {                        // what the call refuses whatever max_faces is
                hipLaunchKernelGGL(k_dc_check_edges, dim3(blocks_for((size_t)S.K)), dim3(kBlock), 0, s, S.head_pos, S.ne_ptr, S.K, d_bad);
                int bad = 0;
                if (flag_fetch(s, d_bad, &bad)) return -1;
                HIP_WAIT(s);
                if (int rc = mesh_refusal(bad, m.nv)) return rc;
                if (bad & kDcTwice) return fail(PCU_HIP_ERR_INVALID, "f must not hold a face that lists a vertex twice");
                if (bad & kDcThreeFaces) return fail(PCU_HIP_ERR_INVALID, "decimate_triangle_mesh_doc produced an empty mesh. This can happen if the input is non-manifold.");
                if (alive <= (unsigned)max_faces) break;
            }
            unsigned long long* ekey = nullptr; unsigned* win = nullptr;
            if (aalloc(ar, &ekey, (size_t)S.K) || aalloc(ar, &win, (size_t)S.K)) return -1;
            HIP_TRY(hipMemsetAsync(owner, 0xff, NV * 8, s));
            HIP_TRY(hipMemsetAsync(counts, 0, kDcCounts * sizeof(unsigned), s));
            hipLaunchKernelGGL(k_dc_claim<T>, dim3(blocks_for((size_t)S.K)), dim3(kBlock), 0, s, S, (const T*)P, ekey, owner);
            hipLaunchKernelGGL(k_dc_wins, dim3(blocks_for((size_t)S.K)), dim3(kBlock), 0, s, S, (const unsigned long long*)ekey, (const unsigned long long*)owner, win, counts);
            HIP_TRY(hipGetLastError());
            tm.mark(2);
            unsigned got[kDcCounts] = {0, 0, 0, 0};
            HIP_TRY(hipMemcpyAsync(got, counts, sizeof got, hipMemcpyDeviceToHost, s));
            HIP_WAIT(s);                        // (honours pcu_hip_cancel)
            ms_structure += tm.span(0, 1); ms_select += tm.span(1, 2);
            if (apply_untimed) ms_apply += tm.span(3, 4);
            apply_untimed = false;
            const unsigned nw = got[0], faces = got[1], need = alive - (unsigned)max_faces;
            if (nw == 0) break;                 // no valid edge is left: the mesh is returned with more than max_faces faces
            if (nw > S.K / 2 || faces < nw || faces > 2 * nw || faces > alive) return fail(PCU_HIP_ERR_RUNTIME, "internal: %u winners remove %u of %u faces", nw, faces, alive);
            tm.mark(3);
            const bool binds = faces > need;
            if (binds && dc_budget(ar, s, S, ekey, win, nw, need, counts)) return -1;
            HIP_TRY(hipMemsetAsync(to, 0xff, NV * 4, s));
            hipLaunchKernelGGL(k_dc_apply<T>, dim3(blocks_for((size_t)S.K)), dim3(kBlock), 0, s, S, (const unsigned*)win, P, to);
            SortedRuns fs;
            if (dc_rank_alive(ar, s, fs, cf, alive, to)) return -1;
            hipLaunchKernelGGL(k_dc_compact, dim3(blocks_for((size_t)alive)), dim3(kBlock), 0, s, (const int*)cf, (const unsigned*)rows, alive, (const unsigned*)fs.flag,
                               (const unsigned*)fs.scan, cf_alt, rows_alt);
            HIP_TRY(hipGetLastError());
            tm.mark(4);
            std::swap(cf, cf_alt); std::swap(rows, rows_alt);
            ++rounds;
            if (!binds) { alive -= faces; collapses += nw; apply_untimed = true; continue; }
            unsigned left = 0, taken = 0;       // the last round: what the budget took comes back
            HIP_TRY(hipMemcpyAsync(&left, fs.scan + (alive - 1), 4, hipMemcpyDeviceToHost, s));
            HIP_TRY(hipMemcpyAsync(&taken, counts + 2, 4, hipMemcpyDeviceToHost, s));
            HIP_WAIT(s);
            ms_apply += tm.span(3, 4);
            if (left > (unsigned)max_faces || left + 1 < (unsigned)max_faces || taken == 0 || taken > nw)
                return fail(PCU_HIP_ERR_RUNTIME, "internal: the budget left %u faces for max_faces = %lld (%u of %u winners taken)", left, (long long)max_faces, taken, nw);
            alive = left; collapses += taken;
            break;
        }
        // the vertices the alive faces list, in order; the faces over them
        ar.a->off = mark;
        SortedRuns vs; int* map = nullptr;
        if (aalloc(ar, &map, NV)) return -1;
        if (mr_rank_referenced(ar, s, vs, cf, 0, alive, unv, d_bad)) return -1;
        hipLaunchKernelGGL(k_mr_map, dim3(blocks_for(NV)), dim3(kBlock), 0, s, (const unsigned*)vs.flag, (const unsigned*)vs.scan, unv, map);
        unsigned kept_v = 0;
        HIP_TRY(hipMemcpyAsync(&kept_v, vs.scan + (NV - 1), 4, hipMemcpyDeviceToHost, s));
        HIP_WAIT(s);
        if (kept_v == 0 || kept_v > unv || alive == 0) return fail(PCU_HIP_ERR_RUNTIME, "internal: %u of %lld vertices listed by %u faces", kept_v, (long long)m.nv, alive);
        char* seg[kParkSegs];       // v, f, corr_v, corr_f
        if (park_reserve(c, {(size_t)kept_v * 3 * sizeof(T), (size_t)alive * 3 * kb, (size_t)kept_v * kb, (size_t)alive * kb}, seg)) return -1;
        hipLaunchKernelGGL(k_mr_rows<T>, dim3(blocks_for(NV)), dim3(kBlock), 0, s, (const T*)P, (const int*)map, unv, reinterpret_cast<T*>(seg[0]), m.f_kind, (void*)seg[2],
                           (void*)nullptr);
        hipLaunchKernelGGL(k_dc_faces_out, dim3(blocks_for((size_t)alive)), dim3(kBlock), 0, s, (const int*)cf, (const unsigned*)rows, alive, (const int*)map, m.f_kind,
                           (void*)seg[1], (void*)seg[3]);
        HIP_TRY(hipGetLastError());
        tm.mark(6);
        HIP_WAIT(s);
        if (apply_untimed) ms_apply += tm.span(3, 4);
        park_commit(c, Parked::Decimated, (int64_t)kept_v, (int64_t)alive);
        *out_nv = (int64_t)kept_v; *out_nf = (int64_t)alive;
        if (st) {
            st->n_queries = m.nf; st->n_passes = (int)rounds; st->n_escalated = collapses;
            st->ms_index = ms_structure; st->ms_search = ms_select; st->ms_tie = ms_apply; st->ms_total = tm.span(5, 6);
        }
        return 0;
    });
}
// The result of this context's last pcu_hip_decimate_triangle_mesh_*. Once. out_v (nv, 3) in v's type; out_f (nf, 3), out_corr_v (nv) and
// out_corr_f (nf) in f's.
static int decimate_take_impl(pcu_hip_ctx* c, int64_t nv, int64_t nf, void* out_v, void* out_f, void* out_corr_v, void* out_corr_f, unsigned flags, void* stream) {
    if (!c || !out_v || !out_f || !out_corr_v || !out_corr_f) return fail(PCU_HIP_ERR_INVALID, "null context / out_v / out_f / out_corr_v / out_corr_f");
    return park_take(c, Parked::Decimated, nv, nf, {out_v, out_f, out_corr_v, out_corr_f}, flags, stream,
                     "pcu_hip_decimate_triangle_mesh_take: this context holds no decimated mesh of %lld vertices and %lld faces");
}
