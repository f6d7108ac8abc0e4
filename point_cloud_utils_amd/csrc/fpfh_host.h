// csrc/fpfh_host.h -- host orchestration of compute_point_cloud_fpfh (kernels and contract: fpfh.h). Included by pcu_hip.hip after the
// operator frame, the index host and radius_host.h (kRadOcc: the grid is radius_impl's).
#pragma once

// What a call takes from the arena beside its dataset (DatasetFrame::bytes).
template <typename T>
static size_t fpfh_bytes(int64_t n, bool on_dev, bool want_counts) {
    const size_t N = (size_t)n;
    size_t b = 2 * align_up(N * sizeof(Pt4<T>), 256) + align_up(N * kFpfhBins * 8, 256) + 16384;
    if (!on_dev) b += align_up(N * 3 * sizeof(T), 256) + align_up(N * kFpfhBins * sizeof(T), 256) + (want_counts ? align_up(N * kFpfhBins * 4, 256) : 0);
    return b;
}

// out_features: n x 33 of T. out_counts: n x 33 int32, or null. A fixed number of launches and one wait: the non-finite word comes back with it.
// stats: n_queries = n, n_passes = 2, n_tie_flagged = the waves of walk 1 that staged their union box, n_tie_true = those that did not,
// n_grid_builds, ms_index (grid, record order, normals), ms_search (walk 1), ms_kernel_search (walk 2), ms_total.
template <typename T>
static int fpfh_impl(pcu_hip_ctx* c, const T* points, const T* normals, int64_t n, double radius, T* out_features, int32_t* out_counts, unsigned flags, void* stream,
                     pcu_hip_stats* st) {
    if (!c) return fail(PCU_HIP_ERR_INVALID, "null context");
    if (int rc = validate_sizes(n, n, "query_points", "dataset_points")) return rc;
    if (!(radius >= 0.0) || std::isinf(radius)) return fail(PCU_HIP_ERR_INVALID, "Invalid radius (%g): must be finite and not negative.", radius);
    if (!points || !normals || !out_features) return fail(PCU_HIP_ERR_INVALID, "null points / normals / out_features");
    const T rt = (T)radius, r2 = rt * rt;                               // one multiply, rounded in T
    const T reach = (T)sqrt((double)r2) * ((T)1 + (T)8 * std::numeric_limits<T>::epsilon());
    DatasetFrame<T> ds{nullptr, points, n, (flags & PCU_HIP_PTRS_ON_DEVICE) != 0};
    const size_t bytes = ds.bytes(kRadOcc) + fpfh_bytes<T>(n, ds.on_dev, out_counts != nullptr);
    return op_run(c, flags, stream, st, bytes, [&](OpFrame& fr) -> int {
        auto& [c, s, on_dev, ar, tm] = fr;      // marks 0-1: index, record order, normals, 1-2: walk 1, 2-3: walk 2
        tm.mark(0);
        const T* d_nrm = nullptr;
        if (ds.stage(ar, s) || stage_in(ar, normals, n, on_dev, s, &d_nrm)) return -1;
        const double h = sqrt((double)r2) * 1.01;                       // radius_impl's grid: cells no smaller than the radius, a ball's box is 3^3 cells
        GridIndex<T> gi;
        if (int rc = ds.grid(ar, s, gi, kRadOcc, IndexFor::Atomic, std::isfinite(h) ? h : 0.0)) return rc;
        const size_t N = (size_t)n;
        Pt4<T> *by_row = nullptr, *nrm = nullptr; double* spfh = nullptr; unsigned* tally = nullptr; T* d_feat = nullptr; int* d_counts = nullptr;
        if (aalloc(ar, &by_row, N) || aalloc(ar, &nrm, N) || aalloc(ar, &spfh, N * kFpfhBins) || aalloc(ar, &tally, 4) || out_room(ar, on_dev, out_features, N * kFpfhBins, &d_feat)) return -1;
        if (out_counts && out_room(ar, on_dev, reinterpret_cast<int*>(out_counts), N * kFpfhBins, &d_counts)) return -1;
        HIP_TRY(hipMemsetAsync(tally, 0, 16, s));
        hipLaunchKernelGGL(k_cells_by_row<T>, dim3(blocks_for(N)), dim3(kBlock), 0, s, gi.gp, gi.sorted, gi.cell_start, (int)n, by_row);
        hipLaunchKernelGGL(k_fpfh_normals<T>, dim3(blocks_for(N)), dim3(kBlock), 0, s, (const Pt4<T>*)by_row, d_nrm, (int)n, nrm);
        FpfhArgs<T> a{};
        a.gp = gi.gp; a.by_row = by_row; a.cell_start = gi.cell_start; a.n = (int)n; a.nrm = nrm; a.r2 = r2; a.reach = reach;
        a.spfh = spfh; a.counts = d_counts; a.features = d_feat; a.n_staged = tally;
        a.cancel_word = g_cancel_mirror.load(std::memory_order_relaxed); a.cancel_gen = t_call_gen;
        tm.mark(1);
        hipLaunchKernelGGL(k_fpfh_walk1<T>, dim3(blocks_for(N)), dim3(kBlock), 0, s, a);      // a wave per 64 records
        tm.mark(2);
        hipLaunchKernelGGL(k_fpfh_walk2<T>, dim3(blocks_for(N)), dim3(kBlock), 0, s, a);      // a lane per record
        HIP_TRY(hipGetLastError());
        tm.mark(3);
        // the rule of every searched cloud (nonfinite_error), read with the call's one read-back
        int nf = 0; unsigned staged = 0;
        if (int rc = nonfinite_fetch(gi.gp, &nf, s)) return rc;
        HIP_TRY(hipMemcpyAsync(&staged, tally, 4, hipMemcpyDeviceToHost, s));
        if (out_give(s, on_dev, out_features, d_feat, N * kFpfhBins) || (out_counts && out_give(s, on_dev, reinterpret_cast<int*>(out_counts), d_counts, N * kFpfhBins))) return -1;
        HIP_WAIT(s);
        if (nf & (kNfNaN | kNfBothInf)) return nonfinite_error(false);
        if (st) {
            st->n_grid_builds = ds.built; st->n_queries = n; st->n_passes = 2; st->n_tie_flagged = staged; st->n_tie_true = (int64_t)((N + 63) / 64) - (int64_t)staged;
            st->ms_index = tm.span(0, 1); st->ms_search = tm.span(1, 2); st->ms_kernel_search = tm.span(2, 3); st->ms_total = tm.span(0, 3);
        }
        return 0;
    });
}
