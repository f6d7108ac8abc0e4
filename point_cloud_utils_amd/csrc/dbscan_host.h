// csrc/dbscan_host.h -- host orchestration of cluster_point_cloud_dbscan (kernels and contract: dbscan.h). Included by pcu_hip.hip after the
// operator frame, the index host, voxel_host.h (own_inclusive_scan, scan_bytes) and radius_host.h (kRadOcc: the grid is radius_impl's).
#pragma once

// What a call takes from the arena beside its dataset (DatasetFrame::bytes).
template <typename T>
static size_t dbscan_bytes(int64_t n, bool on_dev) {
    const size_t N = (size_t)n;
    size_t b = align_up(N * sizeof(Pt4<T>), 256) + 2 * align_up(N, 256) + 3 * align_up(N * 4, 256) + scan_bytes(N) + 16384;
    if (!on_dev) b += align_up(N * 8, 256);
    return b;
}

// out_labels (n int64; -1: noise), out_core (n bytes, 0 / 1; may be null), *out_num_clusters. pidx: the cloud is an index object's (its grid is
// used as it is). A fixed number of launches and one wait: the cluster count and the non-finite word come back together.
template <typename T>
static int dbscan_impl(pcu_hip_ctx* c, const T* points, int64_t n, const pcu_hip_index* pidx, double eps, int64_t min_points, int64_t* out_labels, unsigned char* out_core,
                       int64_t* out_num_clusters, unsigned flags, void* stream, pcu_hip_stats* st) {
    if (!c) return fail(PCU_HIP_ERR_INVALID, "null context");
    if (out_num_clusters) *out_num_clusters = 0;
    if (pidx) if (int rc = index_check<T>(c, pidx, &n)) return rc;
    if (int rc = validate_sizes(n, n, "query_points", "dataset_points")) return rc;
    if (!(eps >= 0.0) || std::isinf(eps)) return fail(PCU_HIP_ERR_INVALID, "Invalid radius (%g): must be finite and not negative.", eps);
    if (min_points < 1) return fail(PCU_HIP_ERR_INVALID, "Invalid min_points (%lld): must be an integer of at least 1.", (long long)min_points);
    if ((!pidx && !points) || !out_labels || !out_num_clusters) return fail(PCU_HIP_ERR_INVALID, "null points / out_labels / out_num_clusters");
    const T rt = (T)eps, r2 = rt * rt;                                  // one multiply, rounded in T
    const T reach = (T)sqrt((double)r2) * ((T)1 + (T)8 * std::numeric_limits<T>::epsilon());
    DatasetFrame<T> ds{pidx, points, n, (flags & PCU_HIP_PTRS_ON_DEVICE) != 0};
    const size_t bytes = ds.bytes(kRadOcc) + dbscan_bytes<T>(n, ds.on_dev);
    return op_run(c, flags, stream, st, bytes, [&](OpFrame& fr) -> int {
        auto& [c, s, on_dev, ar, tm] = fr;      // marks 0-1: index and record order, 1-2: core pass, 2-3: union pass, flatten and ranks, 3-4: border pass
        tm.mark(0);
        if (ds.stage(ar, s)) return -1;
        const double h = sqrt((double)r2) * 1.01;                       // radius_impl's grid: cells no smaller than eps, a ball's box is 3^3 cells
        GridIndex<T> gi;
        if (int rc = ds.grid(ar, s, gi, kRadOcc, IndexFor::Atomic, std::isfinite(h) ? h : 0.0)) return rc;
        const size_t N = (size_t)n; const unsigned un = (unsigned)n;
        Pt4<T>* by_row = nullptr; unsigned char *core_pos = nullptr, *d_core = nullptr; unsigned *parent = nullptr, *flag = nullptr, *rank = nullptr; long long* d_labels = nullptr;
        long long* const h_labels = reinterpret_cast<long long*>(out_labels);
        if (aalloc(ar, &by_row, N) || aalloc(ar, &core_pos, N) || aalloc(ar, &parent, N) || aalloc(ar, &flag, N) || aalloc(ar, &rank, N) || out_room(ar, on_dev, h_labels, N, &d_labels)) return -1;
        if (out_core ? out_room(ar, on_dev, out_core, N, &d_core) : aalloc(ar, &d_core, N)) return -1;
        hipLaunchKernelGGL(k_cells_by_row<T>, dim3(blocks_for(N)), dim3(kBlock), 0, s, gi.gp, gi.sorted, gi.cell_start, (int)n, by_row);
        hipLaunchKernelGGL(k_cc_init, dim3(blocks_for(N)), dim3(kBlock), 0, s, parent, un);
        DbscanArgs<T> a{};
        a.gp = gi.gp; a.by_row = by_row; a.cell_start = gi.cell_start; a.n = (int)n; a.r2 = r2; a.reach = reach;
        a.min_points = (unsigned)std::min<int64_t>(min_points, 0x7fffffffll);          // (more than the row limit either way: nobody is core)
        a.core_pos = core_pos; a.core_row = d_core; a.parent = parent; a.rank = rank; a.labels = d_labels;
        a.cancel_word = g_cancel_mirror.load(std::memory_order_relaxed); a.cancel_gen = t_call_gen;
        const unsigned walk_blocks = blocks_for(N);                     // a wave per 64 records
        tm.mark(1);
        hipLaunchKernelGGL((k_dbscan_walk<T, kDbCore>), dim3(walk_blocks), dim3(kBlock), 0, s, a);
        tm.mark(2);
        hipLaunchKernelGGL((k_dbscan_walk<T, kDbUnion>), dim3(walk_blocks), dim3(kBlock), 0, s, a);
        hipLaunchKernelGGL(k_cc_flatten, dim3(blocks_for(N)), dim3(kBlock), 0, s, parent, un, (unsigned*)nullptr);
        hipLaunchKernelGGL(k_dbscan_roots, dim3(blocks_for(N)), dim3(kBlock), 0, s, (const unsigned*)parent, (const unsigned char*)d_core, un, flag);
        if (own_inclusive_scan<unsigned>(ar, s, flag, rank, N)) return -1;
        tm.mark(3);
        hipLaunchKernelGGL((k_dbscan_walk<T, kDbBorder>), dim3(walk_blocks), dim3(kBlock), 0, s, a);
        HIP_TRY(hipGetLastError());
        tm.mark(4);
        // the rule of every searched cloud (nonfinite_error), read with the call's one read-back; an index object was checked when it was made
        int nf = 0; unsigned count = 0;
        if (!pidx) if (int rc = nonfinite_fetch(gi.gp, &nf, s)) return rc;
        HIP_TRY(hipMemcpyAsync(&count, rank + (N - 1), 4, hipMemcpyDeviceToHost, s));
        if (out_give(s, on_dev, h_labels, d_labels, N) || (out_core && out_give(s, on_dev, out_core, d_core, N))) return -1;
        HIP_WAIT(s);
        if (nf & (kNfNaN | kNfBothInf)) return nonfinite_error(false);
        *out_num_clusters = (int64_t)count;
        if (st) {
            st->n_grid_builds = ds.built; st->n_queries = n; st->n_passes = 3; st->n_escalated = (int64_t)count;
            st->ms_index = tm.span(0, 1); st->ms_search = tm.span(1, 2); st->ms_kernel_search = tm.span(2, 3); st->ms_tie = tm.span(3, 4); st->ms_total = tm.span(0, 4);
        }
        return 0;
    });
}
