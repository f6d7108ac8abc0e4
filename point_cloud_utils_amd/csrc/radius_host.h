// csrc/radius_host.h -- host orchestration of radius_search / radius_count (kernels and contract: radius.h). Included by pcu_hip.hip after the
// operator frame, the parking functions, the index host and voxel_host.h (own_radix_sort, own_inclusive_scan, sort_bytes, scan_bytes, bits_of).
#pragma once

constexpr double kRadOcc = 4.0;                         // the free functions' grid: cells of about the radius, no finer than this many points per cell
constexpr unsigned long long kRadMaxTotal = 1ull << 31; // a result holds fewer neighbours than this: positions inside it fit 32 bits


// What a call takes from the arena beside its dataset (DatasetFrame::bytes).
template <typename T>
static size_t radius_bytes(int64_t nq, int64_t nr, bool on_dev) {
    const size_t NQ = (size_t)nq, NR = (size_t)nr;
    size_t b = align_up(NR * sizeof(Pt4<T>), 256) + sort_bytes(NQ) + 3 * align_up(NQ * 4, 256) + align_up(NQ * 8, 256) + align_up((NQ + 1) * 8, 256) + 2 * scan_bytes(NQ) + 16384;
    if (!on_dev) b += align_up(NQ * 3 * sizeof(T), 256) + align_up(NQ * 8, 256);
    return b;
}
// Rows longer than kRadBlockRow: three stable sorts of their members (dataset row, bits of d2, query row). One wait: how many members they hold.
template <typename T>
static int radius_sort_long(Arena& ar, hipStream_t s, const unsigned* long_len, const unsigned* counts, const unsigned long long* offs, int64_t nq, int64_t nr, T* d2, int* row) {
    unsigned* scan = nullptr; unsigned nl = 0;
    if (aalloc(ar, &scan, (size_t)nq + 1) || own_inclusive_scan<unsigned>(ar, s, long_len, scan, (size_t)nq)) return -1;
    HIP_TRY(hipMemcpyAsync(&nl, scan + (nq - 1), sizeof(unsigned), hipMemcpyDeviceToHost, s));
    HIP_WAIT(s);
    if (!nl) return 0;
    const RadLong L{scan, counts, offs, (int)nq, nl};
    unsigned long long *ka = nullptr, *kb = nullptr; unsigned *ia = nullptr, *ib = nullptr; T* td = nullptr; int* tr = nullptr;
    if (aalloc(ar, &ka, (size_t)nl) || aalloc(ar, &kb, (size_t)nl) || aalloc(ar, &ia, (size_t)nl) || aalloc(ar, &ib, (size_t)nl) || aalloc(ar, &td, (size_t)nl) || aalloc(ar, &tr, (size_t)nl)) return -1;
    const int bits[3] = {bits_of((unsigned long long)(nr - 1)), 8 * (int)sizeof(T), bits_of((unsigned long long)(nq - 1))};
    bool identity = true;
    for (int stage = 0; stage < 3; ++stage) {
        if (!bits[stage]) continue;
        hipLaunchKernelGGL(k_radius_long_key<T>, dim3(blocks_for(nl)), dim3(kBlock), 0, s, L, identity ? (const unsigned*)nullptr : (const unsigned*)ia, stage, (const T*)d2, (const int*)row, ka);
        if (own_radix_sort(ar, s, &ka, &kb, &ia, &ib, identity, (int)nl, bits[stage])) return -1;
        identity = false;
    }
    hipLaunchKernelGGL(k_radius_long_move<T>, dim3(blocks_for(nl)), dim3(kBlock), 0, s, L, identity ? (const unsigned*)nullptr : (const unsigned*)ia, 0, d2, row, td, tr);
    hipLaunchKernelGGL(k_radius_long_move<T>, dim3(blocks_for(nl)), dim3(kBlock), 0, s, L, (const unsigned*)nullptr, 1, d2, row, td, tr);
    HIP_TRY(hipGetLastError());
    return 0;
}

// radius_search (count_only == false): out = (nq + 1) int64 offsets, *out_total = neighbours; the rows are parked for pcu_hip_radius_search_take.
// radius_count (count_only == true): out = (nq) int64 row lengths. pidx: the dataset is an index object's (its grid is used as it is).
template <typename T>
static int radius_impl(pcu_hip_ctx* c, const T* query, int64_t nq, const T* dataset, int64_t nr, const pcu_hip_index* pidx, double radius, int sort_results, bool count_only,
                       int64_t* out, int64_t* out_total, unsigned flags, void* stream, pcu_hip_stats* st) {
    if (!c) return fail(PCU_HIP_ERR_INVALID, "null context");
    if (out_total) *out_total = 0;
    if (!count_only) c->parked = ParkedResult();
    if (pidx) if (int rc = index_check<T>(c, pidx, &nr)) return rc;
    if (int rc = validate_sizes(nq, nr, "query_points", "dataset_points")) return rc;
    if (!(radius >= 0.0) || std::isinf(radius)) return fail(PCU_HIP_ERR_INVALID, "Invalid radius (%g): must be finite and not negative.", radius);
    if (!query || (!pidx && !dataset) || !out || (!count_only && !out_total)) return fail(PCU_HIP_ERR_INVALID, "null query / dataset / output");
    const T rt = (T)radius, r2 = rt * rt;                               // one multiply, rounded in T
    const T reach = (T)sqrt((double)r2) * ((T)1 + (T)8 * std::numeric_limits<T>::epsilon());
    DatasetFrame<T> ds{pidx, dataset, nr, (flags & PCU_HIP_PTRS_ON_DEVICE) != 0};
    const size_t bytes = ds.bytes(kRadOcc) + radius_bytes<T>(nq, nr, ds.on_dev);
    return op_run(c, flags, stream, st, bytes, [&](OpFrame& fr) -> int {
        auto& [c, s, on_dev, ar, tm] = fr;      // marks 0-1: index, record order, query order, 1-2: count pass, 2-3: scan, wait and fill pass, 3-4: row sort
        tm.mark(0);
        const T* dq = nullptr;
        if (stage_in(ar, query, nq, on_dev, s, &dq) || ds.stage(ar, s)) return -1;
        const double h = sqrt((double)r2) * 1.01;                       // the call's own grid: cells no smaller than the radius, a ball's box is 3^3 cells
        GridIndex<T> gi;
        if (int rc = ds.grid(ar, s, gi, kRadOcc, IndexFor::Atomic, std::isfinite(h) ? h : 0.0)) return rc;
        // the records of every cell in ascending row order: the walk's order is then a function of the input (normals.h: k_cells_by_row)
        Pt4<T>* by_row = nullptr;
        if (aalloc(ar, &by_row, (size_t)nr)) return -1;
        hipLaunchKernelGGL(k_cells_by_row<T>, dim3(blocks_for((size_t)nr)), dim3(kBlock), 0, s, gi.gp, gi.sorted, gi.cell_start, (int)nr, by_row);
        // the queries in the cell order of the dataset's grid (a stable sort of their cell keys: equal cells keep the caller's order)
        unsigned long long *ka = nullptr, *kb = nullptr; unsigned *ia = nullptr, *ib = nullptr, *counts = nullptr;
        if (aalloc(ar, &ka, (size_t)nq) || aalloc(ar, &kb, (size_t)nq) || aalloc(ar, &ia, (size_t)nq) || aalloc(ar, &ib, (size_t)nq) || aalloc(ar, &counts, (size_t)nq)) return -1;
        hipLaunchKernelGGL(k_radius_qkeys<T>, dim3(blocks_for((size_t)nq)), dim3(kBlock), 0, s, gi.gp, dq, (int)nq, ka);
        if (own_radix_sort(ar, s, &ka, &kb, &ia, &ib, /*ids_identity=*/true, (int)nq, std::max(1, bits_of((unsigned long long)gi.max_cells)))) return -1;
        RadiusArgs<T> a{};
        a.gp = gi.gp; a.by_row = by_row; a.cell_start = gi.cell_start; a.nr = (int)nr; a.query = dq; a.order = ia; a.nq = (int)nq; a.r2 = r2; a.reach = reach; a.counts = counts;
        a.cancel_word = g_cancel_mirror.load(std::memory_order_relaxed); a.cancel_gen = t_call_gen;
        const unsigned walk_blocks = blocks_for((size_t)nq);           // a wave per 64 queries
        tm.mark(1);
        hipLaunchKernelGGL((k_radius_walk<T, false>), dim3(walk_blocks), dim3(kBlock), 0, s, a);
        HIP_TRY(hipGetLastError());
        tm.mark(2);
        // the rule of every searched cloud (nonfinite_error): read with the call's one read-back; an index object was checked when it was made
        int nf = 0;
        if (!pidx) if (int rc = nonfinite_fetch(gi.gp, &nf, s)) return rc;
        if (st) { st->n_grid_builds = ds.built; st->n_queries = nq; st->n_passes = 1; }
        long long* const h_out = reinterpret_cast<long long*>(out);
        if (count_only) {
            long long* d_out = nullptr;
            if (out_room(ar, on_dev, h_out, (size_t)nq, &d_out)) return -1;
            hipLaunchKernelGGL(k_radius_counts_out, dim3(blocks_for((size_t)nq)), dim3(kBlock), 0, s, (const unsigned*)counts, (int)nq, d_out);
            HIP_TRY(hipGetLastError());
            if (out_give(s, on_dev, h_out, d_out, (size_t)nq)) return -1;
            HIP_WAIT(s);
            if (nf & (kNfNaN | kNfBothInf)) return nonfinite_error(false);
            if (st) { st->ms_index = tm.span(0, 1); st->ms_search = tm.span(1, 2); st->ms_total = tm.span(0, 2); }
            return 0;
        }
        unsigned long long *len64 = nullptr, *offs = nullptr; unsigned *mid_list = nullptr, *long_len = nullptr, *tally = nullptr;
        if (aalloc(ar, &len64, (size_t)nq) || aalloc(ar, &offs, (size_t)nq + 1) || aalloc(ar, &mid_list, (size_t)nq) || aalloc(ar, &long_len, (size_t)nq) || aalloc(ar, &tally, 4)) return -1;
        HIP_TRY(hipMemsetAsync(tally, 0, 16, s));
        HIP_TRY(hipMemsetAsync(offs, 0, 8, s));
        hipLaunchKernelGGL(k_radius_lengths, dim3(blocks_for((size_t)nq)), dim3(kBlock), 0, s, (const unsigned*)counts, (int)nq, len64, mid_list, long_len, tally);
        if (own_inclusive_scan<unsigned long long>(ar, s, len64, offs + 1, (size_t)nq)) return -1;
        unsigned long long total = 0; unsigned tiers[2] = {0, 0};
        HIP_TRY(hipMemcpyAsync(&total, offs + nq, 8, hipMemcpyDeviceToHost, s));
        HIP_TRY(hipMemcpyAsync(tiers, tally, 8, hipMemcpyDeviceToHost, s));
        HIP_WAIT(s);
        if (nf & (kNfNaN | kNfBothInf)) return nonfinite_error(false);
        if (total >= kRadMaxTotal)
            return fail(PCU_HIP_ERR_INVALID, "radius_search: the result would hold %llu neighbours; one call returns at most 2147483647 (2^31 - 1). Use a smaller radius or "
                        "fewer queries per call (radius_count has no such limit).", total);
        // the result's segments -- indices, and the distances, which hold d2 until the rows leave -- and the members' rows behind them
        char *seg[kParkSegs], *wk = nullptr;
        if (park_reserve(c, {(size_t)total * 8, (size_t)total * sizeof(T)}, seg, (size_t)total * 4, &wk)) return -1;
        T* d2 = reinterpret_cast<T*>(seg[1]); int* row = reinterpret_cast<int*>(wk);
        if (total > 0) {
            a.offsets = offs; a.d2 = d2; a.row = row;
            hipLaunchKernelGGL((k_radius_walk<T, true>), dim3(walk_blocks), dim3(kBlock), 0, s, a);
            HIP_TRY(hipGetLastError());
        }
        tm.mark(3);
        if (total > 0 && sort_results) {
            hipLaunchKernelGGL(k_radius_sort_wave<T>, dim3((unsigned)((nq + 15) / 16)), dim3(kBlock), 0, s, (const unsigned long long*)offs, (int)nq, d2, row);
            if (tiers[0]) hipLaunchKernelGGL(k_radius_sort_block<T>, dim3(tiers[0]), dim3(kBlock), 0, s, (const unsigned*)mid_list, (const unsigned long long*)offs, d2, row);
            HIP_TRY(hipGetLastError());
            if (tiers[1]) if (int rc = radius_sort_long<T>(ar, s, long_len, counts, offs, nq, nr, d2, row)) return rc;
        }
        tm.mark(4);
        if (total > 0)
            hipLaunchKernelGGL(k_radius_out<T>, dim3(blocks_for((size_t)total)), dim3(kBlock), 0, s, (const T*)d2, (const int*)row, total, (flags & PCU_HIP_SQUARED) ? 1 : 0,
                               reinterpret_cast<long long*>(seg[0]), d2);
        HIP_TRY(hipGetLastError());
        if (out_give(s, on_dev, h_out, reinterpret_cast<const long long*>(offs), (size_t)nq + 1)) return -1;
        HIP_WAIT(s);
        park_commit(c, Parked::RadiusRows, nq, (int64_t)total);
        *out_total = (int64_t)total;
        if (st) {
            st->n_escalated = (int64_t)total; st->n_tie_flagged = tiers[0]; st->n_tie_true = tiers[1];
            st->ms_index = tm.span(0, 1); st->ms_search = tm.span(1, 2); st->ms_kernel_search = tm.span(2, 3); st->ms_tie = tm.span(3, 4); st->ms_total = tm.span(0, 4);
        }
        return 0;
    });
}
// The rows of this context's last pcu_hip_radius_search_* / pcu_hip_index_radius_search_*. Once.
static int radius_take_impl(pcu_hip_ctx* c, int64_t nq, int64_t total, int64_t* out_idx, void* out_d, unsigned flags, void* stream) {
    if (!c || ((!out_idx || !out_d) && total > 0)) return fail(PCU_HIP_ERR_INVALID, "null context / out_indices / out_dists");
    return park_take(c, Parked::RadiusRows, nq, total, {out_idx, out_d}, flags, stream,
                     "pcu_hip_radius_search_take: this context holds no radius result of %lld queries and %lld neighbours");
}
