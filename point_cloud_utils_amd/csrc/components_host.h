// csrc/components_host.h -- host orchestration of connected_components and flood_fill_3d (kernels and contract: components.h). Included by
// pcu_hip.hip after the operator frame (op_run, stage_faces, out_room / out_give, the flag word's helpers), voxel_host.h (the scan) and
// mesh_host.h (mesh_validate).
#pragma once

// connected_components (src/connected_components.cpp:11-110). out_cv (nv), out_cf (nf), out_nv and out_nf (room for nv; *out_count rows are
// written) in the integer type f_kind names. One wait for the component count and the range flag; with host pointers a second one for the copies.
static int connected_components_impl(pcu_hip_ctx* c, const void* f, int64_t nf, int f_kind, int64_t nv, void* out_cv, void* out_cf, void* out_nv, void* out_nf,
                                     int64_t* out_count, unsigned flags, void* stream, pcu_hip_stats* st) {
    if (!c || !out_count) return fail(PCU_HIP_ERR_INVALID, "null context / out_count");
    *out_count = 0;
    if (int rc = mesh_validate(nv, nf, 0, f_kind)) return rc;
    if (!f || !out_cv || !out_cf || !out_nv || !out_nf) return fail(PCU_HIP_ERR_INVALID, "null f / out_cv / out_cf / out_nv / out_nf");
    const bool on_dev = flags & PCU_HIP_PTRS_ON_DEVICE;
    const size_t NV = (size_t)nv, NF = (size_t)nf, kb = (size_t)int_kind_bytes(f_kind);
    size_t bytes = 5 * align_up(NV * 4, 256) + align_up((NV / kScTile + 2) * 4, 256) + 8192;
    if (!on_dev) bytes += align_up(NF * 3 * kb, 256) + 3 * align_up(NV * kb, 256) + align_up(NF * kb, 256);
    return op_run(c, flags, stream, st, bytes, [&](OpFrame& fr) -> int {
        auto& [c, s, on_dev, ar, tm] = fr;      // marks 0-1: union, 1-2: flatten and rank, 3-4: labels and counts
        const char* d_f = nullptr;
        if (stage_faces(ar, f, NF, f_kind, on_dev, s, &d_f)) return -1;
        unsigned *parent = nullptr, *flag = nullptr, *scan = nullptr, *cnt_v = nullptr, *cnt_f = nullptr; int* d_bad = nullptr;
        if (aalloc(ar, &parent, NV) || aalloc(ar, &flag, NV) || aalloc(ar, &scan, NV) || aalloc(ar, &cnt_v, NV) || aalloc(ar, &cnt_f, NV) || flag_word(ar, s, &d_bad)) return -1;
        const unsigned unv = (unsigned)nv, unf = (unsigned)nf;
        HIP_TRY(hipMemsetAsync(cnt_v, 0, NV * 4, s));
        HIP_TRY(hipMemsetAsync(cnt_f, 0, NV * 4, s));
        tm.mark(0);
        hipLaunchKernelGGL(k_cc_init, dim3(blocks_for(NV)), dim3(kBlock), 0, s, parent, unv);
        hipLaunchKernelGGL(k_cc_faces, dim3(blocks_for(NF)), dim3(kBlock), 0, s, (const void*)d_f, f_kind, unf, unv, parent, d_bad);
        tm.mark(1);
        hipLaunchKernelGGL(k_cc_flatten, dim3(blocks_for(NV)), dim3(kBlock), 0, s, parent, unv, flag);
        if (own_inclusive_scan(ar, s, (const unsigned*)flag, scan, NV)) return -1;
        tm.mark(2);
        int bad = 0; unsigned count = 0;
        if (flag_fetch(s, d_bad, &bad)) return -1;
        HIP_TRY(hipMemcpyAsync(&count, scan + (NV - 1), 4, hipMemcpyDeviceToHost, s));
        HIP_WAIT(s);
        if (bad) return mesh_refusal(bad, nv);
        if (count == 0 || count > unv) return fail(PCU_HIP_ERR_RUNTIME, "internal: %u components of %lld vertices", count, (long long)nv);
        char *const h_cv = static_cast<char*>(out_cv), *const h_cf = static_cast<char*>(out_cf), *const h_nv = static_cast<char*>(out_nv), *const h_nf = static_cast<char*>(out_nf);
        char *d_cv = nullptr, *d_cf = nullptr, *d_nv = nullptr, *d_nf = nullptr;
        if (out_room(ar, on_dev, h_cv, NV * kb, &d_cv) || out_room(ar, on_dev, h_cf, NF * kb, &d_cf) || out_room(ar, on_dev, h_nv, (size_t)count * kb, &d_nv) ||
            out_room(ar, on_dev, h_nf, (size_t)count * kb, &d_nf)) return -1;
        tm.mark(3);
        hipLaunchKernelGGL(k_cc_vertex_labels, dim3(blocks_for(NV)), dim3(kBlock), 0, s, (const unsigned*)parent, (const unsigned*)scan, unv, f_kind, (void*)d_cv, cnt_v);
        hipLaunchKernelGGL(k_cc_face_labels, dim3(blocks_for(NF)), dim3(kBlock), 0, s, (const void*)d_f, f_kind, unf, unv, (const unsigned*)parent, (const unsigned*)scan,
                           (void*)d_cf, cnt_f);
        hipLaunchKernelGGL(k_cc_counts_out, dim3(blocks_for(count)), dim3(kBlock), 0, s, (const unsigned*)cnt_v, (const unsigned*)cnt_f, count, f_kind, (void*)d_nv, (void*)d_nf);
        HIP_TRY(hipGetLastError());
        tm.mark(4);
        if (out_give(s, on_dev, h_cv, d_cv, NV * kb) || out_give(s, on_dev, h_cf, d_cf, NF * kb) || out_give(s, on_dev, h_nv, d_nv, (size_t)count * kb) ||
            out_give(s, on_dev, h_nf, d_nf, (size_t)count * kb)) return -1;
        HIP_WAIT(s);
        *out_count = (int64_t)count;
        if (st) {
            st->n_queries = nf; st->n_escalated = (int64_t)count; st->n_passes = 1;
            st->ms_index = tm.span(0, 1); st->ms_search = tm.span(1, 2); st->ms_tie = tm.span(3, 4); st->ms_total = tm.span(0, 4);
        }
        return 0;
    });
}

// The fill value as the reference's `(npe_Scalar_grid) flood_value` gives it wherever that cast is defined; a double outside an integer
// type's range saturates and a NaN becomes 0 there.
template <typename V>
static V fill_cast(double x) {
    if constexpr (std::is_integral<V>::value) {
        constexpr double top = sizeof(V) == 4 ? 2147483648.0 : 9223372036854775808.0;
        if (x != x) return (V)0;
        if (x >= top) return std::numeric_limits<V>::max();
        if (x <= -top) return std::numeric_limits<V>::min();
    }
    return (V)x;
}

// flood_fill_3d (src/flood_fill_3d.cpp:10-75, point_cloud_utils/_voxels.py:7-30). grid and out (sx, sy, sz), z fastest, must not overlap.
// Four launches and one wait whatever the region looks like.
template <typename V>
static int flood_fill_typed(pcu_hip_ctx* c, const void* grid, void* out, size_t N, unsigned h, unsigned d, unsigned seed, double fill_value, int64_t* out_filled,
                            unsigned flags, void* stream, pcu_hip_stats* st) {
    const bool on_dev = flags & PCU_HIP_PTRS_ON_DEVICE;
    const size_t bytes = align_up(N * 4, 256) + (on_dev ? 0 : 2 * align_up(N * sizeof(V), 256)) + 8192;
    return op_run(c, flags, stream, st, bytes, [&](OpFrame& fr) -> int {
        auto& [c, s, on_dev, ar, tm] = fr;      // marks 0-1: runs and unions, 1-2: flatten, 2-3: the filled copy
        const V* d_in = nullptr; V *const h_out = static_cast<V*>(out), *d_out = nullptr;
        if (stage_any(ar, static_cast<const V*>(grid), N, on_dev, s, &d_in) || out_room(ar, on_dev, h_out, N, &d_out)) return -1;
        unsigned* parent = nullptr; unsigned long long* d_cnt = nullptr;
        if (aalloc(ar, &parent, N) || aalloc(ar, &d_cnt, 1)) return -1;
        const unsigned n = (unsigned)N, nb = blocks_for(N);
        HIP_TRY(hipMemsetAsync(d_cnt, 0, 8, s));
        tm.mark(0);
        hipLaunchKernelGGL(k_fill_init<V>, dim3(nb), dim3(kBlock), 0, s, d_in, n, d, seed, parent);
        hipLaunchKernelGGL(k_fill_union<V>, dim3(nb), dim3(kBlock), 0, s, d_in, n, h, d, seed, parent);
        tm.mark(1);
        hipLaunchKernelGGL(k_cc_flatten, dim3(nb), dim3(kBlock), 0, s, parent, n, (unsigned*)nullptr);
        tm.mark(2);
        hipLaunchKernelGGL(k_fill_write<V>, dim3(std::min((unsigned)((N + kFillTrip - 1) / kFillTrip), kFillMaxBlocks)), dim3(kBlock), 0, s, d_in, d_out, n, seed, (const unsigned*)parent, fill_cast<V>(fill_value), d_cnt);
        HIP_TRY(hipGetLastError());
        tm.mark(3);
        unsigned long long filled = 0;
        HIP_TRY(hipMemcpyAsync(&filled, d_cnt, 8, hipMemcpyDeviceToHost, s));
        if (out_give(s, on_dev, h_out, d_out, N)) return -1;
        HIP_WAIT(s);
        *out_filled = (int64_t)filled;
        if (st) {
            st->n_queries = (int64_t)N; st->n_escalated = (int64_t)filled; st->n_passes = 1;
            st->ms_index = tm.span(0, 1); st->ms_search = tm.span(1, 2); st->ms_tie = tm.span(2, 3); st->ms_total = tm.span(0, 3);
        }
        return 0;
    });
}
static int flood_fill_impl(pcu_hip_ctx* c, const void* grid, void* out, int64_t sx, int64_t sy, int64_t sz, const int64_t* seed3, int kind, double fill_value,
                           int64_t* out_filled, unsigned flags, void* stream, pcu_hip_stats* st) {
    if (!c || !out_filled) return fail(PCU_HIP_ERR_INVALID, "null context / out_filled");
    *out_filled = 0;
    if (!grid || !out || !seed3) return fail(PCU_HIP_ERR_INVALID, "null grid / out / seed3");
    if (kind < 0 || kind > 3) return fail(PCU_HIP_ERR_INVALID, "kind must be one of PCU_HIP_GRID_INT32 / INT64 / FLOAT32 / FLOAT64");
    if (sx <= 0 || sy <= 0 || sz <= 0 || seed3[0] < 0 || seed3[0] >= sx || seed3[1] < 0 || seed3[1] >= sy || seed3[2] < 0 || seed3[2] >= sz)
        return fail(PCU_HIP_ERR_INVALID, "seed point must be inside grid");
    if (sx > kCcMaxIndex || sy > kCcMaxIndex / sx || sz > kCcMaxIndex / (sx * sy))
        return fail(PCU_HIP_ERR_INVALID, "grids with more than 2^31-16 cells are not supported");
    const size_t N = (size_t)(sx * sy * sz);
    const unsigned seed = (unsigned)((seed3[0] * sy + seed3[1]) * sz + seed3[2]);
    const unsigned h = (unsigned)sy, d = (unsigned)sz;
    switch (kind) {
        case 0: return flood_fill_typed<int32_t>(c, grid, out, N, h, d, seed, fill_value, out_filled, flags, stream, st);
        case 1: return flood_fill_typed<long long>(c, grid, out, N, h, d, seed, fill_value, out_filled, flags, stream, st);
        case 2: return flood_fill_typed<float>(c, grid, out, N, h, d, seed, fill_value, out_filled, flags, stream, st);
        default: return flood_fill_typed<double>(c, grid, out, N, h, d, seed, fill_value, out_filled, flags, stream, st);
    }
}
