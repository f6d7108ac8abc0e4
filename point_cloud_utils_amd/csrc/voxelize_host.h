// csrc/voxelize_host.h -- host orchestration of voxelize_triangle_mesh, sparse_voxel_grid_boundary and voxel_grid_geometry (kernels and
// contract: voxelize.h). Included by pcu_hip.hip after the operator frame and the parking functions, voxel_host.h (sort_keys, rank_runs,
// the scan), mesh_host.h (mesh_validate, int_kind_check) and mesh_sample_host.h (ms_mesh_stage / ms_mesh_refuse).
#pragma once

constexpr int64_t kVxMaxRows = 0x7ffffff0ll;                 // rows one sort takes
constexpr unsigned long long kVxLaunchSlices = 1ull << 16;   // slices per launch of the test and emit passes (2^27 candidates); the call's cancellation check runs between launches

static int vx_grid_check(const double* size, const double* origin, const char* size_text, VxGrid* g) {
    if (!size || !origin) return fail(PCU_HIP_ERR_INVALID, "null voxel_size / voxel_origin");
    for (int k = 0; k < 3; ++k) {
        if (!(size[k] > 0.0)) return fail(PCU_HIP_ERR_INVALID, "%s", size_text);
        if (!std::isfinite(size[k]) || !std::isfinite(origin[k])) return fail(PCU_HIP_ERR_INVALID, "voxel_size and voxel_origin must be finite");
        g->size[k] = size[k]; g->origin[k] = origin[k];
    }
    return 0;
}
static int vx_bits_between(int lo, int hi) { return bits_of((unsigned long long)((unsigned)(lo + (1 << 20)) ^ (unsigned)(hi + (1 << 20)))); }

// The rows of the context's last voxelization are parked for pcu_hip_voxelize_take: the row count is the one value the host has to see
// before the caller's output can exist.
static int vx_park(pcu_hip_ctx* c, hipStream_t s, const int* rows, int64_t m) {
    char* seg[kParkSegs];
    if (park_reserve(c, {(size_t)m * 12}, seg)) return -1;
    HIP_TRY(hipMemcpyAsync(seg[0], rows, (size_t)m * 12, hipMemcpyDeviceToDevice, s));
    HIP_WAIT(s);
    park_commit(c, Parked::VoxelRows, m, 0);
    return 0;
}

// voxelize_triangle_mesh (src/voxelize_triangle_mesh.cpp; contract: voxelize.h). Three waits: the flags and the candidate total, the number of
// kept candidates, the number of rows.
template <typename T>
static int voxelize_impl(pcu_hip_ctx* c, const MeshGiven<T>& m, const double* size, const double* origin, int64_t* out_rows, unsigned flags, void* stream,
                         pcu_hip_stats* st) {
    if (!c || !out_rows) return fail(PCU_HIP_ERR_INVALID, "null context / out_rows");
    *out_rows = 0;
    c->parked = ParkedResult();
    if (int rc = mesh_validate(m.nv, m.nf, 0, m.f_kind)) return rc;
    VxGrid g;
    if (int rc = vx_grid_check(size, origin, "Invalid voxel size", &g)) return rc;
    const size_t NF = (size_t)m.nf;
    const size_t bytes = ms_mesh_bytes(m, flags & PCU_HIP_PTRS_ON_DEVICE) + align_up(NF * 24, 256) + 2 * align_up(NF * 8, 256) + (1 << 20);
    return op_run(c, flags, stream, st, bytes, [&](OpFrame& fr) -> int {
        auto& [c, s, on_dev, ar, tm] = fr;      // marks 0-1: extent and scan, 2-3: test pass, 4-5: emit pass, 5-6: sort and unique
        MsMesh<T> M; MsSeen<T> seen;
        tm.mark(0);
        if (ms_mesh_stage(ar, s, m, on_dev, M)) return -1;
        int* ext = nullptr; unsigned long long *cnt = nullptr, *C = nullptr; VxHead* head = nullptr;
        if (aalloc(ar, &ext, NF * 6) || aalloc(ar, &cnt, NF) || aalloc(ar, &C, NF) || aalloc(ar, &head, 1)) return -1;
        int* d_bad = mesh_head_flag(M.head);
        const int nf = (int)m.nf;
        hipLaunchKernelGGL(k_vx_head_init, dim3(1), dim3(64), 0, s, head);
        hipLaunchKernelGGL(k_vx_extent<T>, dim3(blocks_for((size_t)nf)), dim3(kBlock), 0, s, M.v, (const int*)M.fidx, nf, g, ext, cnt, d_bad, head);
        if (own_inclusive_scan(ar, s, (const unsigned long long*)cnt, C, NF)) return -1;
        tm.mark(1);
        unsigned long long total = 0; VxHead hh;
        if (ms_mesh_readback(s, M, false, &seen)) return -1;
        HIP_TRY(hipMemcpyAsync(&total, C + (NF - 1), 8, hipMemcpyDeviceToHost, s));
        HIP_TRY(hipMemcpyAsync(&hh, head, sizeof hh, hipMemcpyDeviceToHost, s));
        HIP_WAIT(s);
        if (int rc = ms_mesh_refuse(seen, m.nv, false)) return rc;
        if (seen.bad & kVxBadRange) return fail(PCU_HIP_ERR_INVALID, "voxelize_triangle_mesh: a voxel coordinate outside [-2^20, 2^20) is not supported (voxel_size too small for this mesh and voxel_origin)");
        if (total > kVxMaxCandidates)
            return fail(PCU_HIP_ERR_INVALID, "voxelize_triangle_mesh: the faces' boxes hold more than 2^32 candidate voxels (voxel_size too small for this mesh)");
        if (total == 0) return fail(PCU_HIP_ERR_RUNTIME, "internal: no candidate voxels");
        // test pass
        const unsigned long long nslices = (total + kVxSlice - 1) / kVxSlice;
        unsigned long long *words = nullptr, *bcnt = nullptr, *bscan = nullptr;
        if (aalloc(ar, &words, (size_t)nslices * kVxWords) || aalloc(ar, &bcnt, (size_t)nslices) || aalloc(ar, &bscan, (size_t)nslices)) return -1;
        int launches = 0;
        tm.mark(2);
        for (unsigned long long s0 = 0; s0 < nslices; s0 += kVxLaunchSlices, ++launches) {
            if (s0) HIP_WAIT(s);
            const unsigned nb = (unsigned)std::min(kVxLaunchSlices, nslices - s0);
            hipLaunchKernelGGL(k_vx_test<T>, dim3(nb), dim3(kVxThreads), 0, s, M.v, (const int*)M.fidx, (const int*)ext, (const unsigned long long*)C, nf, total, s0, g, words, bcnt);
        }
        HIP_TRY(hipGetLastError());
        if (own_inclusive_scan(ar, s, (const unsigned long long*)bcnt, bscan, (size_t)nslices)) return -1;
        tm.mark(3);
        unsigned long long kept = 0;
        HIP_TRY(hipMemcpyAsync(&kept, bscan + (nslices - 1), 8, hipMemcpyDeviceToHost, s));
        HIP_WAIT(s);
        if (kept == 0) return fail(PCU_HIP_ERR_RUNTIME, "internal: no voxel overlaps the mesh");
        if (kept > (unsigned long long)kVxMaxRows) return fail(PCU_HIP_ERR_INVALID, "voxelize_triangle_mesh: more than 2^31-16 overlapping (face, voxel) pairs are not supported");
        // emit pass, sort, unique
        const int K = (int)kept;
        SortedRuns r; int* rows = nullptr;
        if (aalloc(ar, &r.keys, (size_t)K) || aalloc(ar, &rows, (size_t)K * 3)) return -1;
        tm.mark(4);
        for (unsigned long long s0 = 0; s0 < nslices; s0 += kVxLaunchSlices) {
            if (s0) HIP_WAIT(s);
            const unsigned nb = (unsigned)std::min(kVxLaunchSlices, nslices - s0);
            hipLaunchKernelGGL(k_vx_emit, dim3(nb), dim3(kVxThreads), 0, s, (const int*)ext, (const unsigned long long*)C, nf, s0, (const unsigned long long*)words,
                               (const unsigned long long*)bcnt, (const unsigned long long*)bscan, r.keys);
        }
        HIP_TRY(hipGetLastError());
        tm.mark(5);
        const int bits = 3 * std::max(vx_bits_between(hh.lo[0], hh.hi[0]), std::max(vx_bits_between(hh.lo[1], hh.hi[1]), vx_bits_between(hh.lo[2], hh.hi[2])));
        if (sort_keys(ar, s, r, K, bits) || rank_runs(ar, s, r, K)) return -1;
        hipLaunchKernelGGL(k_vx_rows, dim3(blocks_for((size_t)K)), dim3(kBlock), 0, s, (const unsigned long long*)r.keys, (const unsigned*)r.flag, (const unsigned*)r.scan, K,
                           rows);
        HIP_TRY(hipGetLastError());
        tm.mark(6);
        unsigned n_rows = 0;
        HIP_TRY(hipMemcpyAsync(&n_rows, r.scan + (K - 1), 4, hipMemcpyDeviceToHost, s));
        HIP_WAIT(s);
        if (vx_park(c, s, rows, (int64_t)n_rows)) return -1;
        *out_rows = (int64_t)n_rows;
        if (st) {
            st->n_queries = (int64_t)total; st->n_escalated = (int64_t)kept; st->n_passes = launches;
            st->ms_index = tm.span(0, 1); st->ms_search = tm.span(2, 3); st->ms_tie = tm.span(4, 5); st->ms_kernel_search = tm.span(5, 6); st->ms_total = tm.span(0, 6);
        }
        return 0;
    });
}
// The rows of this context's last pcu_hip_voxelize_triangle_mesh_*: out_ijk (rows, 3) int32. They can be taken once.
static int voxelize_take_impl(pcu_hip_ctx* c, int64_t rows, int32_t* out_ijk, unsigned flags, void* stream) {
    if (!c || !out_ijk) return fail(PCU_HIP_ERR_INVALID, "null context / out_ijk");
    return park_take(c, Parked::VoxelRows, rows, 0, {out_ijk}, flags, stream, "pcu_hip_voxelize_take: this context holds no voxelization of %lld rows");
}

// sparse_voxel_grid_boundary (src/sparse_voxel_grid.cpp:473-522). out_idx (n) worst case; *out_count rows are written, ascending.
static int voxel_boundary_impl(pcu_hip_ctx* c, const void* ijk, int64_t n, int kind, int64_t* out_idx, int64_t* out_count, unsigned flags, void* stream) {
    if (!c || !out_count) return fail(PCU_HIP_ERR_INVALID, "null context / out_count");
    *out_count = 0;
    if (n <= 0) return fail(PCU_HIP_ERR_INVALID, "Invalid grid_coordinates has zero rows!");
    if (int rc = int_kind_check(kind)) return rc;
    if (n > kVxMaxRows) return fail(PCU_HIP_ERR_INVALID, "voxel grids with more than 2^31-16 rows are not supported");
    const size_t N = (size_t)n;
    const size_t bytes = sort_bytes(N) + scan_bytes(N) + 2 * align_up(N * 8, 256) + 2 * align_up(N * 4, 256) +      // (codes and rows; flags and scan)
                         ((flags & PCU_HIP_PTRS_ON_DEVICE) ? 0 : align_up(N * 3 * int_kind_bytes(kind), 256)) + (1 << 20);
    return op_run(c, flags, stream, nullptr, bytes, [&](OpFrame& fr) -> int {
        auto& [c, s, on_dev, ar, tm] = fr;
        const char* d_in = nullptr;
        if (stage_faces(ar, ijk, N, kind, on_dev, s, &d_in)) return -1;
        unsigned long long* codes = nullptr; SortedRuns r; int* d_bad = nullptr;
        long long *const h_out = reinterpret_cast<long long*>(out_idx), *d_out = nullptr;
        if (aalloc(ar, &codes, N) || aalloc(ar, &r.keys, N) || flag_word(ar, s, &d_bad) || out_room(ar, on_dev, h_out, N, &d_out)) return -1;
        const int nn = (int)n; const unsigned nb = blocks_for(N);
        hipLaunchKernelGGL(k_vb_codes, dim3(nb), dim3(kBlock), 0, s, (const void*)d_in, kind, nn, codes, r.keys, d_bad);
        if (sort_keys(ar, s, r, nn, 63)) return -1;
        if (rank_flags(ar, s, r, nn, [&, s = s](unsigned* flag) {
                hipLaunchKernelGGL(k_vb_flag, dim3(nb), dim3(kBlock), 0, s, (const unsigned long long*)codes, (const unsigned long long*)r.keys, nn, flag);
            })) return -1;
        hipLaunchKernelGGL(k_vb_rows, dim3(nb), dim3(kBlock), 0, s, (const unsigned*)r.flag, (const unsigned*)r.scan, nn, d_out, (const int*)d_bad);
        HIP_TRY(hipGetLastError());
        int bad = 0; unsigned m = 0;
        if (read_flag_and_last(s, d_bad, r.scan, N, &bad, &m)) return -1;
        HIP_WAIT(s);
        if (bad) return fail(PCU_HIP_ERR_INVALID, "Invalid vertex leads to an overflow integer. Perhaps grid_size is too small.");
        bool copied = false;
        if (out_give(s, on_dev, h_out, d_out, (size_t)m, &copied)) return -1;
        if (copied) HIP_WAIT(s);
        *out_count = (int64_t)m;
        return 0;
    });
}

// voxel_grid_geometry (src/mesh_for_voxels.cpp:11-79): out_v (8 n, 3) float, out_f (12 n, 3) int32
static int voxel_geometry_impl(pcu_hip_ctx* c, const void* ijk, int64_t n, int kind, const double* size, const double* origin, double gap, float* out_v, int32_t* out_f,
                               unsigned flags, void* stream) {
    if (!c) return fail(PCU_HIP_ERR_INVALID, "null context");
    if (n <= 0) return fail(PCU_HIP_ERR_INVALID, "Invalid input point cloud with zero points: points must have shape (n, 3) (n > 0). Got points.shape =(%lld, 3).", (long long)n);
    if (int rc = int_kind_check(kind)) return rc;
    VxGrid g;
    if (int rc = vx_grid_check(size, origin, "Voxel size must be positive", &g)) return rc;
    if (8 * n > 0x7fffffffll) return fail(PCU_HIP_ERR_INVALID, "voxel geometry with more than 2^31-1 vertices does not fit the int32 faces");
    const size_t N = (size_t)n;
    const size_t bytes = (flags & PCU_HIP_PTRS_ON_DEVICE) ? 4096 : align_up(N * 3 * int_kind_bytes(kind), 256) + align_up(N * 96, 256) + align_up(N * 144, 256) + 4096;
    return op_run(c, flags, stream, nullptr, bytes, [&](OpFrame& fr) -> int {
        auto& [c, s, on_dev, ar, tm] = fr;
        const char* d_in = nullptr;
        if (stage_faces(ar, ijk, N, kind, on_dev, s, &d_in)) return -1;
        float* d_v = nullptr; int* d_f = nullptr;
        if (out_room(ar, on_dev, out_v, N * 24, &d_v) || out_room(ar, on_dev, out_f, N * 36, &d_f)) return -1;
        hipLaunchKernelGGL(k_vg_geometry, dim3(blocks_for(12 * N)), dim3(kBlock), 0, s, (const void*)d_in, kind, (long long)n, g, gap, d_v, d_f);
        HIP_TRY(hipGetLastError());
        if (out_give(s, on_dev, out_v, d_v, N * 24) || out_give(s, on_dev, out_f, d_f, N * 36)) return -1;
        HIP_WAIT(s);
        return 0;
    });
}
