// csrc/marching_cubes_host.h -- host orchestration of marching_cubes_sparse_voxel_grid and sparse_voxel_grid_to_hex_mesh (kernels and contract:
// marching_cubes.h). Included by pcu_hip.hip after the operator frame and the parking functions, voxel_host.h (sort_keys, rank_runs, the
// scan), mesh_host.h (int_kind_check) and voxelize_host.h (vx_grid_check, kVxMaxRows).
#pragma once

// Both operators learn the size of their results late, so the results are parked for the matching _take call, as a voxelization's rows are
// (vx_park): here the last kernel writes them into the two segments directly.

// marching_cubes_sparse_voxel_grid. Two waits: the flag word and the number of triangles, the number of vertices. out_counts: (#v, #f).
template <typename T>
static int marching_cubes_impl(pcu_hip_ctx* c, const T* scalars, const T* coords, int64_t n, const void* cubes, int64_t m, int kind, double isovalue,
                               int64_t* out_counts, unsigned flags, void* stream, pcu_hip_stats* st) {
    if (!c || !out_counts) return fail(PCU_HIP_ERR_INVALID, "null context / out_counts");
    out_counts[0] = out_counts[1] = 0;
    c->parked = ParkedResult();
    if (n <= 0) return fail(PCU_HIP_ERR_INVALID, "Invalid grid_coordinates has zero rows!");
    if (m <= 0) return fail(PCU_HIP_ERR_INVALID, "Invalid cube_indices has zero rows!");
    if (int rc = int_kind_check(kind)) return rc;
    if (!scalars || !coords || !cubes) return fail(PCU_HIP_ERR_INVALID, "null grid_scalars / grid_coordinates / cube_indices");
    if (!std::isfinite(isovalue)) return fail(PCU_HIP_ERR_INVALID, "isovalue must be finite");
    if (n > kVxMaxRows) return fail(PCU_HIP_ERR_INVALID, "marching_cubes_sparse_voxel_grid: more than 2^31-16 grid vertices are not supported");
    if (m > kVxMaxRows / 8) return fail(PCU_HIP_ERR_INVALID, "marching_cubes_sparse_voxel_grid: more than (2^31-16)/8 cubes are not supported");
    const size_t N = (size_t)n, M = (size_t)m, ib = (size_t)int_kind_bytes(kind);
    // (the sort of the 3 F corner keys is not in here: F is known after the first wait, and what the arena lacks is allocated on top of it)
    const size_t bytes = ((flags & PCU_HIP_PTRS_ON_DEVICE) ? 0 : 2 * align_up(N * 3 * sizeof(T), 256) + align_up(M * 8 * ib, 256)) + align_up(M * 32, 256) + align_up(M, 256) +
                         3 * align_up(M * 8, 256) + scan_bytes(M) + (1 << 20);
    return op_run(c, flags, stream, st, bytes, [&](OpFrame& fr) -> int {
        auto& [c, s, on_dev, ar, tm] = fr;      // marks 0-1: checks, classify and scan, 2-3: keys, 3-4: sort, 4-5: unique, 5-6: vertices and faces
        const T iso = (T)isovalue;
        const T *S = nullptr, *P = nullptr; const char* d_cubes = nullptr;
        tm.mark(0);
        if (stage_any(ar, scalars, N, on_dev, s, &S) || stage_any(ar, coords, N * 3, on_dev, s, &P) ||
            stage_ints(ar, cubes, M * 8, kind, on_dev, s, &d_cubes)) return -1;
        int *cidx = nullptr, *d_bad = nullptr; unsigned char* mask = nullptr; unsigned long long *cnt = nullptr, *C = nullptr;
        if (aalloc(ar, &cidx, M * 8) || aalloc(ar, &mask, M) || aalloc(ar, &cnt, M) || aalloc(ar, &C, M) || flag_word(ar, s, &d_bad)) return -1;
        hipLaunchKernelGGL(k_mesh_vcheck<T>, dim3(blocks_for(N * 3)), dim3(kBlock), 0, s, P, (long long)N * 3, d_bad, kMeshBadVertex);
        hipLaunchKernelGGL(k_mesh_vcheck<T>, dim3(blocks_for((size_t)N)), dim3(kBlock), 0, s, S, (long long)N, d_bad, kMeshBadVertex);
        hipLaunchKernelGGL(k_mc_classify<T>, dim3(blocks_for(M * 8)), dim3(kBlock), 0, s, (const void*)d_cubes, kind, (long long)m, S, (int)n, iso,
                           cidx, mask, cnt, d_bad);
        if (own_inclusive_scan(ar, s, (const unsigned long long*)cnt, C, M)) return -1;
        tm.mark(1);
        int bad = 0; unsigned long long F = 0;
        if (read_flag_and_last(s, d_bad, C, M, &bad, &F)) return -1;
        HIP_WAIT(s);
        if (bad & kMeshBadVertex) return fail(PCU_HIP_ERR_INVALID, "grid_coordinates and grid_scalars must not contain NaN or infinite values");
        if (bad & kMeshBadFace)
            return fail(PCU_HIP_ERR_INVALID, "cube_indices must hold row indices of grid_coordinates: found an index outside [0, %lld)", (long long)n);
        if (F == 0) return fail(PCU_HIP_ERR_INVALID, "No level set found for isovalue %f", isovalue);
        if (3 * F > (unsigned long long)kVxMaxRows)
            return fail(PCU_HIP_ERR_INVALID, "marching_cubes_sparse_voxel_grid: more than (2^31-16)/3 triangles are not supported");
        // keys, sort, unique
        const int K = (int)(3 * F), hb = bits_of((unsigned long long)(n - 1)), nbk = blocks_for((size_t)K);
        SortedRuns r;
        if (aalloc(ar, &r.keys, (size_t)K)) return -1;
        tm.mark(2);
        hipLaunchKernelGGL(k_mc_emit, dim3(blocks_for((size_t)M)), dim3(kBlock), 0, s, (const int*)cidx, (const unsigned char*)mask,
                           (const unsigned long long*)C, (long long)m, hb, r.keys);
        HIP_TRY(hipGetLastError());
        tm.mark(3);
        if (sort_keys(ar, s, r, K, 2 * hb)) return -1;
        tm.mark(4);
        if (rank_runs(ar, s, r, K)) return -1;
        tm.mark(5);
        unsigned V = 0;
        HIP_TRY(hipMemcpyAsync(&V, r.scan + (K - 1), 4, hipMemcpyDeviceToHost, s));
        HIP_WAIT(s);
        // vertices and faces, straight into the parked segments
        char* seg[kParkSegs];
        if (park_reserve(c, {(size_t)V * 3 * sizeof(T), (size_t)K * ib}, seg)) return -1;
        hipLaunchKernelGGL(k_mc_write<T>, dim3(nbk), dim3(kBlock), 0, s, (const unsigned long long*)r.keys, (const unsigned*)r.ids, (const unsigned*)r.flag,
                           (const unsigned*)r.scan, K, hb, S, P, iso, reinterpret_cast<T*>(seg[0]), (void*)seg[1], kind);
        HIP_TRY(hipGetLastError());
        tm.mark(6);
        HIP_WAIT(s);
        park_commit(c, Parked::Surface, (int64_t)V, (int64_t)F);
        out_counts[0] = (int64_t)V; out_counts[1] = (int64_t)F;
        if (st) {
            st->n_queries = m; st->n_escalated = (int64_t)F; st->n_passes = 1;
            st->ms_index = tm.span(0, 1); st->ms_search = tm.span(2, 3); st->ms_tie = tm.span(3, 4); st->ms_kernel_search = tm.span(4, 6); st->ms_total = tm.span(0, 6);
        }
        return 0;
    });
}
// The result of this context's last pcu_hip_marching_cubes_*: out_v (nv, 3) of its scalar type, out_f (nf, 3) of its index type. Once.
static int marching_cubes_take_impl(pcu_hip_ctx* c, int64_t nv, int64_t nf, void* out_v, void* out_f, unsigned flags, void* stream) {
    if (!c || !out_v || !out_f) return fail(PCU_HIP_ERR_INVALID, "null context / out_v / out_f");
    return park_take(c, Parked::Surface, nv, nf, {out_v, out_f}, flags, stream,
                     "pcu_hip_marching_cubes_take: this context holds no surface of %lld vertices and %lld faces");
}

// sparse_voxel_grid_to_hex_mesh. One wait before the results can be sized: the flag and the number of unique vertices.
static int hex_mesh_impl(pcu_hip_ctx* c, const void* ijk, int64_t k, int kind, const double* size, const double* origin, int out_f64, int64_t* out_nv, unsigned flags,
                         void* stream, pcu_hip_stats* st) {
    if (!c || !out_nv) return fail(PCU_HIP_ERR_INVALID, "null context / out_nv");
    *out_nv = 0;
    c->parked = ParkedResult();
    if (k <= 0) return fail(PCU_HIP_ERR_INVALID, "Invalid grid_coordinates has zero rows!");
    if (int rc = int_kind_check(kind)) return rc;
    if (!ijk) return fail(PCU_HIP_ERR_INVALID, "null grid_coordinates");
    VxGrid g;
    if (int rc = vx_grid_check(size, origin, "Invalid voxel size", &g)) return rc;
    if (k > kVxMaxRows / 8) return fail(PCU_HIP_ERR_INVALID, "sparse_voxel_grid_to_hex_mesh: more than (2^31-16)/8 voxels are not supported");
    const size_t K = (size_t)k * 8;
    const size_t bytes = sort_bytes(K) + scan_bytes(K) + 2 * align_up(K * 4, 256) +
                         ((flags & PCU_HIP_PTRS_ON_DEVICE) ? 0 : align_up((size_t)k * 3 * int_kind_bytes(kind), 256)) + (1 << 20);
    return op_run(c, flags, stream, st, bytes, [&](OpFrame& fr) -> int {
        auto& [c, s, on_dev, ar, tm] = fr;      // marks 0-1: codes, 1-2: sort, 2-3: unique, 3-4: vertices and cubes
        const char* d_in = nullptr;
        tm.mark(0);
        if (stage_faces(ar, ijk, (size_t)k, kind, on_dev, s, &d_in)) return -1;
        SortedRuns r; int* d_bad = nullptr;
        if (aalloc(ar, &r.keys, K) || flag_word(ar, s, &d_bad)) return -1;
        const int KK = (int)K, nb = blocks_for((size_t)KK);
        hipLaunchKernelGGL(k_hx_codes, dim3(nb), dim3(kBlock), 0, s, (const void*)d_in, kind, (long long)K, r.keys, d_bad);
        tm.mark(1);
        if (sort_keys(ar, s, r, KK, 63)) return -1;
        tm.mark(2);
        if (rank_runs(ar, s, r, KK)) return -1;
        tm.mark(3);
        int bad = 0; unsigned V = 0;
        if (read_flag_and_last(s, d_bad, r.scan, K, &bad, &V)) return -1;
        HIP_WAIT(s);
        if (bad) return fail(PCU_HIP_ERR_INVALID, "Invalid vertex leads to an overflow integer. Perhaps grid_size is too small.");
        char* seg[kParkSegs];
        if (park_reserve(c, {(size_t)V * 3 * (out_f64 ? 8 : 4), K * 8}, seg)) return -1;
        if (out_f64) hipLaunchKernelGGL(k_hx_write<double>, dim3(nb), dim3(kBlock), 0, s, (const unsigned long long*)r.keys, (const unsigned*)r.ids, (const unsigned*)r.flag,
                                        (const unsigned*)r.scan, KK, g, reinterpret_cast<double*>(seg[0]), reinterpret_cast<long long*>(seg[1]));
        else hipLaunchKernelGGL(k_hx_write<float>, dim3(nb), dim3(kBlock), 0, s, (const unsigned long long*)r.keys, (const unsigned*)r.ids, (const unsigned*)r.flag,
                                (const unsigned*)r.scan, KK, g, reinterpret_cast<float*>(seg[0]), reinterpret_cast<long long*>(seg[1]));
        HIP_TRY(hipGetLastError());
        tm.mark(4);
        HIP_WAIT(s);
        park_commit(c, Parked::HexMesh, (int64_t)V, k);
        *out_nv = (int64_t)V;
        if (st) {
            st->n_queries = k; st->n_escalated = (int64_t)V; st->n_passes = 1;
            st->ms_index = tm.span(0, 1); st->ms_search = tm.span(1, 2); st->ms_tie = tm.span(2, 3); st->ms_kernel_search = tm.span(3, 4); st->ms_total = tm.span(0, 4);
        }
        return 0;
    });
}
// The result of this context's last pcu_hip_sparse_voxel_grid_to_hex_mesh: out_v (nv, 3) float or double, out_cubes (k, 8) int64. Once.
static int hex_mesh_take_impl(pcu_hip_ctx* c, int64_t nv, int64_t k, void* out_v, int64_t* out_cubes, unsigned flags, void* stream) {
    if (!c || !out_v || !out_cubes) return fail(PCU_HIP_ERR_INVALID, "null context / out_v / out_cubes");
    return park_take(c, Parked::HexMesh, nv, k, {out_v, out_cubes}, flags, stream,
                     "pcu_hip_sparse_voxel_grid_to_hex_mesh_take: this context holds no hex mesh of %lld vertices and %lld cubes");
}
