// csrc/marching_cubes_host.h -- host orchestration of marching_cubes_sparse_voxel_grid and sparse_voxel_grid_to_hex_mesh (kernels and contract:
// marching_cubes.h). Included by pcu_hip.hip after voxelize_host.h (vx_grid_check, vx_kind_bytes, kVxMaxRows) and voxel_host.h (sort, scan).
#pragma once

// Both operators learn the size of their results late, so the results wait in the context's `aux` block for the matching _take call, as a
// voxelization's rows do (vx_park): here the last kernel writes them there directly.
static void mc_unpark(pcu_hip_ctx* c) { c->mc_nv = c->mc_nf = -1; c->hx_nv = c->hx_k = -1; }

// marching_cubes_sparse_voxel_grid. Two waits: the flag word and the number of triangles, the number of vertices. out_counts: (#v, #f).
template <typename T>
static int marching_cubes_impl(pcu_hip_ctx* c, const T* scalars, const T* coords, int64_t n, const void* cubes, int64_t m, int kind, double isovalue,
                               int64_t* out_counts, unsigned flags, void* stream, pcu_hip_stats* st) {
    if (!c || !out_counts) return fail(PCU_HIP_ERR_INVALID, "null context / out_counts");
    out_counts[0] = out_counts[1] = 0;
    mc_unpark(c);
    if (n <= 0) return fail(PCU_HIP_ERR_INVALID, "Invalid grid_coordinates has zero rows!");
    if (m <= 0) return fail(PCU_HIP_ERR_INVALID, "Invalid cube_indices has zero rows!");
    if (kind < 0 || kind > 3) return fail(PCU_HIP_ERR_INVALID, "kind must be one of PCU_HIP_FACE_INT32 / INT64 / UINT32 / UINT64");
    if (!scalars || !coords || !cubes) return fail(PCU_HIP_ERR_INVALID, "null grid_scalars / grid_coordinates / cube_indices");
    if (!std::isfinite(isovalue)) return fail(PCU_HIP_ERR_INVALID, "isovalue must be finite");
    if (n > kVxMaxRows) return fail(PCU_HIP_ERR_INVALID, "marching_cubes_sparse_voxel_grid: more than 2^31-16 grid vertices are not supported");
    if (m > kVxMaxRows / 8) return fail(PCU_HIP_ERR_INVALID, "marching_cubes_sparse_voxel_grid: more than (2^31-16)/8 cubes are not supported");
    const bool on_dev = flags & PCU_HIP_PTRS_ON_DEVICE;
    hipStream_t s = pick_stream(c, flags, stream);
    const size_t N = (size_t)n, M = (size_t)m, ib = (size_t)vx_kind_bytes(kind);
    if (int rc = ms_begin(c, st, (on_dev ? 0 : 2 * align_up(N * 3 * sizeof(T), 256) + align_up(M * 8 * ib, 256)) + align_up(M * 32, 256) + align_up(M, 256) +
                                     3 * align_up(M * 8, 256) + (1 << 20))) return rc;
    c->time_phases = flags & PCU_HIP_TIME_PHASES;
    Arena ar{c};
    Timer tm{c, s, st};             // marks 0-1: checks, classify and scan, 2-3: keys, 3-4: sort, 4-5: unique, 5-6: vertices and faces
    auto run = [&]() -> int {
        const T iso = (T)isovalue;
        const T *S = nullptr, *P = nullptr; const char* d_cubes = nullptr;
        tm.mark(0);
        if (stage_any(ar, scalars, N, on_dev, s, &S) || stage_any(ar, coords, N * 3, on_dev, s, &P) ||
            stage_any(ar, static_cast<const char*>(cubes), M * 8 * ib, on_dev, s, &d_cubes)) return -1;
        int *cidx = nullptr, *d_bad = nullptr; unsigned char* mask = nullptr; unsigned long long *cnt = nullptr, *C = nullptr;
        if (aalloc(ar, &cidx, M * 8) || aalloc(ar, &mask, M) || aalloc(ar, &cnt, M) || aalloc(ar, &C, M) || aalloc(ar, &d_bad, 1)) return -1;
        HIP_TRY(hipMemsetAsync(d_bad, 0, sizeof(int), s));
        hipLaunchKernelGGL(k_mesh_vcheck<T>, dim3((unsigned)((N * 3 + kBlock - 1) / kBlock)), dim3(kBlock), 0, s, P, (long long)N * 3, d_bad, kMeshBadVertex);
        hipLaunchKernelGGL(k_mesh_vcheck<T>, dim3((unsigned)((N + kBlock - 1) / kBlock)), dim3(kBlock), 0, s, S, (long long)N, d_bad, kMeshBadVertex);
        hipLaunchKernelGGL(k_mc_classify<T>, dim3((unsigned)((M * 8 + kBlock - 1) / kBlock)), dim3(kBlock), 0, s, (const void*)d_cubes, kind, (long long)m, S, (int)n, iso,
                           cidx, mask, cnt, d_bad);
        if (own_inclusive_scan(ar, s, (const unsigned long long*)cnt, C, M)) return -1;
        tm.mark(1);
        int bad = 0; unsigned long long F = 0;
        HIP_TRY(hipMemcpyAsync(&bad, d_bad, sizeof(int), hipMemcpyDeviceToHost, s));
        HIP_TRY(hipMemcpyAsync(&F, C + (M - 1), 8, hipMemcpyDeviceToHost, s));
        HIP_WAIT(s);
        if (bad & kMeshBadVertex) return fail(PCU_HIP_ERR_INVALID, "grid_coordinates and grid_scalars must not contain NaN or infinite values");
        if (bad & kMeshBadFace)
            return fail(PCU_HIP_ERR_INVALID, "cube_indices must hold row indices of grid_coordinates: found an index outside [0, %lld)", (long long)n);
        if (F == 0) return fail(PCU_HIP_ERR_INVALID, "No level set found for isovalue %f", isovalue);
        if (3 * F > (unsigned long long)kVxMaxRows)
            return fail(PCU_HIP_ERR_INVALID, "marching_cubes_sparse_voxel_grid: more than (2^31-16)/3 triangles are not supported");
        // keys, sort, unique
        const int K = (int)(3 * F), hb = bits_of((unsigned long long)(n - 1)), nbk = (K + kBlock - 1) / kBlock;
        unsigned long long *ka = nullptr, *kb = nullptr; unsigned *ia = nullptr, *ib2 = nullptr, *flag = nullptr, *scan = nullptr;
        if (aalloc(ar, &ka, (size_t)K) || aalloc(ar, &kb, (size_t)K) || aalloc(ar, &ia, (size_t)K) || aalloc(ar, &ib2, (size_t)K) || aalloc(ar, &flag, (size_t)K) ||
            aalloc(ar, &scan, (size_t)K)) return -1;
        tm.mark(2);
        hipLaunchKernelGGL(k_mc_emit, dim3((unsigned)((M + kBlock - 1) / kBlock)), dim3(kBlock), 0, s, (const int*)cidx, (const unsigned char*)mask,
                           (const unsigned long long*)C, (long long)m, hb, ka);
        HIP_TRY(hipGetLastError());
        tm.mark(3);
        if (own_radix_sort(ar, s, &ka, &kb, &ia, &ib2, /*ids_identity=*/true, K, 2 * hb)) return -1;
        tm.mark(4);
        hipLaunchKernelGGL(k_run_heads_sorted, dim3(nbk), dim3(kBlock), 0, s, (const unsigned long long*)ka, K, flag);
        if (own_inclusive_scan(ar, s, (const unsigned*)flag, scan, (size_t)K)) return -1;
        tm.mark(5);
        unsigned V = 0;
        HIP_TRY(hipMemcpyAsync(&V, scan + (K - 1), 4, hipMemcpyDeviceToHost, s));
        HIP_WAIT(s);
        // vertices and faces, straight into the parking block
        const size_t vbytes = align_up((size_t)V * 3 * sizeof(T), 256);
        if (aux_reserve(c, vbytes + (size_t)K * ib + 256)) return -1;
        hipLaunchKernelGGL(k_mc_write<T>, dim3(nbk), dim3(kBlock), 0, s, (const unsigned long long*)ka, (const unsigned*)ia, (const unsigned*)flag, (const unsigned*)scan, K, hb,
                           S, P, iso, reinterpret_cast<T*>(c->aux), (void*)(c->aux + vbytes), kind);
        HIP_TRY(hipGetLastError());
        tm.mark(6);
        HIP_WAIT(s);
        c->mc_nv = (int64_t)V; c->mc_nf = (int64_t)F; c->mc_vsize = (int)sizeof(T); c->mc_isize = (int)ib;
        out_counts[0] = (int64_t)V; out_counts[1] = (int64_t)F;
        if (st) {
            st->n_queries = m; st->n_escalated = (int64_t)F; st->n_passes = 1;
            st->ms_index = tm.span(0, 1); st->ms_search = tm.span(2, 3); st->ms_tie = tm.span(3, 4); st->ms_kernel_search = tm.span(4, 6); st->ms_total = tm.span(0, 6);
        }
        return 0;
    };
    return attempt_exit(c, run());
}
// The result of this context's last pcu_hip_marching_cubes_*: out_v (nv, 3) of its scalar type, out_f (nf, 3) of its index type. Once.
static int marching_cubes_take_impl(pcu_hip_ctx* c, int64_t nv, int64_t nf, void* out_v, void* out_f, unsigned flags, void* stream) {
    if (!c || !out_v || !out_f) return fail(PCU_HIP_ERR_INVALID, "null context / out_v / out_f");
    if (c->mc_nv < 0 || nv != c->mc_nv || nf != c->mc_nf)
        return fail(PCU_HIP_ERR_INVALID, "pcu_hip_marching_cubes_take: this context holds no surface of %lld vertices and %lld faces", (long long)nv, (long long)nf);
    hipStream_t s = pick_stream(c, flags, stream);
    const hipMemcpyKind dir = (flags & PCU_HIP_PTRS_ON_DEVICE) ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost;
    const size_t vb = (size_t)nv * 3 * (size_t)c->mc_vsize;
    HIP_TRY(hipMemcpyAsync(out_v, c->aux, vb, dir, s));
    HIP_TRY(hipMemcpyAsync(out_f, c->aux + align_up(vb, 256), (size_t)nf * 3 * (size_t)c->mc_isize, dir, s));
    HIP_WAIT(s);
    mc_unpark(c);
    return 0;
}

// sparse_voxel_grid_to_hex_mesh. One wait before the results can be sized: the flag and the number of unique vertices.
static int hex_mesh_impl(pcu_hip_ctx* c, const void* ijk, int64_t k, int kind, const double* size, const double* origin, int out_f64, int64_t* out_nv, unsigned flags,
                         void* stream, pcu_hip_stats* st) {
    if (!c || !out_nv) return fail(PCU_HIP_ERR_INVALID, "null context / out_nv");
    *out_nv = 0;
    mc_unpark(c);
    if (k <= 0) return fail(PCU_HIP_ERR_INVALID, "Invalid grid_coordinates has zero rows!");
    if (kind < 0 || kind > 3) return fail(PCU_HIP_ERR_INVALID, "kind must be one of PCU_HIP_FACE_INT32 / INT64 / UINT32 / UINT64");
    if (!ijk) return fail(PCU_HIP_ERR_INVALID, "null grid_coordinates");
    VxGrid g;
    if (int rc = vx_grid_check(size, origin, "Invalid voxel size", &g)) return rc;
    if (k > kVxMaxRows / 8) return fail(PCU_HIP_ERR_INVALID, "sparse_voxel_grid_to_hex_mesh: more than (2^31-16)/8 voxels are not supported");
    const bool on_dev = flags & PCU_HIP_PTRS_ON_DEVICE;
    hipStream_t s = pick_stream(c, flags, stream);
    const size_t K = (size_t)k * 8;
    if (int rc = ms_begin(c, st, 2 * align_up(K * 8, 256) + 4 * align_up(K * 4, 256) + align_up(256 * ((K + kRsWaveTile - 1) / kRsWaveTile) * 4, 256) +
                                     (on_dev ? 0 : align_up((size_t)k * 3 * vx_kind_bytes(kind), 256)) + (1 << 20))) return rc;
    c->time_phases = flags & PCU_HIP_TIME_PHASES;
    Arena ar{c};
    Timer tm{c, s, st};             // marks 0-1: codes, 1-2: sort, 2-3: unique, 3-4: vertices and cubes
    auto run = [&]() -> int {
        const char* d_in = nullptr;
        tm.mark(0);
        if (stage_any(ar, static_cast<const char*>(ijk), (size_t)k * 3 * vx_kind_bytes(kind), on_dev, s, &d_in)) return -1;
        unsigned long long *ka = nullptr, *kb = nullptr; unsigned *ia = nullptr, *ib = nullptr, *flag = nullptr, *scan = nullptr; int* d_bad = nullptr;
        if (aalloc(ar, &ka, K) || aalloc(ar, &kb, K) || aalloc(ar, &ia, K) || aalloc(ar, &ib, K) || aalloc(ar, &flag, K) || aalloc(ar, &scan, K) || aalloc(ar, &d_bad, 1)) return -1;
        const int KK = (int)K, nb = (KK + kBlock - 1) / kBlock;
        HIP_TRY(hipMemsetAsync(d_bad, 0, sizeof(int), s));
        hipLaunchKernelGGL(k_hx_codes, dim3(nb), dim3(kBlock), 0, s, (const void*)d_in, kind, (long long)K, ka, d_bad);
        tm.mark(1);
        if (own_radix_sort(ar, s, &ka, &kb, &ia, &ib, /*ids_identity=*/true, KK, 63)) return -1;
        tm.mark(2);
        hipLaunchKernelGGL(k_run_heads_sorted, dim3(nb), dim3(kBlock), 0, s, (const unsigned long long*)ka, KK, flag);
        if (own_inclusive_scan(ar, s, (const unsigned*)flag, scan, K)) return -1;
        tm.mark(3);
        int bad = 0; unsigned V = 0;
        HIP_TRY(hipMemcpyAsync(&bad, d_bad, sizeof(int), hipMemcpyDeviceToHost, s));
        HIP_TRY(hipMemcpyAsync(&V, scan + (K - 1), 4, hipMemcpyDeviceToHost, s));
        HIP_WAIT(s);
        if (bad) return fail(PCU_HIP_ERR_INVALID, "Invalid vertex leads to an overflow integer. Perhaps grid_size is too small.");
        const size_t osz = out_f64 ? 8 : 4, vbytes = align_up((size_t)V * 3 * osz, 256);
        if (aux_reserve(c, vbytes + K * 8 + 256)) return -1;
        long long* d_c = reinterpret_cast<long long*>(c->aux + vbytes);
        if (out_f64) hipLaunchKernelGGL(k_hx_write<double>, dim3(nb), dim3(kBlock), 0, s, (const unsigned long long*)ka, (const unsigned*)ia, (const unsigned*)flag,
                                        (const unsigned*)scan, KK, g, reinterpret_cast<double*>(c->aux), d_c);
        else hipLaunchKernelGGL(k_hx_write<float>, dim3(nb), dim3(kBlock), 0, s, (const unsigned long long*)ka, (const unsigned*)ia, (const unsigned*)flag,
                                (const unsigned*)scan, KK, g, reinterpret_cast<float*>(c->aux), d_c);
        HIP_TRY(hipGetLastError());
        tm.mark(4);
        HIP_WAIT(s);
        c->hx_nv = (int64_t)V; c->hx_k = k; c->hx_vsize = (int)osz;
        *out_nv = (int64_t)V;
        if (st) {
            st->n_queries = k; st->n_escalated = (int64_t)V; st->n_passes = 1;
            st->ms_index = tm.span(0, 1); st->ms_search = tm.span(1, 2); st->ms_tie = tm.span(2, 3); st->ms_kernel_search = tm.span(3, 4); st->ms_total = tm.span(0, 4);
        }
        return 0;
    };
    return attempt_exit(c, run());
}
// The result of this context's last pcu_hip_sparse_voxel_grid_to_hex_mesh: out_v (nv, 3) float or double, out_cubes (k, 8) int64. Once.
static int hex_mesh_take_impl(pcu_hip_ctx* c, int64_t nv, int64_t k, void* out_v, int64_t* out_cubes, unsigned flags, void* stream) {
    if (!c || !out_v || !out_cubes) return fail(PCU_HIP_ERR_INVALID, "null context / out_v / out_cubes");
    if (c->hx_nv < 0 || nv != c->hx_nv || k != c->hx_k)
        return fail(PCU_HIP_ERR_INVALID, "pcu_hip_sparse_voxel_grid_to_hex_mesh_take: this context holds no hex mesh of %lld vertices and %lld cubes", (long long)nv, (long long)k);
    hipStream_t s = pick_stream(c, flags, stream);
    const hipMemcpyKind dir = (flags & PCU_HIP_PTRS_ON_DEVICE) ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost;
    const size_t vb = (size_t)nv * 3 * (size_t)c->hx_vsize;
    HIP_TRY(hipMemcpyAsync(out_v, c->aux, vb, dir, s));
    HIP_TRY(hipMemcpyAsync(out_cubes, c->aux + align_up(vb, 256), (size_t)k * 64, dir, s));
    HIP_WAIT(s);
    mc_unpark(c);
    return 0;
}
