// csrc/mesh_sample_host.h -- host orchestration of mesh_face_areas, sample_mesh_random and sample_mesh_poisson_disk (kernels and contract:
// mesh_sample.h; the greedy: poisson_host.h). Included by pcu_hip.hip after the operator frame, voxel_host.h (the scan), poisson_host.h and
// mesh_host.h (mesh_validate, MeshGiven).
#pragma once

// The mesh side of one call on the device: staged vertices, range-checked faces, areas, the scan of the weights.
template <typename T>
struct MsMesh {
    const T* v = nullptr; int* fidx = nullptr; T* area = nullptr; unsigned long long* C = nullptr;
    MeshHead<T>* head = nullptr; MsHead<T>* mh = nullptr;
    int nf = 0;
};
template <typename T>
static size_t ms_mesh_bytes(const MeshGiven<T>& m, bool on_dev) {
    const size_t NF = (size_t)m.nf;
    size_t b = align_up(NF * 12, 256) + align_up(NF * sizeof(T), 256) + 2 * align_up(NF * 8, 256) + align_up((NF / kScTile + 2) * 8, 256) + 8192;
    if (!on_dev) b += align_up((size_t)m.nv * 3 * sizeof(T), 256) + align_up(NF * 3 * int_kind_bytes(m.f_kind), 256);
    return b;
}
// Enqueues staging and the checks of v and f (the range-checked faces, the flag word). No wait.
template <typename T>
static int ms_mesh_stage(Arena& ar, hipStream_t s, const MeshGiven<T>& m, bool on_dev, MsMesh<T>& M) {
    const char* df = nullptr;
    if (stage_in(ar, m.v, m.nv, on_dev, s, &M.v) || stage_faces(ar, m.f, (size_t)m.nf, m.f_kind, on_dev, s, &df)) return -1;
    M.nf = (int)m.nf;
    if (aalloc(ar, &M.head, 1) || aalloc(ar, &M.fidx, (size_t)m.nf * 3)) return -1;
    hipLaunchKernelGGL(k_mesh_head_init<T>, dim3(1), dim3(64), 0, s, M.head);
    hipLaunchKernelGGL(k_mesh_vcheck<T>, dim3(blocks_for((size_t)m.nv * 3)), dim3(kBlock), 0, s, M.v, (long long)m.nv * 3, mesh_head_flag(M.head), kMeshBadVertex);
    hipLaunchKernelGGL(k_mesh_faces<T>, dim3(blocks_for((size_t)m.nf)), dim3(kBlock), 0, s, (const void*)df, m.f_kind, (int)m.nf, (int)m.nv, M.v,
                       M.fidx, M.head);
    HIP_TRY(hipGetLastError());
    return 0;
}
// ms_mesh_stage, then the areas and, with `weights`, the weights and their scan. The areas go into d_area if given: the caller's own memory,
// which k_mesh_areas leaves as it is when the checks of ms_mesh_stage have raised the flag word. No wait.
template <typename T>
static int ms_mesh_enqueue(Arena& ar, hipStream_t s, const MeshGiven<T>& m, bool on_dev, bool weights, T* d_area, MsMesh<T>& M) {
    if (ms_mesh_stage(ar, s, m, on_dev, M)) return -1;
    M.area = d_area;
    if (aalloc(ar, &M.mh, 1) || (!M.area && aalloc(ar, &M.area, (size_t)m.nf))) return -1;
    const unsigned nbf = blocks_for((size_t)m.nf);
    HIP_TRY(hipMemsetAsync(M.mh, 0, sizeof(MsHead<T>), s));
    hipLaunchKernelGGL(k_mesh_areas<T>, dim3(nbf), dim3(kBlock), 0, s, M.v, (const int*)M.fidx, (int)m.nf, M.area, M.mh,
                       (const int*)(d_area ? mesh_head_flag(M.head) : nullptr));
    if (weights) {
        unsigned long long* w = nullptr;
        if (aalloc(ar, &w, (size_t)m.nf) || aalloc(ar, &M.C, (size_t)m.nf)) return -1;
        hipLaunchKernelGGL(k_mesh_weights<T>, dim3(nbf), dim3(kBlock), 0, s, (const T*)M.area, (int)m.nf, (const MsHead<T>*)M.mh, w);
        if (own_inclusive_scan(ar, s, (const unsigned long long*)w, M.C, (size_t)m.nf)) return -1;
    }
    HIP_TRY(hipGetLastError());
    return 0;
}
// What the host reads back in its one wait: the flag word, the largest area and the sum of the weights.
template <typename T>
struct MsSeen {
    int bad = 0; T amax = 0; unsigned long long W = 0;
};
template <typename T>
static int ms_mesh_readback(hipStream_t s, const MsMesh<T>& M, bool weights, MsSeen<T>* h) {
    if (flag_fetch(s, mesh_head_flag(M.head), &h->bad)) return -1;
    if (weights) {
        HIP_TRY(hipMemcpyAsync(&h->amax, M.mh, sizeof(T), hipMemcpyDeviceToHost, s));       // (the bit pattern of a non-negative T, or of a NaN)
        HIP_TRY(hipMemcpyAsync(&h->W, M.C + (M.nf - 1), 8, hipMemcpyDeviceToHost, s));
    }
    return 0;
}
template <typename T>
static int ms_mesh_refuse(const MsSeen<T>& h, int64_t nv, bool weights) {
    if (h.bad) return mesh_refusal(h.bad, nv);
    if (!weights) return 0;
    if (!std::isfinite(h.amax)) return fail(PCU_HIP_ERR_INVALID, "face areas overflow the scalar type of v");
    if (h.amax == (T)0) return fail(PCU_HIP_ERR_INVALID, "Mesh has zero area");
    return 0;
}

// mesh_face_areas (src/face_areas.cpp:17-79)
template <typename T>
static int mesh_face_areas_impl(pcu_hip_ctx* c, const MeshGiven<T>& m, T* out_area, unsigned flags, void* stream, pcu_hip_stats* st) {
    if (!c) return fail(PCU_HIP_ERR_INVALID, "null context");
    if (int rc = mesh_validate(m.nv, m.nf, 0, m.f_kind)) return rc;
    const bool on_dev = flags & PCU_HIP_PTRS_ON_DEVICE;
    return op_run(c, flags, stream, st, ms_mesh_bytes(m, on_dev), [&](OpFrame& fr) -> int {
        auto& [c, s, on_dev, ar, tm] = fr;
        MsMesh<T> M; MsSeen<T> seen;
        if (ms_mesh_enqueue<T>(ar, s, m, on_dev, false, on_dev ? out_area : nullptr, M) || ms_mesh_readback(s, M, false, &seen) ||
            out_give(s, on_dev, out_area, (const T*)M.area, (size_t)m.nf)) return -1;
        HIP_WAIT(s);
        if (int rc = ms_mesh_refuse(seen, m.nv, false)) return rc;
        if (st) { st->n_queries = m.nf; st->n_passes = 1; }
        return 0;
    });
}

// sample_mesh_random (src/sample_mesh.cpp:91-115)
template <typename T>
static void ms_sample_launch(hipStream_t s, const MsMesh<T>& M, unsigned seed, int64_t n, long long* d_fi, T* d_bc) {
    const int64_t per = (int64_t)kBlock * kMsPerLane;
    hipLaunchKernelGGL(k_mesh_sample<T>, dim3((unsigned)((n + per - 1) / per)), dim3(kBlock), 0, s, (const unsigned long long*)M.C, M.nf, seed, (long long)n, d_fi, d_bc);
}
template <typename T>
static int sample_mesh_random_impl(pcu_hip_ctx* c, const MeshGiven<T>& m, int64_t n, unsigned seed, int64_t* out_fi, T* out_bc, unsigned flags,
                                   void* stream, pcu_hip_stats* st) {
    if (!c) return fail(PCU_HIP_ERR_INVALID, "null context");
    if (int rc = mesh_validate(m.nv, m.nf, 0, m.f_kind)) return rc;
    if (n <= 0) return fail(PCU_HIP_ERR_INVALID, "num_samples must be positive");
    if (n > kMeshMaxRows) return mesh_row_limit();
    const bool on_dev = flags & PCU_HIP_PTRS_ON_DEVICE;
    const size_t out_bytes = on_dev ? 0 : align_up((size_t)n * 8, 256) + align_up((size_t)n * 3 * sizeof(T), 256);
    return op_run(c, flags, stream, st, ms_mesh_bytes(m, on_dev) + out_bytes, [&](OpFrame& fr) -> int {
        auto& [c, s, on_dev, ar, tm] = fr;
        MsMesh<T> M; MsSeen<T> seen;
        if (ms_mesh_enqueue<T>(ar, s, m, on_dev, true, nullptr, M)) return -1;
        long long *const h_fi = reinterpret_cast<long long*>(out_fi), *d_fi = nullptr; T* d_bc = nullptr;
        if (out_room(ar, on_dev, h_fi, (size_t)n, &d_fi) || out_room(ar, on_dev, out_bc, (size_t)n * 3, &d_bc)) return -1;
        ms_sample_launch(s, M, seed, n, d_fi, d_bc);              // (writes nothing for a mesh that is refused below: W = 0)
        HIP_TRY(hipGetLastError());
        if (ms_mesh_readback(s, M, true, &seen) || out_give(s, on_dev, h_fi, (const long long*)d_fi, (size_t)n) ||
            out_give(s, on_dev, out_bc, (const T*)d_bc, (size_t)n * 3)) return -1;
        HIP_WAIT(s);
        if (int rc = ms_mesh_refuse(seen, m.nv, true)) return rc;
        if (st) { st->n_queries = n; st->n_passes = 1; }
        return 0;
    });
}

// sample_mesh_poisson_disk (src/sample_mesh.cpp:34-75): N_c candidates of sample_mesh_random, their positions, the greedy of poisson.h over
// them (at `radius` if it is positive, else searching the radius for num_samples), the kept candidates' rows. out_fi == nullptr: only
// *out_count = N_c is computed. Otherwise out_fi / out_bc have room for `capacity` rows and *out_count rows are written.
static double ms_candidates(double oversampling, int64_t num_samples, double radius, double W, double amax) {
    const double total_area = (W * 0x1p-36) * amax;
    const double n_est = radius > 0.0 ? std::ceil(total_area / (0.7 * M_PI * radius * radius)) : 0.0;
    return std::ceil(oversampling * std::max(std::max((double)num_samples, n_est), 1.0));
}
template <typename T>
static int sample_mesh_poisson_impl(pcu_hip_ctx* c, const MeshGiven<T>& m, int64_t num_samples, double radius, unsigned seed, double tolerance,
                                    double oversampling, int64_t capacity, int64_t* out_fi, T* out_bc, int64_t* out_count, unsigned flags,
                                    void* stream, pcu_hip_stats* st) {
    if (!c || !out_count) return fail(PCU_HIP_ERR_INVALID, "null context / out_count");
    *out_count = 0;
    if (int rc = mesh_validate(m.nv, m.nf, 0, m.f_kind)) return rc;
    if (num_samples <= 0 && radius <= 0.0) return fail(PCU_HIP_ERR_INVALID, "Cannot have both num_samples <= 0 and radius <= 0");
    const float tol = (float)tolerance, of = (float)oversampling;
    if (!(tol > 0.0f && tol <= 1.0f)) return fail(PCU_HIP_ERR_INVALID, "sample_num_tolerance must be in (0, 1]");
    if (!(of >= 1.0f)) return fail(PCU_HIP_ERR_INVALID, "oversampling_factor must be >= 1.0");
    if (num_samples <= 0 && std::isnan(radius)) return fail(PCU_HIP_ERR_INVALID, "radius must not be NaN");
    if (num_samples > kMeshMaxRows) return mesh_row_limit();
    const bool by_radius = radius > 0.0;
    const int64_t target = by_radius ? 0 : num_samples;
    const bool on_dev = flags & PCU_HIP_PTRS_ON_DEVICE;
    // the arena for the candidate count known here (without the radius' estimate: the caller's capacity stands in for it)
    const double guess = ms_candidates((double)of, num_samples, 0.0, 0.0, 0.0);
    const int64_t ng = std::max<int64_t>(guess <= (double)kMeshMaxRows ? (int64_t)guess : 0, std::min<int64_t>(std::max<int64_t>(capacity, 0), kMeshMaxRows));
    size_t bytes = ms_mesh_bytes(m, on_dev);
    if (out_fi) bytes += (on_dev ? 1 : 2) * (align_up((size_t)ng * 8, 256) + align_up((size_t)ng * 3 * sizeof(T), 256)) + align_up((size_t)ng * 3 * sizeof(T), 256) +
                         align_up((size_t)ng * 4, 256) + pd_body_bytes<T>(ng, target);
    return op_run(c, flags, stream, st, bytes, [&](OpFrame& fr) -> int {
        auto& [c, s, on_dev, ar, tm] = fr;
        MsMesh<T> M; MsSeen<T> seen;
        if (ms_mesh_enqueue<T>(ar, s, m, on_dev, true, nullptr, M) || ms_mesh_readback(s, M, true, &seen)) return -1;
        HIP_WAIT(s);
        if (int rc = ms_mesh_refuse(seen, m.nv, true)) return rc;
        const double ncd = ms_candidates((double)of, num_samples, radius, (double)seen.W, (double)seen.amax);
        if (!(ncd <= (double)kMeshMaxRows))
            return fail(PCU_HIP_ERR_INVALID, "sample_mesh_poisson_disk needs %g candidates: more than 2^27-16 rows are not supported", ncd);
        const int64_t nc = (int64_t)ncd;
        if (!out_fi) { *out_count = nc; return 0; }
        long long *c_fi = nullptr; T *c_bc = nullptr, *P = nullptr; int32_t* idx = nullptr;
        if (aalloc(ar, &c_fi, (size_t)nc) || aalloc(ar, &c_bc, (size_t)nc * 3) || aalloc(ar, &P, (size_t)nc * 3) || aalloc(ar, &idx, (size_t)nc)) return -1;
        ms_sample_launch(s, M, seed, nc, c_fi, c_bc);
        hipLaunchKernelGGL(k_mesh_positions<T>, dim3(blocks_for((size_t)nc)), dim3(kBlock), 0, s, M.v, (const int*)M.fidx, (const long long*)c_fi,
                           (const T*)c_bc, (int)nc, P);
        HIP_TRY(hipGetLastError());
        PdRun<T> R;
        int64_t cnt = 0;
        if (int rc = pd_body<T>(ar, s, P, nc, radius, target, seed, tol, idx, &cnt, R)) return rc;
        if (cnt > capacity) return fail(PCU_HIP_ERR_INVALID, "sample_mesh_poisson_disk keeps %lld rows: the output arrays hold %lld", (long long)cnt, (long long)capacity);
        long long *const h_fi = reinterpret_cast<long long*>(out_fi), *d_fi = nullptr; T* d_bc = nullptr;
        if (out_room(ar, on_dev, h_fi, (size_t)cnt, &d_fi) || out_room(ar, on_dev, out_bc, (size_t)cnt * 3, &d_bc)) return -1;
        if (cnt > 0) {
            hipLaunchKernelGGL(k_mesh_keep<T>, dim3(blocks_for((size_t)cnt)), dim3(kBlock), 0, s, (const int32_t*)idx, (int)cnt, (const long long*)c_fi,
                               (const T*)c_bc, d_fi, d_bc);
            HIP_TRY(hipGetLastError());
            if (out_give(s, on_dev, h_fi, (const long long*)d_fi, (size_t)cnt) || out_give(s, on_dev, out_bc, (const T*)d_bc, (size_t)cnt * 3)) return -1;
        }
        HIP_WAIT(s);
        *out_count = cnt;
        if (st) { st->n_queries = nc; st->n_passes = R.rounds; st->n_grid_builds = R.radii; }
        return 0;
    });
}
