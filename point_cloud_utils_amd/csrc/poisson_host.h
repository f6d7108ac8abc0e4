// csrc/poisson_host.h -- host orchestration of Poisson-disk downsampling (kernels and contract: poisson.h). Included by pcu_hip.hip after
// the grid index (index_host.h), the operator frame (op_run) and voxel_host.h (the scan).
#pragma once

// The working set of one call: a grid index over the cloud (rebuilt for every radius) and the per-record / per-cell state of the rounds.
template <typename T>
struct PdRun {
    GridIndex<T> gi;
    const T* pts = nullptr;
    PdArgs<T> a{};
    unsigned seed = 0;
    int rounds = 0, radii = 0;
};
constexpr double kPdOccupancy = 4.0;       // points per cell when r is below the cloud's spacing (cells are never narrower than r)
constexpr int kPdPoll = 4;                 // rounds enqueued between two reads of the undecided counter

// Grid over the cloud with cells at least h_want wide; returns its parameters (for the bounding box and the non-finite flags).
template <typename T>
static int pd_build(PdRun<T>& R, double h_want, hipStream_t s, GridParams<T>* host_gp) {
    R.gi.h_want = h_want;
    if (index_build(R.gi, R.pts, kPdOccupancy, s)) return -1;
    if (host_gp) {
        HIP_TRY(hipMemcpyAsync(host_gp, R.gi.gp, sizeof(GridParams<T>), hipMemcpyDeviceToHost, s));
        HIP_WAIT(s);
    }
    return 0;
}
// One greedy run at radius r (in T): *count = samples. The states stay on the device for the compaction.
template <typename T>
static int pd_run(PdRun<T>& R, T r, hipStream_t s, int64_t* count) {
    // cells at least r wide (slightly more: the reach of a close pair includes rounding), capped where the grid arithmetic stays finite
    const double hcap = sizeof(T) == 4 ? 1e30 : 1e300;
    if (pd_build<T>(R, std::min((double)r * 1.01, hcap), s, nullptr)) return -1;
    const int n = R.gi.n, nb = blocks_for((size_t)n);
    PdArgs<T>& a = R.a;
    a.gp = R.gi.gp; a.sorted = R.gi.sorted; a.cell_start = R.gi.cell_start;
    a.r2 = r * r;
    a.reach = r * ((T)1 + (T)8 * Limits<T>::eps);
    HIP_TRY(hipMemsetAsync(a.cellmin, 0xff, (size_t)R.gi.max_cells * sizeof(unsigned long long), s));
    HIP_TRY(hipMemsetAsync(a.nsamp, 0, (size_t)R.gi.max_cells * sizeof(unsigned), s));
    HIP_TRY(hipMemsetAsync(a.counters, 0, 2 * sizeof(unsigned), s));
    hipLaunchKernelGGL(k_pd_init<T>, dim3(nb), dim3(kBlock), 0, s, a, R.seed);
    unsigned h[2] = {1u, 0u};
    const int first = R.rounds;
    while (h[0] != 0) {
        // (every round decides the lowest undecided point at least: more rounds than points would be a defect, not a slow input)
        if ((int64_t)(R.rounds - first) > (int64_t)n + kPdPoll) return fail(PCU_HIP_ERR_RUNTIME, "internal: Poisson-disk rounds make no progress");
        for (int k = 0; k < kPdPoll; ++k) {
            hipLaunchKernelGGL(k_pd_cellmin<T>, dim3(nb), dim3(kBlock), 0, s, a);
            hipLaunchKernelGGL(k_pd_decide<T>, dim3(nb), dim3(kBlock), 0, s, a);
            hipLaunchKernelGGL(k_pd_remove<T>, dim3(nb), dim3(kBlock), 0, s, a);
            ++R.rounds;
        }
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipMemcpyAsync(h, a.counters, sizeof h, hipMemcpyDeviceToHost, s));
        HIP_WAIT(s);
    }
    ++R.radii;
    *count = (int64_t)h[1];
    return 0;
}

// The argument checks of downsample_point_cloud_poisson_disk (src/sample_point_cloud.cpp:253-273), in its order; *tol: the tolerance as the
// reference's float argument.
static int pd_check_args(int64_t n, double radius, int64_t target, double tolerance, float* tol) {
    if (target <= 0 && radius <= 0.0) return fail(PCU_HIP_ERR_INVALID, "Cannot have both num_samples <= 0 and radius <= 0");
    if (target <= 0 && std::isnan(radius)) return fail(PCU_HIP_ERR_INVALID, "radius must not be NaN");
    *tol = (float)tolerance;                                   // (npe_default_arg(sample_num_tolerance, float, 0.04))
    if (!(*tol > 0.0f && *tol <= 1.0f)) return fail(PCU_HIP_ERR_INVALID, "sample_num_tolerance must be in (0, 1]");
    if (n <= 0) return fail(PCU_HIP_ERR_INVALID, "Invalid point set with zero elements: v must have shape (n, 3) with n > 0.");
    if (n > 0x07fffff0ll) return fail(PCU_HIP_ERR_INVALID, "point clouds with more than 2^27-16 rows are not supported");
    return 0;
}
// What pd_body takes from the arena for n device-resident rows (target >= n > 0 returns every row: no index, no rounds).
template <typename T>
static size_t pd_body_bytes(int64_t n, int64_t target) {
    if (target > 0 && target >= n) return 4096;
    const size_t N = (size_t)n;
    const int mc = max_cells_for(n, kPdOccupancy);
    return index_bytes<T>(n, kPdOccupancy) + align_up(N * 8, 256) + align_up(N, 256) + 5 * align_up(N * 4, 256) +
           align_up((size_t)mc * 12 + 64, 256) + align_up((N / kScTile + 2) * 4, 256) + 65536;
}
// The greedy and its radius search (:275-329) over device-resident rows, in an arena the caller has begun: d_out (room for n int32, on the
// device) receives the samples' rows in ascending order, *count their number. The compaction is enqueued on s, not waited for.
template <typename T>
static int pd_body(Arena& ar, hipStream_t s, const T* d_pts, int64_t n, double radius, int64_t target, unsigned seed, float tol, int32_t* d_out,
                   int64_t* count, PdRun<T>& R) {
    const size_t N = (size_t)n;
    const int nb = blocks_for((size_t)n);
    if (target > 0 && target >= n) {                           // :275-279
        hipLaunchKernelGGL(k_pd_iota, dim3(nb), dim3(kBlock), 0, s, (int)n, d_out);
        HIP_TRY(hipGetLastError());
        *count = n;
        return 0;
    }
    int rc = 0;
    R.seed = seed; R.pts = d_pts;
    if ((rc = index_alloc(ar, R.gi, n, kPdOccupancy, IndexFor::Atomic))) return rc;
    PdArgs<T>& a = R.a;
    a.n = (int)n;
    if ((rc = aalloc(ar, &a.prio, N)) || (rc = aalloc(ar, &a.state, N)) || (rc = aalloc(ar, &a.cell, N)) || (rc = aalloc(ar, &a.slist, N)) ||
        (rc = aalloc(ar, &a.cellmin, (size_t)R.gi.max_cells)) || (rc = aalloc(ar, &a.nsamp, (size_t)R.gi.max_cells)) || (rc = aalloc(ar, &a.counters, 16))) return rc;
    // the bounding box (target mode) and the non-finite check: a first build, read back
    GridParams<T> hg;
    if ((rc = pd_build(R, 0.0, s, &hg))) return rc;
    if (hg.nonfinite) return fail(PCU_HIP_ERR_INVALID, "v must not contain NaN or infinite coordinates");
    int64_t cnt = 0;
    if (target <= 0) {
        if ((rc = pd_run(R, (T)radius, s, &cnt))) return rc;
    } else {
        // :281-329, step for step in T
        const size_t nmin = (size_t)(int)((T)target * (T)(1.0f - tol)), nmax = (size_t)(int)((T)target * (T)(1.0f + tol));
        T e[3];
        for (int j = 0; j < 3; ++j) e[j] = hg.gmax[j] - hg.gmin[j];
        const T bbsize = std::sqrt(((e[0] * e[0]) + (e[1] * e[1])) + (e[2] * e[2]));
        if (!std::isfinite(bbsize)) return fail(PCU_HIP_ERR_INVALID, "the bounding box diagonal of v overflows its scalar type");
        if (bbsize == (T)0) {
            // all rows equal: the reference's doubling loop never ends (every radius is 0). One run at r = inf: the row of lowest priority.
            if ((rc = pd_run(R, std::numeric_limits<T>::infinity(), s, &cnt))) return rc;
        } else {
            T rmin = (T)((double)bbsize / 50.0), rmax = rmin;
            do {
                rmin = (T)((double)rmin / 2.0);
                if ((rc = pd_run(R, rmin, s, &cnt))) return rc;
            } while (cnt < target);
            // (stops also once r * r is infinite in T: a larger radius could not change the result)
            do {
                rmax = (T)((double)rmax * 2.0);
                if ((rc = pd_run(R, rmax, s, &cnt))) return rc;
            } while (cnt > target && std::isfinite(rmax * rmax));
            for (int it = 0; it < 20 && ((size_t)cnt < nmin || (size_t)cnt > nmax); ++it) {
                const T cur = (T)((double)(rmin + rmax) / 2.0);
                if ((rc = pd_run(R, cur, s, &cnt))) return rc;
                if (cnt > target) rmin = cur;
                if (cnt < target) rmax = cur;
            }
        }
    }
    // compaction of the last run: flags by row, inclusive scan, rows in ascending order
    unsigned *flag = nullptr, *scan = nullptr;
    if ((rc = aalloc(ar, &flag, N)) || (rc = aalloc(ar, &scan, N))) return rc;
    hipLaunchKernelGGL(k_pd_flags<T>, dim3(nb), dim3(kBlock), 0, s, R.gi.sorted, a.state, (int)n, flag);
    if ((rc = own_inclusive_scan(ar, s, flag, scan, N))) return rc;
    hipLaunchKernelGGL(k_pd_compact, dim3(nb), dim3(kBlock), 0, s, flag, scan, (int)n, d_out);
    HIP_TRY(hipGetLastError());
    *count = cnt;
    return 0;
}

// downsample_point_cloud_poisson_disk (src/sample_point_cloud.cpp:253-333). out_idx: room for n int32; *out_count entries are written.
template <typename T>
static int poisson_disk_impl(pcu_hip_ctx* c, const T* pts, int64_t n, double radius, int64_t target, unsigned seed, double tolerance,
                             int32_t* out_idx, int64_t* out_count, unsigned flags, void* stream, pcu_hip_stats* st) {
    if (!c) return fail(PCU_HIP_ERR_INVALID, "null context");
    if (st) memset(st, 0, sizeof *st);
    *out_count = 0;
    float tol = 0.0f;
    if (int rc = pd_check_args(n, radius, target, tolerance, &tol)) return rc;
    const size_t N = (size_t)n;
    const bool all_rows = target > 0 && target >= n;
    size_t need = pd_body_bytes<T>(n, target);
    if (!(flags & PCU_HIP_PTRS_ON_DEVICE)) need += (all_rows ? 0 : align_up(N * 3 * sizeof(T), 256)) + align_up(N * 4, 256);
    return op_run(c, flags, stream, st, need, [&](OpFrame& fr) -> int {
        auto& [c, s, on_dev, ar, tm] = fr;
        PdRun<T> R;
        const T* d_pts = nullptr;
        if (!all_rows) if (int rc = stage_in(ar, pts, n, on_dev, s, &d_pts)) return rc;
        int32_t* d_out = nullptr;
        if (int rc = out_room(ar, on_dev, out_idx, N, &d_out)) return rc;
        int64_t cnt = 0;
        if (int rc = pd_body<T>(ar, s, d_pts, n, radius, target, seed, tol, d_out, &cnt, R)) return rc;
        if (out_give(s, on_dev, out_idx, d_out, (size_t)cnt)) return -1;
        HIP_WAIT(s);
        *out_count = cnt;
        if (st && !all_rows) { st->n_queries = n; st->n_passes = R.rounds; st->n_grid_builds = R.radii; }
        return 0;
    });
}
