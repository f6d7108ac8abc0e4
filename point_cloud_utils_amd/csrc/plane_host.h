// csrc/plane_host.h -- host side of segment_point_cloud_plane (kernels: plane.h; the contract in numpy: tests/plane_contract.py). Included by
// pcu_hip.hip after the operator frame, voxel_host.h (own_inclusive_scan, scan_bytes) and icp_host.h (kIcpJacobiSweeps).
//
// The solve is float64 on the host with + - * /, sqrt and comparisons only, every expression written as plane_contract.py writes it: the unit is
// built with -ffp-contract=off and the host target has no FMA, so that C++ and Python round alike.
#pragma once

enum { kPlaneOk = 0, kPlaneNoPlane = 1 };          // pcu_hip_plane_result::status

static PlaneMods plane_mods(unsigned n) {
    PlaneMods md;
    for (unsigned a = 0; a < 3; ++a) md.m[a] = ~0ull / (unsigned long long)(n - a);
    return md;
}
// Cyclic Jacobi on a symmetric 3x3: pairs (0,1) (0,2) (1,2), kIcpJacobiSweeps sweeps, a zero entry skipped; the rotations of icp_jacobi4.
static void plane_jacobi3(double A[3][3], double V[3][3]) {
    static const int pairs[3][2] = {{0, 1}, {0, 2}, {1, 2}};
    for (int i = 0; i < 3; ++i) for (int k = 0; k < 3; ++k) V[i][k] = i == k ? 1.0 : 0.0;
    for (int sweep = 0; sweep < kIcpJacobiSweeps; ++sweep)
        for (const auto& pq : pairs) {
            const int p = pq[0], q = pq[1];
            const double apq = A[p][q];
            if (apq == 0.0) continue;
            const double theta = (A[q][q] - A[p][p]) / (2.0 * apq);
            const double den = fabs(theta) + sqrt(theta * theta + 1.0);
            const double t = theta >= 0.0 ? 1.0 / den : -1.0 / den;
            const double c = 1.0 / sqrt(t * t + 1.0), s = t * c;
            for (int k = 0; k < 3; ++k) { const double akp = A[k][p], akq = A[k][q]; A[k][p] = c * akp - s * akq; A[k][q] = s * akp + c * akq; }
            for (int k = 0; k < 3; ++k) { const double apk = A[p][k], aqk = A[q][k]; A[p][k] = c * apk - s * aqk; A[q][k] = s * apk + c * aqk; }
            A[p][q] = A[q][p] = 0.0;
            for (int k = 0; k < 3; ++k) { const double vkp = V[k][p], vkq = V[k][q]; V[k][p] = c * vkp - s * vkq; V[k][q] = s * vkp + c * vkq; }
        }
}
// The refitted plane from the ten sums about o: the test's record, and [nv, -kk] into plane.
static PlaneHyp plane_refit(const double* S, const double* o, double t2, double* plane) {
    const double cnt = S[0];
    double mu[3], C[3][3], V[3][3];
    for (int a = 0; a < 3; ++a) mu[a] = S[1 + a] / cnt;
    const double* Suu = S + 4;
    int k = 0;
    for (int a = 0; a < 3; ++a) for (int b = a; b < 3; ++b) { C[a][b] = C[b][a] = Suu[k++] - S[1 + a] * mu[b]; }
    plane_jacobi3(C, V);
    int best = 0;
    for (int i = 1; i < 3; ++i) if (C[i][i] < C[best][best]) best = i;
    const double v0 = V[0][best], v1 = V[1][best], v2 = V[2][best];
    const double ln = sqrt((v0 * v0 + v1 * v1) + v2 * v2);
    PlaneHyp q;
    q.c0 = v0 / ln; q.c1 = v1 / ln; q.c2 = v2 / ln;
    const double m0 = o[0] + mu[0], m1 = o[1] + mu[1], m2 = o[2] + mu[2];
    q.k = (q.c0 * m0 + q.c1 * m1) + q.c2 * m2;
    q.bound = t2 * ((q.c0 * q.c0 + q.c1 * q.c1) + q.c2 * q.c2);
    plane[0] = q.c0; plane[1] = q.c1; plane[2] = q.c2; plane[3] = -q.k;
    return q;
}
// Negated if the first of a, b, c that is not zero is negative.
static void plane_sign(double* plane) {
    for (int a = 0; a < 3; ++a)
        if (plane[a] != 0.0) {
            if (plane[a] < 0.0) for (int b = 0; b < 4; ++b) plane[b] = -plane[b];
            return;
        }
}

// The hypotheses [0, H) against every row, in launches of about launch_tests tests: at most two in the queue, the host waiting (cancellably)
// for launch i - 1 before it enqueues launch i + 1, as kd_search_launch does.
template <typename T>
static int plane_score_launch(pcu_hip_ctx* c, hipStream_t s, const T* pts, int64_t n, const PlaneHyp* hyp, unsigned H, int64_t launch_tests, unsigned* scores, int* n_launches) {
    const unsigned per = (unsigned)std::min<int64_t>(std::max<int64_t>(launch_tests / n / 64, 1) * 64, 1 << 20);      // hypotheses of a launch: a multiple of 64
    const unsigned waves = (unsigned)((n + 64 * kPlaneRows - 1) / (64 * kPlaneRows)), bx = (waves + kPlaneScoreBlock / 64 - 1) / (kPlaneScoreBlock / 64);
    const bool pieces = H > per;
    if (pieces) for (auto& e : c->cev) if (!e) HIP_TRY(hipEventCreateWithFlags(&e, hipEventDisableTiming));
    int i = 0;
    for (unsigned h0 = 0; h0 < H; h0 += per, ++i) {
        const unsigned h1 = std::min(H, h0 + per), groups = (h1 - h0 + 63) / 64;
        const unsigned by = std::min(groups, std::max(1u, (unsigned)kPlaneScoreWaves / waves)), slice = (groups + by - 1) / by * 64;
        hipLaunchKernelGGL(k_plane_score<T>, dim3(bx, (groups * 64 + slice - 1) / slice), dim3(kPlaneScoreBlock), 0, s, pts, (unsigned)n, hyp, h0, h1, slice, scores);
        HIP_TRY(hipGetLastError());
        if (pieces) {
            HIP_TRY(hipEventRecord(c->cev[i & 1], s));
            if (i >= 1) { if (int w = wait_event(c->cev[(i - 1) & 1], s)) return w; }
        }
    }
    *n_launches = i;
    return 0;
}

template <typename T>
static size_t plane_bytes(int64_t n, int64_t H, bool on_dev) {
    const size_t N = (size_t)n, nblocks = (N + kIcpRows - 1) / kIcpRows;
    size_t b = align_up((size_t)H * sizeof(PlaneHyp), 256) + align_up((size_t)H * 4, 256) + 2 * align_up(N * 4, 256) + scan_bytes(N) +
               align_up(kPlaneSums * nblocks * 8, 256) + align_up(kPlaneSums * ((nblocks + 63) / 64) * 8, 256) + 16384;
    if (!on_dev) b += align_up(N * 3 * sizeof(T), 256) + align_up(N * 8, 256);
    return b;
}

// out: host memory. out_inliers: room for n int64 rows (the first out->num_inliers are the result, ascending). launch_tests: 0 (the default,
// kPlaneLaunchTests) or the tests of a scoring launch (tests). One wait without refit, two with it.
// stats: n_queries = n, n_passes = scoring launches, n_escalated = the winner's score, ms_index (hypotheses), ms_search (scoring), ms_total.
template <typename T>
static int plane_impl(pcu_hip_ctx* c, const T* points, int64_t n, double thr, int64_t H, unsigned seed, int refit, int64_t launch_tests, pcu_hip_plane_result* out,
                      int64_t* out_inliers, unsigned flags, void* stream, pcu_hip_stats* st) {
    if (!c) return fail(PCU_HIP_ERR_INVALID, "null context");
    if (n < 3) return fail(PCU_HIP_ERR_INVALID, "Invalid number of points (%lld): a plane needs at least 3.", (long long)n);
    if (n > kMeshMaxRows) return fail(PCU_HIP_ERR_INVALID, "meshes and point clouds with more than 2^27-16 rows are not supported");
    if (!(thr >= 0.0) || std::isinf(thr)) return fail(PCU_HIP_ERR_INVALID, "Invalid distance_threshold (%g): must be finite and not negative.", thr);
    if (H < 1 || H > (1 << 20)) return fail(PCU_HIP_ERR_INVALID, "Invalid num_iterations (%lld): must be an integer in [1, 2**20].", (long long)H);
    if (launch_tests < 0) return fail(PCU_HIP_ERR_INVALID, "Invalid launch_tests (%lld): must not be negative.", (long long)launch_tests);
    if (!points || !out || !out_inliers) return fail(PCU_HIP_ERR_INVALID, "null points / result / out_inliers");
    memset(out, 0, sizeof *out);
    const bool dev_ptrs = (flags & PCU_HIP_PTRS_ON_DEVICE) != 0;
    return op_run(c, flags, stream, st, plane_bytes<T>(n, H, dev_ptrs), [&](OpFrame& fr) -> int {
        auto& [c, s, on_dev, ar, tm] = fr;      // marks 0-1: staging and hypotheses, 1-2: scoring and winner, 2-3: refit and inliers
        tm.mark(0);
        const size_t N = (size_t)n; const unsigned uH = (unsigned)H;
        const T* d_pts = nullptr;
        if (stage_any(ar, points, N * 3, on_dev, s, &d_pts)) return -1;
        PlaneHyp* d_hyp = nullptr; unsigned *d_scores = nullptr, *flag = nullptr, *rank = nullptr; PlaneBest* d_best = nullptr; long long* d_inl = nullptr;
        long long* const h_inl = reinterpret_cast<long long*>(out_inliers);
        if (aalloc(ar, &d_hyp, (size_t)H) || aalloc(ar, &d_scores, (size_t)H) || aalloc(ar, &d_best, 1) || aalloc(ar, &flag, N) || aalloc(ar, &rank, N) ||
            out_room(ar, on_dev, h_inl, N, &d_inl)) return -1;
        const PlaneMods md = plane_mods((unsigned)n);
        const double t2 = thr * thr;
        HIP_TRY(hipMemsetAsync(d_scores, 0, (size_t)H * 4, s));
        hipLaunchKernelGGL(k_plane_hypotheses<T>, dim3((uH + 255) / 256), dim3(256), 0, s, d_pts, (unsigned)n, md, seed, uH, t2, d_hyp);
        tm.mark(1);
        int launches = 0;
        if (int rc = plane_score_launch<T>(c, s, d_pts, n, d_hyp, uH, launch_tests ? launch_tests : kPlaneLaunchTests, d_scores, &launches)) return rc;
        hipLaunchKernelGGL(k_plane_best<T>, dim3(1), dim3(1024), 0, s, (const unsigned*)d_scores, (const PlaneHyp*)d_hyp, uH, d_pts, (unsigned)n, md, seed, d_best);
        HIP_TRY(hipGetLastError());
        tm.mark(2);
        PlaneBest best{}; PlaneHyp final_q{};
        double plane[4] = {0, 0, 0, 0};
        if (refit) {
            const int nblocks = (int)((N + kIcpRows - 1) / kIcpRows), nfold = (nblocks + 63) / 64;
            double *d_part = nullptr, *d_part2 = nullptr; IcpRecord* d_rec = nullptr; int* d_zero = nullptr;
            if (aalloc(ar, &d_part, (size_t)kPlaneSums * nblocks) || aalloc(ar, &d_part2, (size_t)kPlaneSums * nfold) || aalloc(ar, &d_rec, 1) || aalloc(ar, &d_zero, 1)) return -1;
            HIP_TRY(hipMemsetAsync(d_zero, 0, sizeof(int), s));
            hipLaunchKernelGGL(k_plane_sums<T>, dim3((unsigned)nblocks), dim3(kIcpBlock), 0, s, d_pts, (int)n, (const PlaneBest*)d_best, d_part, nblocks);
            hipLaunchKernelGGL(k_icp_fold, dim3(1), dim3(kIcpBlock), 0, s, d_part, d_part2, nblocks, kPlaneSums, (const int*)d_zero, d_rec);
            HIP_TRY(hipGetLastError());
            IcpRecord rec;
            HIP_TRY(hipMemcpyAsync(&rec, d_rec, sizeof rec, hipMemcpyDeviceToHost, s));
            HIP_TRY(hipMemcpyAsync(&best, d_best, sizeof best, hipMemcpyDeviceToHost, s));
            HIP_WAIT(s);                                                // the first wait: the sums and the winner
            if (best.score) final_q = plane_refit(rec.sums, best.o, t2, plane);
        }
        unsigned count = 0;
        if (!refit || best.score) {
            hipLaunchKernelGGL(k_plane_mark<T>, dim3(blocks_for(N)), dim3(kBlock), 0, s, d_pts, (int)n, refit ? (const PlaneBest*)nullptr : (const PlaneBest*)d_best, final_q, flag);
            if (own_inclusive_scan<unsigned>(ar, s, flag, rank, N)) return -1;
            hipLaunchKernelGGL(k_plane_emit, dim3(blocks_for(N)), dim3(kBlock), 0, s, (const unsigned*)flag, (const unsigned*)rank, (int)n, d_inl);
            HIP_TRY(hipGetLastError());
            tm.mark(3);
            HIP_TRY(hipMemcpyAsync(&count, rank + (N - 1), 4, hipMemcpyDeviceToHost, s));
            if (!refit) HIP_TRY(hipMemcpyAsync(&best, d_best, sizeof best, hipMemcpyDeviceToHost, s));
            // (host memory: all n rows travel with this wait -- the count is not known before it; the caller keeps the first num_inliers)
            if (out_give(s, on_dev, h_inl, d_inl, N)) return -1;
            HIP_WAIT(s);                                                // the results
        } else tm.mark(3);
        if (best.score == 0) { out->status = kPlaneNoPlane; count = 0; }
        else {
            if (!refit) {
                const PlaneHyp& q = best.hyp;
                const double l = sqrt((q.c0 * q.c0 + q.c1 * q.c1) + q.c2 * q.c2);
                plane[0] = q.c0 / l; plane[1] = q.c1 / l; plane[2] = q.c2 / l; plane[3] = -q.k / l;
            }
            plane_sign(plane);
            memcpy(out->plane, plane, sizeof plane);
            out->status = kPlaneOk; out->best_iteration = (int64_t)best.h;
        }
        out->num_inliers = (int64_t)count; out->score = (int64_t)best.score;
        if (st) {
            st->n_queries = n; st->n_passes = launches; st->n_escalated = (int64_t)best.score;
            st->ms_index = tm.span(0, 1); st->ms_search = tm.span(1, 2); st->ms_total = tm.span(0, 3);
        }
        return 0;
    });
}
