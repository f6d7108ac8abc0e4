// csrc/plane_host.h -- host side of segment_point_cloud_plane (kernels: plane.h, consensus.h; the contract in numpy: tests/plane_contract.py).
// Included by pcu_hip.hip after the operator frame, voxel_host.h (scan_bytes), icp_host.h (jacobi_sym) and consensus_host.h (the scoring
// launcher, the result tail, the shared refusals).
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
// The refitted plane from the ten sums about o: the test's record, and [nv, -kk] into plane.
static PlaneHyp plane_refit(const double* S, const double* o, double t2, double* plane) {
    const double cnt = S[0];
    double mu[3], C[3][3], V[3][3];
    for (int a = 0; a < 3; ++a) mu[a] = S[1 + a] / cnt;
    const double* Suu = S + 4;
    int k = 0;
    for (int a = 0; a < 3; ++a) for (int b = a; b < 3; ++b) { C[a][b] = C[b][a] = Suu[k++] - S[1 + a] * mu[b]; }
    jacobi_sym<3>(C, V);                                                // (plane_contract.py: jacobi3)
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

template <typename T>
static size_t plane_bytes(int64_t n, int64_t H, bool on_dev) {
    const size_t N = (size_t)n, nblocks = (N + kIcpRows - 1) / kIcpRows;
    size_t b = align_up((size_t)H * sizeof(PlaneHyp), 256) + align_up((size_t)H * 4, 256) + 2 * align_up(N * 4, 256) + scan_bytes(N) +
               align_up(kPlaneSums * nblocks * 8, 256) + align_up(kPlaneSums * ((nblocks + 63) / 64) * 8, 256) + 16384;
    if (!on_dev) b += align_up(N * 3 * sizeof(T), 256) + align_up(N * 8, 256);
    return b;
}

// out: host memory. out_inliers: room for n int64 rows (the first out->num_inliers are the result, ascending). launch_tests: 0 (the default,
// kConsensusLaunchTests) or the tests of a scoring launch (tests). One wait without refit, two with it. stats: consensus_report's.
template <typename T>
static int plane_impl(pcu_hip_ctx* c, const T* points, int64_t n, double thr, int64_t H, unsigned seed, int refit, int64_t launch_tests, pcu_hip_plane_result* out,
                      int64_t* out_inliers, unsigned flags, void* stream, pcu_hip_stats* st) {
    if (!c) return fail(PCU_HIP_ERR_INVALID, "null context");
    if (n < 3) return fail(PCU_HIP_ERR_INVALID, "Invalid number of points (%lld): a plane needs at least 3.", (long long)n);
    if (n > kMeshMaxRows) return fail(PCU_HIP_ERR_INVALID, "meshes and point clouds with more than 2^27-16 rows are not supported");
    if (int rc = consensus_check("distance_threshold", thr, H)) return rc;
    if (int rc = consensus_check_launch_tests(launch_tests)) return rc;
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
        using M = PlaneModel<T>;
        int launches = 0;
        if (int rc = consensus_score_launch<M>(k_consensus_score<M>, c, s, d_pts, n, d_hyp, uH, launch_tests, d_scores, &launches)) return rc;
        hipLaunchKernelGGL(k_consensus_best<M>, dim3(1), dim3(1024), 0, s, (const unsigned*)d_scores, (const PlaneHyp*)d_hyp, uH, typename M::Draw{d_pts, (unsigned)n, md, seed}, d_best);
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
        if (int rc = consensus_inliers<M>(fr, {d_pts, n, d_best, flag, rank, d_inl, h_inl, nullptr, nullptr}, refit != 0, best, final_q, &count, [](const PlaneBest*) {})) return rc;
        if (best.score == 0) out->status = kPlaneNoPlane;
        else {
            if (!refit) {
                const PlaneHyp& q = best.hyp;
                const double l = sqrt((q.c0 * q.c0 + q.c1 * q.c1) + q.c2 * q.c2);
                plane[0] = q.c0 / l; plane[1] = q.c1 / l; plane[2] = q.c2 / l; plane[3] = -q.k / l;
            }
            plane_sign(plane);
            memcpy(out->plane, plane, sizeof plane);
            out->status = kPlaneOk;
        }
        consensus_report(fr, n, launches, best.score, best.h, count, out, st);
        return 0;
    });
}
