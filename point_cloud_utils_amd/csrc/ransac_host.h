// csrc/ransac_host.h -- host side of register_point_clouds_ransac (kernels: ransac.h, consensus.h; the contract in numpy:
// tests/ransac_contract.py). Included by pcu_hip.hip after the operator frame, voxel_host.h (scan_bytes), icp_host.h (icp_horn),
// consensus_host.h (the scoring launcher, the result tail, the shared refusals) and plane_host.h (plane_mods).
//
// The one solve of the call -- Horn's closed form on the winner's inliers -- is icp_horn as it stands: float64 on the host, written as
// icp_contract.py writes it.
#pragma once

enum { kRansacOk = 0, kRansacNoAlignment = 1 };     // pcu_hip_ransac_result::status

template <typename T>
static size_t ransac_bytes(int64_t n, int64_t m, int64_t nc, int64_t H, bool on_dev) {
    const size_t C = (size_t)nc, nblocks = (C + kIcpRows - 1) / kIcpRows;
    size_t b = align_up(6 * C * 8, 256) + align_up((size_t)H * sizeof(RansacHyp), 256) + align_up((size_t)H * 4, 256) + 2 * align_up(C * 4, 256) + scan_bytes(C) +
               align_up(kIcpSumsPoint * nblocks * 8, 256) + align_up(kIcpSumsPoint * ((nblocks + 63) / 64) * 8, 256) + 16384;
    if (!on_dev) b += align_up((size_t)n * 3 * sizeof(T), 256) + align_up((size_t)m * 3 * sizeof(T), 256) + align_up(C * 16, 256) + align_up(C * 8, 256);
    return b;
}

static void ransac_transform(const RansacHyp& q, double* M) {
    for (int a = 0; a < 3; ++a) { for (int b = 0; b < 3; ++b) M[4 * a + b] = q.R[3 * a + b]; M[4 * a + 3] = q.tr[a]; }
    M[12] = M[13] = M[14] = 0.0; M[15] = 1.0;
}

// corr: nc rows [source row, target row]. out: host memory. out_inliers: room for nc int64 rows (the first out->num_inliers are the result,
// ascending). launch_tests: 0 (the default, kConsensusLaunchTests) or the tests of a scoring launch (tests). One wait without refit, two with
// it; the flag word of k_ransac_gather arrives with the first. stats: consensus_report's (ms_index: gather and hypotheses).
template <typename T>
static int ransac_impl(pcu_hip_ctx* c, const T* source, int64_t n, const T* target, int64_t m, const int64_t* corr, int64_t nc, double thr, int64_t H, unsigned seed,
                       double ratio, int refit, int64_t launch_tests, pcu_hip_ransac_result* out, int64_t* out_inliers, unsigned flags, void* stream, pcu_hip_stats* st) {
    if (!c) return fail(PCU_HIP_ERR_INVALID, "null context");
    if (n < 1 || m < 1) return fail(PCU_HIP_ERR_INVALID, "Invalid input point cloud with zero points: source_points and target_points must have shape (n, 3) and (m, 3) (n, m > 0).");
    if (n > kMeshMaxRows || m > kMeshMaxRows) return fail(PCU_HIP_ERR_INVALID, "meshes and point clouds with more than 2^27-16 rows are not supported");
    if (nc < 3) return fail(PCU_HIP_ERR_INVALID, "Invalid number of correspondences (%lld): a rigid transform needs at least 3.", (long long)nc);
    if (nc > kMeshMaxRows) return fail(PCU_HIP_ERR_INVALID, "correspondences with more than 2^27-16 rows are not supported");
    if (int rc = consensus_check("max_correspondence_distance", thr, H)) return rc;
    if (!(ratio >= 0.0 && ratio <= 1.0)) return fail(PCU_HIP_ERR_INVALID, "Invalid edge_length_ratio (%g): must be in [0, 1].", ratio);
    if (int rc = consensus_check_launch_tests(launch_tests)) return rc;
    if (!source || !target || !corr || !out || !out_inliers) return fail(PCU_HIP_ERR_INVALID, "null source / target / correspondences / result / out_inliers");
    memset(out, 0, sizeof *out);
    const bool dev_ptrs = (flags & PCU_HIP_PTRS_ON_DEVICE) != 0;
    return op_run(c, flags, stream, st, ransac_bytes<T>(n, m, nc, H, dev_ptrs), [&](OpFrame& fr) -> int {
        auto& [c, s, on_dev, ar, tm] = fr;      // marks 0-1: staging, gather and hypotheses, 1-2: scoring and winner, 2-3: refit and inliers
        tm.mark(0);
        const size_t C = (size_t)nc; const unsigned uH = (unsigned)H;
        const T *d_src = nullptr, *d_tgt = nullptr; const long long* d_corr = nullptr;
        if (stage_any(ar, source, (size_t)n * 3, on_dev, s, &d_src) || stage_any(ar, target, (size_t)m * 3, on_dev, s, &d_tgt) ||
            stage_any(ar, reinterpret_cast<const long long*>(corr), C * 2, on_dev, s, &d_corr)) return -1;
        double *d_pk = nullptr, *d_part = nullptr, *d_part2 = nullptr; RansacHyp* d_hyp = nullptr; unsigned *d_scores = nullptr, *flag = nullptr, *rank = nullptr;
        RansacBest* d_best = nullptr; IcpRecord* d_rec = nullptr; int* d_flags = nullptr; long long* d_inl = nullptr;
        long long* const h_inl = reinterpret_cast<long long*>(out_inliers);
        const int nblocks = (int)((C + kIcpRows - 1) / kIcpRows), nfold = (nblocks + 63) / 64;
        if (aalloc(ar, &d_pk, 6 * C) || aalloc(ar, &d_hyp, (size_t)H) || aalloc(ar, &d_scores, (size_t)H) || aalloc(ar, &d_best, 1) || aalloc(ar, &flag, C) ||
            aalloc(ar, &rank, C) || aalloc(ar, &d_part, (size_t)kIcpSumsPoint * nblocks) || aalloc(ar, &d_part2, (size_t)kIcpSumsPoint * nfold) || aalloc(ar, &d_rec, 1) ||
            aalloc(ar, &d_flags, 1) || out_room(ar, on_dev, h_inl, C, &d_inl)) return -1;
        const PlaneMods md = plane_mods((unsigned)nc);
        const double t2 = thr * thr, r2 = ratio * ratio;
        HIP_TRY(hipMemsetAsync(d_scores, 0, (size_t)H * 4, s));
        HIP_TRY(hipMemsetAsync(d_flags, 0, sizeof(int), s));
        hipLaunchKernelGGL(k_ransac_gather<T>, dim3(blocks_for(C)), dim3(kBlock), 0, s, d_src, (long long)n, d_tgt, (long long)m, d_corr, (unsigned)nc, d_pk, d_flags);
        hipLaunchKernelGGL(k_ransac_hypotheses, dim3((uH + 255) / 256), dim3(256), 0, s, (const double*)d_pk, (unsigned)nc, md, seed, uH, r2, t2, d_hyp);
        HIP_TRY(hipGetLastError());
        tm.mark(1);
        using M = RansacModel;
        int launches = 0;
        if (int rc = consensus_score_launch<M>(k_ransac_score, c, s, d_pk, nc, d_hyp, uH, launch_tests, d_scores, &launches)) return rc;
        hipLaunchKernelGGL(k_consensus_best<M>, dim3(1), dim3(1024), 0, s, (const unsigned*)d_scores, (const RansacHyp*)d_hyp, uH, M::Draw{}, d_best);
        HIP_TRY(hipGetLastError());
        tm.mark(2);
        auto bad_rows = [&](int f) -> int {
            if (f & kRansacBadSource) return fail(PCU_HIP_ERR_INVALID, "correspondences[:, 0] must hold rows of source_points: found an entry outside [0, %lld)", (long long)n);
            return fail(PCU_HIP_ERR_INVALID, "correspondences[:, 1] must hold rows of target_points: found an entry outside [0, %lld)", (long long)m);
        };
        RansacBest best{}; RansacHyp final_q{}; IcpRecord rec{};
        if (refit) {
            hipLaunchKernelGGL(k_ransac_sums<kIcpSumsPoint>, dim3((unsigned)nblocks), dim3(kIcpBlock), 0, s, (const double*)d_pk, (int)nc, (const RansacBest*)d_best, final_q, d_part, nblocks);
            hipLaunchKernelGGL(k_icp_fold, dim3(1), dim3(kIcpBlock), 0, s, d_part, d_part2, nblocks, kIcpSumsPoint, (const int*)d_flags, d_rec);
            HIP_TRY(hipGetLastError());
            HIP_TRY(hipMemcpyAsync(&rec, d_rec, sizeof rec, hipMemcpyDeviceToHost, s));
            HIP_TRY(hipMemcpyAsync(&best, d_best, sizeof best, hipMemcpyDeviceToHost, s));
            HIP_WAIT(s);                                                // the first wait: the flag word, the sums and the winner
            if (rec.flags) return bad_rows(rec.flags);
            final_q = best.hyp;
            const long long count = (long long)rec.sums[0];
            if (count >= 3) {
                IcpStep D;
                icp_horn(rec.sums, count, D);
                for (int a = 0; a < 3; ++a) { for (int b = 0; b < 3; ++b) final_q.R[3 * a + b] = D.R[a][b]; final_q.tr[a] = D.t[a]; }
                final_q.bound = t2;
            }
        }
        unsigned count = 0;
        if (int rc = consensus_inliers<M>(fr, {d_pk, nc, d_best, flag, rank, d_inl, h_inl, d_rec, &rec}, refit != 0, best, final_q, &count, [&](const RansacBest* from) {
                hipLaunchKernelGGL(k_ransac_sums<2>, dim3((unsigned)nblocks), dim3(kIcpBlock), 0, fr.s, (const double*)d_pk, (int)nc, from, final_q, d_part, nblocks);
                hipLaunchKernelGGL(k_icp_fold, dim3(1), dim3(kIcpBlock), 0, fr.s, d_part, d_part2, nblocks, 2, (const int*)d_flags, d_rec);
            })) return rc;
        if (rec.flags) return bad_rows(rec.flags);
        if (!refit) final_q = best.hyp;
        static const double eye[16] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1};
        if (best.score == 0) { out->status = kRansacNoAlignment; memcpy(out->transform, eye, sizeof eye); }
        else {
            ransac_transform(final_q, out->transform);
            out->status = kRansacOk;
            out->fitness = (double)count / (double)nc;
            out->inlier_rmse = count ? sqrt(rec.sums[1] / (double)count) : 0.0;
        }
        consensus_report(fr, nc, launches, best.score, best.h, count, out, st);
        return 0;
    });
}
