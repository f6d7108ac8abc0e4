// csrc/consensus_host.h -- the host side that every RANSAC operator shares (kernels: consensus.h). Included by pcu_hip.hip
// after the operator frame, launch_in_pieces, voxel_host.h (own_inclusive_scan) and icp_host.h (IcpRecord's users), ahead of plane_host.h and
// ransac_host.h. An operator validates with the helpers below, enqueues its hypotheses, calls consensus_score_launch and k_consensus_best,
// refits in its own way, and ends with consensus_inliers and consensus_report.
#pragma once

// The refusals the operators share; `name` is the operator's name for its threshold.
static int consensus_check(const char* name, double thr, int64_t H) {
    if (!(thr >= 0.0) || std::isinf(thr)) return fail(PCU_HIP_ERR_INVALID, "Invalid %s (%g): must be finite and not negative.", name, thr);
    if (H < 1 || H > (1 << 20)) return fail(PCU_HIP_ERR_INVALID, "Invalid num_iterations (%lld): must be an integer in [1, 2**20].", (long long)H);
    return 0;
}
static int consensus_check_launch_tests(int64_t launch_tests) {
    if (launch_tests < 0) return fail(PCU_HIP_ERR_INVALID, "Invalid launch_tests (%lld): must not be negative.", (long long)launch_tests);
    return 0;
}

// The hypotheses [0, H) against every row, in launches of about launch_tests tests (0: kConsensusLaunchTests): at most two in the queue, the
// host waiting (cancellably) for launch i - 1 before it enqueues launch i + 1 (launch_in_pieces). kernel: k_consensus_score<M>, or the
// operator's own kernel of that shape and those arguments (ransac.h: k_ransac_score).
template <typename M, typename Kernel>
static int consensus_score_launch(Kernel kernel, pcu_hip_ctx* c, hipStream_t s, const typename M::Elem* data, int64_t n, const typename M::Hyp* hyp, unsigned H, int64_t launch_tests,
                                  unsigned* scores, int* n_launches) {
    if (!launch_tests) launch_tests = kConsensusLaunchTests;
    const unsigned per = (unsigned)std::min<int64_t>(std::max<int64_t>(launch_tests / n / 64, 1) * 64, 1 << 20);      // hypotheses of a launch: a multiple of 64
    const unsigned waves = (unsigned)((n + 64 * M::kRows - 1) / (64 * M::kRows)), bx = (waves + kConsensusScoreBlock / 64 - 1) / (kConsensusScoreBlock / 64);
    *n_launches = (int)((H + per - 1) / per);
    return launch_in_pieces(c, s, *n_launches, [&](int i) {
        const unsigned h0 = (unsigned)i * per, h1 = std::min(H, h0 + per), groups = (h1 - h0 + 63) / 64;
        const unsigned by = std::min(groups, std::max(1u, (unsigned)kConsensusScoreWaves / waves)), slice = (groups + by - 1) / by * 64;
        hipLaunchKernelGGL(kernel, dim3(bx, (groups * 64 + slice - 1) / slice), dim3(kConsensusScoreBlock), 0, s, data, (unsigned)n, hyp, h0, h1, slice, scores);
    });
}

// What the result tail works on: the operator's data (n rows), the winner on the device, and the room of the flags, their ranks and the rows
// (d_inl on the device, h_inl the caller's); d_rec / rec, where the operator wants a record of its own sums read with the same wait, else null.
template <typename M>
struct ConsensusTail {
    const typename M::Elem* data; int64_t n; const typename M::Best* d_best;
    unsigned *flag, *rank; long long *d_inl, *h_inl;
    const IcpRecord* d_rec; IcpRecord* rec;
};
// The result tail. Unless the refit's wait has shown that no hypothesis has an inlier (refit && !best.score): the flags of the final model --
// the winner on the device without refit, the host's `given` with it --, their scan, the ascending rows; more(from) enqueues what the
// operator wants beside them; then one wait brings the count, the rows, without refit the winner (into best), and rec.
template <typename M, typename More>
static int consensus_inliers(OpFrame& fr, const ConsensusTail<M>& t, bool refit, typename M::Best& best, const typename M::Hyp& given, unsigned* count, More more) {
    auto& [c, s, on_dev, ar, tm] = fr;
    const size_t N = (size_t)t.n;
    const auto [data, n, d_best, flag, rank, d_inl, h_inl, d_rec, rec] = t;
    *count = 0;
    if (refit && !best.score) { tm.mark(3); return 0; }
    const typename M::Best* const from = refit ? nullptr : d_best;
    hipLaunchKernelGGL(k_consensus_mark<M>, dim3(blocks_for(N)), dim3(kBlock), 0, s, data, (unsigned)n, from, given, flag);
    if (own_inclusive_scan<unsigned>(ar, s, flag, rank, N)) return -1;
    hipLaunchKernelGGL(k_consensus_emit, dim3(blocks_for(N)), dim3(kBlock), 0, s, (const unsigned*)flag, (const unsigned*)rank, (int)n, d_inl);
    more(from);
    HIP_TRY(hipGetLastError());
    tm.mark(3);
    HIP_TRY(hipMemcpyAsync(count, rank + (N - 1), 4, hipMemcpyDeviceToHost, s));
    if (d_rec) HIP_TRY(hipMemcpyAsync(rec, d_rec, sizeof *rec, hipMemcpyDeviceToHost, s));
    if (!refit) HIP_TRY(hipMemcpyAsync(&best, d_best, sizeof best, hipMemcpyDeviceToHost, s));
    // (host memory: all n rows travel with this wait -- the count is not known before it; the caller keeps the first num_inliers)
    if (out_give(s, on_dev, h_inl, d_inl, N)) return -1;
    HIP_WAIT(s);                                                        // the results
    if (best.score == 0) *count = 0;
    return 0;
}

// What both results and their statistics say alike. stats: n_queries = n, n_passes = scoring launches, n_escalated = the winner's score,
// ms_index (up to the hypotheses), ms_search (scoring), ms_total.
template <typename Result>
static void consensus_report(OpFrame& fr, int64_t n, int launches, unsigned score, unsigned h, unsigned count, Result* out, pcu_hip_stats* st) {
    if (score) out->best_iteration = (int64_t)h;
    out->num_inliers = (int64_t)count; out->score = (int64_t)score;
    if (st) {
        st->n_queries = n; st->n_passes = launches; st->n_escalated = (int64_t)score;
        st->ms_index = fr.tm.span(0, 1); st->ms_search = fr.tm.span(1, 2); st->ms_total = fr.tm.span(0, 3);
    }
}
