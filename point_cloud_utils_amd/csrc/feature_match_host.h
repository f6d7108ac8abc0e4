// csrc/feature_match_host.h -- host orchestration of match_point_features (kernels and contract: feature_match.h). Included by pcu_hip.hip
// after the operator frame.
#pragma once

// How one direction of the search is cut: blocks of kFmQueries queries along x; the dataset split along y while there are few query blocks.
struct FmCut { unsigned qblocks; int splits, split_rows; };
static FmCut fm_cut(int64_t n, int64_t m) {
    FmCut k;
    k.qblocks = (unsigned)((n + kFmQueries - 1) / kFmQueries);
    const int64_t tiles = (m + kFmTile - 1) / kFmTile;
    const int64_t want = std::min<int64_t>(tiles, std::max<int64_t>(1, 1024 / (int64_t)k.qblocks));
    k.split_rows = (int)((tiles + want - 1) / want) * kFmTile;
    k.splits = (int)((m + k.split_rows - 1) / k.split_rows);
    return k;
}
template <typename T>
static size_t fm_direction_bytes(int64_t n, int64_t m) {
    const FmCut k = fm_cut(n, m);
    return align_up((size_t)k.splits * (size_t)n * sizeof(T), 256) + align_up((size_t)k.splits * (size_t)n * 4, 256);
}
// nearest (n int64) and d2 (n of T) of the rows of q (n x D) among the rows of d (m x D), all on the device
template <typename T>
static int fm_direction(Arena& ar, hipStream_t s, const T* q, int64_t n, const T* d, int64_t m, int D, long long* out_j, T* out_d) {
    const FmCut k = fm_cut(n, m);
    FmArgs<T> a{};
    a.q = q; a.d = d; a.n = (int)n; a.m = (int)m; a.D = D; a.split_rows = k.split_rows;
    if (aalloc(ar, &a.part_d, (size_t)k.splits * (size_t)n) || aalloc(ar, &a.part_j, (size_t)k.splits * (size_t)n)) return -1;
    a.cancel_word = g_cancel_mirror.load(std::memory_order_relaxed); a.cancel_gen = t_call_gen;
    const dim3 grid(k.qblocks, (unsigned)k.splits);
    if (D == 33) {
        hipLaunchKernelGGL((k_feature_match<T, 33>), grid, dim3(kBlock), fm_lds_bytes<T>(33, false), s, a);
    } else {
        // (D = 128 in float64 takes 99 KiB of LDS: above the 64 KiB a kernel gets unasked)
        static std::atomic<unsigned long long> attr_set[2];
        if (attr_unset_here(attr_set[sizeof(T) == 4 ? 0 : 1]))
            HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void*>(&k_feature_match<T, 0>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)fm_lds_bytes<T>(kFmMaxD, true)));
        hipLaunchKernelGGL((k_feature_match<T, 0>), grid, dim3(kBlock), fm_lds_bytes<T>(D, true), s, a);
    }
    hipLaunchKernelGGL(k_feature_match_fold<T>, dim3(blocks_for((size_t)n)), dim3(kBlock), 0, s, (const T*)a.part_d, (const int*)a.part_j, k.splits, (int)n, out_j, out_d);
    HIP_TRY(hipGetLastError());
    return 0;
}

// out_nearest (n int64; -1: no candidate), out_d2 (n of T), out_mutual (n bytes, 0 / 1; may be null). One wait.
// stats: n_queries = n, n_passes = 1 or 2 (mutual), n_escalated = the dataset splits of the forward search, ms_search, ms_total.
template <typename T>
static int match_features_impl(pcu_hip_ctx* c, const T* query, int64_t n, const T* dataset, int64_t m, int64_t dims, int64_t* out_nearest, T* out_d2, unsigned char* out_mutual,
                               unsigned flags, void* stream, pcu_hip_stats* st) {
    if (!c) return fail(PCU_HIP_ERR_INVALID, "null context");
    if (n <= 0 || m <= 0)
        return fail(PCU_HIP_ERR_INVALID, "Invalid input set with zero elements: query_features and dataset_features must have shape (n, D) and (m, D). "
                    "Got query_features.shape = (%lld, %lld), dataset_features.shape = (%lld, %lld).", (long long)n, (long long)dims, (long long)m, (long long)dims);
    if (n > kMeshMaxRows || m > kMeshMaxRows) return fail(PCU_HIP_ERR_INVALID, "point clouds with more than 2^27-16 rows are not supported");
    if (dims < 1 || dims > kFmMaxD) return fail(PCU_HIP_ERR_INVALID, "Invalid feature dimension (%lld): must be in [1, 128].", (long long)dims);
    if (!query || !dataset || !out_nearest || !out_d2) return fail(PCU_HIP_ERR_INVALID, "null query_features / dataset_features / output");
    const bool dev = (flags & PCU_HIP_PTRS_ON_DEVICE) != 0, mutual = out_mutual != nullptr;
    const size_t N = (size_t)n, M = (size_t)m, D = (size_t)dims;
    size_t bytes = fm_direction_bytes<T>(n, m) + 16384;
    if (!dev) bytes += align_up(N * D * sizeof(T), 256) + align_up(M * D * sizeof(T), 256) + align_up(N * 8, 256) + align_up(N * sizeof(T), 256) + align_up(N, 256);
    if (mutual) bytes += fm_direction_bytes<T>(m, n) + align_up(M * 8, 256) + align_up(M * sizeof(T), 256);
    return op_run(c, flags, stream, st, bytes, [&](OpFrame& fr) -> int {
        auto& [c, s, on_dev, ar, tm] = fr;      // marks 0-1: the search, both directions
        tm.mark(0);
        const T *dq = nullptr, *dd = nullptr;
        if (stage_any(ar, query, N * D, on_dev, s, &dq) || stage_any(ar, dataset, M * D, on_dev, s, &dd)) return -1;
        long long *d_j = nullptr, *back_j = nullptr; T *d_d = nullptr, *back_d = nullptr; unsigned char* d_mut = nullptr;
        long long* const h_j = reinterpret_cast<long long*>(out_nearest);
        if (out_room(ar, on_dev, h_j, N, &d_j) || out_room(ar, on_dev, out_d2, N, &d_d) || (mutual && out_room(ar, on_dev, out_mutual, N, &d_mut))) return -1;
        if (int rc = fm_direction<T>(ar, s, dq, n, dd, m, (int)dims, d_j, d_d)) return rc;
        if (mutual) {
            if (aalloc(ar, &back_j, M) || aalloc(ar, &back_d, M)) return -1;
            if (int rc = fm_direction<T>(ar, s, dd, m, dq, n, (int)dims, back_j, back_d)) return rc;
            hipLaunchKernelGGL(k_feature_match_mutual, dim3(blocks_for(N)), dim3(kBlock), 0, s, (const long long*)d_j, (const long long*)back_j, (int)n, d_mut);
            HIP_TRY(hipGetLastError());
        }
        tm.mark(1);
        if (out_give(s, on_dev, h_j, d_j, N) || out_give(s, on_dev, out_d2, d_d, N) || (mutual && out_give(s, on_dev, out_mutual, d_mut, N))) return -1;
        HIP_WAIT(s);
        if (st) { st->n_queries = n; st->n_passes = mutual ? 2 : 1; st->n_escalated = fm_cut(n, m).splits; st->ms_search = tm.span(0, 1); st->ms_total = tm.span(0, 1); }
        return 0;
    });
}
