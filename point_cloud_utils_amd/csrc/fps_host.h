// csrc/fps_host.h -- host orchestration of farthest-point downsampling (kernels and contract: fps.h). Included by pcu_hip.hip after the operator
// frame and the index host.
#pragma once

constexpr double kFpsOcc = (double)kFpsBucket / 4.0;     // the call's own grid: a bucket spans about four cells of the snake order, not a long row of small ones
constexpr int kFpsInFlight = 8;                          // replays in the queue before the host waits (cancellably) for the oldest
// the context's block: what differs between the calls on one layout (FpsCall) at 0, then the words the host or a kernel writes between launches
constexpr size_t kFpsDevBase = 512, kFpsDevStart = 516, kFpsDevBad = 520, kFpsDevCounters = 528, kFpsDevBytes = 1024;

static int64_t fps_block_rows(size_t elem) { return kFpsBlockRows / (int64_t)(elem / 4); }

// The chain of kFpsChain iteration launches, one executable graph per context and scalar type, kept with the layout it was captured for (as
// the kd-level graphs are kept with their key): calls on clouds of one size from one place find it again; what differs between such calls
// (outputs, num_samples, the start row) the nodes read from the context's block.
template <typename T>
static int fps_graph(pcu_hip_ctx* c, hipStream_t w, const FpsArgs<T>& a, hipGraphExec_t* out) {
    pcu_hip_ctx::FpsGraph& G = c->fps_graph[sizeof(T) == 4 ? 0 : 1];
    static_assert(sizeof(FpsArgs<T>) <= sizeof G.key, "the key holds a layout");
    if (!G.exec || memcmp(G.key, &a, sizeof a) != 0) {
        if (G.exec) { (void)hipGraphExecDestroy(G.exec); G.exec = nullptr; }
        if (G.graph) { (void)hipGraphDestroy(G.graph); G.graph = nullptr; }
        const FpsCall<T>* call = reinterpret_cast<const FpsCall<T>*>(c->fps_dev);
        HIP_TRY(hipStreamBeginCapture(w, hipStreamCaptureModeThreadLocal));
        for (int k = 0; k < kFpsChain; ++k) hipLaunchKernelGGL(k_fps_iter<T>, dim3(kFpsBlocks), dim3(kFpsThreads), 0, w, a, call, k);
        HIP_TRY(hipStreamEndCapture(w, &G.graph));
        HIP_TRY(hipGraphInstantiate(&G.exec, G.graph, nullptr, nullptr, 0));
        memcpy(G.key, &a, sizeof a);
    }
    *out = G.exec;
    return 0;
}

// pidx: the cloud is an index object's (its copy of the rows and its grid are used as they are).
template <typename T>
static int fps_impl(pcu_hip_ctx* c, const T* pts, int64_t n, const pcu_hip_index* pidx, int64_t m, int64_t start, int64_t* out_idx, T* out_d,
                    int64_t* out_counters, unsigned flags, void* stream, pcu_hip_stats* st) {
    if (!c) return fail(PCU_HIP_ERR_INVALID, "null context");
    if (out_counters) out_counters[0] = out_counters[1] = 0;
    if (pidx) if (int rc = index_check<T>(c, pidx, &n)) return rc;
    if (n <= 0) return fail(PCU_HIP_ERR_INVALID, "Invalid input point cloud with zero points: points must have shape (n, 3) (n > 0). Got points.shape =(%lld, 3).", (long long)n);
    if (n > kMeshMaxRows) return fail(PCU_HIP_ERR_INVALID, "meshes and point clouds with more than 2^27-16 rows are not supported");
    if (m < 1 || m > n) return fail(PCU_HIP_ERR_INVALID, "Invalid num_samples (%lld): must be at least 1 and at most the number of points (%lld).", (long long)m, (long long)n);
    if (start < 0 || start >= n) return fail(PCU_HIP_ERR_INVALID, "Invalid start_index (%lld): must be a row of points, in [0, %lld).", (long long)start, (long long)n);
    if ((!pidx && !pts) || !out_idx) return fail(PCU_HIP_ERR_INVALID, "null points / out_idx");
    const unsigned force = flags & (PCU_HIP_FPS_ONE_BLOCK | PCU_HIP_FPS_GRID);
    if (force == (PCU_HIP_FPS_ONE_BLOCK | PCU_HIP_FPS_GRID)) return fail(PCU_HIP_ERR_INVALID, "both farthest-point paths forced");
    const bool fits = n <= fps_block_rows(sizeof(T));
    if ((force & PCU_HIP_FPS_ONE_BLOCK) && !fits) return fail(PCU_HIP_ERR_INVALID, "the one-block path holds at most %lld rows of this type", (long long)fps_block_rows(sizeof(T)));
    const bool one_block = force ? (force & PCU_HIP_FPS_ONE_BLOCK) != 0 : fits;
    const bool on_dev = (flags & PCU_HIP_PTRS_ON_DEVICE) != 0;
    const size_t N = (size_t)n, M = (size_t)m;
    const int nb = (int)((n + kFpsBucket - 1) / kFpsBucket), per = (nb + kFpsBlocks - 1) / kFpsBlocks;
    const size_t slots = (size_t)kFpsBlocks * per;
    DatasetFrame<T> ds{pidx, pts, n, on_dev};                           // (the one-block path takes the rows and no grid)
    size_t bytes = 65536 + ds.bytes(kFpsOcc, !one_block) + (on_dev ? 0 : align_up(M * 8, 256) + align_up(M * sizeof(T), 256));
    if (!one_block) bytes += align_up(N * sizeof(T), 256) + align_up(slots * 6 * sizeof(T), 256) + 3 * align_up(slots * 8, 256) +
                             align_up(slots * 3 * sizeof(T), 256) + 3 * align_up(2 * kFpsBlocks * 8, 256) + align_up(6 * kFpsBlocks * sizeof(T), 256);
    return op_run(c, flags, stream, st, bytes, [&](OpFrame& fr) -> int {
        auto& [c, s, on_dev_, ar, tm] = fr;      // marks 0-1: staging, index, bucket state; 1-2: the iterations
        tm.mark(0);
        if (!c->fps_dev) {
            HIP_TRY(hipMalloc((void**)&c->fps_dev, kFpsDevBytes));
            for (auto& e : c->fps_ev) HIP_TRY(hipEventCreateWithFlags(&e, hipEventDisableTiming));
        }
        if (ds.stage(ar, s)) return -1;
        long long *const h_idx = reinterpret_cast<long long*>(out_idx), *d_idx = nullptr; T* d_d = nullptr;
        if (out_room(ar, on_dev, h_idx, M, &d_idx) || (out_d && out_room(ar, on_dev, out_d, M, &d_d))) return -1;
        int* const d_bad = reinterpret_cast<int*>(c->fps_dev + kFpsDevBad);
        unsigned long long* const d_cnt = reinterpret_cast<unsigned long long*>(c->fps_dev + kFpsDevCounters);
        const int squared = (flags & PCU_HIP_SQUARED) ? 1 : 0;
        int bad = 0;
        if (one_block) {
            HIP_TRY(hipMemsetAsync(d_bad, 0, sizeof(int), s));
            tm.mark(1);
            constexpr int P = kFpsBlockRows / kFpsBlockThreads / (int)(sizeof(T) / 4);       // points per lane: 64 registers of (x, y, z, mind) in either type
            hipLaunchKernelGGL((k_fps_block<T, P>), dim3(1), dim3(kFpsBlockThreads), 0, s, ds.rows, (int)n, (int)m, (int)start, d_idx, d_d, squared, d_bad);
            HIP_TRY(hipGetLastError());
            if (flag_fetch(s, d_bad, &bad)) return -1;
        } else {
            GridIndex<T> gi;
            if (int rc = ds.grid(ar, s, gi, kFpsOcc, IndexFor::Atomic)) return rc;
            // the rule of this call: no NaN, no infinity (an index object may hold single-signed infinities: refused here). Before the
            // iterations are enqueued, so that their arithmetic never sees one.
            int nf = 0;
            if (int rc = nonfinite_fetch(gi.gp, &nf, s)) return rc;
            HIP_WAIT(s);
            if (nf) return fail(PCU_HIP_ERR_INVALID, "points must not contain NaN or infinite coordinates");
            FpsArgs<T> a;
            memset(&a, 0, sizeof a);                                    // (its bytes are the graph's key, padding included)
            a.rec = gi.sorted; a.n = (int)n; a.nb = nb; a.per = per;
            if (aalloc(ar, &a.mind, N) || aalloc(ar, &a.box, slots * 6) || aalloc(ar, &a.bmax, slots) || aalloc(ar, &a.brow, slots) || aalloc(ar, &a.bpos, slots) || aalloc(ar, &a.bxyz, slots * 3) || aalloc(ar, &a.pxyz, 6 * (size_t)kFpsBlocks) ||
                aalloc(ar, &a.pv, 2 * (size_t)kFpsBlocks) || aalloc(ar, &a.prow, 2 * (size_t)kFpsBlocks) || aalloc(ar, &a.ppos, 2 * (size_t)kFpsBlocks)) return -1;
            a.start_pos = reinterpret_cast<int*>(c->fps_dev + kFpsDevStart);
            int* const d_base = reinterpret_cast<int*>(c->fps_dev + kFpsDevBase);
            a.base = d_base;
            a.counters = out_counters ? d_cnt : nullptr;
            FpsCall<T> call{};
            call.out_idx = d_idx; call.out_d = d_d; call.m = (int)m; call.start_row = (int)start; call.squared = squared;
            hipLaunchKernelGGL(k_fps_setup<T>, dim3(1), dim3(1), 0, s, reinterpret_cast<FpsCall<T>*>(c->fps_dev), call, a.counters);
            hipLaunchKernelGGL(k_fps_init<T>, dim3(nb), dim3(64), 0, s, a, (int)start);
            HIP_TRY(hipGetLastError());
            tm.mark(1);
            // The chain runs on a stream that can be captured: the caller's, or -- when that is the legacy default stream -- the context's
            // own, forked from the caller's and joined to it again.
            hipStream_t w = s ? s : c->own_stream;
            if (w != s) { HIP_TRY(hipEventRecord(c->jev[0], s)); HIP_TRY(hipStreamWaitEvent(w, c->jev[0], 0)); }
            hipGraphExec_t exec = nullptr;
            if (int rc = fps_graph<T>(c, w, a, &exec)) return rc;
            const int replays = (int)((m + kFpsChain - 1) / kFpsChain);
            for (int r = 0; r < replays; ++r) {
                if (cancel_requested()) return cancelled(s);
                HIP_TRY(hipMemsetD32Async(reinterpret_cast<hipDeviceptr_t>(d_base), r * kFpsChain, 1, w));
                HIP_TRY(hipGraphLaunch(exec, w));
                HIP_TRY(hipEventRecord(c->fps_ev[r % kFpsInFlight], w));
                if (r + 1 >= kFpsInFlight) { if (int rc = wait_event(c->fps_ev[(r + 1) % kFpsInFlight], s)) return rc; }
            }
            if (w != s) { HIP_TRY(hipEventRecord(c->jev[1], w)); HIP_TRY(hipStreamWaitEvent(s, c->jev[1], 0)); }
        }
        tm.mark(2);
        unsigned long long cnt[2] = {0, 0};
        if (!one_block && out_counters) HIP_TRY(hipMemcpyAsync(cnt, d_cnt, sizeof cnt, hipMemcpyDeviceToHost, s));
        if (out_give(s, on_dev, h_idx, d_idx, M) || out_give(s, on_dev, out_d, d_d, M)) return -1;
        HIP_WAIT(s);
        if (bad) return fail(PCU_HIP_ERR_INVALID, "points must not contain NaN or infinite coordinates");
        if (out_counters) { out_counters[0] = (int64_t)cnt[0]; out_counters[1] = (int64_t)cnt[1]; }
        if (st) {
            st->n_queries = n; st->n_passes = one_block ? 1 : (int)((m + kFpsChain - 1) / kFpsChain); st->n_grid_builds = ds.built;
            st->ms_index = tm.span(0, 1); st->ms_search = tm.span(1, 2); st->ms_total = tm.span(0, 2);
        }
        return 0;
    });
}
