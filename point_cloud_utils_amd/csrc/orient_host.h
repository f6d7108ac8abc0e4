// csrc/orient_host.h -- host orchestration of orient_point_cloud_normals (kernels and contract: orient.h). Included by pcu_hip.hip after knn_impl,
// aux_reserve and the operator frame.
//
// The neighbour array is knn_impl's, composed as normals_knn_impl and icp_host.h compose it: the search begins a call of its own on the context
// (ctx_begin hands it the arena from its start), so what has to outlive it -- the staged inputs of a call with host pointers, the neighbour rows
// and their distances -- lives in c->aux. Everything after the search is one op_run frame over the arena.
#pragma once

// What the frame takes from the arena.
template <typename T>
static size_t orient_bytes(int64_t n, int m, bool on_dev, bool want_flipped) {
    const size_t N = (size_t)n;
    size_t b = align_up(N * (size_t)m, 256) + 3 * align_up(N * 4, 256) + 2 * align_up(N * 8, 256) + align_up(kOrCounts * 4, 256) + 8192;
    if (!on_dev) b += align_up(N * 3 * sizeof(T), 256) + (want_flipped ? align_up(N, 256) : 0);
    return b;
}

// out_normals: n x 3 of T. out_flipped: n bytes (1: the row's normal was negated), or null. One wait per round and one for the results.
// stats: n_queries = n, n_passes = rounds, n_escalated = trees, n_grid_builds = the search's, ms_index (search), ms_search (rounds), ms_tie (outputs), ms_total.
template <typename T>
static int orient_impl(pcu_hip_ctx* c, const T* points, const T* normals, int64_t n, int64_t k, int max_leaf, T* out_normals, unsigned char* out_flipped,
                       unsigned flags, void* stream, pcu_hip_stats* st) {
    if (!c) return fail(PCU_HIP_ERR_INVALID, "null context");
    if (k <= 0) return fail(PCU_HIP_ERR_INVALID, "Invalid number of neighbors (%lld) must be greater than 0.", (long long)k);
    if (int rc = validate_sizes(n, n, "query_points", "dataset_points")) return rc;
    if (!points || !normals || !out_normals) return fail(PCU_HIP_ERR_INVALID, "null points / normals / out_normals");
    const bool on_dev = (flags & PCU_HIP_PTRS_ON_DEVICE) != 0, timed = st && (flags & PCU_HIP_TIME_PHASES);
    hipStream_t s = pick_stream(c, flags, stream);
    const size_t N = (size_t)n;
    const int m = (int)std::min<int64_t>(k, n - 1) + 1;                 // the row itself and k others, as far as the cloud has them
    auto al = [](size_t v) { return align_up(v, 256); };
    const size_t b_in = al(N * 3 * sizeof(T));
    if (aux_reserve(c, (on_dev ? 0 : 2 * b_in) + al(N * m * 8) + al(N * m * sizeof(T)) + 4096)) return PCU_HIP_ERR_RUNTIME;
    char* cur = c->aux;
    auto take = [&](size_t bytes) { char* r = cur; cur += al(bytes); return r; };
    const T *d_pts = points, *d_nrm = normals;
    if (!on_dev) {
        T* t = (T*)take(N * 3 * sizeof(T)); HIP_TRY(hipMemcpyAsync(t, points, N * 3 * sizeof(T), hipMemcpyHostToDevice, s)); d_pts = t;
        T* u = (T*)take(N * 3 * sizeof(T)); HIP_TRY(hipMemcpyAsync(u, normals, N * 3 * sizeof(T), hipMemcpyHostToDevice, s)); d_nrm = u;
    }
    long long* d_nbr = (long long*)take(N * m * 8);
    T* d_dist = (T*)take(N * m * sizeof(T));
    if (timed) (void)hipEventRecord(c->ev[0], s);                       // (mark 0: the search clears the timing flags it is not given)
    const unsigned kflags = (flags | PCU_HIP_PTRS_ON_DEVICE | PCU_HIP_SQUARED | PCU_HIP_STREAM_GIVEN) & ~(unsigned)(PCU_HIP_TIME_PHASES | PCU_HIP_TIME_KERNELS);
    pcu_hip_stats kst; memset(&kst, 0, sizeof kst);
    // the rule of every searched cloud (nonfinite_error) is the search's own: it refuses the call here
    if (int rc = knn_impl<T>(c, d_pts, n, d_pts, n, m, max_leaf, d_dist, (int64_t*)d_nbr, kflags, (void*)s, &kst)) return rc;
    return op_run(c, flags, stream, st, orient_bytes<T>(n, m, on_dev, out_flipped != nullptr), [&](OpFrame& fr) -> int {
        auto& [c, s, on_dev, ar, tm] = fr;      // marks 0-1: the search, 1-2: the rounds, 2-3: the outputs
        tm.mark(1);
        unsigned *word = nullptr, *hook = nullptr, *top = nullptr, *counts = nullptr; unsigned long long *best_w = nullptr, *best_e = nullptr;
        T* d_out = nullptr; unsigned char *d_flip = nullptr, *dead = nullptr;
        if (aalloc(ar, &word, N) || aalloc(ar, &hook, N) || aalloc(ar, &top, N) || aalloc(ar, &best_w, N) || aalloc(ar, &best_e, N) || aalloc(ar, &counts, (size_t)kOrCounts) || aalloc(ar, &dead, N * (size_t)m) ||
            out_room(ar, on_dev, out_normals, N * 3, &d_out) || (out_flipped && out_room(ar, on_dev, out_flipped, N, &d_flip))) return -1;
        const unsigned un = (unsigned)n, row_blocks = blocks_for(N);
        const unsigned long long slots = (unsigned long long)N * (unsigned)m, m_inv = ~0ull / (unsigned)m;
        const unsigned slot_blocks = blocks_for((size_t)slots);
        HIP_TRY(hipMemsetAsync(counts, 0, kOrCounts * 4, s));
        HIP_TRY(hipMemsetAsync(dead, 0, (size_t)slots, s));
        hipLaunchKernelGGL(k_orient_init, dim3(row_blocks), dim3(kBlock), 0, s, word, top, best_w, best_e, un);
        int rounds = 0; int64_t trees = n;
        for (; n > 1; ++rounds) {
            if (rounds == kOrMaxRounds) return fail(PCU_HIP_ERR_RUNTIME, "internal: the spanning forest took more than %d rounds", kOrMaxRounds);
            hipLaunchKernelGGL((k_orient_offer<T, 0>), dim3(slot_blocks), dim3(kBlock), 0, s, d_nrm, (const long long*)d_nbr, un, (unsigned)m, m_inv, slots, (const unsigned*)word, dead, best_w, best_e);
            hipLaunchKernelGGL((k_orient_offer<T, 1>), dim3(slot_blocks), dim3(kBlock), 0, s, d_nrm, (const long long*)d_nbr, un, (unsigned)m, m_inv, slots, (const unsigned*)word, dead, best_w, best_e);
            hipLaunchKernelGGL(k_orient_hook, dim3(row_blocks), dim3(kBlock), 0, s, (const unsigned*)word, (const unsigned long long*)best_w, (const unsigned long long*)best_e, un, hook, counts + rounds);
            HIP_TRY(hipGetLastError());
            unsigned hooks = 0;
            HIP_TRY(hipMemcpyAsync(&hooks, counts + rounds, 4, hipMemcpyDeviceToHost, s));
            HIP_WAIT(s);                                                // (a cancel request between two rounds ends the call here)
            trees -= hooks;
            if (hooks == 0) break;                                      // no root found an edge: nothing was offered, best_w / best_e are clear
            hipLaunchKernelGGL(k_orient_flatten<T>, dim3(row_blocks), dim3(kBlock), 0, s, d_pts, word, (const unsigned*)hook, best_w, best_e, top, un);
        }
        tm.mark(2);
        hipLaunchKernelGGL(k_orient_write<T>, dim3(row_blocks), dim3(kBlock), 0, s, d_nrm, (const unsigned*)word, (const unsigned*)top, un, d_out, d_flip);
        HIP_TRY(hipGetLastError());
        tm.mark(3);
        if (out_give(s, on_dev, out_normals, d_out, N * 3) || (out_flipped && out_give(s, on_dev, out_flipped, d_flip, N))) return -1;
        HIP_WAIT(s);
        if (st) {
            st->n_queries = n; st->n_passes = rounds; st->n_escalated = trees; st->n_grid_builds = kst.n_grid_builds;
            st->ms_index = tm.span(0, 1); st->ms_search = tm.span(1, 2); st->ms_tie = tm.span(2, 3); st->ms_total = tm.span(0, 3);
        }
        return 0;
    });
}
