// csrc/index_host.h -- host side of the grid index (kernels and their argument structs: grid.h, grid2.h). Included by pcu_hip.hip after the
// context / arena helpers and before the search driver.
//
// An index is built in one of four forms, all live, and index_build_choose() is the one function that says which:
//   staged one-pass       k_bucket_onepass3 -> k_bucket_sort2 (grid2.h)                              index_build_staged
//   first-form one-pass   k_bucket_onepass -> k_bucket_sort                                          index_build_bucketed
//   two-pass bucketed     k_bucket_count -> k_bucket_scatter -> k_bucket_sort -> k_bucket_large      index_build_bucketed
//   atomic                k_count -> k_scan_reduce -> k_scan_apply -> k_scatter                      index_atomic_passes
#pragma once

template <typename T>
struct GridIndex {
    GridParams<T>* gp = nullptr;
    unsigned* cell_start = nullptr;       // counts, scanned in place
    Pt4<T>* sorted = nullptr;
    unsigned* cell_of = nullptr; unsigned* rank = nullptr; unsigned* block_sums = nullptr;
    T* bbox_partial = nullptr;
    int n = 0, max_cells = 0, scan_blocks = 0;
    // bucketed build (grid.h): cells per bucket = 1 << shift; nb_max = host bound on the number of buckets
    bool bucketed = false; int shift = 0, nb_max = 0, n_zero = 0;
    double h_want = 0.0;                  // > 0: cells at least this large (fixed-radius searches)
    Pt4<T>* tmp = nullptr; unsigned *bucket_total = nullptr, *bucket_start = nullptr, *block_base = nullptr, *large_list = nullptr, *n_large = nullptr;
    bool one_pass = false;                // build with k_bucket_onepass (tmp holds nb_max slots of kLargeBucket records); cleared after an overflow
    T* xpartial = nullptr;                // one-pass build, second form (grid2.h): the scatter blocks' bbox partials
    bool lean = false;                    // the Pt4 records of `sorted` are not written (grid2.h: fused k = 1 calls read the coordinate + row-id streams only);
                                          // make_pt4() fills them in when some other kernel needs them
    const T* src = nullptr; double occ_built = 0.0;       // what the index was built from (rebuild after an overflow)
    bool shared_grid = false;             // asked for: this cloud and its partner of a two-sided call are laid over ONE grid (grid2.h: Build2Side::spts1); allocated for
                                          // the larger cloud's plan. Cleared by a build that did not take the second-form one-pass path
};

// ------------------------------------------------------------------------------------------------ layout: what an index takes from its arena
static int max_cells_for(int64_t n, double occ) {
    double c = (double)n / (occ > 0 ? occ : 1.0) * 1.25 + 64.0;
    if (c > 64.0 * 1024 * 1024) c = 64.0 * 1024 * 1024;
    return (int)c;
}
// Bucketed build: applicable when the cells split into <= kBkMaxBuckets buckets of <= 4096 cells (~kBucketPts = 4096 expected points
// each) and the (block, bucket) reservation table stays small; otherwise (tiny or huge clouds, very coarse grids) the atomic build.
// Workspace of the one-pass variant: every bucket owns a fixed slot of kLargeBucket = 8192 records in `tmp`, i.e. max(n, buckets x 8192)
// records -- about 4x the cloud at 1M points (67 MB instead of 16), bounded by kBkMaxBuckets x 8192 records (2 GiB for float64) beyond
// which it grows with n like everything else.
static bool bucket_plan(int64_t n, double occ, int* shift, int* nb_max) {
    static const bool off = [] { const char* e = getenv("PCU_HIP_INDEX"); return e && strcmp(e, "atomic") == 0; }();
    static const int64_t n_min = getenv("PCU_HIP_BUCKET_MIN") ? atoll(getenv("PCU_HIP_BUCKET_MIN")) : 64;         // below: the atomic build (round 4: 32768; see wave_only_below)
    if (off || n < n_min || occ > 64.0) return false;
    const int mc = max_cells_for(n, occ);
    int sh = 5;
    while (sh < 12 && (double)(2 << sh) * occ <= (double)kBucketPts) ++sh;             // largest bucket with <= ~kBucketPts expected points
    while (sh < 12 && ((mc >> sh) + 1) > kBkMaxBuckets) ++sh;
    const int nb = (mc >> sh) + 1;
    if (nb > kBkMaxBuckets) return false;
    if ((double)(1 << sh) * occ > 0.5 * (double)kLargeBucket) return false;
    const int64_t blocks = (n + kBkBlockPts - 1) / kBkBlockPts;
    if (blocks * (int64_t)nb > 32ll * 1024 * 1024) return false;      // (block, bucket) reservation table: at most 128 MB
    *shift = sh; *nb_max = nb;
    return true;
}
// What index_alloc reserves for: the atomic build only, the bucketed build with both scatter passes, or with the one-pass scatter (the
// largest: slots in `tmp`, `xpartial`). The bucketed kinds fall back to the atomic one where bucket_plan says so.
enum class IndexFor { Atomic, TwoPass, OnePass };
struct PlanFor { int64_t n = 0; };        // the cell / bucket plan of a larger cloud: the partner this cloud shares its grid with (GridIndex::shared_grid)
// The ONE walk over an index's allocations: over a real arena it hands the memory out, over a counting one (index_bytes) it measures.
template <typename T>
static int index_alloc(Arena& a, GridIndex<T>& g, int64_t n, double occ, IndexFor kind, PlanFor plan = PlanFor()) {
    const int64_t np = plan.n > n ? plan.n : n;
    const bool one_pass = kind == IndexFor::OnePass;
    g.n = (int)n; g.max_cells = max_cells_for(np, occ); g.scan_blocks = g.max_cells / kScanChunk + 1;
    g.bucketed = kind != IndexFor::Atomic && bucket_plan(np, occ, &g.shift, &g.nb_max);
    if (aalloc(a, &g.gp, 1)) return -1;
    // (cell_start sits 256 bytes INTO its block: the k = 1 / k > 1 lane kernels read the row table of a query in the first cell of the first row
    // from one word BEFORE cell_start (search.h: "uniform four-word tables"; the word is never used, but its address must be mapped -- also when
    // the block is an overflow hipMalloc of its own))
    if (aalloc(a, &g.cell_start, (size_t)g.max_cells + 1 + kBkMaxBuckets + 8 + 64)) return -1;    // + bucket totals + large-bucket count (zeroed together)
    g.cell_start += 64;
    if (a.alloc((void**)&g.sorted, sorted_records_bytes((size_t)n, sizeof(Pt4<T>), sizeof(T)))) return -1;        // + the +inf sentinel records + the coordinates-only copy (pcu_types.h: xyz_of)
    if (aalloc(a, &g.cell_of, (size_t)n)) return -1;
    if (aalloc(a, &g.rank, (size_t)n)) return -1;
    if (aalloc(a, &g.block_sums, (size_t)g.scan_blocks + 1)) return -1;
    if (aalloc(a, &g.bbox_partial, (size_t)kBboxBlocks * kBboxStride)) return -1;
    g.n_zero = g.max_cells + 1;
    if (g.bucketed) {
        g.bucket_total = g.cell_start + g.max_cells + 1; g.n_large = g.bucket_total + g.nb_max; g.n_zero = g.max_cells + 1 + g.nb_max + 1;
        g.one_pass = one_pass;
        if (aalloc(a, &g.tmp, one_pass ? std::max((size_t)n, (size_t)g.nb_max * kLargeBucket) : (size_t)n)) return -1;
        if (aalloc(a, &g.bucket_start, (size_t)g.nb_max + 1) || aalloc(a, &g.large_list, (size_t)g.nb_max + 1)) return -1;
        if (aalloc(a, &g.block_base, (size_t)((n + kBkBlockPts - 1) / kBkBlockPts) * g.nb_max)) return -1;
        if (one_pass && aalloc(a, &g.xpartial, (size_t)((n + 2047) / 2048) * kXPartStride)) return -1;        // (one partial per scatter block: 2048 points at least, grid2.h)
    }
    return 0;
}
// Bytes of the largest form of an index over n points: the walk above on an arena that only counts (no block, room for everything). The
// pointers the walk hands back are offsets from a null base: never dereferenced, and formally not even valid arithmetic -- `g` is thrown away.
template <typename T>
static size_t index_bytes(int64_t n, double occ) {
    ArenaState count; count.cap = ~(size_t)0 >> 1;
    Arena a(&count); GridIndex<T> g;
    (void)index_alloc(a, g, n, occ, IndexFor::OnePass);
    return count.off;
}
// "Both clouds of a call are built the same way": one launch set serves both only then. Callers that hold copies of the indexes (pair_setup's
// jobs) apply it before they copy; the build applies it to whatever it is given.
template <typename T>
static void index_same_form(GridIndex<T>& a, GridIndex<T>& b) {
    if (a.bucketed && b.bucketed && a.one_pass != b.one_pass) a.one_pass = b.one_pass = false;
}

// ------------------------------------------------------------------------------------------------ kernel arguments, by field name
template <typename T>
static GridSide<T> grid_side(const GridIndex<T>& g) {
    GridSide<T> r{};
    r.gp = g.gp; r.partial = g.bbox_partial; r.nparts = kBboxBlocks; r.n = g.n; r.occupancy = g.occ_built; r.max_cells = g.max_cells;
    r.sentinel = g.sorted + g.n; r.h_want = g.h_want; r.pts = g.src;
    return r;
}
template <typename T>
static BboxSide<T> bbox_side(const GridIndex<T>& g, void* zero2, int n_zero2) {
    BboxSide<T> r{};
    r.pts = g.src; r.n = g.n; r.partial = g.bbox_partial; r.counts = g.cell_start; r.n_counts = g.n_zero;
    r.zero2 = (unsigned*)zero2; r.n_zero2 = n_zero2; r.gp = g.gp;
    return r;
}
template <typename T>
static BucketSide<T> bucket_side(const GridIndex<T>& g) {
    BucketSide<T> r{};
    r.pts = g.src; r.n = g.n; r.gp = g.gp; r.shift = g.shift; r.nb_stride = g.nb_max;
    r.bucket_total = g.bucket_total; r.block_base = g.block_base; r.bucket_start = g.bucket_start; r.tmp = g.tmp; r.cell_start = g.cell_start; r.rank_tmp = g.rank;
    r.sorted = g.sorted; r.large_list = g.large_list; r.n_large = g.n_large; r.cap = g.one_pass ? kLargeBucket : 0u;
    return r;
}
template <typename T>
static LargeJob<T> large_job(const GridIndex<T>& g) {
    LargeJob<T> r{};
    r.gp = g.gp; r.bucket_start = g.bucket_start; r.large_list = g.large_list; r.n_large = g.n_large;
    r.tmp = g.tmp; r.rank_tmp = g.rank; r.cell_start = g.cell_start; r.sorted = g.sorted; r.n_pts = g.n;
    return r;
}
// Side k of a staged build whose scatter blocks hold bpts points; fw: the context's current set of fill words. The cloud's own grid from its own
// sample, no layout handed down, no stage timer: the caller adds those.
template <typename T>
static void build2_side(Build2Side<T>& r, const GridIndex<T>& g, int k, int bpts, unsigned long long* fw) {
    r = Build2Side<T>{};
    r.pts = g.src; r.n = g.n; r.gp = g.gp; r.shift = g.shift;
    r.occupancy = g.occ_built; r.max_cells = g.max_cells; r.h_want = g.h_want;
    r.fill = fw + (size_t)k * kStagedMaxBuckets; r.ovf = fw + 2 * kStagedMaxBuckets + k;
    r.tmp = g.tmp; r.cap = kLargeBucket;
    r.xpartial = g.xpartial; r.n_xpart = (g.n + bpts - 1) / bpts;
    r.cell_start = g.cell_start; r.sorted = g.sorted; r.want_pt4 = g.lean ? 0 : 1;
    r.n_large = g.n_large;
    r.spts0 = g.src; r.sn0 = g.n; r.spts1 = nullptr; r.sn1 = 0; r.n_layout = g.n;
}

// ------------------------------------------------------------------------------------------------ stage timers (diagnostics)
// PCU_HIP_PROF_BUILD / PCU_HIP_PROF_BUILD2: the build kernels sum the per-stage time of every block's thread 0 into device words (100 MHz ticks,
// one word counts the blocks), printed per build; this synchronises the stream. The words are allocated once, zeroed before a launch (arm) and
// read back after it (report). A timer is a function-local static of the build that uses it: the variable is read at the first build of that form.
struct StageTimer {
    const bool on; const int words;
    long long* dev = nullptr;
    StageTimer(const char* env, int nwords) : on(getenv(env) != nullptr), words(nwords) {}
    long long* arg() const { return on ? dev : nullptr; }      // what the kernel is given
    int arm(hipStream_t s) {
        if (!on) return 0;
        if (!dev) HIP_TRY(hipMalloc((void**)&dev, words * sizeof(long long)));
        HIP_TRY(hipMemsetAsync(dev, 0, words * sizeof(long long), s));
        return 0;
    }
    // "[<tag> prof] blocks N | mean us per block: <stage> x.xx  <stage> x.xx ...": slot i = stage i, slot `count` = number of blocks; us = ticks / (blocks x 100) on every line
    int report(hipStream_t s, const char* tag, int count, std::initializer_list<const char*> stages) {
        if (!on) return 0;
        long long h[16]; HIP_TRY(hipMemcpyAsync(h, dev, words * sizeof(long long), hipMemcpyDeviceToHost, s)); HIP_WAIT(s);
        const double nb = h[count] > 0 ? (double)h[count] * 100.0 : 100.0;
        fprintf(stderr, "[%s prof] blocks %lld | mean us per block:", tag, h[count]);
        int i = 0;
        for (const char* st : stages) { fprintf(stderr, "%s%s %.2f", i ? "  " : " ", st, h[i] / nb); ++i; }
        fprintf(stderr, "\n");
        return 0;
    }
};

// ------------------------------------------------------------------------------------------------ which form
enum class BuildForm { Atomic, TwoPass, OnePass, Staged };
struct BuildChoice {
    BuildForm form[2];          // per cloud (the second = the first when one is built); Staged is taken by all clouds of a call or none
    bool grid_in_scatter;       // the scatter blocks lay the grid out themselves: no k_make_grid launch
    int pts;                    // Staged: points per thread of the scatter blocks
};
// Decides how one or two indexes -- already of the same form, index_same_form -- are built. Nothing is launched or changed.
template <typename T>
static BuildChoice index_build_choose(const GridIndex<T>& a, const GridIndex<T>* b, const pcu_hip_ctx* ctx) {
    auto form_of = [](const GridIndex<T>& g) { return !g.bucketed ? BuildForm::Atomic : (g.one_pass ? BuildForm::OnePass : BuildForm::TwoPass); };
    BuildChoice ch{{form_of(a), form_of(b ? *b : a)}, false, 0};
    // When every cloud of the call takes the one-pass bucket build, its blocks lay out the grid themselves (grid.h: k_bucket_onepass)
    // and the k_make_grid launch is skipped. (bbox + grid layout in ONE launch, the last block folding the partials, was measured in
    // round 2: 16.7 us against 8.1 + 4.9 us for the two launches; removed.)
    static const bool grid_kernel = getenv("PCU_HIP_GRID_KERNEL") != nullptr;          // (always the separate k_make_grid launch)
    ch.grid_in_scatter = !grid_kernel && ch.form[0] == BuildForm::OnePass && ch.form[1] == BuildForm::OnePass;
    // The one-pass build's second form (grid2.h): k_bucket_onepass3 -> k_bucket_sort2, while the bucket tables fit beside the scatter's stage.
    // PCU_HIP_BUILD_V1=1 (and the diagnostics of the first form, PCU_HIP_GRID_KERNEL / PCU_HIP_PROF_BUILD) keep the round-3 chain.
    static const bool build_v1 = getenv("PCU_HIP_BUILD_V1") != nullptr || getenv("PCU_HIP_PROF_BUILD") != nullptr;
    // A scatter block's (block, bucket) runs must stay long for the staged copies to pay: below ~12 records per run the padding to whole
    // 8-record groups and the hole records the sort then reads cost more than the first form's per-record scatter (4M-point clouds:
    // 0.40 ms against 0.285, config 3).
    const int run_floor = 12 * std::max(a.nb_max, b ? b->nb_max : 0);
    if (!(ch.grid_in_scatter && !build_v1 && ctx && ctx->fill2 && a.xpartial && (!b || b->xpartial) && a.nb_max <= kStagedMaxBuckets &&
          (!b || b->nb_max <= kStagedMaxBuckets) && kBkThreads * StagedPts<T>::n >= run_floor)) return ch;
    ch.form[0] = ch.form[1] = BuildForm::Staged;
    // points per thread of the scatter blocks: the most (longest runs per (block, bucket), fewest reservations)
    ch.pts = StagedPts<T>::n;
    const long long ntot = (long long)a.n + (b ? b->n : 0);
    static const int n_cu = [] { hipDeviceProp_t pr; int d = 0; (void)hipGetDevice(&d); return hipGetDeviceProperties(&pr, d) == hipSuccess ? pr.multiProcessorCount : 256; }();
    // (measured, profiles/r06_build_ab.txt: halving the blocks to get a block per CU -- or two per CU at 2 x 1M -- LOSES: every stage of a
    // block takes as long with half the points, reservations and padding double; only launches of a handful of blocks are cut up)
    while (ch.pts > 2 && (ntot + (long long)kBkThreads * ch.pts - 1) / ((long long)kBkThreads * ch.pts) < n_cu / 16 && kBkThreads * (ch.pts / 2) >= run_floor) ch.pts /= 2;
    return ch;
}

// What index_build_pair / index_build take beside the clouds.
struct BuildOpts {
    bool defer_large = false;                   // two-pass form: leave the placement of over-full buckets (index_large_pass) to the caller
    void* zero2 = nullptr; int n_zero2 = 0;     // a small region (the call's result block) zeroed on the way by the first launch
    pcu_hip_ctx* ctx = nullptr;                 // whose fill words / handed-down layout the staged form uses; none: never staged
    bool keep_layout = false;                   // two-sided fused calls: hand the grid layout down from the context's previous call
};

// ------------------------------------------------------------------------------------------------ staged one-pass form
// The layout handed down from the context's previous call (grid2.h: GridGeo): two-sided fused calls only (their *_end knows how to restart a
// call whose layout was refused as stale). geo_match points both sides at the context's two layout slots -- to write this call's layout, and,
// when the key is the previous call's, to read that one's -- and returns whether geo_commit may claim them afterwards. The key: everything
// grid_layout and the sample depend on besides the points themselves.
// INVARIANT: from geo_match on the slots are invalid; they become valid in geo_commit, which the build calls only once BOTH launches are enqueued
// (valid[] is set after the sort launch, whose first blocks write the layout before the next call's kernels run). A build that fails on the way
// returns between the two and so leaves no claim on memory nobody wrote.
template <typename T>
static bool geo_match(pcu_hip_ctx* ctx, const GridIndex<T>& a, const GridIndex<T>& b, bool shared, Build2Side<T>& s0, Build2Side<T>& s1) {
    static const bool geo_off = getenv("PCU_HIP_NO_GEO_CACHE") != nullptr;
    if (geo_off || !ctx->geo.dev || a.n < kPrepSamples || b.n < kPrepSamples) return false;
    pcu_hip_ctx::GeoCache& gc = ctx->geo;
    const double occa = a.occ_built, occb = b.occ_built;
    const bool hit = gc.valid[0] && gc.valid[1] && gc.n[0] == a.n && gc.n[1] == b.n && gc.occ == occa && occa == occb && gc.h_want == a.h_want && a.h_want == b.h_want &&
                     gc.max_cells == a.max_cells && a.max_cells == b.max_cells && gc.shared == shared && gc.n_layout == s0.n_layout && gc.tsize == (int)sizeof(T);
    static_assert(sizeof(GridGeo<T>) <= 256, "two layouts fit the context's block");
    GridGeo<T>* const g0 = reinterpret_cast<GridGeo<T>*>(gc.dev), *const g1 = reinterpret_cast<GridGeo<T>*>(gc.dev + 256);
    s0.geo_out = g0; s1.geo_out = g1;
    if (hit) { s0.geo_in = g0; s1.geo_in = g1; }
    DEBUG_SKEW("[layout] handed down: %d (n %d %d, shared %d)\n", (int)hit, a.n, b.n, (int)shared);
    gc.valid[0] = gc.valid[1] = false;
    gc.n[0] = a.n; gc.n[1] = b.n; gc.occ = occa; gc.h_want = a.h_want; gc.max_cells = a.max_cells; gc.shared = shared; gc.n_layout = s0.n_layout; gc.tsize = (int)sizeof(T);
    return occa == occb && a.h_want == b.h_want && a.max_cells == b.max_cells;
}
static void geo_commit(pcu_hip_ctx* ctx) { ctx->geo.valid[0] = ctx->geo.valid[1] = true; }

template <typename T>
static int index_build_staged(GridIndex<T>& a, GridIndex<T>* b, hipStream_t s, const BuildOpts& o, int pts) {
    pcu_hip_ctx* const ctx = o.ctx;
    unsigned long long* const fw = ctx->fill2 + (size_t)ctx->fill_parity * kFillWords;
    const int bpts = kBkThreads * pts;
    const int nbcap = (std::max(a.nb_max, b ? b->nb_max : 0) + 63) / 64 * 64;
    Build2Args<T> sa;
    Build2Side<T>& s0 = sa.a[0], &s1 = sa.a[1];
    build2_side(s0, a, 0, bpts, fw);
    s0.zero_next = ctx->fill2 + (size_t)(ctx->fill_parity ^ 1) * kFillWords; s0.n_zero_next = kFillWords;       // (side 0 zeroes for both)
    s0.zero2 = (unsigned*)o.zero2; s0.n_zero2 = o.n_zero2;
    if (b) build2_side(s1, *b, 1, bpts, fw); else s1 = s0;
    // one grid for both clouds (GridIndex::shared_grid): same plan (index_alloc's PlanFor), same occupancy, both at least a sample large
    const bool shared = b && a.shared_grid && b->shared_grid && a.occ_built == b->occ_built && a.max_cells == b->max_cells && a.shift == b->shift && a.nb_max == b->nb_max &&
                        a.h_want == b->h_want && a.n >= kPrepSamples && b->n >= kPrepSamples;
    if (b) a.shared_grid = b->shared_grid = shared; else a.shared_grid = false;
    if (shared) {
        s0.spts0 = s1.spts0 = a.src; s0.sn0 = s1.sn0 = a.n; s0.spts1 = s1.spts1 = b->src; s0.sn1 = s1.sn1 = b->n;
        s0.n_layout = s1.n_layout = std::max(a.n, b->n);
    }
    const bool geo_arm = o.keep_layout && b && geo_match(ctx, a, *b, shared, s0, s1);
    const int c0 = s0.n_xpart, c1 = b ? s1.n_xpart : 0;
    static StageTimer prof("PCU_HIP_PROF_BUILD2", 16);         // k_bucket_onepass3, then k_bucket_sort2
    if (int rc = prof.arm(s)) return rc;
    s0.prof = s1.prof = prof.arg();
    static std::atomic<unsigned long long> attr_set2[2];
    if (attr_unset_here(attr_set2[sizeof(T) == 4 ? 0 : 1])) {
        if (StagedPts<T>::n >= 8) HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void*>(&k_bucket_onepass3<T, 8>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)onepass3_lds_bytes<T>(8)));
        HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void*>(&k_bucket_onepass3<T, 4>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)onepass3_lds_bytes<T>(4)));
        HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void*>(&k_bucket_onepass3<T, 2>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)onepass3_lds_bytes<T>(2)));
        HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void*>(&k_bucket_sort2<T>), hipFuncAttributeMaxDynamicSharedMemorySize,
                                    (int)bucket_sort_lds_bytes<T>(kBkMaxCellsPerBucket)));
    }
    const size_t lds1 = onepass3_lds_bytes<T>(pts, nbcap);
    if (pts == 8) hipLaunchKernelGGL((k_bucket_onepass3<T, 8>), dim3(c0 + c1), dim3(kBkThreads), lds1, s, sa, c0, nbcap);
    else if (pts == 4) hipLaunchKernelGGL((k_bucket_onepass3<T, 4>), dim3(c0 + c1), dim3(kBkThreads), lds1, s, sa, c0, nbcap);
    else hipLaunchKernelGGL((k_bucket_onepass3<T, 2>), dim3(c0 + c1), dim3(kBkThreads), lds1, s, sa, c0, nbcap);
    if (int rc = prof.report(s, "onepass3", 15, {"layout", "points in", "keys+ranks", "scan+reservations", "staging", "run copies", "drain"})) return rc;
    const int t0 = a.nb_max, t1 = b ? b->nb_max : 0;
    const int cnt_cap = 1 << std::max(a.shift, b ? b->shift : 0);
    if (int rc = prof.arm(s)) return rc;
    hipLaunchKernelGGL(k_bucket_sort2<T>, dim3(t0 + t1 + (b ? 2 : 1)), dim3(kSortThreads), bucket_sort_lds_bytes<T>(cnt_cap), s, sa, t0, t1, cnt_cap, b ? 2 : 1);
    // Fill-word parity (grid2.h "no memset"): this build used set fill_parity, left zeroed by its predecessor, and its scatter zeroes the other
    // set for its successor. INVARIANT: the flip comes only now, when both launches are enqueued, so the other set WILL be zeroed for the next
    // build; an error return above leaves the parity alone.
    ctx->fill_parity ^= 1;
    if (int rc = prof.report(s, "sort2", 7, {"head", "load+rank", "scan", "place", "copies", "drain"})) return rc;
    HIP_TRY(hipGetLastError());
    if (geo_arm) geo_commit(ctx);
    return 0;
}

// ------------------------------------------------------------------------------------------------ bucketed forms
// Placement of the records of over-full buckets (grid.h): one launch for up to two indexes built back to back.
template <typename T>
static void index_large_pass(const GridIndex<T>& a, const GridIndex<T>* b, hipStream_t s) {
    const bool ua = a.bucketed, ub = b && b->bucketed;
    if (!ua && !ub) return;
    const LargeJob<T> ja = large_job(ua ? a : *b), jb = large_job(ua && ub ? *b : (ua ? a : *b));
    hipLaunchKernelGGL(k_bucket_large<T>, dim3(4 * kBboxBlocks), dim3(kBlock), 0, s, ja, jb, (ua && ub) ? 2 : 1);        // (grid-strided; 256 blocks left the chip three quarters empty: 111 us on a Gaussian cloud)
    // every record is placed now: searches may use the index (GridParams::has_large)
    if (ua) (void)hipMemsetAsync(reinterpret_cast<char*>(a.gp) + offsetof(GridParams<T>, has_large), 0, sizeof(int), s);
    if (ub) (void)hipMemsetAsync(reinterpret_cast<char*>(b->gp) + offsetof(GridParams<T>, has_large), 0, sizeof(int), s);
}
// The bucket passes of the bucketed clouds among a (and b): first-form one-pass or two-pass scatter, then the sort both share. Bucketed sides
// share their launches; a side too small / too coarse for buckets takes the atomic passes (index_build_pair).
template <typename T>
static int index_build_bucketed(const GridIndex<T>& a, const GridIndex<T>* b, hipStream_t s, const BuildOpts& o) {
    const GridIndex<T>* bs[2]; int nbs = 0;
    if (a.bucketed) bs[nbs++] = &a;
    if (b && b->bucketed) bs[nbs++] = b;
    if (!nbs) return 0;
    const BucketSide<T> s0 = bucket_side(*bs[0]), s1 = nbs > 1 ? bucket_side(*bs[1]) : s0;
    const int c0 = (bs[0]->n + kBkBlockPts - 1) / kBkBlockPts, c1 = nbs > 1 ? (bs[1]->n + kBkBlockPts - 1) / kBkBlockPts : 0;
    static StageTimer prof_onepass("PCU_HIP_PROF_BUILD", 8), prof_sort("PCU_HIP_PROF_BUILD", 8);         // k_bucket_onepass, k_bucket_sort
    if (int rc = prof_sort.arm(s)) return rc;
    const bool one_pass = bs[0]->one_pass;
    if (one_pass) {
        if (int rc = prof_onepass.arm(s)) return rc;
        // (the grid sides in the order of the bucket sides: both clouds are bucketed whenever two are built this way)
        hipLaunchKernelGGL(k_bucket_onepass<T>, dim3(c0 + c1), dim3(kBkThreads), 0, s, s0, s1, c0, prof_onepass.arg(), grid_side(*bs[0]), grid_side(*bs[nbs - 1]));
        if (int rc = prof_onepass.report(s, "onepass", 7, {"zero+loads", "keys+LDS ranks", "slot reservations", "stores"})) return rc;
    }
    else {
        hipLaunchKernelGGL(k_bucket_count<T>, dim3(c0 + c1), dim3(kBkThreads), 0, s, s0, s1, c0);
        hipLaunchKernelGGL(k_bucket_scatter<T>, dim3(c0 + c1), dim3(kBkThreads), 0, s, s0, s1, c0);
    }
    const int t0 = bs[0]->nb_max, t1 = nbs > 1 ? bs[1]->nb_max : 0;
    const int cnt_cap = 1 << std::max(bs[0]->shift, nbs > 1 ? bs[1]->shift : 0);
    const size_t lds = bucket_sort_lds_bytes<T>(cnt_cap);
    static std::atomic<unsigned long long> attr_set[2];
    if (attr_unset_here(attr_set[sizeof(T) == 4 ? 0 : 1]))
        HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void*>(&k_bucket_sort<T>), hipFuncAttributeMaxDynamicSharedMemorySize,
                                    (int)bucket_sort_lds_bytes<T>(kBkMaxCellsPerBucket)));
    // One launch for both clouds, like the other passes (1024 threads / 4096-point buckets: all blocks of both clouds are
    // resident at once; measured 0.174 vs 0.186 ms per step against one launch per cloud).
    hipLaunchKernelGGL(k_bucket_sort<T>, dim3(t0 + t1), dim3(kSortThreads), lds, s, s0, s1, t0, prof_sort.arg(), cnt_cap);
    if (int rc = prof_sort.report(s, "bucket_sort", 7, {"head", "zero+sync", "load+rank", "scan", "place"})) return rc;
    if (!o.defer_large && !one_pass) index_large_pass<T>(a, b, s);        // (a one-pass build has no over-full buckets: it overflows instead)
    return 0;
}

// ------------------------------------------------------------------------------------------------ atomic form
// Count, scan, scatter over a grid that is laid out and whose counts are zero. closed: a sub-box level (only the points inside the box are indexed).
template <typename T>
static void index_atomic_passes(const GridIndex<T>& g, const T* d_pts, hipStream_t s, bool closed = false) {
    const int n = g.n, nb = (n + kBlock - 1) / kBlock;
    hipLaunchKernelGGL(k_count<T>, dim3(nb), dim3(kBlock), 0, s, d_pts, n, g.gp, g.cell_of, g.rank, g.cell_start);
    hipLaunchKernelGGL(k_scan_reduce<T>, dim3(g.scan_blocks), dim3(kBlock), 0, s, g.cell_start, g.gp, g.block_sums);
    hipLaunchKernelGGL(k_scan_apply<T>, dim3(g.scan_blocks), dim3(kBlock), 0, s, g.cell_start, g.gp, g.block_sums, closed ? 0xffffffffu : (unsigned)n);
    hipLaunchKernelGGL(k_scatter<T>, dim3(nb), dim3(kBlock), 0, s, d_pts, n, g.cell_of, g.rank, g.cell_start, g.sorted);
}

// ------------------------------------------------------------------------------------------------ the build
// Enqueue the build of one or two indexes on `s`: every pass is ONE launch serving both clouds (grid.h: blocks [0, nb0)
// work on the first, the rest on the second). No memset, no host synchronisation.
template <typename T>
static int index_build_pair(GridIndex<T>& a, const T* pa, double occa, GridIndex<T>* b, const T* pb, double occb, hipStream_t s, const BuildOpts& o = BuildOpts()) {
    a.src = pa; a.occ_built = occa;
    if (b) { b->src = pb; b->occ_built = occb; index_same_form(a, *b); }
    const BuildChoice ch = index_build_choose(a, b, o.ctx);
    if (ch.form[0] == BuildForm::Staged) return index_build_staged(a, b, s, o, ch.pts);
    a.lean = false; if (b) b->lean = false;            // (every other build writes the Pt4 records)
    a.shared_grid = false; if (b) b->shared_grid = false;      // (... and lays every cloud over its own grid)
    const BboxSide<T> x0 = bbox_side(a, o.zero2, o.n_zero2), x1 = b ? bbox_side(*b, nullptr, 0) : x0;
    hipLaunchKernelGGL(k_bbox_partial<T>, dim3(b ? 2 * kBboxBlocks : kBboxBlocks), dim3(kBlock), 0, s, x0, x1, kBboxBlocks);
    if (!ch.grid_in_scatter) hipLaunchKernelGGL(k_make_grid<T>, dim3(b ? 2 : 1), dim3(kBlock), 0, s, grid_side(a), grid_side(b ? *b : a));
    if (int rc = index_build_bucketed(a, b, s, o)) return rc;
    if (!a.bucketed) index_atomic_passes(a, pa, s);
    if (b && !b->bucketed) index_atomic_passes(*b, pb, s);
    HIP_TRY(hipGetLastError());
    return 0;
}
template <typename T>
static int index_build(GridIndex<T>& g, const T* d_pts, double occ, hipStream_t s, const BuildOpts& o = BuildOpts()) {
    return index_build_pair<T>(g, d_pts, occ, nullptr, nullptr, 0.0, s, o);
}

// ------------------------------------------------------------------------------------------------ refitted grids
// Refitted grids for unbalanced clouds (grid.h): core range of the cloud by three zooming histogram rounds, then
// uniform grids of a chosen cell count over that range. Everything is enqueued on `s` (no host sync).
template <typename T>
static int core_range_enqueue(Arena& ar, const GridIndex<T>& base, const T* d_pts, hipStream_t s, QuantState<T>** out_qs) {
    QuantState<T>* qs = nullptr; unsigned *partial = nullptr, *hist = nullptr;
    if (aalloc(ar, &qs, 1) || aalloc(ar, &partial, (size_t)kHistBlocks * 3 * (kHistBins + 2)) || aalloc(ar, &hist, 3 * (kHistBins + 2))) return -1;
    hipLaunchKernelGGL(k_quant_init<T>, dim3(1), dim3(64), 0, s, base.gp, qs);
    for (int r = 0; r < 3; ++r) {
        hipLaunchKernelGGL(k_hist_axis<T>, dim3(kHistBlocks), dim3(kBlock), 0, s, d_pts, base.n, qs, partial);
        hipLaunchKernelGGL(k_hist_merge, dim3((3 * (kHistBins + 2) + kBlock - 1) / kBlock), dim3(kBlock), 0, s, partial, kHistBlocks, hist);
        hipLaunchKernelGGL(k_quant_zoom<T>, dim3(3), dim3(64), 0, s, qs, hist, base.n);
    }
    HIP_TRY(hipGetLastError());
    *out_qs = qs;
    return 0;
}
template <typename T>
static int index_build_refit(Arena& ar, GridIndex<T>& g, const GridIndex<T>& base, const T* d_pts, const QuantState<T>* qs,
                             double target_cells, hipStream_t s, bool closed = false, const double* target_dev = nullptr) {
    // closed: sub-box level (only the points inside the box are indexed); target_dev: cell count decided on the device
    const int n = base.n;
    if (target_cells < 1.0) target_cells = 1.0;
    if (index_alloc(ar, g, n, (double)n / target_cells, IndexFor::Atomic)) return -1;
    hipLaunchKernelGGL(k_make_grid_refit<T>, dim3(1), dim3(64), 0, s, g.gp, base.gp, qs, target_cells, g.max_cells, g.sorted + n, n,
                       closed ? 1 : 0, target_dev);
    HIP_TRY(hipMemsetAsync(g.cell_start, 0, ((size_t)g.max_cells + 1) * 4, s));
    index_atomic_passes(g, d_pts, s, closed);
    HIP_TRY(hipGetLastError());
    return 0;
}
// Sub-box level over the heavy cells of `parent` (cells holding more than `thresh` points): enqueue only.
template <typename T>
static int index_build_heavy(Arena& ar, GridIndex<T>& g, const GridIndex<T>& parent, const T* d_pts, double occ, unsigned thresh, hipStream_t s,
                             const double** stats_dev = nullptr) {
    // stats_dev: device pair {cell count chosen for the level, number of points in heavy cells of the parent}
    QuantState<T>* qs = nullptr; T* pbox = nullptr; double *pcnt = nullptr, *target = nullptr;
    if (aalloc(ar, &qs, 1) || aalloc(ar, &pbox, (size_t)kBboxBlocks * 6) || aalloc(ar, &pcnt, (size_t)kBboxBlocks * 2) || aalloc(ar, &target, 2)) return -1;
    // (a bucketed parent keeps no per-point cell ids -- its cell_of storage is the row -> slot table -- the kernel recomputes them)
    hipLaunchKernelGGL(k_heavy_partial<T>, dim3(kBboxBlocks), dim3(kBlock), 0, s, d_pts, parent.n, parent.gp, parent.bucketed ? nullptr : parent.cell_of,
                       parent.cell_start, thresh, pbox, pcnt);
    hipLaunchKernelGGL(k_heavy_finish<T>, dim3(1), dim3(64), 0, s, parent.gp, pbox, pcnt, kBboxBlocks, occ, 16.0 * 1024 * 1024, qs, target);
    if (stats_dev) *stats_dev = target;
    return index_build_refit(ar, g, parent, d_pts, qs, (double)parent.n / occ, s, /*closed=*/true, target);
}
