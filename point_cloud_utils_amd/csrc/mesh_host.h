// csrc/mesh_host.h -- host orchestration of closest_points_on_mesh, ray_mesh_intersection (kernels, contracts and index layout: mesh.h),
// triangle_soup_fast_winding_number and signed_distance_to_mesh (mesh_winding.h), and the frames of every index that is an element tree
// (TreeIndex, tree_index_create, tree_index_check, tree_call), which pc_winding_host.h and surfel_host.h use too. Included by pcu_hip.hip
// after the operator frame (op_run, stage_any, stage_faces, out_room / out_give, the flag word's helpers, index_out_begin) and voxel_host.h (sort_bytes, the radix sort).
#pragma once

// An element tree kept on the GPU as a search index: one block owned by the object, not by a call's arena. The three handle types of the ABI
// (the mesh's here, the dipole tree's in pc_winding_host.h, the surfel tree's in surfel_host.h) are this record under their own names.
struct TreeIndex {
    int elem_size = 0;            // 4: float, 8: double
    int device = 0;
    int64_t count = 0;            // faces or points
    void* mem = nullptr;
    MeshIdx<float> m32; MeshIdx<double> m64;
};
template <typename T> static MeshIdx<T>& tree_idx(TreeIndex* p) { if constexpr (sizeof(T) == 4) return p->m32; else return p->m64; }
template <typename T> static const MeshIdx<T>& tree_idx(const TreeIndex* p) { if constexpr (sizeof(T) == 4) return p->m32; else return p->m64; }
template <typename H> static void tree_index_free(H* p) {        // (H: the handle type it was made as)
    if (!p) return;
    if (p->mem) (void)hipFree(p->mem);
    delete p;
}
struct pcu_hip_mesh_index : TreeIndex {};
// the leaves of a tree over `count` elements, `leaf` to a leaf, rounded up to a power of two
static int leaves_pow2(int64_t count, int leaf) {
    const int64_t leaves = (count + leaf - 1) / leaf;
    int P = 1;
    while (P < leaves) P <<= 1;
    return P;
}
// `moments`: with the centres, radii and moments of mesh_winding.h (34 more T per node, about 17 per face)
template <typename T>
static size_t mesh_index_bytes(int64_t nf, bool moments) {
    const size_t N = (size_t)nf, P = (size_t)leaves_pow2(nf, kMeshLeaf);
    size_t b = align_up(sizeof(MeshHead<T>), 256) + align_up(N * 9 * sizeof(T), 256) + align_up(N * 4, 256) + align_up(2 * P * 6 * sizeof(T), 256) + 1024;
    if (moments) b += align_up(2 * P * 4 * sizeof(T), 256) + align_up(2 * P * 30 * sizeof(T), 256);
    return b;
}
static int int_kind_check(int kind) {
    return (kind < 0 || kind > 3) ? fail(PCU_HIP_ERR_INVALID, "kind must be one of PCU_HIP_FACE_INT32 / INT64 / UINT32 / UINT64") : 0;
}
template <typename T>
static size_t mesh_build_bytes(int64_t nv, int64_t nf, int f_kind, bool on_dev, bool moments) {
    size_t b = sort_bytes((size_t)nf) + align_up((size_t)nf * 12, 256) + 4096;
    if (moments) b += align_up(2 * (size_t)leaves_pow2(nf, kMeshLeaf) * sizeof(double), 256);      // (the nodes' areas)
    if (!on_dev) b += align_up((size_t)nv * 3 * sizeof(T), 256) + align_up((size_t)nf * 3 * int_kind_bytes(f_kind), 256);
    return b;
}
// the query phase: the sort, the result staging of host output and rows3 staged (n,3) arrays (inputs and barycentrics)
template <typename T>
static size_t mesh_run_bytes(int64_t n, int rows3, bool on_dev) {
    size_t b = sort_bytes((size_t)n) + 4096;
    if (!on_dev) b += rows3 * align_up((size_t)n * 3 * sizeof(T), 256) + align_up((size_t)n * sizeof(T), 256) + align_up((size_t)n * 8, 256);
    return b;
}
static int mesh_row_limit() { return fail(PCU_HIP_ERR_INVALID, "meshes and point clouds with more than 2^27-16 rows are not supported"); }
// validate_mesh (src/common/common.h:133-147) and this package's row limit
static int mesh_validate(int64_t nv, int64_t nf, int64_t np, int f_kind) {
    if (nv <= 0 || nf <= 0)
        return fail(PCU_HIP_ERR_INVALID, "Invalid input mesh with zero elements: v and f must have shape (n, 3) and (m, 3) (n, m > 0). Got v.shape =(%lld, 3), f.shape = (%lld, 3).",
                    (long long)nv, (long long)nf);
    if (np < 0) return fail(PCU_HIP_ERR_INVALID, "negative number of query points");
    if (int_kind_check(f_kind)) return fail(PCU_HIP_ERR_INVALID, "f_kind must be one of PCU_HIP_FACE_INT32 / INT64 / UINT32 / UINT64");
    if (nv > kMeshMaxRows || nf > kMeshMaxRows || np > kMeshMaxRows) return mesh_row_limit();
    return 0;
}

// Enqueues the build on s and waits once (the validity flags). `ari` gives the buffers of the index, `ar` the temporaries. `moments`: the
// expansion data of mesh_winding.h too, bottom-up like the boxes: one launch for the leaves and one per level.
template <typename T>
static int mesh_build(Arena& ari, Arena& ar, hipStream_t s, const T* v, int64_t nv, const void* f, int64_t nf, int f_kind, bool on_dev, bool moments,
                      MeshIdx<T>& M) {
    const T* dv = nullptr; const char* df = nullptr;
    if (stage_in(ar, v, nv, on_dev, s, &dv) || stage_faces(ar, f, (size_t)nf, f_kind, on_dev, s, &df)) return -1;
    M.nf = (int)nf; M.P = leaves_pow2(nf, kMeshLeaf);
    int* fidx = nullptr;
    if (aalloc(ari, &M.head, 1) || aalloc(ari, &M.tri, (size_t)nf * 9) || aalloc(ari, &M.face, (size_t)nf) || aalloc(ari, &M.box, (size_t)M.P * 12) ||
        aalloc(ar, &fidx, (size_t)nf * 3)) return -1;
    const unsigned nbf = blocks_for((size_t)nf);
    hipLaunchKernelGGL(k_mesh_head_init<T>, dim3(1), dim3(64), 0, s, M.head);
    int* d_bad = mesh_head_flag(M.head);
    hipLaunchKernelGGL(k_mesh_vcheck<T>, dim3(blocks_for((size_t)nv * 3)), dim3(kBlock), 0, s, dv, (long long)nv * 3, d_bad, kMeshBadVertex);
    hipLaunchKernelGGL(k_mesh_faces<T>, dim3(nbf), dim3(kBlock), 0, s, (const void*)df, f_kind, (int)nf, (int)nv, dv, fidx, M.head);
    hipLaunchKernelGGL(k_mesh_frame<T>, dim3(1), dim3(64), 0, s, M.head);
    HIP_TRY(hipGetLastError());
    int bad = 0;
    if (flag_fetch(s, d_bad, &bad)) return -1;
    HIP_WAIT(s);
    if (bad) return mesh_refusal(bad, nv);
    unsigned long long *ka = nullptr, *kb = nullptr; unsigned *ia = nullptr, *ib = nullptr;
    if (aalloc(ar, &ka, (size_t)nf) || aalloc(ar, &kb, (size_t)nf) || aalloc(ar, &ia, (size_t)nf) || aalloc(ar, &ib, (size_t)nf)) return -1;
    hipLaunchKernelGGL(k_mesh_codes<T>, dim3(nbf), dim3(kBlock), 0, s, dv, (const int*)fidx, (int)nf, (const MeshHead<T>*)M.head, ka);
    if (own_radix_sort(ar, s, &ka, &kb, &ia, &ib, /*ids_identity=*/true, (int)nf, 63)) return -1;
    hipLaunchKernelGGL(k_mesh_gather<T>, dim3(nbf), dim3(kBlock), 0, s, dv, (const int*)fidx, (const unsigned*)ia, (int)nf, M.tri, M.face);
    hipLaunchKernelGGL(k_mesh_leaves<T>, dim3(blocks_for((size_t)M.P)), dim3(kBlock), 0, s, (const T*)M.tri, (int)nf, M.P, (const MeshHead<T>*)M.head, M.box);
    for (int m = M.P / 2; m >= 1; m /= 2) hipLaunchKernelGGL(k_mesh_refit<T>, dim3(blocks_for((size_t)m)), dim3(kBlock), 0, s, M.box, m);
    if (moments) {
        double* area = nullptr;
        if (aalloc(ari, &M.ctr, (size_t)M.P * 8) || aalloc(ari, &M.mom, (size_t)M.P * 60) || aalloc(ar, &area, (size_t)M.P * 2)) return -1;
        hipLaunchKernelGGL(k_mesh_mleaves<T>, dim3(blocks_for((size_t)M.P)), dim3(kBlock), 0, s, (const T*)M.tri, (int)nf, M.P, (const T*)M.box, M.ctr, M.mom, area);
        for (int m = M.P / 2; m >= 1; m /= 2)
            hipLaunchKernelGGL(k_mesh_mrefit<T>, dim3(blocks_for((size_t)m)), dim3(kBlock), 0, s, (const T*)M.box, M.ctr, M.mom, area, m);
    }
    HIP_TRY(hipGetLastError());
    return 0;
}

// ---------------------------------------------------------------------------------------------------- the operators
// All answer, per row, with one T (distance / t / w / s) and, unless kFaces is false, one int64 id (a face; surfel_host.h: a point) and,
// unless kBary is false too, three T barycentrics. What differs is
// an Op: its inputs, how many (n,3) arrays a call with host arrays stages (kRows3, inputs and barycentrics), whether it needs the moments of
// mesh_winding.h (kMoments), its checks ahead of the mesh's, the kernel and the bits of the sort key, the walk kernel with its parameters and
// the message of each bit of the flag word.
template <typename T>
struct MeshPointsOp {                           // closest_points_on_mesh (src/closest_point_on_mesh.cpp:25-50)
    const T* p;
    using Params = MeshQuery<T>;
    static constexpr int kRows3 = 2, kKeyBits = 30;
    static constexpr bool kMoments = false, kFaces = true, kBary = true;
    int validate(int64_t) const { return 0; }
    int stage(Arena& ar, hipStream_t s, int64_t n, bool on_dev) { return stage_in(ar, p, n, on_dev, s, &p); }
    void keys(hipStream_t s, int64_t n, const MeshHead<T>* h, unsigned long long* k, int* d_bad) const {
        hipLaunchKernelGGL(k_mesh_qcodes<T>, dim3(blocks_for((size_t)n)), dim3(kBlock), 0, s, p, (int)n, h, k, d_bad);
    }
    void walk(hipStream_t s, MeshQuery<T> a, T* val, int64_t n) const {
        a.p = p; a.np = (int)n; a.out_d = val;
        hipLaunchKernelGGL(k_mesh_closest<T>, dim3((unsigned)((n + kMeshBlock - 1) / kMeshBlock)), dim3(kMeshBlock), 0, s, a);
    }
    static int message(int) { return fail(PCU_HIP_ERR_INVALID, "p must not contain NaN or infinite coordinates"); }
};
template <typename T>
struct MeshRaysOp {                             // ray_mesh_intersection (src/ray_mesh_intersection.cpp:107-177)
    const T* o; int64_t o_rows; const T* d; double ray_near, ray_far;
    using Params = MeshRays<T>;
    static constexpr int kRows3 = 3, kKeyBits = kMeshRayKeyBits;
    static constexpr bool kMoments = false, kFaces = true, kBary = true;
    int validate(int64_t n) const {
        if (n < 0) return fail(PCU_HIP_ERR_INVALID, "negative number of rays");
        if (n > kMeshMaxRows) return mesh_row_limit();
        if (o_rows != 1 && o_rows != n)
            return fail(PCU_HIP_ERR_INVALID, "ray_o and ray_d must have the same number of rows (one ray origin per ray direction). "
                                             "(Note: ray_o can have one row to use the same origin for all directions)");
        if (ray_near != ray_near || ray_far != ray_far) return fail(PCU_HIP_ERR_INVALID, "ray_near and ray_far must not be NaN");
        return 0;
    }
    int o_stride(int64_t n) const { return o_rows == 1 && n != 1 ? 0 : 3; }
    int stage(Arena& ar, hipStream_t s, int64_t n, bool on_dev) { return (stage_in(ar, o, o_rows, on_dev, s, &o) || stage_in(ar, d, n, on_dev, s, &d)) ? -1 : 0; }
    void keys(hipStream_t s, int64_t n, const MeshHead<T>* h, unsigned long long* k, int* d_bad) const {
        hipLaunchKernelGGL(k_mesh_rkeys<T>, dim3(blocks_for((size_t)n)), dim3(kBlock), 0, s, o, o_stride(n), d, (int)n, h, k, d_bad);
    }
    void walk(hipStream_t s, MeshRays<T> a, T* val, int64_t n) const {
        a.o = o; a.o_stride = o_stride(n); a.d = d; a.n = (int)n; a.near = (T)ray_near; a.far = (T)ray_far; a.out_t = val;
        hipLaunchKernelGGL(k_mesh_rays<T>, dim3((unsigned)((n + kMeshBlock - 1) / kMeshBlock)), dim3(kMeshBlock), 0, s, a);
    }
    static int message(int bad) {
        return fail(PCU_HIP_ERR_INVALID, "%s must not contain NaN or infinite coordinates", (bad & kMeshBadOrigin) ? "ray_o" : "ray_d");
    }
};
static int mesh_beta_check(double beta) {
    return beta > 0.0 ? 0 : fail(PCU_HIP_ERR_INVALID, "beta must be greater than 0 (finite, or +inf for the plain sum over all faces)");
}
template <typename T>
struct MeshWindingOp : MeshPointsOp<T> {        // triangle_soup_fast_winding_number (src/fast_winding_numbers.cpp:20-34): one T per row, no face
    double beta;
    using Params = MeshSigned<T>;
    static constexpr int kRows3 = 1;
    static constexpr bool kMoments = true, kFaces = false;
    int validate(int64_t) const { return mesh_beta_check(beta); }
    void walk(hipStream_t s, MeshSigned<T> a, T* val, int64_t n) const {
        a.p = this->p; a.np = (int)n; a.beta = (T)beta; a.out_val = val;
        hipLaunchKernelGGL(k_mesh_winding<T>, dim3((unsigned)((n + kMeshBlock - 1) / kMeshBlock)), dim3(kMeshBlock), 0, s, a);
    }
};
template <typename T>
struct MeshSdfOp : MeshPointsOp<T> {            // signed_distance_to_mesh (src/signed_distance.cpp:22-56)
    double lower, upper, beta;
    using Params = MeshSigned<T>;
    static constexpr bool kMoments = true;
    int validate(int64_t) const {
        if (lower != lower || upper != upper) return fail(PCU_HIP_ERR_INVALID, "lower_bound and upper_bound must not be NaN");
        if (lower > upper) return fail(PCU_HIP_ERR_INVALID, "lower_bound must not be greater than upper_bound");
        return mesh_beta_check(beta);
    }
    void walk(hipStream_t s, MeshSigned<T> a, T* val, int64_t n) const {
        a.p = this->p; a.np = (int)n; a.beta = (T)beta; a.out_val = val;
        a.lower = (T)(float)lower; a.upper = (T)(float)upper;           // (the reference declares the bounds float)
        hipLaunchKernelGGL(k_mesh_sdf<T>, dim3((unsigned)((n + kMeshBlock - 1) / kMeshBlock)), dim3(kMeshBlock), 0, s, a);
    }
};

// Enqueues the rows of one operator and waits for them. Events 1 / 2 of the context bracket the query phase.
template <typename T, typename Op>
static int mesh_run(Arena& ar, hipStream_t s, const MeshIdx<T>& M, Op op, int64_t n, bool on_dev, T* out_val, int64_t* out_fi, T* out_bc, Timer& tm) {
    tm.mark(1);
    if (n == 0) { tm.mark(2); HIP_WAIT(s); return 0; }
    if (op.stage(ar, s, n, on_dev)) return -1;
    int* d_bad = nullptr;
    unsigned long long *ka = nullptr, *kb = nullptr; unsigned *ia = nullptr, *ib = nullptr;
    if (flag_word(ar, s, &d_bad) || aalloc(ar, &ka, (size_t)n) || aalloc(ar, &kb, (size_t)n) || aalloc(ar, &ia, (size_t)n) || aalloc(ar, &ib, (size_t)n)) return -1;
    T *d_val = nullptr, *d_bc = out_bc; long long *const h_fi = reinterpret_cast<long long*>(out_fi), *d_fi = h_fi;
    if (out_room(ar, on_dev, out_val, (size_t)n, &d_val) || (Op::kFaces && (out_room(ar, on_dev, h_fi, (size_t)n, &d_fi) ||
                                                                          (Op::kBary && out_room(ar, on_dev, out_bc, (size_t)n * 3, &d_bc))))) return -1;
    op.keys(s, n, M.head, ka, d_bad);
    if (own_radix_sort(ar, s, &ka, &kb, &ia, &ib, /*ids_identity=*/true, (int)n, Op::kKeyBits)) return -1;
    typename Op::Params a{};
    a.order = ia; a.ix = M; a.out_fi = d_fi; a.out_bc = d_bc;
    a.cancel_word = g_cancel_mirror.load(std::memory_order_relaxed); a.cancel_gen = t_call_gen;
    op.walk(s, a, d_val, n);
    HIP_TRY(hipGetLastError());
    tm.mark(2);
    int bad = 0;
    if (flag_fetch(s, d_bad, &bad) || out_give(s, on_dev, out_val, d_val, (size_t)n) || out_give(s, on_dev, h_fi, d_fi, (size_t)n) ||
        out_give(s, on_dev, out_bc, d_bc, (size_t)n * 3)) return -1;
    HIP_WAIT(s);
    return bad ? Op::message(bad) : 0;
}
static void mesh_stats(pcu_hip_stats* st, Timer& tm, int64_t np, bool built) {
    if (!st) return;
    st->n_queries = np; st->n_passes = 1; st->n_grid_builds = built ? 1 : 0;
    if (built) st->ms_index = tm.span(0, 1);
    st->ms_search = tm.span(1, 2);
    st->ms_total = built ? tm.span(0, 2) : st->ms_search;
}

// ---------------------------------------------------------------------------------------------------- the frames of an index
// The refusals ahead of a call's own: `given`: the structure comes with the call; otherwise the handle `ix` must fit the call and the context.
template <typename T>
static int tree_index_check(pcu_hip_ctx* c, const TreeIndex* ix, bool given, const char* noun, pcu_hip_stats* st) {
    if (!c || !(given || ix)) return given ? fail(PCU_HIP_ERR_INVALID, "null context") : fail(PCU_HIP_ERR_INVALID, "null context / %s", noun);
    if (st) memset(st, 0, sizeof *st);
    if (given) return 0;
    if (ix->elem_size != (int)sizeof(T)) return fail(PCU_HIP_ERR_INVALID, "the %s was built for the other scalar type", noun);
    if (ix->device != c->device) return fail(PCU_HIP_ERR_INVALID, "the %s lives on another device than the context", noun);
    return 0;
}
// One validated call of an operator. Index given (`ix`): rows and temporaries in the call's arena; otherwise `build(ar, s, on_dev, built, op)`
// makes the tree there too, out of `given_bytes` more.
template <typename T, typename Op, typename Build>
static int tree_call(pcu_hip_ctx* c, unsigned flags, void* stream, pcu_hip_stats* st, const TreeIndex* ix, size_t given_bytes, Build build, Op op, int64_t n,
                     T* out_val, int64_t* out_fi, T* out_bc) {
    const size_t bytes = mesh_run_bytes<T>(n, Op::kRows3, flags & PCU_HIP_PTRS_ON_DEVICE) + (ix ? 0 : given_bytes);
    return op_run(c, flags, stream, st, bytes, [&](OpFrame& fr) -> int {
        auto& [c, s, on_dev, ar, tm] = fr;
        MeshIdx<T> built;
        if (!ix) { tm.mark(0); if (int rc = build(ar, s, on_dev, built, op)) return rc; }
        if (int rc = mesh_run<T>(ar, s, ix ? tree_idx<T>(ix) : built, op, n, on_dev, out_val, out_fi, out_bc, tm)) return rc;
        mesh_stats(st, tm, n, !ix);
        return 0;
    });
}
// Makes a handle H over its own block of `index_bytes`, after the caller's index_out_begin and validation: `build(ari, ar, s, h)` enqueues
// into the block (`ari`) with temporaries from the context (`ar`, `build_bytes`). A failure of any kind leaves no handle behind.
template <typename T, typename H, typename Build>
static int tree_index_create(pcu_hip_ctx* c, unsigned flags, void* stream, int64_t count, size_t index_bytes, size_t build_bytes, const char* noun, H** out,
                             Build build) {
    hipStream_t s = pick_stream(c, flags, stream);
    H* h = new H();
    h->elem_size = (int)sizeof(T); h->device = c->device; h->count = count;
    if (hipMalloc(&h->mem, index_bytes) != hipSuccess) { h->mem = nullptr; tree_index_free(h); return fail(PCU_HIP_ERR_RUNTIME, "out of device memory for the %s", noun); }
    if (ctx_begin(c, build_bytes)) { tree_index_free(h); return PCU_HIP_ERR_RUNTIME; }
    ArenaState blk;                                 // a bump allocator over the index's own block
    blk.base = static_cast<char*>(h->mem); blk.cap = index_bytes;
    Arena ari{&blk}, ar{c};
    int rc = build(ari, ar, s, *h);
    if (!rc) rc = wait_stream(s);                   // (the temporaries go back to the context with this call)
    rc = attempt_exit(c, index_block_exit(blk, rc, noun));
    if (rc) { (void)hipStreamSynchronize(s); tree_index_free(h); return rc; }
    *out = h;
    return 0;
}

// One call of a mesh operator, the mesh given (`mesh`) or its index (`ix`).
template <typename T> struct MeshGiven { const T* v; int64_t nv; const void* f; int64_t nf; int f_kind; };
template <typename T, typename Op>
static int mesh_call(pcu_hip_ctx* c, const MeshGiven<T>* mesh, const pcu_hip_mesh_index* ix, Op op, int64_t n, T* out_val, int64_t* out_fi, T* out_bc,
                     unsigned flags, void* stream, pcu_hip_stats* st) {
    if (int rc = tree_index_check<T>(c, ix, mesh != nullptr, "mesh index", st)) return rc;
    if (!mesh && Op::kMoments && !tree_idx<T>(ix).mom) return fail(PCU_HIP_ERR_INVALID, "the mesh index was created without PCU_HIP_MESH_MOMENTS");
    if (int rc = op.validate(n)) return rc;
    if (mesh) { if (int rc = mesh_validate(mesh->nv, mesh->nf, n, mesh->f_kind)) return rc; }
    else if (n < 0 || n > kMeshMaxRows) return mesh_row_limit();
    const bool on_dev = flags & PCU_HIP_PTRS_ON_DEVICE;
    const size_t given = mesh ? mesh_index_bytes<T>(mesh->nf, Op::kMoments) + mesh_build_bytes<T>(mesh->nv, mesh->nf, mesh->f_kind, on_dev, Op::kMoments) : 0;
    return tree_call<T>(c, flags, stream, st, mesh ? nullptr : ix, given, [&](Arena& ar, hipStream_t s, bool on_dev, MeshIdx<T>& built, Op&) {
        return mesh_build<T>(ar, ar, s, mesh->v, mesh->nv, mesh->f, mesh->nf, mesh->f_kind, on_dev, Op::kMoments, built);
    }, op, n, out_val, out_fi, out_bc);
}

template <typename T>
static int mesh_index_create_impl(pcu_hip_ctx* c, const T* v, int64_t nv, const void* f, int64_t nf, int f_kind, unsigned flags, void* stream,
                                  pcu_hip_mesh_index** out) {
    if (int rc = index_out_begin(c, out)) return rc;
    if (int rc = mesh_validate(nv, nf, 0, f_kind)) return rc;
    const bool on_dev = flags & PCU_HIP_PTRS_ON_DEVICE, moments = flags & PCU_HIP_MESH_MOMENTS;
    return tree_index_create<T>(c, flags, stream, nf, mesh_index_bytes<T>(nf, moments), mesh_build_bytes<T>(nv, nf, f_kind, on_dev, moments), "mesh index", out,
                                [&](Arena& ari, Arena& ar, hipStream_t s, pcu_hip_mesh_index& h) {
        return mesh_build<T>(ari, ar, s, v, nv, f, nf, f_kind, on_dev, moments, tree_idx<T>(&h));
    });
}
