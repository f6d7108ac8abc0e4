// csrc/surfel_host.h -- host orchestration of ray_surfel_intersection, RaySurfelIntersector and pointcloud_surfel_geometry (kernels and
// contract: surfel.h). The surfel tree is a MeshIdx whose elements are points (rows (p, A, B)): its handle, its create and its calls go
// through the frames of mesh_host.h (TreeIndex, tree_index_create, tree_call), the rays through mesh_run like the mesh's. Included by
// pcu_hip.hip after pc_winding_host.h.
#pragma once

// An oriented point cloud with radii kept on the GPU as its surfel tree (pcu_hip_surfel_index_*): the TreeIndex of mesh_host.h over points,
// and the table its walk needs.
struct pcu_hip_surfel_index : TreeIndex {
    const void* table = nullptr;  // (subdivs, 2): cos, sin in the scalar type, inside mem
    int subdivs = 0;
};
template <typename T> static size_t surfel_table_bytes(int subdivs) { return align_up((size_t)subdivs * 2 * sizeof(T), 256); }
// head, table, 9 T and a row per point, a box per node
template <typename T>
static size_t surfel_index_bytes(int64_t np, int subdivs) {
    const size_t N = (size_t)np, P = (size_t)leaves_pow2(np, kSurfelLeaf);
    return align_up(sizeof(MeshHead<T>), 256) + surfel_table_bytes<T>(subdivs) + align_up(N * 9 * sizeof(T), 256) + align_up(N * 4, 256) +
           align_up(2 * P * 6 * sizeof(T), 256) + 1024;
}
// the sort and, for host arrays, p, n and r staged
template <typename T>
static size_t surfel_build_bytes(int64_t np, bool on_dev) {
    size_t b = sort_bytes((size_t)np) + 4096;
    if (!on_dev) b += 2 * align_up((size_t)np * 3 * sizeof(T), 256) + align_up((size_t)np * sizeof(T), 256);
    return b;
}
static int surfel_validate(int64_t np, int subdivs) {
    if (subdivs < 4) return fail(PCU_HIP_ERR_INVALID, "Invalid geometry_subdivisions_1 is less than or equal to 4.");     // (the reference's text)
    if (np < 0) return fail(PCU_HIP_ERR_INVALID, "negative number of points");
    return np > kMeshMaxRows ? mesh_row_limit() : 0;
}
static int surfel_refuse(int bad) {
    if (bad & kSurfelBadP) return fail(PCU_HIP_ERR_INVALID, "p must not contain NaN or infinite coordinates");
    if (bad & kSurfelBadN) return fail(PCU_HIP_ERR_INVALID, "n must not contain NaN or infinite coordinates");
    if (bad & kSurfelBadR) return fail(PCU_HIP_ERR_INVALID, "r must not contain NaN or infinite values");
    if (bad & kSurfelBadL) return fail(PCU_HIP_ERR_INVALID, "the length of a normal overflows the scalar type of p");
    if (bad & kSurfelBadV) return fail(PCU_HIP_ERR_INVALID, "surfel vertices overflow the scalar type of p");
    return 0;
}
// The table of the contract, rounded to T once. Waits for the copy: the host array goes with this function.
template <typename T>
static int surfel_table(Arena& ar, hipStream_t s, int subdivs, const T** out) {
    std::vector<T> host((size_t)subdivs * 2);
    for (int j = 0; j < subdivs; ++j) {
        const double a = 6.283185307179586 * j / subdivs;
        host[2 * (size_t)j] = (T)cos(a); host[2 * (size_t)j + 1] = (T)sin(a);
    }
    T* d = nullptr;
    if (aalloc(ar, &d, host.size())) return -1;
    HIP_TRY(hipMemcpyAsync(d, host.data(), host.size() * sizeof(T), hipMemcpyHostToDevice, s));
    HIP_WAIT(s);
    *out = d;
    return 0;
}

// Enqueues the build on s and waits once (the validity flags). `ari` gives the buffers of the index, `ar` the temporaries.
template <typename T>
static int surfel_build(Arena& ari, Arena& ar, hipStream_t s, const T* p, const T* n, const T* r, int64_t np, int subdivs, bool on_dev, MeshIdx<T>& M,
                        const T** table) {
    const T *dp = nullptr, *dn = nullptr, *dr = nullptr;
    if (stage_in(ar, p, np, on_dev, s, &dp) || stage_in(ar, n, np, on_dev, s, &dn) || stage_any(ar, r, (size_t)np, on_dev, s, &dr)) return -1;
    M.nf = (int)np; M.P = leaves_pow2(np, kSurfelLeaf);
    unsigned long long *ka = nullptr, *kb = nullptr; unsigned *ia = nullptr, *ib = nullptr;
    if (aalloc(ari, &M.head, 1) || surfel_table<T>(ari, s, subdivs, table) || aalloc(ari, &M.tri, (size_t)np * 9) || aalloc(ari, &M.face, (size_t)np) ||
        aalloc(ari, &M.box, (size_t)M.P * 12) ||
        aalloc(ar, &ka, (size_t)np) || aalloc(ar, &kb, (size_t)np) || aalloc(ar, &ia, (size_t)np) || aalloc(ar, &ib, (size_t)np)) return -1;
    const unsigned nbp = blocks_for((size_t)np), nbl = blocks_for((size_t)M.P);
    int* d_bad = mesh_head_flag(M.head);
    hipLaunchKernelGGL(k_mesh_head_init<T>, dim3(1), dim3(64), 0, s, M.head);
    if (np > 0) hipLaunchKernelGGL(k_surfel_check<T>, dim3(nbp), dim3(kBlock), 0, s, dp, dn, dr, (int)np, subdivs, *table, M.head);
    else hipLaunchKernelGGL(k_surfel_head_empty<T>, dim3(1), dim3(64), 0, s, M.head);
    hipLaunchKernelGGL(k_mesh_frame<T>, dim3(1), dim3(64), 0, s, M.head);
    HIP_TRY(hipGetLastError());
    if (np > 0) {
        hipLaunchKernelGGL(k_pc_codes<T>, dim3(nbp), dim3(kBlock), 0, s, dp, (int)np, (const MeshHead<T>*)M.head, ka);
        HIP_TRY(hipGetLastError());
        if (own_radix_sort(ar, s, &ka, &kb, &ia, &ib, /*ids_identity=*/true, (int)np, 63)) return -1;
        hipLaunchKernelGGL(k_surfel_gather<T>, dim3(nbp), dim3(kBlock), 0, s, dp, dn, dr, (const unsigned*)ia, (int)np, M.tri, M.face);
    }
    hipLaunchKernelGGL(k_surfel_leaves<T>, dim3(nbl), dim3(kBlock), 0, s, (const T*)M.tri, (int)np, M.P, subdivs, *table, (const MeshHead<T>*)M.head, M.box);
    for (int m = M.P / 2; m >= 1; m /= 2) hipLaunchKernelGGL(k_mesh_refit<T>, dim3(blocks_for((size_t)m)), dim3(kBlock), 0, s, M.box, m);
    HIP_TRY(hipGetLastError());
    int bad = 0;
    if (flag_fetch(s, d_bad, &bad)) return -1;
    HIP_WAIT(s);
    return surfel_refuse(bad);
}

template <typename T>
struct SurfelRaysOp : MeshRaysOp<T> {           // ray_surfel_intersection (src/ray_point_cloud_intersection.cpp:343-384): a point id and t per row
    const T* table; int subdivs;
    using Params = SurfelRays<T>;
    static constexpr int kRows3 = 2;
    static constexpr bool kBary = false;
    void walk(hipStream_t s, SurfelRays<T> a, T* val, int64_t n) const {
        a.o = this->o; a.o_stride = this->o_stride(n); a.d = this->d; a.n = (int)n; a.near = (T)this->ray_near; a.far = (T)this->ray_far; a.out_t = val;
        a.table = table; a.subdivs = subdivs;
        hipLaunchKernelGGL(k_surfel_rays<T>, dim3((unsigned)((n + kMeshBlock - 1) / kMeshBlock)), dim3(kMeshBlock), 0, s, a);
    }
};

// One call, the cloud given (`sf`) or its index (`ix`).
template <typename T> struct SurfelGiven { const T* p; const T* n; const T* r; int64_t np; int subdivs; };
template <typename T>
static int surfel_call(pcu_hip_ctx* c, const SurfelGiven<T>* sf, const pcu_hip_surfel_index* ix, const T* ray_o, int64_t o_rows, const T* ray_d, int64_t n,
                       double ray_near, double ray_far, int64_t* out_pid, T* out_t, unsigned flags, void* stream, pcu_hip_stats* st) {
    if (int rc = tree_index_check<T>(c, ix, sf != nullptr, "surfel index", st)) return rc;
    SurfelRaysOp<T> op{{ray_o, o_rows, ray_d, ray_near, ray_far}, sf ? nullptr : static_cast<const T*>(ix->table), sf ? sf->subdivs : ix->subdivs};
    if (sf) { if (int rc = surfel_validate(sf->np, sf->subdivs)) return rc; }
    if (int rc = op.validate(n)) return rc;
    const size_t given = sf ? surfel_index_bytes<T>(sf->np, sf->subdivs) + surfel_build_bytes<T>(sf->np, flags & PCU_HIP_PTRS_ON_DEVICE) : 0;
    return tree_call<T>(c, flags, stream, st, sf ? nullptr : ix, given, [&](Arena& ar, hipStream_t s, bool on_dev, MeshIdx<T>& built, SurfelRaysOp<T>& op) {
        return surfel_build<T>(ar, ar, s, sf->p, sf->n, sf->r, sf->np, sf->subdivs, on_dev, built, &op.table);
    }, op, n, out_t, out_pid, nullptr);
}

template <typename T>
static int surfel_index_create_impl(pcu_hip_ctx* c, const T* p, const T* n, const T* r, int64_t np, int subdivs, unsigned flags, void* stream,
                                    pcu_hip_surfel_index** out) {
    if (int rc = index_out_begin(c, out)) return rc;
    if (int rc = surfel_validate(np, subdivs)) return rc;
    const bool on_dev = flags & PCU_HIP_PTRS_ON_DEVICE;
    return tree_index_create<T>(c, flags, stream, np, surfel_index_bytes<T>(np, subdivs), surfel_build_bytes<T>(np, on_dev), "surfel index", out,
                                [&](Arena& ari, Arena& ar, hipStream_t s, pcu_hip_surfel_index& h) {
        const T* table = nullptr;
        const int rc = surfel_build<T>(ari, ar, s, p, n, r, np, subdivs, on_dev, tree_idx<T>(&h), &table);
        h.table = table; h.subdivs = subdivs;
        return rc;
    });
}

// pointcloud_surfel_geometry (src/ray_point_cloud_intersection.cpp:321-340): (np (subdivs + 1), 3) vertices in T, (np subdivs, 3) int32 faces
template <typename T>
static int surfel_geometry_impl(pcu_hip_ctx* c, const T* p, const T* n, const T* r, int64_t np, int subdivs, T* out_v, int32_t* out_f, unsigned flags,
                                void* stream, pcu_hip_stats* st) {
    if (!c) return fail(PCU_HIP_ERR_INVALID, "null context");
    if (st) memset(st, 0, sizeof *st);
    if (int rc = surfel_validate(np, subdivs)) return rc;
    if (np * ((int64_t)subdivs + 1) > 0x7fffffffll)
        return fail(PCU_HIP_ERR_INVALID, "surfel geometry with more than 2^31-1 vertices does not fit the int32 faces");
    if (np == 0) return 0;
    const size_t nv = (size_t)np * ((size_t)subdivs + 1), nf = (size_t)np * (size_t)subdivs;
    size_t bytes = surfel_table_bytes<T>(subdivs) + 4096;
    if (!(flags & PCU_HIP_PTRS_ON_DEVICE)) bytes += surfel_build_bytes<T>(np, false) + align_up(nv * 3 * sizeof(T), 256) + align_up(nf * 12, 256);
    return op_run(c, flags, stream, st, bytes, [&](OpFrame& fr) -> int {
        auto& [c, s, on_dev, ar, tm] = fr;
        const T *dp = nullptr, *dn = nullptr, *dr = nullptr, *table = nullptr;
        if (stage_in(ar, p, np, on_dev, s, &dp) || stage_in(ar, n, np, on_dev, s, &dn) || stage_any(ar, r, (size_t)np, on_dev, s, &dr) ||
            surfel_table<T>(ar, s, subdivs, &table)) return -1;
        T* d_v = nullptr; int *d_f = nullptr, *d_bad = nullptr;
        if (flag_word(ar, s, &d_bad) || out_room(ar, on_dev, out_v, nv * 3, &d_v) || out_room(ar, on_dev, out_f, nf * 3, &d_f)) return -1;
        hipLaunchKernelGGL(k_surfel_geometry<T>, dim3(blocks_for((size_t)np)), dim3(kBlock), 0, s, dp, dn, dr, (int)np, subdivs, table, d_v, d_f, d_bad);
        HIP_TRY(hipGetLastError());
        int bad = 0;
        if (flag_fetch(s, d_bad, &bad) || out_give(s, on_dev, out_v, d_v, nv * 3) || out_give(s, on_dev, out_f, d_f, nf * 3)) return -1;
        HIP_WAIT(s);
        if (int rc = surfel_refuse(bad)) return rc;
        if (st) { st->n_queries = np; st->n_passes = 1; }
        return 0;
    });
}
