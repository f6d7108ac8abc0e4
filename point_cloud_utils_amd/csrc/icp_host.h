// csrc/icp_host.h -- host side of register_point_clouds_icp (kernels: icp.h; the contract in numpy: tests/icp_contract.py). Included by pcu_hip.hip
// after knn_impl, aux_reserve and index_create_impl. The loop composes knn_impl as normals_knn_impl does: the call's buffers live in c->aux, which
// survives the search's use of the arena.
//
// The solve is float64 on the host with + - * /, sqrt and comparisons only, every expression written as icp_contract.py writes it: the unit is built
// with -ffp-contract=off and the host target has no FMA, so that C++ and Python round alike.
#pragma once

enum { kIcpConverged = 0, kIcpMaxIterations = 1, kIcpNoCorrespondences = 2, kIcpDegenerate = 3 };     // pcu_hip_icp_result::status
constexpr int kIcpJacobiSweeps = 16;         // icp_contract.py: JACOBI_SWEEPS, and why

struct IcpStep { double R[3][3]; double t[3]; };

static void icp_quat_to_rot(double w, double x, double y, double z, double R[3][3]) {
    const double xx = x * x, yy = y * y, zz = z * z, xy = x * y, xz = x * z, yz = y * z, wx = w * x, wy = w * y, wz = w * z;
    R[0][0] = 1.0 - 2.0 * (yy + zz); R[0][1] = 2.0 * (xy - wz);       R[0][2] = 2.0 * (xz + wy);
    R[1][0] = 2.0 * (xy + wz);       R[1][1] = 1.0 - 2.0 * (xx + zz); R[1][2] = 2.0 * (yz - wx);
    R[2][0] = 2.0 * (xz - wy);       R[2][1] = 2.0 * (yz + wx);       R[2][2] = 1.0 - 2.0 * (xx + yy);
}
// Cyclic Jacobi on a symmetric NxN (4: Horn's solve here; 3: the plane refit of plane_host.h): the pairs of the upper triangle row by row --
// (0,1) (0,2) .. (1,2) .. --, kIcpJacobiSweeps sweeps, a zero entry skipped.
template <int N>
static void jacobi_sym(double A[N][N], double V[N][N]) {
    for (int i = 0; i < N; ++i) for (int k = 0; k < N; ++k) V[i][k] = i == k ? 1.0 : 0.0;
    for (int sweep = 0; sweep < kIcpJacobiSweeps; ++sweep)
        for (int p = 0; p < N; ++p)
            for (int q = p + 1; q < N; ++q) {
                const double apq = A[p][q];
                if (apq == 0.0) continue;
                const double theta = (A[q][q] - A[p][p]) / (2.0 * apq);
                const double den = fabs(theta) + sqrt(theta * theta + 1.0);
                const double t = theta >= 0.0 ? 1.0 / den : -1.0 / den;
                const double c = 1.0 / sqrt(t * t + 1.0), s = t * c;
                for (int k = 0; k < N; ++k) { const double akp = A[k][p], akq = A[k][q]; A[k][p] = c * akp - s * akq; A[k][q] = s * akp + c * akq; }
                for (int k = 0; k < N; ++k) { const double apk = A[p][k], aqk = A[q][k]; A[p][k] = c * apk - s * aqk; A[q][k] = s * apk + c * aqk; }
                A[p][q] = A[q][p] = 0.0;
                for (int k = 0; k < N; ++k) { const double vkp = V[k][p], vkq = V[k][q]; V[k][p] = c * vkp - s * vkq; V[k][q] = s * vkp + c * vkq; }
            }
}
// Point-to-point: Horn's closed form from the 17 sums.
static void icp_horn(const double* S, long long count, IcpStep& D) {
    const double c = (double)count;
    const double *Sp = S + 2, *Sq = S + 5, *Spq = S + 8;
    double mp[3], mq[3], H[3][3];
    for (int a = 0; a < 3; ++a) { mp[a] = Sp[a] / c; mq[a] = Sq[a] / c; }
    for (int a = 0; a < 3; ++a) for (int b = 0; b < 3; ++b) H[a][b] = Spq[3 * a + b] - Sp[a] * mq[b];
    const double Sxx = H[0][0], Sxy = H[0][1], Sxz = H[0][2], Syx = H[1][0], Syy = H[1][1], Syz = H[1][2], Szx = H[2][0], Szy = H[2][1], Szz = H[2][2];
    double N[4][4] = {{(Sxx + Syy) + Szz, Syz - Szy, Szx - Sxz, Sxy - Syx},
                      {Syz - Szy, (Sxx - Syy) - Szz, Sxy + Syx, Szx + Sxz},
                      {Szx - Sxz, Sxy + Syx, (Syy - Sxx) - Szz, Syz + Szy},
                      {Sxy - Syx, Szx + Sxz, Syz + Szy, (Szz - Sxx) - Syy}};
    double V[4][4];
    jacobi_sym<4>(N, V);
    int best = 0;
    for (int i = 1; i < 4; ++i) if (N[i][i] > N[best][best]) best = i;
    const double w = V[0][best], x = V[1][best], y = V[2][best], z = V[3][best];
    const double nrm = sqrt(((w * w + x * x) + y * y) + z * z);
    icp_quat_to_rot(w / nrm, x / nrm, y / nrm, z / nrm, D.R);
    for (int a = 0; a < 3; ++a) D.t[a] = mq[a] - (((D.R[a][0] * mp[0]) + (D.R[a][1] * mp[1])) + (D.R[a][2] * mp[2]));
}
// Point-to-plane: A x = -b by Cholesky from the 30 sums; false when a pivot is not > 0 (NaN included).
static bool icp_plane_step(const double* S, IcpStep& D) {
    double A[6][6], L[6][6] = {}, y[6], x[6];
    const double* b = S + 23;
    int k = 2;
    for (int u = 0; u < 6; ++u) for (int v = u; v < 6; ++v) { A[u][v] = A[v][u] = S[k++]; }
    for (int i = 0; i < 6; ++i)
        for (int j = 0; j <= i; ++j) {
            double s = A[i][j];
            for (int q = 0; q < j; ++q) s = s - L[i][q] * L[j][q];
            if (i == j) { if (!(s > 0.0)) return false; L[i][i] = sqrt(s); }
            else L[i][j] = s / L[j][j];
        }
    for (int i = 0; i < 6; ++i) { double s = -b[i]; for (int q = 0; q < i; ++q) s = s - L[i][q] * y[q]; y[i] = s / L[i][i]; }
    for (int i = 5; i >= 0; --i) { double s = y[i]; for (int q = i + 1; q < 6; ++q) s = s - L[q][i] * x[q]; x[i] = s / L[i][i]; }
    const double hx = x[0] / 2.0, hy = x[1] / 2.0, hz = x[2] / 2.0;
    const double nrm = sqrt(((1.0 + hx * hx) + hy * hy) + hz * hz);
    icp_quat_to_rot(1.0 / nrm, hx / nrm, hy / nrm, hz / nrm, D.R);
    D.t[0] = x[3]; D.t[1] = x[4]; D.t[2] = x[5];
    return true;
}
// M <- D o M (rows 0 .. 2 of the row-major 4x4; row 3 stays 0 0 0 1)
static void icp_compose(const IcpStep& D, double* M) {
    double out[12];
    for (int a = 0; a < 3; ++a) {
        for (int b = 0; b < 3; ++b) out[4 * a + b] = ((D.R[a][0] * M[b]) + (D.R[a][1] * M[4 + b])) + (D.R[a][2] * M[8 + b]);
        out[4 * a + 3] = (((D.R[a][0] * M[3]) + (D.R[a][1] * M[7])) + (D.R[a][2] * M[11])) + D.t[a];
    }
    memcpy(M, out, sizeof out);
}

// The free function's own target index: freed on every way out, after what the call enqueued.
struct IcpOwnIndex {
    pcu_hip_index* p = nullptr; hipStream_t s = nullptr;
    ~IcpOwnIndex() { if (p) { (void)hipStreamSynchronize(s); index_free(p); } }
};

// pidx: the target is an index object's (its grid is used as it is); else `target` (m rows) is indexed once for the call. normals: m rows, or
// null (point-to-point). init: 16 doubles in host memory (row-major 4x4), or null (identity). out: host memory. out_corr: n int64, or null.
// stats: n_queries = n, n_passes = evaluations, n_grid_builds = evaluations (the transformed source's grid, inside the search) + 1 for an own index.
template <typename T>
static int icp_impl(pcu_hip_ctx* c, const T* source, int64_t n, const T* target, int64_t m, const pcu_hip_index* pidx, const T* normals, const double* init,
                    double max_dist, int64_t max_iterations, double tol_fitness, double tol_rmse, pcu_hip_icp_result* out, int64_t* out_corr,
                    unsigned flags, void* stream, pcu_hip_stats* st) {
    if (!c) return fail(PCU_HIP_ERR_INVALID, "null context");
    if (pidx) if (int rc = index_check<T>(c, pidx, &m)) return rc;
    if (int rc = validate_sizes(n, m, "query_points", "dataset_points")) return rc;
    if (!(max_dist >= 0.0)) return fail(PCU_HIP_ERR_INVALID, "Invalid max_correspondence_distance (%g): must not be NaN or negative.", max_dist);
    if (max_iterations < 0) return fail(PCU_HIP_ERR_INVALID, "Invalid max_iterations (%lld): must be an integer of at least 0.", (long long)max_iterations);
    if (!(tol_fitness >= 0.0) || std::isinf(tol_fitness)) return fail(PCU_HIP_ERR_INVALID, "Invalid relative_fitness (%g): must be finite and not negative.", tol_fitness);
    if (!(tol_rmse >= 0.0) || std::isinf(tol_rmse)) return fail(PCU_HIP_ERR_INVALID, "Invalid relative_rmse (%g): must be finite and not negative.", tol_rmse);
    double M[16] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1};
    if (init) {
        bool ok = init[12] == 0.0 && init[13] == 0.0 && init[14] == 0.0 && init[15] == 1.0;
        for (int i = 0; i < 12; ++i) ok = ok && std::isfinite(init[i]);
        if (!ok) return fail(PCU_HIP_ERR_INVALID, "Invalid init_transform: must be a finite (4, 4) matrix with last row [0, 0, 0, 1].");
        memcpy(M, init, 12 * sizeof(double));
    }
    if (!source || (!pidx && !target) || !out) return fail(PCU_HIP_ERR_INVALID, "null source / target / result");
    const bool on_dev = flags & PCU_HIP_PTRS_ON_DEVICE, plane = normals != nullptr;
    hipStream_t s = pick_stream(c, flags, stream);
    if (st) memset(st, 0, sizeof *st);
    IcpOwnIndex own; own.s = s;
    if (!pidx) {
        if (int rc = index_create_impl<T>(c, target, m, 1, flags, stream, &own.p)) return rc;
        pidx = own.p;
    }
    const size_t N = (size_t)n, Mr = (size_t)m;
    const int nsums = plane ? kIcpSumsPlane : kIcpSumsPoint;
    const int nblocks = (int)((N + kIcpRows - 1) / kIcpRows), nfold = (nblocks + 63) / 64;
    auto al = [](size_t v) { return align_up(v, 256); };
    const size_t b_src = al(N * 3 * sizeof(T));
    const size_t need = (on_dev ? 0 : b_src + (plane ? al(Mr * 3 * sizeof(T)) : 0)) + b_src + al(N * sizeof(T)) + al(N * 8) +
                        ((out_corr && !on_dev) ? al(N * 8) : 0) + al((size_t)nsums * nblocks * 8) + al((size_t)nsums * nfold * 8) + 2 * 256;
    if (aux_reserve(c, need + 4096)) return PCU_HIP_ERR_RUNTIME;
    char* cur = c->aux;
    auto take = [&](size_t bytes) { char* r = cur; cur += al(bytes); return r; };
    const T* d_src = source; const T* d_nrm = normals;
    if (!on_dev) {
        T* t = (T*)take(N * 3 * sizeof(T)); HIP_TRY(hipMemcpyAsync(t, source, N * 3 * sizeof(T), hipMemcpyHostToDevice, s)); d_src = t;
        if (plane) { T* u = (T*)take(Mr * 3 * sizeof(T)); HIP_TRY(hipMemcpyAsync(u, normals, Mr * 3 * sizeof(T), hipMemcpyHostToDevice, s)); d_nrm = u; }
    }
    T* d_p = (T*)take(N * 3 * sizeof(T));
    T* d_d2 = (T*)take(N * sizeof(T));
    long long* d_j = (long long*)take(N * 8);
    long long* d_corr = reinterpret_cast<long long*>(out_corr);
    if (out_corr && !on_dev) d_corr = (long long*)take(N * 8);
    double* d_part = (double*)take((size_t)nsums * nblocks * 8);
    double* d_part2 = (double*)take((size_t)nsums * nfold * 8);
    IcpRecord* d_rec = (IcpRecord*)take(sizeof(IcpRecord));
    int* d_flags = (int*)take(sizeof(int));
    HIP_TRY(hipMemsetAsync(d_flags, 0, sizeof(int), s));
    const unsigned kflags = (flags | PCU_HIP_PTRS_ON_DEVICE | PCU_HIP_SQUARED | PCU_HIP_STREAM_GIVEN) & ~(unsigned)(PCU_HIP_TIME_PHASES | PCU_HIP_TIME_KERNELS);
    const T rt = (T)max_dist;
    IcpSumsArgs<T> a{};
    a.p = d_p; a.d2 = d_d2; a.j = d_j; a.target = static_cast<const T*>(pidx->pts); a.normals = d_nrm; a.m = (long long)m; a.n = (int)n;
    a.r2 = rt * rt;                                                     // one multiply, rounded in T
    a.corr = d_corr; a.part = d_part; a.nblocks = nblocks; a.flags = d_flags;
    IcpRecord rec;
    double fitness = 0.0, rmse = 0.0, prev_fitness = 0.0, prev_rmse = 0.0;
    int64_t it = 0; int evals = 0, status = kIcpConverged;
    for (;;) {
        IcpXform X; memcpy(X.m, M, sizeof X.m);
        hipLaunchKernelGGL(k_icp_transform<T>, dim3((unsigned)((N + 255) / 256)), dim3(256), 0, s, d_src, (int)n, X, d_p);
        HIP_TRY(hipGetLastError());
        pcu_hip_stats kst;
        if (int rc = knn_impl<T>(c, d_p, n, (const T*)nullptr, m, 1, 10, d_d2, (int64_t*)d_j, kflags, (void*)s, &kst, pidx)) return rc;
        if (plane) hipLaunchKernelGGL((k_icp_sums<T, kIcpPlane>), dim3((unsigned)nblocks), dim3(kIcpBlock), 0, s, a);
        else hipLaunchKernelGGL((k_icp_sums<T, kIcpPoint>), dim3((unsigned)nblocks), dim3(kIcpBlock), 0, s, a);
        hipLaunchKernelGGL(k_icp_fold, dim3(1), dim3(kIcpBlock), 0, s, d_part, d_part2, nblocks, nsums, (const int*)d_flags, d_rec);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipMemcpyAsync(&rec, d_rec, sizeof rec, hipMemcpyDeviceToHost, s));
        HIP_WAIT(s);                                                    // (a cancel request between two evaluations ends the call here)
        ++evals;
        if (rec.flags & kIcpBadRow) return fail(PCU_HIP_ERR_RUNTIME, "internal: the search returned a row outside the target");
        const long long count = (long long)rec.sums[0];
        fitness = (double)count / (double)n;
        rmse = count ? sqrt(rec.sums[1] / (double)count) : 0.0;
        if (count == 0) { status = kIcpNoCorrespondences; break; }
        if (it > 0 && fabs(fitness - prev_fitness) < tol_fitness && fabs(rmse - prev_rmse) < tol_rmse) { status = kIcpConverged; break; }
        if (it == max_iterations) { status = kIcpMaxIterations; break; }
        IcpStep D;
        if (plane) { if (!icp_plane_step(rec.sums, D)) { status = kIcpDegenerate; break; } }
        else icp_horn(rec.sums, count, D);
        icp_compose(D, M);
        prev_fitness = fitness; prev_rmse = rmse;
        ++it;
    }
    if (out_corr && !on_dev) {
        HIP_TRY(hipMemcpyAsync(out_corr, d_corr, N * 8, hipMemcpyDeviceToHost, s));
        HIP_WAIT(s);
    }
    memcpy(out->transform, M, sizeof M);
    out->fitness = fitness; out->inlier_rmse = rmse; out->iterations = it; out->status = status; out->n_evaluations = evals;
    if (st) { st->n_queries = n; st->n_passes = evals; st->n_grid_builds = evals + (own.p ? 1 : 0); }
    return 0;
}
