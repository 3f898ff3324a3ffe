// svds: the k largest singular triplets of a sparse or a dense matrix by thick-restart
// Golub-Kahan-Lanczos bidiagonalisation from bases of m <= 64 vectors (algorithm:
// include/eigsol_hip.h).  The driver reaches the matrix through LinearOp (linear_op.hpp): y = A x by
// the single-vector SpMV / GEMV, y = A^H x by the SpMV of the adjoint handle (eigsol_csr_adjoint,
// below) or by the dense adjoint kernel (dense_adjoint.hip).
//
// A is M x N.  V is N x (m + 1) and U is M x m on the device, column-major, in the matrix dtype, with
// columns on 16-byte boundaries; the projected matrix B (m x m, upper triangular: the bidiagonal of
// the cycle's own steps beside the diagonal and the spike column a thick restart leaves) is kept on
// the host.  Per step the host enqueues the two products and two orthogonalisation steps
// (krylov_orth.hpp: classical Gram-Schmidt with one reorthogonalisation, against all of U for
// u_j and all of V for v_{j+1}) and waits for nothing; a cycle's one wait reads the columns of B, the
// betas and the breakdown word.  The small SVD of B runs on the host (small_svd.hpp); the bases are
// rotated in place by ks_mul_kernel.  No floating-point atomics anywhere: two runs give equal bits.
//
// Out of scope: the smallest or interior singular values, block Lanczos, single precision,
// double-double, row-sharded matrices, a session / step form and matrix-free operators.
#include <algorithm>
#include <cmath>
#include <complex>
#include <cstring>

#include "kernels_common.hpp"
#include "krylov_orth.hpp"
#include "linear_op.hpp"
#include "scratch.hpp"
#include "small_eig.hpp"
#include "small_svd.hpp"

namespace eigsol {

namespace dev {

__device__ __forceinline__ double svds_scale(double x, double r) { return x * r; }
__device__ __forceinline__ cplx svds_scale(cplx x, double r) { return cplx{x.re * r, x.im * r}; }

// npart[blockIdx] = the workgroup's partial of ||y - sigma x||^2
template <class S>
__global__ __launch_bounds__(kThreads) void svds_resid_kernel(const S* __restrict__ y, const S* __restrict__ x,
                                                              double sigma, int64_t n, double* __restrict__ npart) {
    __shared__ double sm[kWaves];
    double a2 = 0.0;
    const int64_t stride = (int64_t)gridDim.x * kThreads;
    for (int64_t r = (int64_t)blockIdx.x * kThreads + threadIdx.x; r < n; r += stride)
        a2 += sq_abs(sub(y[r], svds_scale(x[r], sigma)));
    a2 = ks::block_sum_all(a2, sm);
    if (threadIdx.x == 0) npart[blockIdx.x] = a2;
}

// out[0] = the sum of npart in a fixed order (one workgroup)
__global__ __launch_bounds__(kThreads) void svds_sum_kernel(const double* __restrict__ npart, int nparts,
                                                            double* __restrict__ out) {
    __shared__ double sm[kWaves];
    double s = 0.0;
    for (int g = threadIdx.x; g < nparts; g += kThreads) s += npart[g];
    s = ks::block_sum_all(s, sm);
    if (threadIdx.x == 0) out[0] = s;
}

}  // namespace dev

namespace {

using smalleig::cd;
using smalleig::host_of;
using smallsvd::jacobi_svd;

template <class S>
int svds_run(LinearOp A, bool build_adjoint, const eigsol_svds_options* o, const void* v0v, double* s_out, void* U_out, void* V_out,
             double* residuals, int32_t* restarts, int32_t* applications, int32_t* converged) {
    using HS = typename host_of<S>::type;
    constexpr bool real = std::is_same_v<S, double>;
    const int64_t M = A.nrows(), N = A.ncols();
    const int m = o->ncv, k = o->nsv;
    eigsol_ctx* ctx = const_cast<eigsol_ctx*>(A.ctx());
    hipStream_t st = ctx->stream;

    // v_0 = v0 / ||v0|| on the host
    const HS* v0 = static_cast<const HS*>(v0v);
    std::vector<HS> v0n(v0, v0 + N);
    {
        double mx = 0.0;
        for (const HS& z : v0n) mx = std::max(mx, std::abs(z));
        double s = 0.0;
        if (mx > 0.0 && std::isfinite(mx))
            for (const HS& z : v0n) s += smallsvd::abs2_s(z / mx);
        const double nrm = mx * std::sqrt(s);
        if (!(nrm > 0.0) || !std::isfinite(nrm)) return fail(EIGSOL_E_INVALID, "svds: v0 has no finite nonzero norm");
        for (HS& z : v0n) z /= nrm;
    }

    EIGSOL_HIP(hipSetDevice(ctx->device));
    struct Owned {   // the adjoint handle of a caller that gave none
        eigsol_csr* h = nullptr;
        ~Owned() {
            if (h) eigsol_csr_destroy(h);
        }
    } own;
    if (build_adjoint) {
        EIGSOL_TRY(eigsol_csr_adjoint(A.csr, &own.h));
        A.csr_h = own.h;
    }
    // columns start on 16-byte boundaries for every M and N
    const int64_t ldu = real ? ((M + 1) & ~(int64_t)1) : M;
    const int64_t ldv = real ? ((N + 1) & ~(int64_t)1) : N;
    const int mb = m + 1, mw = m + 2;   // leading dimensions of the device copies of the steps' columns
    DevBuf vbuf, ubuf, bdev, wdev, qx, qy;
    OrthWs<S> wsU, wsV;
    EIGSOL_TRY(vbuf.alloc((size_t)ldv * (m + 1) * sizeof(S)));
    EIGSOL_TRY(ubuf.alloc((size_t)ldu * m * sizeof(S)));
    EIGSOL_TRY(bdev.alloc((size_t)mb * m * sizeof(S)));
    EIGSOL_TRY(wdev.alloc((size_t)mw * m * sizeof(S)));
    EIGSOL_TRY(qx.alloc((size_t)mb * m * sizeof(S)));
    EIGSOL_TRY(qy.alloc((size_t)mb * m * sizeof(S)));
    EIGSOL_TRY(wsU.alloc(ctx, M, st));
    EIGSOL_TRY(wsV.alloc(ctx, N, st));
    S* V = vbuf.as<S>();
    S* U = ubuf.as<S>();
    S* BD = bdev.as<S>();
    S* WD = wdev.as<S>();
    EIGSOL_HIP(hipMemsetAsync(BD, 0, (size_t)mb * m * sizeof(S), st));
    EIGSOL_HIP(hipMemsetAsync(WD, 0, (size_t)mw * m * sizeof(S), st));
    EIGSOL_HIP(hipMemcpyAsync(V, v0n.data(), (size_t)N * sizeof(S), hipMemcpyHostToDevice, st));

    StageClock T, E;   // T: four marks per step (A, orthogonalisation, A^H, orthogonalisation); E: a restart, the finish
    EIGSOL_TRY(T.start(4 * m));
    EIGSOL_TRY(E.start(1));
    std::vector<double> tms((size_t)4 * m);
    double ms[4] = {0.0, 0.0, 0.0, 0.0};
    bool restart_timed = false;

    std::vector<HS> Bh((size_t)m * m, HS(0)), Bd((size_t)mb * m), Wd((size_t)mw * m), G, X, Y, hlast;
    std::vector<double> sv;
    int32_t hb = 0;
    int p = 0, dl = m, dr = m, apps = 0, cycle = 0;
    bool conv = false;
    const double eps23 = std::pow(0x1p-52, 2.0 / 3.0);
    auto Bat = [&](int i, int j) -> HS& { return Bh[(size_t)j * m + i]; };
    auto finite = [](const HS& z) { return std::isfinite(std::abs(z)); };

    for (cycle = 1; cycle <= o->max_restarts; ++cycle) {
        for (int j = p; j < m; ++j) {                    // expansion: nothing here waits for the device
            S* vj = V + (size_t)j * ldv;
            S* uj = U + (size_t)j * ldu;
            S* vn = V + (size_t)(j + 1) * ldv;
            const int q = 4 * (j - p);
            EIGSOL_TRY(T.mark(q, st));
            EIGSOL_TRY(A.apply(vj, uj));
            EIGSOL_TRY(T.mark(q + 1, st));
            EIGSOL_TRY(orth_step<S>(wsU, U, ldu, j, uj, M, BD + (size_t)j * mb, (double)m, st));
            EIGSOL_TRY(T.mark(q + 2, st));
            EIGSOL_TRY(A.apply_h(uj, vn));
            EIGSOL_TRY(T.mark(q + 3, st));
            EIGSOL_TRY(orth_step<S>(wsV, V, ldv, j + 1, vn, N, WD + (size_t)j * mw, (double)m, st));
        }
        EIGSOL_TRY(T.mark(4 * (m - p), st));
        // the cycle's one host wait: the steps' columns and the breakdown word
        EIGSOL_HIP(hipMemcpyAsync(Bd.data(), BD, Bd.size() * sizeof(S), hipMemcpyDeviceToHost, st));
        EIGSOL_HIP(hipMemcpyAsync(Wd.data(), WD, Wd.size() * sizeof(S), hipMemcpyDeviceToHost, st));
        EIGSOL_HIP(hipMemcpyAsync(&hb, wsV.bword.p, sizeof(hb), hipMemcpyDeviceToHost, st));
        EIGSOL_HIP(stream_wait(st));
        T.read(tms.data(), 4 * (m - p));
        for (int i = 0; i < m - p; ++i) {
            ms[0] += tms[4 * i];
            ms[1] += tms[4 * i + 2];
            ms[2] += tms[4 * i + 1] + tms[4 * i + 3];
        }
        if (restart_timed) {
            double te[1];
            E.read(te, 1);
            ms[3] += te[0];
            restart_timed = false;
        }
        // a breakdown of u_j (alpha) leaves u_j = 0, so the v half of the same step breaks down too:
        // the word of the v halves alone finds the step, alpha_j = 0 tells the two kinds apart
        const int jb = hb ? hb - 1 : m;                  // the step that broke down
        const bool alpha_bd = hb && std::abs(Bd[(size_t)jb * mb + jb]) == 0.0;
        const int full = hb ? (alpha_bd ? jb : jb + 1) : m;   // steps whose u_j is a basis vector
        apps += 2 * (full - p) + (alpha_bd ? 1 : 0);
        for (int j = p; j < full; ++j)
            for (int i = 0; i <= j; ++i) Bat(i, j) = Bd[(size_t)j * mb + i];
        bool fin = true;
        for (int j = 0; j < full; ++j)
            for (int i = 0; i <= j; ++i) fin = fin && finite(Bat(i, j));
        const double beta = hb ? 0.0 : std::abs(Wd[(size_t)(m - 1) * mw + m]);
        if (!fin || !std::isfinite(beta)) return fail(EIGSOL_E_SOLVER, "svds: the projected matrix is not finite");
        if (hb) {
            const int d = full;
            if (d < k)
                return fail(EIGSOL_E_SOLVER, "svds: invariant subspace of dimension " + std::to_string(d) + " < nsv");
            dl = d;
            dr = alpha_bd ? d + 1 : d;
            bool ok;
            if (alpha_bd) {   // [B[:d, :d] | h_j] through its conjugate transpose
                hlast.assign(Bd.begin() + (size_t)jb * mb, Bd.begin() + (size_t)jb * mb + d);
                for (const HS& z : hlast)
                    if (!finite(z)) return fail(EIGSOL_E_SOLVER, "svds: the projected matrix is not finite");
                G.assign((size_t)(d + 1) * d, HS(0));
                for (int c = 0; c < d; ++c) {
                    for (int r = 0; r < d; ++r) G[(size_t)c * (d + 1) + r] = smallsvd::conj_s(Bat(c, r));
                    G[(size_t)c * (d + 1) + d] = smallsvd::conj_s(hlast[c]);
                }
                ok = jacobi_svd<HS>(d + 1, d, G, sv, Y, X);
            } else {
                G.assign((size_t)d * d, HS(0));
                for (int c = 0; c < d; ++c)
                    for (int r = 0; r < d; ++r) G[(size_t)c * d + r] = Bat(r, c);
                ok = jacobi_svd<HS>(d, d, G, sv, X, Y);
            }
            if (!ok) return fail(EIGSOL_E_SOLVER, "svds: the SVD of the projected matrix did not converge");
            conv = true;
            break;
        }
        G = Bh;
        if (!jacobi_svd<HS>(m, m, G, sv, X, Y))
            return fail(EIGSOL_E_SOLVER, "svds: the SVD of the projected matrix did not converge");
        bool all = o->tolerance >= 0.0;
        for (int i = 0; i < k && all; ++i)
            all = beta * std::abs(X[(size_t)i * m + (m - 1)]) <= o->tolerance * std::max(sv[i], eps23 * sv[0]);
        if (all) {
            conv = true;
            break;
        }
        if (cycle == o->max_restarts) break;

        // restart: keep the k leading singular triplets of B (X and Y are next written after the next wait)
        p = k;
        EIGSOL_TRY(E.mark(0, st));
        EIGSOL_HIP(hipMemcpyAsync(qy.p, Y.data(), (size_t)m * p * sizeof(S), hipMemcpyHostToDevice, st));
        EIGSOL_HIP(hipMemcpyAsync(qx.p, X.data(), (size_t)m * p * sizeof(S), hipMemcpyHostToDevice, st));
        EIGSOL_TRY((launch_mul<S, S>(ctx, V, ldv, N, m, p, (const S*)qy.as<S>(), V, ldv, st)));
        EIGSOL_TRY((launch_mul<S, S>(ctx, U, ldu, M, m, p, (const S*)qx.as<S>(), U, ldu, st)));
        EIGSOL_HIP(hipMemcpyAsync(V + (size_t)p * ldv, V + (size_t)m * ldv, (size_t)N * sizeof(S),
                                  hipMemcpyDeviceToDevice, st));
        EIGSOL_TRY(E.mark(1, st));
        restart_timed = true;
        std::fill(Bh.begin(), Bh.end(), HS(0));
        for (int i = 0; i < p; ++i) Bat(i, i) = sv[i];
    }
    if (cycle > o->max_restarts) cycle = o->max_restarts;

    // the triplets of the last decomposition: U_k = U[:, :dl] X_k, V_k = V[:, :dr] Y_k, explicit residuals
    EIGSOL_TRY(E.mark(0, st));
    DevBuf ukb, vkb, yb, outs;
    EIGSOL_TRY(ukb.alloc((size_t)ldu * k * sizeof(S)));
    EIGSOL_TRY(vkb.alloc((size_t)ldv * k * sizeof(S)));
    EIGSOL_TRY(yb.alloc((size_t)std::max(ldu, ldv) * sizeof(S)));
    EIGSOL_TRY(outs.alloc((size_t)2 * k * sizeof(double)));
    S* UK = ukb.as<S>();
    S* VK = vkb.as<S>();
    EIGSOL_HIP(hipMemcpyAsync(qx.p, X.data(), (size_t)dl * k * sizeof(S), hipMemcpyHostToDevice, st));
    EIGSOL_HIP(hipMemcpyAsync(qy.p, Y.data(), (size_t)dr * k * sizeof(S), hipMemcpyHostToDevice, st));
    EIGSOL_TRY((launch_mul<S, S>(ctx, U, ldu, M, dl, k, (const S*)qx.as<S>(), UK, ldu, st)));
    EIGSOL_TRY((launch_mul<S, S>(ctx, V, ldv, N, dr, k, (const S*)qy.as<S>(), VK, ldv, st)));
    const dim3 blk(dev::kThreads);
    for (int c = 0; c < k; ++c) {
        const S* u = UK + (size_t)c * ldu;
        const S* v = VK + (size_t)c * ldv;
        S* y = yb.as<S>();
        EIGSOL_TRY(A.apply(v, y));
        hipLaunchKernelGGL((dev::svds_resid_kernel<S>), dim3(wsU.grid), blk, 0, st, (const S*)y, u, sv[c], M,
                           wsU.npart.template as<double>());
        hipLaunchKernelGGL(dev::svds_sum_kernel, dim3(1), blk, 0, st, (const double*)wsU.npart.template as<double>(), wsU.grid,
                           outs.as<double>() + 2 * c);
        EIGSOL_HIP(hipGetLastError());
        EIGSOL_TRY(A.apply_h(u, y));
        hipLaunchKernelGGL((dev::svds_resid_kernel<S>), dim3(wsV.grid), blk, 0, st, (const S*)y, v, sv[c], N,
                           wsV.npart.template as<double>());
        hipLaunchKernelGGL(dev::svds_sum_kernel, dim3(1), blk, 0, st, (const double*)wsV.npart.template as<double>(), wsV.grid,
                           outs.as<double>() + 2 * c + 1);
        EIGSOL_HIP(hipGetLastError());
    }
    std::vector<double> rn((size_t)2 * k, 0.0);
    EIGSOL_HIP(hipMemcpyAsync(rn.data(), outs.p, rn.size() * sizeof(double), hipMemcpyDeviceToHost, st));
    const bool vectors = U_out || V_out;
    std::vector<HS> Uh, Vh;
    if (vectors) {   // the phase is V's, so V is read for U alone too
        Vh.resize((size_t)N * k);
        for (int c = 0; c < k; ++c)
            EIGSOL_HIP(hipMemcpyAsync(Vh.data() + (size_t)c * N, VK + (size_t)c * ldv, (size_t)N * sizeof(S),
                                      hipMemcpyDeviceToHost, st));
        if (U_out) {
            Uh.resize((size_t)M * k);
            for (int c = 0; c < k; ++c)
                EIGSOL_HIP(hipMemcpyAsync(Uh.data() + (size_t)c * M, UK + (size_t)c * ldu, (size_t)M * sizeof(S),
                                          hipMemcpyDeviceToHost, st));
        }
    }
    EIGSOL_TRY(E.mark(1, st));
    EIGSOL_HIP(stream_wait(st));
    {
        double te[1];
        E.read(te, 1);
        ms[3] += te[0];
    }
    for (int q = 0; q < 4; ++q) ctx->svds_ms[q] = ms[q];
    // the largest-modulus component of v_i (the first on ties) real and positive; the same factor on u_i
    for (int c = 0; c < k && vectors; ++c) {
        HS* v = Vh.data() + (size_t)c * N;
        int64_t bi = 0;
        double best = -1.0;
        for (int64_t i = 0; i < N; ++i) {
            const double a = std::abs(v[i]);
            if (a > best) {
                best = a;
                bi = i;
            }
        }
        if (!(best > 0.0)) continue;
        const HS f = smallsvd::conj_s(v[bi]) / best;   // a real column: exactly +-1
        for (int64_t i = 0; i < N; ++i) v[i] = i == bi ? HS(best) : v[i] * f;
        if (U_out) {
            HS* u = Uh.data() + (size_t)c * M;
            for (int64_t i = 0; i < M; ++i) u[i] *= f;
        }
    }
    if (U_out) std::memcpy(U_out, Uh.data(), Uh.size() * sizeof(HS));
    if (V_out) std::memcpy(V_out, Vh.data(), Vh.size() * sizeof(HS));
    for (int c = 0; c < k; ++c) {
        s_out[c] = sv[c];
        if (residuals) residuals[c] = std::hypot(std::sqrt(std::max(rn[2 * c], 0.0)), std::sqrt(std::max(rn[2 * c + 1], 0.0)));
    }
    if (restarts) *restarts = cycle;
    if (applications) *applications = apps;
    if (converged) *converged = conv ? 1 : 0;
    return EIGSOL_OK;
}

// the checks every matrix kind shares, then the run
int svds_entry(const LinearOp& A, bool build_adjoint, const eigsol_svds_options* opts, const void* v0, double* s, void* U, void* V,
               double* residuals, int32_t* restarts, int32_t* applications, int32_t* converged) {
    if (A.dtype() != EIGSOL_F64 && A.dtype() != EIGSOL_C128)
        return fail(EIGSOL_E_UNSUPPORTED, "svds: only double and complex double matrices are supported");
    if (A.nrows() == 0 || A.ncols() == 0) return fail(EIGSOL_E_ZERO_SIZE, "svds: matrix has zero size");
    if (opts->nsv < 1) return fail(EIGSOL_E_INVALID, "svds: nsv must be at least 1");
    if (opts->ncv > dev::ks::kMaxBasis) return fail(EIGSOL_E_INVALID, "svds: ncv must be at most 64");
    if (opts->ncv < opts->nsv + 2) return fail(EIGSOL_E_INVALID, "svds: ncv must be at least nsv + 2");
    if (opts->ncv > std::min(A.nrows(), A.ncols()))
        return fail(EIGSOL_E_INVALID, "svds: ncv exceeds the smaller matrix dimension");
    if (opts->max_restarts < 1) return fail(EIGSOL_E_INVALID, "svds: max_restarts must be at least 1");
    if (A.dtype() == EIGSOL_C128)
        return svds_run<cplx>(A, build_adjoint, opts, v0, s, U, V, residuals, restarts, applications, converged);
    return svds_run<double>(A, build_adjoint, opts, v0, s, U, V, residuals, restarts, applications, converged);
}

}  // namespace
}  // namespace eigsol

using namespace eigsol;

extern "C" {

int eigsol_csr_adjoint(eigsol_csr* A, eigsol_csr** out) {
    if (!A || !out) return fail(EIGSOL_E_INVALID, "eigsol_csr_adjoint: null pointer");
    *out = nullptr;
    if (A->dist) return fail(EIGSOL_E_UNSUPPORTED, "eigsol_csr_adjoint: row-sharded matrix");
    if (A->dtype != EIGSOL_F64 && A->dtype != EIGSOL_C128)
        return fail(EIGSOL_E_UNSUPPORTED, "eigsol_csr_adjoint: only double and complex double matrices are supported");
    // A's CSR arrays are the CSC arrays of its transpose
    std::vector<int32_t> rp((size_t)A->nrows + 1), ci((size_t)A->nnz);
    std::vector<double> v((size_t)A->nnz * (A->dtype == EIGSOL_C128 ? 2 : 1));
    EIGSOL_TRY(eigsol_csr_download(A, rp.data(), ci.data(), v.data()));
    if (A->dtype == EIGSOL_C128)
        for (int64_t e = 0; e < A->nnz; ++e) v[2 * e + 1] = -v[2 * e + 1];
    return eigsol_csr_create_from_csc(A->ctx, (eigsol_dtype)A->dtype, A->ncols, A->nrows, A->nnz, rp.data(), ci.data(),
                                      v.data(), out);
}

int eigsol_svds_csr(eigsol_csr* A, eigsol_csr* AH, const eigsol_svds_options* opts, const void* v0, double* s, void* U,
                    void* V, double* residuals, int32_t* restarts, int32_t* applications, int32_t* converged) {
    if (!A || !opts || !v0 || !s) return fail(EIGSOL_E_INVALID, "eigsol_svds_csr: null pointer");
    if (A->dist || (AH && AH->dist)) return fail(EIGSOL_E_UNSUPPORTED, "svds: row-sharded matrix");
    if (AH && (AH->nrows != A->ncols || AH->ncols != A->nrows || AH->dtype != A->dtype || AH->ctx != A->ctx))
        return fail(EIGSOL_E_INVALID, "svds: the adjoint handle's shape, dtype or context does not match");
    return svds_entry(LinearOp(A, AH), AH == nullptr, opts, v0, s, U, V, residuals, restarts, applications, converged);
}

int eigsol_svds_dense(eigsol_dense* A, const eigsol_svds_options* opts, const void* v0, double* s, void* U, void* V,
                      double* residuals, int32_t* restarts, int32_t* applications, int32_t* converged) {
    if (!A || !opts || !v0 || !s) return fail(EIGSOL_E_INVALID, "eigsol_svds_dense: null pointer");
    return svds_entry(LinearOp(A), false, opts, v0, s, U, V, residuals, restarts, applications, converged);
}

int eigsol_svds_stage_times(eigsol_ctx* ctx, double* ms4) {
    if (!ctx || !ms4) return fail(EIGSOL_E_INVALID, "eigsol_svds_stage_times: null pointer");
    for (int q = 0; q < 4; ++q) ms4[q] = ctx->svds_ms[q];
    return EIGSOL_OK;
}

}  // extern "C"
