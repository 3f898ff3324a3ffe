// Krylov-Schur (thick-restart Arnoldi): k eigenpairs of a sparse or a dense matrix, of largest
// modulus or nearest a shift, from a Krylov basis of m <= 64 vectors (algorithm:
// include/eigsol_hip.h).  The driver reaches the matrix through LinearOp (linear_op.hpp).
//
// The basis V is n x (m + 1), column-major, so that a basis vector is a contiguous operand of the
// single-vector SpMV layouts and of the shifted solves.  Per Arnoldi step the host enqueues the
// operator and the seven kernels of an orthogonalisation step and waits for nothing; h and beta stay
// on the device.  Those kernels, the in-place basis rotation of a restart and their launchers are in
// krylov_orth.hpp, shared with svds.hip.
//
// Out of scope: single precision, double-double, row-sharded matrices, a session /
// step form, generalised problems and selections other than largest modulus / nearest sigma.
#include <algorithm>
#include <cmath>
#include <complex>

#include "kernels_common.hpp"
#include "krylov_orth.hpp"
#include "linear_op.hpp"
#include "scratch.hpp"
#include "shifted.hpp"
#include "small_eig.hpp"

namespace eigsol {

namespace dev {
namespace ks {

// ------------------------------------------------------------------ norms and residuals of Ritz vectors
// npart[blockIdx] = the workgroup's partial of ||x||^2
__global__ __launch_bounds__(kThreads) void ks_sqnorm_kernel(const cplx* __restrict__ x, int64_t n,
                                                             double* __restrict__ npart) {
    __shared__ double sm[kWaves];
    double a2 = 0.0;
    const int64_t stride = (int64_t)gridDim.x * kThreads;
    for (int64_t r = (int64_t)blockIdx.x * kThreads + threadIdx.x; r < n; r += stride) a2 += sq_abs(x[r]);
    a2 = block_sum_all(a2, sm);
    if (threadIdx.x == 0) npart[blockIdx.x] = a2;
}

// out[0] = the sum of npart in a fixed order (one workgroup)
__global__ __launch_bounds__(kThreads) void ks_sum_kernel(const double* __restrict__ npart, int nparts,
                                                          double* __restrict__ out) {
    __shared__ double sm[kWaves];
    double s = 0.0;
    for (int g = threadIdx.x; g < nparts; g += kThreads) s += npart[g];
    s = block_sum_all(s, sm);
    if (threadIdx.x == 0) out[0] = s;
}

// complex x -> its real and imaginary parts (the two operands of a real matrix's SpMV)
__global__ __launch_bounds__(kThreads) void ks_split_kernel(const cplx* __restrict__ x, int64_t n,
                                                            double* __restrict__ xr, double* __restrict__ xi) {
    const int64_t stride = (int64_t)gridDim.x * kThreads;
    for (int64_t r = (int64_t)blockIdx.x * kThreads + threadIdx.x; r < n; r += stride) {
        const cplx v = x[r];
        xr[r] = v.re;
        xi[r] = v.im;
    }
}

// npart[blockIdx] = the workgroup's partial of ||y - lambda x||^2; y = yc, or yr + i yi when yc is null
__global__ __launch_bounds__(kThreads) void ks_resid_kernel(const cplx* __restrict__ yc, const double* __restrict__ yr,
                                                            const double* __restrict__ yi, const cplx* __restrict__ x,
                                                            int64_t n, double lre, double lim,
                                                            double* __restrict__ npart) {
    __shared__ double sm[kWaves];
    const cplx lam{lre, lim};
    double a2 = 0.0;
    const int64_t stride = (int64_t)gridDim.x * kThreads;
    for (int64_t r = (int64_t)blockIdx.x * kThreads + threadIdx.x; r < n; r += stride) {
        const cplx y = yc ? yc[r] : cplx{yr[r], yi[r]};
        a2 += sq_abs(sub(y, mul(lam, x[r])));
    }
    a2 = block_sum_all(a2, sm);
    if (threadIdx.x == 0) npart[blockIdx.x] = a2;
}

}  // namespace ks
}  // namespace dev

// ====================================================================================== host
namespace {

using smalleig::cd;
using smalleig::host_of;
using smalleig::ritz_order;
using smalleig::small_eig;

template <class T> inline T conj_h(T v);
template <> inline double conj_h<double>(double v) { return v; }
template <> inline cd conj_h<cd>(cd v) { return std::conj(v); }
inline double abs2_h(double v) { return v * v; }
inline double abs2_h(cd v) { return std::norm(v); }

// Q (m x p, column-major): an orthonormal basis of the span of the ncand columns of C (m x ncand,
// column-major, destroyed), which has rank p: Gram-Schmidt with column pivoting, every chosen
// vector orthogonalised twice.  false: the span has rank below p.
template <class T>
bool orth_basis(int m, int ncand, int p, std::vector<T>& C, std::vector<T>& Q) {
    Q.assign((size_t)m * p, T(0));
    std::vector<char> used(ncand, 0);
    auto col_norm = [&](int c) {
        double s = 0.0;
        for (int i = 0; i < m; ++i) s += abs2_h(C[(size_t)c * m + i]);
        return std::sqrt(s);
    };
    for (int s = 0; s < p; ++s) {
        int best = -1;
        double bn = 0.0;
        for (int c = 0; c < ncand; ++c) {
            if (used[c]) continue;
            const double nn = col_norm(c);
            if (best < 0 || nn > bn) {
                best = c;
                bn = nn;
            }
        }
        if (best < 0 || !(bn > 1e-8)) return false;   // the candidates are unit eigenvectors' parts
        used[best] = 1;
        T* q = &Q[(size_t)s * m];
        for (int i = 0; i < m; ++i) q[i] = C[(size_t)best * m + i];
        for (int pass = 0; pass < 2; ++pass) {
            for (int a = 0; a < s; ++a) {
                const T* qa = &Q[(size_t)a * m];
                T d = T(0);
                for (int i = 0; i < m; ++i) d += conj_h(qa[i]) * q[i];
                for (int i = 0; i < m; ++i) q[i] -= qa[i] * d;
            }
            double nn = 0.0;
            for (int i = 0; i < m; ++i) nn += abs2_h(q[i]);
            nn = std::sqrt(nn);
            if (!(nn > 0.0)) return false;
            for (int i = 0; i < m; ++i) q[i] /= nn;
        }
        for (int c = 0; c < ncand; ++c) {
            if (used[c]) continue;
            T* cc = &C[(size_t)c * m];
            T d = T(0);
            for (int i = 0; i < m; ++i) d += conj_h(q[i]) * cc[i];
            for (int i = 0; i < m; ++i) cc[i] -= q[i] * d;
        }
    }
    return true;
}

template <class S>
int krylov_run(const LinearOp& A, const eigsol_krylov_options* o, const void* sigma, const void* v0v, double* eigenvalues,
               double* eigenvectors, double* residuals, int32_t* restarts, int32_t* applications, int32_t* converged) {
    using HS = typename host_of<S>::type;
    constexpr bool real = std::is_same_v<S, double>;
    const int64_t n = A.nrows();
    const int m = o->ncv, k = o->nev;
    const bool invert = o->mode == EIGSOL_KRYLOV_SHIFT_INVERT;
    const eigsol_ctx* ctx = A.ctx();
    hipStream_t st = ctx->stream;

    // v_0 = v0 / ||v0|| on the host
    const HS* v0 = static_cast<const HS*>(v0v);
    std::vector<HS> v0n(v0, v0 + n);
    {
        double mx = 0.0;
        for (const HS& z : v0n) mx = std::max(mx, std::abs(z));
        double s = 0.0;
        if (mx > 0.0 && std::isfinite(mx))
            for (const HS& z : v0n) s += abs2_h(z / mx);
        const double nrm = mx * std::sqrt(s);
        if (!(nrm > 0.0) || !std::isfinite(nrm))
            return fail(EIGSOL_E_INVALID, "krylov_schur: v0 has no finite nonzero norm");
        for (HS& z : v0n) z /= nrm;
    }

    EIGSOL_HIP(hipSetDevice(ctx->device));
    struct FactorGuard {
        ShiftFactor* f = nullptr;
        ~FactorGuard() {
            if (f) shift_factor_free(f);
        }
    } fac;
    cd sig(0.0, 0.0);
    if (invert) {
        double sr = 0.0, si = 0.0;
        load_scalar(sigma, A.dtype(), sr, si);
        sig = cd(sr, si);
        EIGSOL_TRY(A.factor(sigma, &fac.f));
    }

    // columns start on 16-byte boundaries for every n
    const int64_t ldv = real ? ((n + 1) & ~(int64_t)1) : n;
    DevBuf vbuf, sdev, qdev, xk, ybuf, ysdev;
    OrthWs<S> ws;
    EIGSOL_TRY(vbuf.alloc((size_t)ldv * (m + 1) * sizeof(S)));
    EIGSOL_TRY(sdev.alloc((size_t)(m + 1) * m * sizeof(S)));
    EIGSOL_TRY(qdev.alloc((size_t)m * m * sizeof(S)));
    EIGSOL_TRY(ysdev.alloc((size_t)m * k * sizeof(cplx)));
    EIGSOL_TRY(ws.alloc(ctx, n, st));
    S* V = vbuf.as<S>();
    S* SD = sdev.as<S>();
    EIGSOL_HIP(hipMemsetAsync(SD, 0, (size_t)(m + 1) * m * sizeof(S), st));
    EIGSOL_HIP(hipMemcpyAsync(V, v0n.data(), (size_t)n * sizeof(S), hipMemcpyHostToDevice, st));

    const int ms = m + 1;                                // leading dimension of S
    std::vector<HS> Sh((size_t)ms * m, HS(0)), Sd((size_t)ms * m), Qh, Cand, BQ;
    std::vector<cd> Bc, w, Y, theta(m);
    std::vector<int> order;
    int32_t hb = 0;
    int p = 0, d = m, apps = 0, cycle = 0;
    bool conv = false;
    const double eps23 = std::pow(0x1p-52, 2.0 / 3.0);
    auto Sat = [&](int i, int j) -> HS& { return Sh[(size_t)j * ms + i]; };

    for (cycle = 1; cycle <= o->max_restarts; ++cycle) {
        for (int j = p; j < m; ++j) {                    // expansion: nothing here waits for the device
            S* vj = V + (size_t)j * ldv;
            S* wj = V + (size_t)(j + 1) * ldv;
            if (invert) EIGSOL_TRY(shift_solve_launch(fac.f, vj, wj));
            else EIGSOL_TRY(A.apply(vj, wj));
            EIGSOL_TRY(orth_step<S>(ws, V, ldv, j + 1, wj, n, SD + (size_t)j * ms, (double)m, st));
        }
        // the cycle's one host wait: S, the breakdown word and the factor's error word
        EIGSOL_HIP(hipMemcpyAsync(Sd.data(), SD, Sd.size() * sizeof(S), hipMemcpyDeviceToHost, st));
        EIGSOL_HIP(hipMemcpyAsync(&hb, ws.bword.p, sizeof(hb), hipMemcpyDeviceToHost, st));
        EIGSOL_HIP(stream_wait(st));
        if (invert) EIGSOL_TRY(shift_error(fac.f));
        d = hb ? hb : m;                                 // a breakdown at step j left dimension j + 1
        apps += d - p;
        for (int j = p; j < d; ++j)
            for (int i = 0; i <= j + 1; ++i) Sat(i, j) = Sd[(size_t)j * ms + i];
        bool finite = true;
        Bc.assign((size_t)d * d, cd(0));
        for (int i = 0; i < d; ++i)
            for (int j = 0; j < d; ++j) {
                const cd z = cd(Sat(i, j));
                Bc[(size_t)i * d + j] = z;
                finite = finite && std::isfinite(z.real()) && std::isfinite(z.imag());
            }
        for (int j = 0; j < d && !hb; ++j) finite = finite && std::isfinite(std::abs(cd(Sat(d, j))));
        if (!finite) return fail(EIGSOL_E_SOLVER, "krylov_schur: the Rayleigh matrix is not finite");
        if (!small_eig(d, Bc, w, Y))
            return fail(EIGSOL_E_SOLVER, "krylov_schur: eig of the Rayleigh matrix did not converge");
        order = ritz_order(w);
        theta.assign(d, cd(0));
        for (int j = 0; j < d; ++j) theta[j] = w[order[j]];
        if (hb) {
            if (d < k)
                return fail(EIGSOL_E_SOLVER, "krylov_schur: invariant subspace of dimension " + std::to_string(d) +
                                                 " < nev");
            conv = true;
            break;
        }
        bool all = o->tolerance >= 0.0;
        for (int i = 0; i < k && all; ++i) {
            cd e(0.0, 0.0);
            for (int l = 0; l < m; ++l) e += cd(Sat(m, l)) * Y[(size_t)l * m + order[i]];
            all = std::abs(e) <= o->tolerance * std::max(eps23, std::abs(theta[i]));
        }
        if (all) {
            conv = true;
            break;
        }
        if (cycle == o->max_restarts) break;

        // restart: keep the invariant subspace of B of theta_0 .. theta_{p-1}
        p = k;
        if (real && theta[k - 1].imag() > 0.0 &&
            std::abs(theta[k] - std::conj(theta[k - 1])) <= 1e-8 * std::abs(theta[k - 1]))
            p = k + 1;
        const int ncand = real ? 2 * p : p;
        Cand.assign((size_t)m * ncand, HS(0));
        for (int c = 0; c < p; ++c)
            for (int i = 0; i < m; ++i) {
                const cd y = Y[(size_t)i * m + order[c]];
                if constexpr (real) {
                    Cand[(size_t)c * m + i] = y.real();
                    Cand[(size_t)(p + c) * m + i] = y.imag();
                } else {
                    Cand[(size_t)c * m + i] = y;
                }
            }
        if (!orth_basis<HS>(m, ncand, p, Cand, Qh))
            return fail(EIGSOL_E_SOLVER, "krylov_schur: the restart basis lost rank");
        // S <- [Q^H B Q; b^T Q] in rows 0 .. p, zero elsewhere
        BQ.assign((size_t)ms * p, HS(0));                // [B; b^T] Q, (m + 1) x p
        for (int c = 0; c < p; ++c)
            for (int l = 0; l < m; ++l) {
                const HS q = Qh[(size_t)c * m + l];
                for (int i = 0; i < ms; ++i) BQ[(size_t)c * ms + i] += Sat(i, l) * q;
            }
        std::fill(Sh.begin(), Sh.end(), HS(0));
        for (int c = 0; c < p; ++c) {
            for (int a = 0; a < p; ++a) {
                HS s = HS(0);
                for (int i = 0; i < m; ++i) s += conj_h(Qh[(size_t)a * m + i]) * BQ[(size_t)c * ms + i];
                Sat(a, c) = s;
            }
            Sat(p, c) = BQ[(size_t)c * ms + m];
        }
        // V[:, :p] <- V[:, :m] Q, v_p <- v_m (Qh is next written after the next wait)
        EIGSOL_HIP(hipMemcpyAsync(qdev.p, Qh.data(), (size_t)m * p * sizeof(S), hipMemcpyHostToDevice, st));
        EIGSOL_TRY((launch_mul<S, S>(ctx, V, ldv, n, m, p, (const S*)qdev.as<S>(), V, ldv, st)));
        EIGSOL_HIP(hipMemcpyAsync(V + (size_t)p * ldv, V + (size_t)m * ldv, (size_t)n * sizeof(S),
                                  hipMemcpyDeviceToDevice, st));
    }
    if (cycle > o->max_restarts) cycle = o->max_restarts;

    // Ritz pairs of the last decomposition: x_i = V[:, :d] y_i to unit norm, explicit residuals
    EIGSOL_TRY(xk.alloc((size_t)n * k * sizeof(cplx)));
    EIGSOL_TRY(ybuf.alloc((size_t)4 * n * sizeof(double)));   // complex A x, or [xr | xi | A xr | A xi]
    cplx* X = xk.as<cplx>();
    double* np_ = ws.npart.template as<double>();
    DevBuf outs;
    EIGSOL_TRY(outs.alloc((size_t)k * sizeof(double)));
    std::vector<cd> Ys((size_t)d * k);
    std::vector<double> xn(k, 1.0), rn(k, 0.0);
    const dim3 blk(dev::kThreads), grid(ws.grid);
    auto ritz_vectors = [&]() -> int {
        for (int c = 0; c < k; ++c)
            for (int i = 0; i < d; ++i) Ys[(size_t)c * d + i] = Y[(size_t)i * d + order[c]] / xn[c];
        EIGSOL_HIP(hipMemcpyAsync(ysdev.p, Ys.data(), Ys.size() * sizeof(cd), hipMemcpyHostToDevice, st));
        EIGSOL_TRY((launch_mul<S, cplx>(ctx, V, ldv, n, d, k, (const cplx*)ysdev.as<cplx>(), X, n, st)));
        return EIGSOL_OK;
    };
    EIGSOL_TRY(ritz_vectors());
    for (int c = 0; c < k; ++c) {
        hipLaunchKernelGGL(ks::ks_sqnorm_kernel, grid, blk, 0, st, (const cplx*)(X + (size_t)c * n), n, np_);
        hipLaunchKernelGGL(ks::ks_sum_kernel, dim3(1), blk, 0, st, (const double*)np_, ws.grid, outs.as<double>() + c);
        EIGSOL_HIP(hipGetLastError());
    }
    EIGSOL_HIP(hipMemcpyAsync(xn.data(), outs.p, (size_t)k * sizeof(double), hipMemcpyDeviceToHost, st));
    EIGSOL_HIP(stream_wait(st));
    for (int c = 0; c < k; ++c) {
        xn[c] = std::sqrt(xn[c]);
        if (!(xn[c] > 0.0) || !std::isfinite(xn[c]))
            return fail(EIGSOL_E_SOLVER, "krylov_schur: Ritz vector " + std::to_string(c) + " has no finite norm");
    }
    EIGSOL_TRY(ritz_vectors());
    std::vector<cd> lam(k);
    for (int c = 0; c < k; ++c) lam[c] = invert ? sig + 1.0 / theta[c] : theta[c];
    for (int c = 0; c < k; ++c) {
        const cplx* x = X + (size_t)c * n;
        if constexpr (real) {
            double* xr = ybuf.as<double>();
            double *xi = xr + n, *yr = xr + 2 * n, *yi = xr + 3 * n;
            hipLaunchKernelGGL(ks::ks_split_kernel, grid, blk, 0, st, x, n, xr, xi);
            EIGSOL_HIP(hipGetLastError());
            EIGSOL_TRY(A.apply(xr, yr));
            EIGSOL_TRY(A.apply(xi, yi));
            hipLaunchKernelGGL(ks::ks_resid_kernel, grid, blk, 0, st, (const cplx*)nullptr, (const double*)yr,
                               (const double*)yi, x, n, lam[c].real(), lam[c].imag(), np_);
        } else {
            cplx* y = ybuf.as<cplx>();
            EIGSOL_TRY(A.apply(x, y));
            hipLaunchKernelGGL(ks::ks_resid_kernel, grid, blk, 0, st, (const cplx*)y, (const double*)nullptr,
                               (const double*)nullptr, x, n, lam[c].real(), lam[c].imag(), np_);
        }
        EIGSOL_HIP(hipGetLastError());
        hipLaunchKernelGGL(ks::ks_sum_kernel, dim3(1), blk, 0, st, (const double*)np_, ws.grid, outs.as<double>() + c);
        EIGSOL_HIP(hipGetLastError());
    }
    EIGSOL_HIP(hipMemcpyAsync(rn.data(), outs.p, (size_t)k * sizeof(double), hipMemcpyDeviceToHost, st));
    if (eigenvectors)
        EIGSOL_HIP(hipMemcpyAsync(eigenvectors, X, (size_t)n * k * sizeof(cplx), hipMemcpyDeviceToHost, st));
    EIGSOL_HIP(stream_wait(st));
    for (int c = 0; c < k; ++c) {
        eigenvalues[2 * c] = lam[c].real();
        eigenvalues[2 * c + 1] = lam[c].imag();
        if (residuals) residuals[c] = std::sqrt(std::max(rn[c], 0.0));
    }
    if (restarts) *restarts = cycle;
    if (applications) *applications = apps;
    if (converged) *converged = conv ? 1 : 0;
    return EIGSOL_OK;
}

template <class S>
int orth_entry(eigsol_ctx* ctx, int64_t n, int j, const S* V, int64_t ldv, S* w, double* h_out, double* beta_out,
               double* wnorm_out) {
    hipStream_t st = ctx->stream;
    OrthWs<S> ws;
    EIGSOL_TRY(ws.alloc(ctx, n, st));
    EIGSOL_TRY(orth_step<S>(ws, V, ldv, j, w, n, nullptr, (double)ks::kMaxBasis, st));
    using HS = typename host_of<S>::type;
    std::vector<HS> h(j);
    double sc[2] = {0.0, 0.0};
    EIGSOL_HIP(hipMemcpyAsync(h.data(), ws.h.p, (size_t)j * sizeof(S), hipMemcpyDeviceToHost, st));
    EIGSOL_HIP(hipMemcpyAsync(sc, ws.scal.p, sizeof(sc), hipMemcpyDeviceToHost, st));
    EIGSOL_HIP(stream_wait(st));   // also before the workspace is freed
    if (h_out)
        for (int i = 0; i < j; ++i) {
            h_out[2 * i] = cd(h[i]).real();
            h_out[2 * i + 1] = cd(h[i]).imag();
        }
    if (beta_out) *beta_out = sc[1];
    if (wnorm_out) *wnorm_out = std::sqrt(sc[0]);
    return EIGSOL_OK;
}

template <class S>
int rotate_entry(eigsol_ctx* ctx, int64_t n, int m, int p, S* V, int64_t ldv, const S* Q) {
    hipStream_t st = ctx->stream;
    DevBuf q;
    EIGSOL_TRY(q.alloc((size_t)m * p * sizeof(S)));
    EIGSOL_HIP(hipMemcpyAsync(q.p, Q, (size_t)m * p * sizeof(S), hipMemcpyHostToDevice, st));
    EIGSOL_TRY((launch_mul<S, S>(ctx, V, ldv, n, m, p, (const S*)q.as<S>(), V, ldv, st)));
    EIGSOL_HIP(stream_wait(st));   // Q's device copy is freed on return
    return EIGSOL_OK;
}

// the checks every matrix kind shares, then the run
int krylov_entry(const LinearOp& A, int64_t ncols, const eigsol_krylov_options* opts, const void* sigma,
                 const void* v0, double* eigenvalues, double* eigenvectors, double* residuals, int32_t* restarts,
                 int32_t* applications, int32_t* converged) {
    if (A.dtype() != EIGSOL_F64 && A.dtype() != EIGSOL_C128)
        return fail(EIGSOL_E_UNSUPPORTED, "krylov_schur: only double and complex double matrices are supported");
    if (A.nrows() != ncols) return fail(EIGSOL_E_NOT_SQUARE, "krylov_schur: matrix must be square");
    if (A.nrows() == 0) return fail(EIGSOL_E_ZERO_SIZE, "krylov_schur: matrix has zero size");
    if (opts->nev < 1) return fail(EIGSOL_E_INVALID, "krylov_schur: nev must be at least 1");
    if (opts->ncv > dev::ks::kMaxBasis) return fail(EIGSOL_E_INVALID, "krylov_schur: ncv must be at most 64");
    if (opts->ncv < opts->nev + 2) return fail(EIGSOL_E_INVALID, "krylov_schur: ncv must be at least nev + 2");
    if (opts->ncv > A.nrows()) return fail(EIGSOL_E_INVALID, "krylov_schur: ncv exceeds the matrix order");
    if (opts->max_restarts < 1) return fail(EIGSOL_E_INVALID, "krylov_schur: max_restarts must be at least 1");
    if (A.dtype() == EIGSOL_C128)
        return krylov_run<cplx>(A, opts, sigma, v0, eigenvalues, eigenvectors, residuals, restarts, applications,
                                converged);
    return krylov_run<double>(A, opts, sigma, v0, eigenvalues, eigenvectors, residuals, restarts, applications,
                              converged);
}

}  // namespace
}  // namespace eigsol

using namespace eigsol;

extern "C" {

int eigsol_krylov_csr(eigsol_csr* A, const eigsol_krylov_options* opts, const void* sigma, const void* v0,
                      double* eigenvalues, double* eigenvectors, double* residuals, int32_t* restarts,
                      int32_t* applications, int32_t* converged) {
    if (!A || !opts || !v0 || !eigenvalues) return fail(EIGSOL_E_INVALID, "eigsol_krylov_csr: null pointer");
    if (opts->mode != EIGSOL_KRYLOV_LM && opts->mode != EIGSOL_KRYLOV_SHIFT_INVERT)
        return fail(EIGSOL_E_INVALID, "krylov_schur: unknown mode");
    if (opts->mode == EIGSOL_KRYLOV_SHIFT_INVERT && !sigma)
        return fail(EIGSOL_E_INVALID, "eigsol_krylov_csr: null sigma in shift-invert mode");
    if (A->dist) return fail(EIGSOL_E_UNSUPPORTED, "krylov_schur: row-sharded matrix");
    return krylov_entry(LinearOp(A), A->ncols, opts, sigma, v0, eigenvalues, eigenvectors, residuals, restarts,
                        applications, converged);
}

int eigsol_krylov_dense(eigsol_dense* A, const eigsol_krylov_options* opts, const void* sigma, const void* v0,
                        double* eigenvalues, double* eigenvectors, double* residuals, int32_t* restarts,
                        int32_t* applications, int32_t* converged) {
    if (!A || !opts || !v0 || !eigenvalues) return fail(EIGSOL_E_INVALID, "eigsol_krylov_dense: null pointer");
    if (opts->mode != EIGSOL_KRYLOV_LM && opts->mode != EIGSOL_KRYLOV_SHIFT_INVERT)
        return fail(EIGSOL_E_INVALID, "krylov_schur: unknown mode");
    if (opts->mode == EIGSOL_KRYLOV_SHIFT_INVERT && !sigma)
        return fail(EIGSOL_E_INVALID, "eigsol_krylov_dense: null sigma in shift-invert mode");
    return krylov_entry(LinearOp(A), A->ncols, opts, sigma, v0, eigenvalues, eigenvectors, residuals, restarts,
                        applications, converged);
}

int eigsol_krylov_orth(eigsol_ctx* ctx, int dtype, int64_t n, int32_t j, const void* V_dev, int64_t ldv, void* w_dev,
                       double* h_out, double* beta_out, double* wnorm_out) {
    if (!ctx || !V_dev || !w_dev) return fail(EIGSOL_E_INVALID, "eigsol_krylov_orth: null pointer");
    if (dtype != EIGSOL_F64 && dtype != EIGSOL_C128)
        return fail(EIGSOL_E_UNSUPPORTED, "eigsol_krylov_orth: only double and complex double are supported");
    if (n < 1 || j < 1 || j > dev::ks::kMaxBasis || ldv < n)
        return fail(EIGSOL_E_INVALID, "eigsol_krylov_orth: needs n >= 1, 1 <= j <= 64 and ldv >= n");
    EIGSOL_HIP(hipSetDevice(ctx->device));
    if (dtype == EIGSOL_C128)
        return orth_entry<cplx>(ctx, n, j, (const cplx*)V_dev, ldv, (cplx*)w_dev, h_out, beta_out, wnorm_out);
    return orth_entry<double>(ctx, n, j, (const double*)V_dev, ldv, (double*)w_dev, h_out, beta_out, wnorm_out);
}

int eigsol_krylov_rotate(eigsol_ctx* ctx, int dtype, int64_t n, int32_t m, int32_t p, void* V_dev, int64_t ldv,
                         const void* Q) {
    if (!ctx || !V_dev || !Q) return fail(EIGSOL_E_INVALID, "eigsol_krylov_rotate: null pointer");
    if (dtype != EIGSOL_F64 && dtype != EIGSOL_C128)
        return fail(EIGSOL_E_UNSUPPORTED, "eigsol_krylov_rotate: only double and complex double are supported");
    if (n < 1 || m < 1 || m > dev::ks::kMaxBasis || p < 1 || p > m || ldv < n)
        return fail(EIGSOL_E_INVALID, "eigsol_krylov_rotate: needs n >= 1, 1 <= p <= m <= 64 and ldv >= n");
    EIGSOL_HIP(hipSetDevice(ctx->device));
    if (dtype == EIGSOL_C128) return rotate_entry<cplx>(ctx, n, m, p, (cplx*)V_dev, ldv, (const cplx*)Q);
    return rotate_entry<double>(ctx, n, m, p, (double*)V_dev, ldv, (const double*)Q);
}

}  // extern "C"
