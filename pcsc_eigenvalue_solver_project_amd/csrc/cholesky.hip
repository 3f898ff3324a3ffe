// Dense Cholesky factorisation, blocked triangular solves with many right-hand sides, and the generalised
// symmetric-definite eigenproblem A x = lambda B x (gfx950; EIGSOL_F64 / EIGSOL_C128).
//
//   a. both lower triangles are mirrored on the device (herm_prepare), which also flags a non-finite entry;
//   b. B = L L^H, right-looking with block width NB = RankKMax<S> (64 real, 32 complex): the diagonal block
//      in LDS by one workgroup (chol_diag), the panel L21 = B21 L11^-H one row per lane with L11 in LDS
//      (chol_panel), the trailing update B22 -= L21 L21^H on the fp64 matrix cores, one rank-NB tile per
//      workgroup over the tiles on and below the diagonal (chol_syrk).  A pivot that is not > 0 (NaN
//      included) writes its column to a device word if that is still unset; nothing waits for it;
//   c. C = L^-1 A L^-H as (L^-1 (L^-1 A)^H)^H: the blocked left lower solve (substitution with the diagonal
//      block in LDS, one right-hand side per lane: trsm_diag; then X_below -= L_below,k X_k by rankk_update)
//      twice, a tiled conjugate transpose through padded LDS between and after (conj_transpose);
//   d. the standard solver on C without leaving the device (eigh_device, eigh.hip);
//   e. X = L^-H Y: L^H formed by the transpose kernel, then the blocked left upper solve from the last block
//      row up (trsm_diag<upper>, rankk_update), and eigh's phase convention.  X^H B X = I.
// No floating-point atomics; every sum has a fixed order, so two runs give the same bits.
#include <cmath>
#include <string>

#include "cholesky.hpp"
#include "kernels_common.hpp"
#include "mfma_rankk.hpp"
#include "scratch.hpp"

namespace eigsol {
namespace dev {

__device__ __forceinline__ bool finite_c(double a) { return isfinite(a); }
__device__ __forceinline__ bool finite_c(cplx a) { return isfinite(a.re) && isfinite(a.im); }
__device__ __forceinline__ double real_c(double a) { return a; }
__device__ __forceinline__ double real_c(cplx a) { return a.re; }

// upper triangle <- conj of the lower one, the diagonal's imaginary part dropped; *flag = 1 where the lower
// triangle holds a non-finite entry (every thread that finds one stores the same value)
template <class S>
__global__ __launch_bounds__(256) void herm_prepare(S* A, int n, int* flag) {
    const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (idx >= (int64_t)n * n) return;
    const int i = (int)(idx % n);
    const int64_t j = idx / n;
    if (i < j) {
        A[idx] = conj_c(A[j + (int64_t)i * n]);
        return;
    }
    S v = A[idx];
    if (i == j) {
        set_re_im(v, real_c(v), 0.0);
        A[idx] = v;
    }
    if (!finite_c(v)) *flag = 1;
}

// The diagonal block (rows and columns [k0, k0 + nb), nb <= NB) factored in LDS, column by column.
// A failed pivot leaves NaN or Inf behind; nothing loops on the data.
template <class S>
__global__ __launch_bounds__(256) void chol_diag(S* A, int64_t ld, int k0, int nb, long long* info) {
    constexpr int NB = RankKMax<S>::value;
    __shared__ S sa[NB][NB + 1];   // sa[column][row]
    const int tid = threadIdx.x;
    S* blk = A + k0 + (int64_t)k0 * ld;
    for (int idx = tid; idx < nb * nb; idx += 256) {
        const int i = idx % nb, j = idx / nb;
        if (i >= j) sa[j][i] = blk[i + (int64_t)j * ld];
    }
    for (int j = 0; j < nb; ++j) {
        __syncthreads();
        const double d = real_c(sa[j][j]);
        if (!(d > 0.0) && tid == 0 && *info < 0) *info = k0 + j;
        const double s = sqrt(d);
        __syncthreads();
        for (int i = j + 1 + tid; i < nb; i += 256) sa[j][i] = divr(sa[j][i], s);
        if (tid == 0) set_re_im(sa[j][j], s, 0.0);
        __syncthreads();
        const int cnt = nb - j - 1;
        for (int idx = tid; idx < cnt * cnt; idx += 256) {
            const int ii = idx % cnt, kk = idx / cnt;
            if (ii >= kk) {
                const int i = j + 1 + ii, k = j + 1 + kk;
                sa[k][i] = sub(sa[k][i], mul(sa[j][i], conj_c(sa[j][k])));
            }
        }
    }
    __syncthreads();
    for (int idx = tid; idx < nb * nb; idx += 256) {
        const int i = idx % nb, j = idx / nb;
        if (i >= j) blk[i + (int64_t)j * ld] = sa[j][i];
    }
}

// A triangular nb x nb block (lower: entries on and below the diagonal, else on and above) into LDS as
// st[row][column]
template <class S, bool kUpper>
__device__ __forceinline__ void load_tri(const S* T, int64_t ld, int nb, S (*st)[RankKMax<S>::value]) {
    for (int idx = threadIdx.x; idx < nb * nb; idx += 64) {
        const int i = idx % nb, k = idx / nb;
        if (kUpper ? i <= k : i >= k) st[i][k] = T[i + (int64_t)k * ld];
    }
}

// L21 = B21 L11^-H: rows [r0, r0 + m) of the block column [k0, k0 + nb), r0 = k0 + nb.  One row per lane,
// the 64 rows of a workgroup in LDS (xs[column][lane]): x_j = (b_j - sum_{k<j} x_k conj(l_jk)) / l_jj.
template <class S>
__global__ __launch_bounds__(64) void chol_panel(S* A, int64_t ld, int k0, int nb, int m) {
    constexpr int NB = RankKMax<S>::value;
    __shared__ S sl[NB][NB];
    __shared__ S xs[NB][64];
    load_tri<S, false>(A + k0 + (int64_t)k0 * ld, ld, nb, sl);
    const int lane = threadIdx.x, r = blockIdx.x * 64 + lane;
    S* row = A + (k0 + nb + min(r, m - 1)) + (int64_t)k0 * ld;
    for (int j = 0; j < nb; ++j) xs[j][lane] = row[(int64_t)j * ld];
    __syncthreads();
    for (int j = 0; j < nb; ++j) {
        S acc = xs[j][lane];
#pragma unroll 4
        for (int k = 0; k < j; ++k) acc = sub(acc, mul(xs[k][lane], conj_c(sl[j][k])));
        xs[j][lane] = divr(acc, real_c(sl[j][j]));
    }
    if (r < m)
        for (int j = 0; j < nb; ++j) row[(int64_t)j * ld] = xs[j][lane];
}

// B22 -= L21 L21^H, the 64 x 64 tiles on and below the diagonal only
template <class S>
__global__ __launch_bounds__(256) void chol_syrk(int m, int K, const S* L21, int64_t ld, S* C) {
    if (blockIdx.x < blockIdx.y) return;
    rankk_tile<S, false, true>(blockIdx.x, blockIdx.y, m, m, K, -1.0, L21, ld, L21, ld, C, ld);
}

// X <- T^-1 X for a triangular nb x nb block T (real diagonal) and nb x ncols X: one right-hand side per
// lane, substitution in LDS (T as st[row][column], the workgroup's 64 columns of X as xs[row][lane]).
template <class S, bool kUpper>
__global__ __launch_bounds__(64) void trsm_diag(const S* T, int64_t ldt, int nb, S* X, int64_t ldx, int ncols) {
    constexpr int NB = RankKMax<S>::value;
    __shared__ S st[NB][NB];
    __shared__ S xs[NB][65];
    load_tri<S, kUpper>(T, ldt, nb, st);
    const int lane = threadIdx.x, c0 = blockIdx.x * 64;
    const int nc = min(64, ncols - c0);
    for (int idx = lane; idx < nb * nc; idx += 64) {
        const int i = idx % nb, c = idx / nb;
        xs[i][c] = X[i + (int64_t)(c0 + c) * ldx];
    }
    __syncthreads();
    if (lane < nc) {
        if constexpr (kUpper) {
            for (int i = nb - 1; i >= 0; --i) {
                S acc = xs[i][lane];
#pragma unroll 4
                for (int k = nb - 1; k > i; --k) acc = sub(acc, mul(st[i][k], xs[k][lane]));
                xs[i][lane] = divr(acc, real_c(st[i][i]));
            }
        } else {
            for (int i = 0; i < nb; ++i) {
                S acc = xs[i][lane];
#pragma unroll 4
                for (int k = 0; k < i; ++k) acc = sub(acc, mul(st[i][k], xs[k][lane]));
                xs[i][lane] = divr(acc, real_c(st[i][i]));
            }
        }
    }
    __syncthreads();
    for (int idx = lane; idx < nb * nc; idx += 64) {
        const int i = idx % nb, c = idx / nb;
        X[i + (int64_t)(c0 + c) * ldx] = xs[i][c];
    }
}

template <class S>
__global__ __launch_bounds__(256) void zero_strict_upper(S* A, int n) {
    const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (idx >= (int64_t)n * n) return;
    if ((int64_t)(idx % n) < idx / n) A[idx] = s_zero<S>();
}

}  // namespace dev

namespace {

inline unsigned grid_nn(int64_t n) { return (unsigned)((n * n + 255) / 256); }

// B (n x n, lower triangle) <- L in place; stream-ordered, no host wait.  *info (device, preset to -1)
// receives the first column whose pivot is not > 0.
template <class S>
int cholesky_device(hipStream_t st, S* B, int64_t n, long long* info) {
    constexpr int NB = dev::RankKMax<S>::value;
    for (int64_t k0 = 0; k0 < n; k0 += NB) {
        const int nb = (int)std::min<int64_t>(NB, n - k0);
        hipLaunchKernelGGL(dev::chol_diag<S>, dim3(1), dim3(256), 0, st, B, n, (int)k0, nb, info);
        const int m = (int)(n - k0 - nb);
        if (m > 0) {
            hipLaunchKernelGGL(dev::chol_panel<S>, dim3((m + 63) / 64), dim3(64), 0, st, B, n, (int)k0, nb, m);
            hipLaunchKernelGGL(dev::chol_syrk<S>, dim3((m + 63) / 64, (m + 63) / 64), dim3(256), 0, st, m, nb,
                               B + (k0 + nb) + k0 * n, n, B + (k0 + nb) + (k0 + nb) * n);
        }
    }
    EIGSOL_HIP(hipGetLastError());
    return EIGSOL_OK;
}

// X (n x ncols) <- L^-1 X, L lower triangular n x n
template <class S>
int trsm_left_lower(hipStream_t st, const S* L, int64_t ldl, int64_t n, S* X, int64_t ldx, int64_t ncols) {
    constexpr int NB = dev::RankKMax<S>::value;
    if (n <= 0 || ncols <= 0) return EIGSOL_OK;
    for (int64_t k0 = 0; k0 < n; k0 += NB) {
        const int nb = (int)std::min<int64_t>(NB, n - k0);
        hipLaunchKernelGGL((dev::trsm_diag<S, false>), dim3((unsigned)((ncols + 63) / 64)), dim3(64), 0, st,
                           L + k0 + k0 * ldl, ldl, nb, X + k0, ldx, (int)ncols);
        const int64_t m = n - k0 - nb;
        if (m > 0)
            rankk_update<S, true>(st, (int)m, (int)ncols, nb, -1.0, L + (k0 + nb) + k0 * ldl, ldl, X + k0, ldx,
                                  X + k0 + nb, ldx);
    }
    EIGSOL_HIP(hipGetLastError());
    return EIGSOL_OK;
}

// X (n x ncols) <- U^-1 X, U upper triangular n x n
template <class S>
int trsm_left_upper(hipStream_t st, const S* U, int64_t ldu, int64_t n, S* X, int64_t ldx, int64_t ncols) {
    constexpr int NB = dev::RankKMax<S>::value;
    if (n <= 0 || ncols <= 0) return EIGSOL_OK;
    for (int64_t k0 = ((n - 1) / NB) * NB; k0 >= 0; k0 -= NB) {
        const int nb = (int)std::min<int64_t>(NB, n - k0);
        hipLaunchKernelGGL((dev::trsm_diag<S, true>), dim3((unsigned)((ncols + 63) / 64)), dim3(64), 0, st,
                           U + k0 + k0 * ldu, ldu, nb, X + k0, ldx, (int)ncols);
        if (k0 > 0) rankk_update<S, true>(st, (int)k0, (int)ncols, nb, -1.0, U + k0 * ldu, ldu, X + k0, ldx, X, ldx);
    }
    EIGSOL_HIP(hipGetLastError());
    return EIGSOL_OK;
}

template <class S>
void conj_transpose(hipStream_t st, int64_t n, const S* In, S* Out) {
    hipLaunchKernelGGL(dev::conj_transpose<S>, dim3((unsigned)((n + 31) / 32), (unsigned)((n + 31) / 32)), dim3(256), 0, st,
                       (int)n, (int)n, In, n, Out, n);
}

// device words of one call: info (first failed pivot, -1), then the non-finite flags of A and B
struct Words {
    long long info;
    int flag_a, flag_b;
};

int not_definite(const char* who, long long col, int64_t* info) {
    if (info) *info = col;
    return fail(EIGSOL_E_SOLVER, std::string(who) + ": B is not positive definite: the pivot of column " +
                                     std::to_string(col) + " is not > 0");
}

template <class S>
int cholesky_host(eigsol_ctx* ctx, int64_t n, const void* B_host, void* L_host, int64_t* info) {
    hipStream_t st = ctx->stream;
    DevBuf dB, dw;
    EIGSOL_TRY(dB.alloc((size_t)n * n * sizeof(S)));
    EIGSOL_TRY(dw.alloc(sizeof(Words)));
    Words w{-1, 0, 0};
    EIGSOL_HIP(hipMemcpyAsync(dw.p, &w, sizeof(Words), hipMemcpyHostToDevice, st));
    EIGSOL_HIP(hipMemcpyAsync(dB.p, B_host, (size_t)n * n * sizeof(S), hipMemcpyHostToDevice, st));
    Words* W = dw.as<Words>();
    hipLaunchKernelGGL(dev::herm_prepare<S>, dim3(grid_nn(n)), dim3(256), 0, st, dB.as<S>(), (int)n, &W->flag_b);
    EIGSOL_TRY(cholesky_device<S>(st, dB.as<S>(), n, &W->info));
    hipLaunchKernelGGL(dev::zero_strict_upper<S>, dim3(grid_nn(n)), dim3(256), 0, st, dB.as<S>(), (int)n);
    EIGSOL_HIP(hipGetLastError());
    EIGSOL_HIP(hipMemcpyAsync(L_host, dB.p, (size_t)n * n * sizeof(S), hipMemcpyDeviceToHost, st));
    EIGSOL_HIP(hipMemcpyAsync(&w, dw.p, sizeof(Words), hipMemcpyDeviceToHost, st));
    EIGSOL_HIP(hipStreamSynchronize(st));
    if (w.info >= 0) return not_definite("eigsol_cholesky_dense", w.info, info);
    if (w.flag_b) return fail(EIGSOL_E_SOLVER, "eigsol_cholesky_dense: the lower triangle holds a non-finite entry");
    return EIGSOL_OK;
}

template <class S>
int geigh_host(eigsol_ctx* ctx, int64_t n, const void* A_host, const void* B_host, int select, int64_t il, int64_t iu,
               double vl, double vu, int method, double* w_out, void* Z_out, int64_t* m_out, int64_t* not_converged,
               int64_t* info) {
    constexpr int dtype = dtype_of<S>::value;
    hipStream_t st = ctx->stream;
    const bool vectors = Z_out != nullptr;
    const size_t bytes = (size_t)n * n * sizeof(S);
    StageClock clock;   // cholesky, standardise, (the standard problem: timed by eigh), back solve, download
    EIGSOL_TRY(clock.start(5));
    DevBuf dA, dB, dT, dw, dZ;
    EIGSOL_TRY(dA.alloc(bytes));
    EIGSOL_TRY(dB.alloc(bytes));
    EIGSOL_TRY(dT.alloc(bytes));
    EIGSOL_TRY(dw.alloc(sizeof(Words)));
    Words w{-1, 0, 0};
    EIGSOL_HIP(hipMemcpyAsync(dw.p, &w, sizeof(Words), hipMemcpyHostToDevice, st));
    EIGSOL_HIP(hipMemcpyAsync(dA.p, A_host, bytes, hipMemcpyHostToDevice, st));
    EIGSOL_HIP(hipMemcpyAsync(dB.p, B_host, bytes, hipMemcpyHostToDevice, st));
    Words* W = dw.as<Words>();
    S *A = dA.as<S>(), *B = dB.as<S>(), *T = dT.as<S>();
    EIGSOL_TRY(clock.mark(0, st));
    // ---- a, b. mirror both, B = L L^H
    hipLaunchKernelGGL(dev::herm_prepare<S>, dim3(grid_nn(n)), dim3(256), 0, st, A, (int)n, &W->flag_a);
    hipLaunchKernelGGL(dev::herm_prepare<S>, dim3(grid_nn(n)), dim3(256), 0, st, B, (int)n, &W->flag_b);
    EIGSOL_TRY(cholesky_device<S>(st, B, n, &W->info));
    EIGSOL_HIP(hipMemcpyAsync(&w, dw.p, sizeof(Words), hipMemcpyDeviceToHost, st));
    EIGSOL_TRY(clock.mark(1, st));
    // ---- c. C = (L^-1 (L^-1 A)^H)^H, left in dA (eigh_device reads its lower triangle)
    EIGSOL_TRY(trsm_left_lower<S>(st, B, n, n, A, n, n));
    conj_transpose<S>(st, n, A, T);
    EIGSOL_TRY(trsm_left_lower<S>(st, B, n, n, T, n, n));
    conj_transpose<S>(st, n, T, A);
    EIGSOL_HIP(hipGetLastError());
    EIGSOL_TRY(clock.mark(2, st));
    EIGSOL_HIP(hipStreamSynchronize(st));
    if (w.info >= 0) return not_definite("eigsol_geigh_dense", w.info, info);
    if (w.flag_a || w.flag_b)
        return fail(EIGSOL_E_SOLVER, std::string("eigsol_geigh_dense: the lower triangle of ") + (w.flag_b ? "B" : "A") +
                                         " holds a non-finite entry");
    double ms[5];
    double* g = ctx->geigh_ms;
    for (int q = 0; q < 7; ++q) g[q] = 0.0;
    clock.read(ms, 5);
    g[0] = ms[0];
    g[1] = ms[1];
    if (vectors) conj_transpose<S>(st, n, B, T);   // T = L^H, for step e
    else dT.release();
    // ---- d. the standard problem
    EIGSOL_TRY(eigh_device_m(ctx, dtype, n, dA, select, il, iu, vl, vu, method, w_out, vectors, dZ, m_out, not_converged));
    for (int q = 0; q < 4; ++q) g[2 + q] = ctx->eigh_ms[q];
    const int64_t m = *m_out;
    if (!vectors || m == 0) return EIGSOL_OK;
    // ---- e. X = L^-H Y, then the phase convention
    EIGSOL_TRY(clock.mark(3, st));
    EIGSOL_TRY(trsm_left_upper<S>(st, T, n, n, dZ.as<S>(), n, m));
    EIGSOL_TRY(eigh_fix_phase_device(st, dtype, n, m, dZ.p));
    EIGSOL_TRY(clock.mark(4, st));
    EIGSOL_HIP(hipMemcpyAsync(Z_out, dZ.p, (size_t)n * m * sizeof(S), hipMemcpyDeviceToHost, st));
    EIGSOL_TRY(clock.mark(5, st));
    EIGSOL_HIP(hipStreamSynchronize(st));
    clock.read(ms, 5);
    g[6] = ms[3];
    g[5] += ms[4];   // the download counts with eigh's back-transformation
    return EIGSOL_OK;
}

// the checks both entries share, after the null-pointer and selection checks
int check_dtype_order(const char* who, int dtype, int64_t n) {
    if (dtype_wide(dtype) || dtype_single(dtype))
        return fail(EIGSOL_E_UNSUPPORTED, std::string(who) + ": double and complex double matrices only");
    if (!dtype_valid(dtype)) return fail(EIGSOL_E_INVALID, std::string(who) + ": unknown dtype");
    if (n > (dtype == EIGSOL_C128 ? hess_max_order_c128() : hess_max_order_f64()))
        return fail(EIGSOL_E_UNSUPPORTED, std::string(who) + ": n above the order the blocked Hessenberg reduction accepts");
    return EIGSOL_OK;
}

}  // namespace
}  // namespace eigsol

using namespace eigsol;

extern "C" {

int eigsol_cholesky_dense(eigsol_ctx* ctx, int dtype, int64_t n, const void* B_colmajor, void* L_colmajor, int64_t* info) {
    if (info) *info = -1;
    if (n < 0) return fail(EIGSOL_E_INVALID, "eigsol_cholesky_dense: negative order");
    if (n == 0) return EIGSOL_OK;
    if (!ctx || !B_colmajor || !L_colmajor) return fail(EIGSOL_E_INVALID, "eigsol_cholesky_dense: null pointer");
    EIGSOL_TRY(check_dtype_order("eigsol_cholesky_dense", dtype, n));
    EIGSOL_HIP(hipSetDevice(ctx->device));
    return dtype == EIGSOL_C128 ? cholesky_host<cplx>(ctx, n, B_colmajor, L_colmajor, info)
                                : cholesky_host<double>(ctx, n, B_colmajor, L_colmajor, info);
}

int eigsol_geigh_dense_m(eigsol_ctx* ctx, int dtype, int64_t n, const void* A_colmajor, const void* B_colmajor,
                         const eigsol_eigh_options* opts, int32_t method, double* w, void* Z, int64_t* m_out,
                         int64_t* not_converged, int64_t* info) {
    if (info) *info = -1;
    if (method != EIGSOL_EIGH_METHOD_STEIN && method != EIGSOL_EIGH_METHOD_DC)
        return fail(EIGSOL_E_INVALID, "eigsol_geigh_dense: unknown method");
    if (n < 0) return fail(EIGSOL_E_INVALID, "eigsol_geigh_dense: negative order");
    if (n == 0) {
        if (m_out) *m_out = 0;
        if (not_converged) *not_converged = 0;
        return EIGSOL_OK;
    }
    if (!ctx || !A_colmajor || !B_colmajor || !w || !m_out) return fail(EIGSOL_E_INVALID, "eigsol_geigh_dense: null pointer");
    int select;
    int64_t il, iu;
    double vl, vu;
    EIGSOL_TRY(eigh_parse_selection("eigsol_geigh_dense", n, opts, &select, &il, &iu, &vl, &vu));
    EIGSOL_TRY(check_dtype_order("eigsol_geigh_dense", dtype, n));
    EIGSOL_HIP(hipSetDevice(ctx->device));
    return dtype == EIGSOL_C128
               ? geigh_host<cplx>(ctx, n, A_colmajor, B_colmajor, select, il, iu, vl, vu, method, w, Z, m_out, not_converged, info)
               : geigh_host<double>(ctx, n, A_colmajor, B_colmajor, select, il, iu, vl, vu, method, w, Z, m_out, not_converged, info);
}

int eigsol_geigh_dense(eigsol_ctx* ctx, int dtype, int64_t n, const void* A_colmajor, const void* B_colmajor,
                       const eigsol_eigh_options* opts, double* w, void* Z, int64_t* m_out, int64_t* not_converged,
                       int64_t* info) {
    return eigsol_geigh_dense_m(ctx, dtype, n, A_colmajor, B_colmajor, opts, EIGSOL_EIGH_METHOD_STEIN, w, Z, m_out,
                                not_converged, info);
}

int eigsol_geigh_stage_times(eigsol_ctx* ctx, double* ms7) {
    if (!ctx || !ms7) return fail(EIGSOL_E_INVALID, "eigsol_geigh_stage_times: null pointer");
    for (int q = 0; q < 7; ++q) ms7[q] = ctx->geigh_ms[q];
    return EIGSOL_OK;
}

}  // extern "C"
