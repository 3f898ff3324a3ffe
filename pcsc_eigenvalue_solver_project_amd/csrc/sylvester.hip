// Sylvester and Lyapunov equations by Bartels-Stewart (gfx950; EIGSOL_F64 and EIGSOL_C128):
//   A X + X B = C      A = U R U^H, B = V S V^H (schur_device, schur.hip), F = U^H C V, R Y + Y S = F, X = U Y V^H
//   A X + X A^H = Q    one Schur form, F = U^H Q U, R Y + Y R^H = F, X = U Y U^H
// and the triangular stage on its own, R Y + Y op(S) = F in place in F, op(S) = S or S^H (trans_b).
//
// The triangular stage.  R (m x m) and S (n x n) are upper triangular (complex) or quasi-triangular with
// schur's standard 2 x 2 blocks (real).  Each is cut into blocks of NB = RankKMax<S> (64 real, 32 complex)
// rows; a boundary that would split a 2 x 2 block moves up one row, so a block has NB - 1 or NB rows.  The
// starts are computed on the host (syl_starts) from the sub-diagonal's non-zero pattern, which
// eigsol_trsyl_dense has on the host and the full drivers download with one host wait (n bytes per matrix)
// before the first wavefront; the loop itself has no host wait.
//   Block (i, j) of Y needs the blocks below it in its block column and the blocks left of it in its block
// row (right of it with trans_b).  Wavefront d = (p - 1 - i) + t, t = j (q - 1 - j with trans_b), of the
// p x q blocks is three launches:
//   1. syl_block_kernel, one workgroup per block: R_ii Y_ij + Y_ij op(S_jj) = F_ij in LDS;
//   2. syl_update_cols: F(0:s_i, j) -= R(0:s_i, i) Y_ij, 64 x 64 tiles of rankk_tile, all blocks in one launch
//      (targets in different block columns);
//   3. syl_update_rows: F(i, rest) -= Y_ij op(S)(j, rest), likewise (targets in different block rows).
// A column update of one block and a row update of another meet in one tile of F, hence two launches.
//   The block kernel keeps R_ii, S_jj and F_ij in LDS with leading dimension NB + 1 (65 doubles / 33 cplx:
// 3 x 64 x 65 x 8 = 99840 bytes real, 3 x 32 x 33 x 16 = 50688 bytes complex, of the CU's 160 KB); the odd
// leading dimension puts a walk along a row and the lanes' different rows and columns on different banks.
// Unknowns are grouped by the 1 x 1 / 2 x 2 diagonal blocks of R_ii (row groups) and S_jj (column groups);
// the group pairs of one anti-diagonal are independent, so there are (row groups + column groups - 1)
// dependent steps.  Four lanes share a pair, one per entry of its right-hand side
//   f(a, b) - R(a, below) y(below, b) - y(a, before) op(S)(before, b)
// and the first of them solves the pair's system of order 1, 2 or 4 by Gaussian elimination with complete
// pivoting (LAPACK dlasy2's method); complex unknowns are 1 x 1, y = rhs / (r_aa + op(s)_bb).  A pivot
// below smin = max(eps max(max|R_ii|, max|S_jj|), 2^-1022 / eps) in modulus is replaced by smin and the
// workgroup stores 1 to its slot of the flag array; syl_sum_flags adds the slots after the last wavefront.
// No atomics and every sum in a fixed order: two runs give the same bits.  No overflow scale factor.
//
// The four products of the transforms (syl_gemm) add K = NB columns at a time into a zeroed output through
// rankk_tile, in ascending order inside one launch: the workgroup that owns a 64 x 64 tile of the output walks
// the chunks itself, which is what a sequence of rankk_update launches would compute, without the launches.
#include <algorithm>
#include <cmath>
#include <cstring>
#include <vector>

#include "schur.hpp"
#include "sylvester.hpp"   // the partition rule, syl_block_kernel, syl_gemm and the host checks: shared with sqrtm.hip

namespace eigsol {
namespace dev {

// pat[k], k < n: bit 0: T(k + 1, k) != 0 (k < n - 1), bit 1: T(k, k) < 0
__global__ __launch_bounds__(256) void syl_subdiag(const double* T, int64_t n, unsigned char* pat) {
    const int64_t k = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (k >= n) return;
    const int nz = k + 1 < n && T[(k + 1) + k * n] != 0.0 ? 1 : 0;
    pat[k] = (unsigned char)(nz | (T[k + k * n] < 0.0 ? 2 : 0));
}

// F(0:s_i, block column j) -= R(0:s_i, block i) Y_ij for block t0 + blockIdx.z of wavefront d
template <class S>
__global__ __launch_bounds__(256) void syl_update_cols(const S* R, int64_t ldr, S* F, int64_t ldf, const int* rs, const int* cs,
                                                       int p, int q, int d, int t0, int trans) {
    int i, j;
    if (!syl_block_of(t0 + (int)blockIdx.z, p, q, d, trans, i, j)) return;
    const int r0 = rs[i], K = rs[i + 1] - r0, c0 = cs[j], nn = cs[j + 1] - c0;
    if ((int)blockIdx.x * 64 >= r0) return;
    rankk_tile<S, true>(blockIdx.x, 0, r0, nn, K, -1.0, R + (int64_t)r0 * ldr, ldr, F + r0 + (int64_t)c0 * ldf, ldf,
                        F + (int64_t)c0 * ldf, ldf);
}

// F(block row i, rest) -= Y_ij op(S)(block j, rest): rest is right of block column j, or left of it (kTrans)
template <class S, bool kTrans>
__global__ __launch_bounds__(256) void syl_update_rows(const S* Sm, int64_t lds, S* F, int64_t ldf, int n, const int* rs,
                                                       const int* cs, int p, int q, int d, int t0) {
    int i, j;
    if (!syl_block_of(t0 + (int)blockIdx.z, p, q, d, kTrans ? 1 : 0, i, j)) return;
    const int r0 = rs[i], mr = rs[i + 1] - r0, c0 = cs[j], c1 = cs[j + 1], K = c1 - c0;
    const S* const Y = F + r0 + (int64_t)c0 * ldf;
    if constexpr (!kTrans) {
        const int nn = n - c1;
        if ((int)blockIdx.y * 64 >= nn) return;
        rankk_tile<S, true>(0, blockIdx.y, mr, nn, K, -1.0, Y, ldf, Sm + c0 + (int64_t)c1 * lds, lds, F + r0 + (int64_t)c1 * ldf, ldf);
    } else {
        const int nn = c0;
        if ((int)blockIdx.y * 64 >= nn) return;
        rankk_tile<S, false, true>(0, blockIdx.y, mr, nn, K, -1.0, Y, ldf, Sm + (int64_t)c0 * lds, lds, F + r0, ldf);
    }
}

__global__ __launch_bounds__(256) void syl_sum_flags(const int* flags, int cnt, int* out) {
    __shared__ int part[256];
    int s = 0;
    for (int k = threadIdx.x; k < cnt; k += 256) s += flags[k];
    part[threadIdx.x] = s;
    __syncthreads();
    for (int w = 128; w > 0; w >>= 1) {
        if ((int)threadIdx.x < w) part[threadIdx.x] += part[threadIdx.x + w];
        __syncthreads();
    }
    if (threadIdx.x == 0) *out = part[0];
}

}  // namespace dev

std::vector<int> syl_starts(int64_t n, int NB, const std::vector<unsigned char>& sub) {
    std::vector<int> s{0};
    while (s.back() < n) {
        int e = (int)std::min<int64_t>((int64_t)s.back() + NB, n);
        if (e < n && !sub.empty() && sub[e - 1]) --e;
        s.push_back(e);
    }
    return s;
}

int syl_check_args(const char* who, eigsol_ctx* ctx, int dtype, int64_t m, int64_t n) {
    if (dtype_wide(dtype) || dtype_single(dtype))
        return fail(EIGSOL_E_UNSUPPORTED, std::string(who) + ": double and complex double matrices only");
    if (!dtype_valid(dtype)) return fail(EIGSOL_E_INVALID, std::string(who) + ": unknown dtype");
    if (std::max(m, n) > (dtype == EIGSOL_C128 ? hess_max_order_c128() : hess_max_order_f64()))
        return fail(EIGSOL_E_UNSUPPORTED, std::string(who) + ": an order above the one the blocked Hessenberg reduction accepts");
    EIGSOL_HIP(hipSetDevice(ctx->device));
    return EIGSOL_OK;
}

namespace {

// The triangular stage on device arrays (leading dimensions m, n, m), stream-ordered, no host wait.  `work`
// receives the starts and the flags; *d_pert (device) the number of perturbed blocks.
template <class S>
int trsyl_device(hipStream_t st, int64_t m, int64_t n, const S* R, const S* Sm, bool trans, S* F, const std::vector<int>& rs,
                 const std::vector<int>& cs, DevBuf& work, int* d_pert) {
    const int p = (int)rs.size() - 1, q = (int)cs.size() - 1;
    EIGSOL_TRY(work.alloc(((size_t)p + q + 2 + (size_t)p * q) * sizeof(int)));
    int* const d_rs = work.as<int>();
    int* const d_cs = d_rs + p + 1;
    int* const d_flags = d_cs + q + 1;
    EIGSOL_HIP(hipMemcpyAsync(d_rs, rs.data(), (size_t)(p + 1) * sizeof(int), hipMemcpyHostToDevice, st));
    EIGSOL_HIP(hipMemcpyAsync(d_cs, cs.data(), (size_t)(q + 1) * sizeof(int), hipMemcpyHostToDevice, st));
    EIGSOL_HIP(hipMemsetAsync(d_flags, 0, (size_t)p * q * sizeof(int), st));
    constexpr size_t lds = dev::syl_lds_bytes<S>();
    EIGSOL_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(dev::syl_block_kernel<S>),
                                   hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    const unsigned trow = (unsigned)((m + 63) / 64), tcol = (unsigned)((n + 63) / 64);
    const int tr = trans ? 1 : 0;
    for (int d = 0; d < p + q - 1; ++d) {
        const int t0 = std::max(0, d - (p - 1)), cnt = std::min(d, q - 1) - t0 + 1;
        hipLaunchKernelGGL(dev::syl_block_kernel<S>, dim3((unsigned)cnt), dim3(dev::kSylThreads), lds, st, R, m, Sm, n, F, m, d_rs,
                           d_cs, p, q, d, t0, tr, d_flags);
        if (p > 1)
            hipLaunchKernelGGL(dev::syl_update_cols<S>, dim3(trow, 1, (unsigned)cnt), dim3(256), 0, st, R, m, F, m, d_rs, d_cs, p, q,
                               d, t0, tr);
        if (q > 1) {
            if (trans)
                hipLaunchKernelGGL((dev::syl_update_rows<S, true>), dim3(1, tcol, (unsigned)cnt), dim3(256), 0, st, Sm, n, F, m,
                                   (int)n, d_rs, d_cs, p, q, d, t0);
            else
                hipLaunchKernelGGL((dev::syl_update_rows<S, false>), dim3(1, tcol, (unsigned)cnt), dim3(256), 0, st, Sm, n, F, m,
                                   (int)n, d_rs, d_cs, p, q, d, t0);
        }
    }
    hipLaunchKernelGGL(dev::syl_sum_flags, dim3(1), dim3(256), 0, st, d_flags, p * q, d_pert);
    EIGSOL_HIP(hipGetLastError());
    return EIGSOL_OK;
}

template <class S>
int trsyl_host(eigsol_ctx* ctx, int64_t m, int64_t n, const void* R_host, const void* S_host, bool trans, void* F_inout,
               int32_t* perturbed) {
    constexpr int NB = dev::RankKMax<S>::value;
    if (!all_finite<S>(R_host, m * m) || !all_finite<S>(S_host, n * n) || !all_finite<S>(F_inout, m * n))
        return fail(EIGSOL_E_SOLVER, "eigsol_trsyl_dense: an input holds a non-finite entry");
    std::vector<unsigned char> subr, subs;
    if (!syl_structure_ok<S>(static_cast<const S*>(R_host), m, subr))
        return fail(EIGSOL_E_INVALID, "eigsol_trsyl_dense: R is not (quasi-)triangular");
    if (!syl_structure_ok<S>(static_cast<const S*>(S_host), n, subs))
        return fail(EIGSOL_E_INVALID, "eigsol_trsyl_dense: S is not (quasi-)triangular");
    const std::vector<int> rs = syl_starts(m, NB, subr), cs = syl_starts(n, NB, subs);
    hipStream_t st = ctx->stream;
    DevBuf dR, dS, dF, work, dpert;
    EIGSOL_TRY(dR.alloc((size_t)m * m * sizeof(S)));
    EIGSOL_TRY(dS.alloc((size_t)n * n * sizeof(S)));
    EIGSOL_TRY(dF.alloc((size_t)m * n * sizeof(S)));
    EIGSOL_TRY(dpert.alloc(sizeof(int)));
    EIGSOL_HIP(hipMemcpyAsync(dR.p, R_host, (size_t)m * m * sizeof(S), hipMemcpyHostToDevice, st));
    EIGSOL_HIP(hipMemcpyAsync(dS.p, S_host, (size_t)n * n * sizeof(S), hipMemcpyHostToDevice, st));
    EIGSOL_HIP(hipMemcpyAsync(dF.p, F_inout, (size_t)m * n * sizeof(S), hipMemcpyHostToDevice, st));
    EIGSOL_TRY(trsyl_device<S>(st, m, n, dR.as<S>(), dS.as<S>(), trans, dF.as<S>(), rs, cs, work, dpert.as<int>()));
    int pert = 0;
    EIGSOL_HIP(hipMemcpyAsync(F_inout, dF.p, (size_t)m * n * sizeof(S), hipMemcpyDeviceToHost, st));
    EIGSOL_HIP(hipMemcpyAsync(&pert, dpert.p, sizeof(int), hipMemcpyDeviceToHost, st));
    EIGSOL_HIP(hipStreamSynchronize(st));
    if (perturbed) *perturbed = pert;
    return EIGSOL_OK;
}

// B_host null: the Lyapunov equation A X + X A^H = C (m == n)
template <class S>
int sylvester_host(eigsol_ctx* ctx, const char* who, int64_t m, int64_t n, const void* A_host, const void* B_host,
                   const void* C_host, int max_iter, void* X_out, int32_t* perturbed, int32_t* converged) {
    constexpr int NB = dev::RankKMax<S>::value;
    const bool lyap = B_host == nullptr;
    if (!all_finite<S>(A_host, m * m) || (!lyap && !all_finite<S>(B_host, n * n)) || !all_finite<S>(C_host, m * n))
        return fail(EIGSOL_E_SOLVER, std::string(who) + ": an input holds a non-finite entry");
    hipStream_t st = ctx->stream;
    StageClock clock, clock_a, clock_b;
    EIGSOL_TRY(clock.start(5));
    EIGSOL_TRY(clock_a.start(4));
    EIGSOL_TRY(clock_b.start(4));
    for (int k = 0; k < 5; ++k) ctx->sylvester_ms[k] = 0.0;
    SchurDevice sa, sb;
    EIGSOL_TRY(clock.mark(0, st));
    EIGSOL_TRY(schur_device<S>(ctx, m, A_host, max_iter, true, sa, clock_a));
    sa.w.release();
    sa.rot.release();
    EIGSOL_TRY(clock.mark(1, st));
    if (!lyap) {
        EIGSOL_TRY(schur_device<S>(ctx, n, B_host, max_iter, true, sb, clock_b));
        sb.w.release();
        sb.rot.release();
    }
    EIGSOL_TRY(clock.mark(2, st));
    if (sa.failed || sb.failed) {
        EIGSOL_HIP(hipStreamSynchronize(st));
        clock.read(ctx->sylvester_ms, 2);
        if (converged) *converged = 0;
        if (perturbed) *perturbed = 0;
        return EIGSOL_OK;
    }
    const S* const U = sa.Z.as<S>();
    const S* const R = sa.T.as<S>();
    const S* const V = lyap ? U : sb.Z.as<S>();
    const S* const Sm = lyap ? R : sb.T.as<S>();
    // ---- the partition (one host wait), then F = U^H C V
    DevBuf scratch, dC, dW, dUt, work, dpert;
    std::vector<unsigned char> subr, subs;
    EIGSOL_TRY(syl_device_pattern<S>(st, R, m, scratch, subr));
    if (!lyap) EIGSOL_TRY(syl_device_pattern<S>(st, Sm, n, scratch, subs));
    const std::vector<int> rs = syl_starts(m, NB, subr), cs = lyap ? rs : syl_starts(n, NB, subs);
    EIGSOL_TRY(dC.alloc((size_t)m * n * sizeof(S)));
    EIGSOL_TRY(dW.alloc((size_t)m * n * sizeof(S)));
    EIGSOL_TRY(dUt.alloc((size_t)m * m * sizeof(S)));
    EIGSOL_TRY(dpert.alloc(sizeof(int)));
    EIGSOL_HIP(hipMemcpyAsync(dC.p, C_host, (size_t)m * n * sizeof(S), hipMemcpyHostToDevice, st));
    hipLaunchKernelGGL(dev::conj_transpose<S>, dim3((unsigned)((m + 31) / 32), (unsigned)((m + 31) / 32)), dim3(256), 0, st,
                       (int)m, (int)m, U, m, dUt.as<S>(), m);
    EIGSOL_TRY(syl_product<S>(st, false, m, n, m, dUt.as<S>(), m, dC.as<S>(), m, dW.as<S>()));   // W = U^H C
    EIGSOL_TRY(syl_product<S>(st, false, m, n, n, dW.as<S>(), m, V, n, dC.as<S>()));             // F = W V
    EIGSOL_TRY(clock.mark(3, st));
    // ---- R Y + Y op(S) = F
    EIGSOL_TRY(trsyl_device<S>(st, m, n, R, Sm, lyap, dC.as<S>(), rs, cs, work, dpert.as<int>()));
    EIGSOL_TRY(clock.mark(4, st));
    // ---- X = U Y V^H
    EIGSOL_TRY(syl_product<S>(st, false, m, n, m, U, m, dC.as<S>(), m, dW.as<S>()));   // W = U Y
    EIGSOL_TRY(syl_product<S>(st, true, m, n, n, dW.as<S>(), m, V, n, dC.as<S>()));    // X = W V^H
    int pert = 0;
    EIGSOL_HIP(hipMemcpyAsync(X_out, dC.p, (size_t)m * n * sizeof(S), hipMemcpyDeviceToHost, st));
    EIGSOL_HIP(hipMemcpyAsync(&pert, dpert.p, sizeof(int), hipMemcpyDeviceToHost, st));
    EIGSOL_TRY(clock.mark(5, st));
    EIGSOL_HIP(hipStreamSynchronize(st));
    clock.read(ctx->sylvester_ms, 5);
    if (perturbed) *perturbed = pert;
    if (converged) *converged = 1;
    return EIGSOL_OK;
}

}  // namespace
}  // namespace eigsol

using namespace eigsol;

extern "C" {

int eigsol_trsyl_dense(eigsol_ctx* ctx, int dtype, int64_t m, int64_t n, const void* R_colmajor, const void* S_colmajor,
                       int trans_b, void* F_inout, int32_t* perturbed) {
    if (m < 0 || n < 0) return fail(EIGSOL_E_INVALID, "eigsol_trsyl_dense: negative order");
    if (!ctx) return fail(EIGSOL_E_INVALID, "eigsol_trsyl_dense: null context");
    if (m == 0 || n == 0) {
        if (perturbed) *perturbed = 0;
        return EIGSOL_OK;
    }
    if (!R_colmajor || !S_colmajor || !F_inout) return fail(EIGSOL_E_INVALID, "eigsol_trsyl_dense: null pointer");
    EIGSOL_TRY(syl_check_args("eigsol_trsyl_dense", ctx, dtype, m, n));
    return dtype == EIGSOL_C128 ? trsyl_host<cplx>(ctx, m, n, R_colmajor, S_colmajor, trans_b != 0, F_inout, perturbed)
                                : trsyl_host<double>(ctx, m, n, R_colmajor, S_colmajor, trans_b != 0, F_inout, perturbed);
}

int eigsol_sylvester_dense(eigsol_ctx* ctx, int dtype, int64_t m, int64_t n, const void* A_colmajor, const void* B_colmajor,
                           const void* C_colmajor, const eigsol_solver_options* opts, void* X_out, int32_t* perturbed,
                           int32_t* converged) {
    const char* who = "eigsol_sylvester_dense";
    if (m < 0 || n < 0) return fail(EIGSOL_E_INVALID, std::string(who) + ": negative order");
    if (!ctx) return fail(EIGSOL_E_INVALID, std::string(who) + ": null context");
    const int max_iter = opts ? opts->max_iterations : 1000;
    if (m == 0 || n == 0) {
        if (perturbed) *perturbed = 0;
        if (converged) *converged = 1;
        return EIGSOL_OK;
    }
    if (!A_colmajor || !B_colmajor || !C_colmajor || !X_out) return fail(EIGSOL_E_INVALID, std::string(who) + ": null pointer");
    if (max_iter < 1) return fail(EIGSOL_E_INVALID, std::string(who) + ": max_iterations < 1");
    EIGSOL_TRY(syl_check_args(who, ctx, dtype, m, n));
    return dtype == EIGSOL_C128
               ? sylvester_host<cplx>(ctx, who, m, n, A_colmajor, B_colmajor, C_colmajor, max_iter, X_out, perturbed, converged)
               : sylvester_host<double>(ctx, who, m, n, A_colmajor, B_colmajor, C_colmajor, max_iter, X_out, perturbed, converged);
}

int eigsol_lyapunov_dense(eigsol_ctx* ctx, int dtype, int64_t n, const void* A_colmajor, const void* Q_colmajor,
                          const eigsol_solver_options* opts, void* X_out, int32_t* perturbed, int32_t* converged) {
    const char* who = "eigsol_lyapunov_dense";
    if (n < 0) return fail(EIGSOL_E_INVALID, std::string(who) + ": negative order");
    if (!ctx) return fail(EIGSOL_E_INVALID, std::string(who) + ": null context");
    const int max_iter = opts ? opts->max_iterations : 1000;
    if (n == 0) {
        if (perturbed) *perturbed = 0;
        if (converged) *converged = 1;
        return EIGSOL_OK;
    }
    if (!A_colmajor || !Q_colmajor || !X_out) return fail(EIGSOL_E_INVALID, std::string(who) + ": null pointer");
    if (max_iter < 1) return fail(EIGSOL_E_INVALID, std::string(who) + ": max_iterations < 1");
    EIGSOL_TRY(syl_check_args(who, ctx, dtype, n, n));
    return dtype == EIGSOL_C128
               ? sylvester_host<cplx>(ctx, who, n, n, A_colmajor, nullptr, Q_colmajor, max_iter, X_out, perturbed, converged)
               : sylvester_host<double>(ctx, who, n, n, A_colmajor, nullptr, Q_colmajor, max_iter, X_out, perturbed, converged);
}

int eigsol_sylvester_stage_times(eigsol_ctx* ctx, double* ms5) {
    if (!ctx || !ms5) return fail(EIGSOL_E_INVALID, "eigsol_sylvester_stage_times: null pointer");
    for (int q = 0; q < 5; ++q) ms5[q] = ctx->sylvester_ms[q];
    return EIGSOL_OK;
}

}  // extern "C"
