// Principal matrix square root through the Schur form (gfx950; EIGSOL_F64 and EIGSOL_C128):
//   A = Z T Z^H (schur_device, schur.hip),  U = T^(1/2) on the device,  X = Z U Z^H (two syl_product calls)
// and the triangular stage on its own, U^2 = T for an upper triangular (complex) or quasi-triangular (real, 2 x 2
// blocks with complex eigenvalues) T.  X^2 = A and every eigenvalue of X lies in the closed right half plane.
//
// The triangular stage (Bjorck and Hammarling's recurrence, Higham's real Schur variant, by blocks).  T is cut
// into p blocks by syl_starts with NB = RankKMax<S> (64 real, 32 complex) rows, the partition of the Sylvester
// solvers, so no 2 x 2 block is split.  U starts as a copy of T and is overwritten block by block:
//   1. sqrtm_diag_kernel, one launch, one workgroup per diagonal block: U_ii = T_ii^(1/2) in LDS (below);
//   2. for the block super-diagonals s = 1 .. p - 1, two launches each:
//      a. sqrtm_accumulate: U_ij <- T_ij - sum_{i < k < j} U_ik U_kj for the p - s blocks (i, i + s), one workgroup
//         per block, k ascending through rankk_tile on the matrix cores; each lane reads back the entries it
//         stored itself, so the launch is bit for bit a sequence of rank-K launches.  Left-looking: a tile has
//         one writer and a fixed order.  s = 1: the sum is empty and U_ij is T_ij already, no launch;
//      b. sylvester.hip's syl_block_kernel with its right-hand sides summed first (kSumFirst: the products on
//         their own, taken from f(a, b) once; the Sylvester solvers keep their running difference and their
//         bits), with R = S = F = U, both partitions the starts, no transposition, wavefront d = p - 1 + s from t0 = s: syl_block_of then gives j = t, i = t - s, which is
//         block super-diagonal s.  It solves U_ii Y + Y U_jj = F_ij in place.  Its Kronecker solve assumes nothing
//         of the 2 x 2 blocks' form, and it groups by U_ii's sub-diagonal, non-zero exactly where T's is;
//   3. syl_sum_flags adds the flag slots of all blocks, diagonal ones included.
// That is 1 + 2 (p - 1) launches (one fewer for p > 1: s = 1 has no sum) and no host wait.
//
// A diagonal block in LDS (leading dimension NB + 1).  Its rows are grouped by the 1 x 1 / 2 x 2 diagonal blocks
// of T_ii.  First every group's own root (small_sqrt.hpp): the principal scalar root, or for a real 2 x 2 block
// alpha I + (B - theta I) / (2 alpha).  Then the group super-diagonals e = 1, 2, ..: the pairs (g, g + e) of one e
// are independent; four lanes share a pair, one per entry of its right-hand side
//   t(a, b) - sum_k u(a, k) u(k, b),  k strictly between the two groups, in index order,
// and the first of them solves U_gg Y + Y U_hh = rhs of order 1, 2 or 4 by syl_solve4 (complex: one division by
// Smith's method).  A pivot below smin = max(eps max|U_gg|, 2^-1022 / eps), the maximum over the entries of the
// block's group roots, is replaced by smin and the block's flag slot is set by a plain store.
// No atomics, every sum in a fixed order: two runs give the same bits.  The root of a real T is real, the root
// of a diagonal T is the entrywise principal root.  No overflow scaling.
//
// A real A with a negative real eigenvalue has no real root.  The pass that brings T's sub-diagonal pattern to the
// host (syl_device_pattern, one host wait, n bytes) also carries the sign of the diagonal; a negative 1 x 1 block
// ends the call with *needs_complex = 1 and X untouched, and the caller passes A as complex.  The complex T of
// such a matrix holds its real eigenvalues with imaginary parts of rounding size and either sign, which would put
// their roots on either half of the imaginary axis: where every entry of a complex A is real, sqrtm_real_axis
// sets the imaginary part of a diagonal entry with Re < 0 and |Im| <= n eps ||A||_F to +0 first.
#include <algorithm>
#include <cmath>
#include <cstring>
#include <vector>

#include "schur.hpp"
#include "small_sqrt.hpp"
#include "sqrtm.hpp"
#include "sylvester.hpp"

namespace eigsol {
namespace dev {

__device__ __forceinline__ double sqrtm_scalar(double v) { return sqrt(v); }
__device__ __forceinline__ cplx sqrtm_scalar(cplx v) { return sqrt_principal(v); }

// One workgroup: U_bb = T_bb^(1/2) for diagonal block b = blockIdx.x, in place in U (see the head of this file).
template <class S>
__global__ __launch_bounds__(kSylThreads) void sqrtm_diag_kernel(S* U, int64_t ldu, const int* rs, int p, int* flags) {
    constexpr bool kReal = std::is_same_v<S, double>;
    constexpr int NB = RankKMax<S>::value, LD = NB + 1;
    __shared__ S sU[NB * LD];
    __shared__ S srhs[kSylThreads];
    __shared__ double red[kSylThreads];
    __shared__ int gs[NB + 1];
    __shared__ int ngs, pert;
    const int tid = threadIdx.x, blk = blockIdx.x;
    if (blk >= p) return;
    const int r0 = rs[blk], na = rs[blk + 1] - r0;
    if (na < 1 || na > NB) return;
    for (int idx = tid; idx < na * na; idx += kSylThreads) {
        const int a = idx % na, k = idx / na;
        sU[a + k * LD] = U[(r0 + a) + (int64_t)(r0 + k) * ldu];
    }
    __syncthreads();
    if (tid == 0) {
        int g = 0;
        for (int k = 0; k < na;) {
            gs[g++] = k;
            bool two = false;
            if constexpr (kReal) two = k + 1 < na && sU[(k + 1) + k * LD] != 0.0;
            k += two ? 2 : 1;
        }
        gs[g] = na;
        ngs = g;
        pert = 0;
    }
    __syncthreads();
    const int ng = ngs;
    // ---- the groups' own roots
    double amax = 0.0;
    if (tid < ng) {
        const int k = gs[tid], sz = gs[tid + 1] - k;
        if (sz == 1) {
            const S u = sqrtm_scalar(sU[k + k * LD]);
            sU[k + k * LD] = u;
            amax = mod_abs(u);
        } else if constexpr (kReal) {
            double u[4];
            if (sqrt_block2(sU[k + k * LD], sU[(k + 1) + k * LD], sU[k + (k + 1) * LD], sU[(k + 1) + (k + 1) * LD], u)) {
                sU[k + k * LD] = u[0];
                sU[(k + 1) + k * LD] = u[1];
                sU[k + (k + 1) * LD] = u[2];
                sU[(k + 1) + (k + 1) * LD] = u[3];
                amax = fmax(fmax(fabs(u[0]), fabs(u[1])), fmax(fabs(u[2]), fabs(u[3])));
            } else {
                pert = 1;   // a 2 x 2 block with real eigenvalues: the host entries refuse it
            }
        }
    }
    red[tid] = amax;
    __syncthreads();
    for (int w = kSylThreads / 2; w > 0; w >>= 1) {
        if (tid < w) red[tid] = fmax(red[tid], red[tid + w]);
        __syncthreads();
    }
    const double eps = 2.220446049250313e-16, tiny = 2.2250738585072014e-308;
    const double smin = fmax(eps * red[0], tiny / eps);
    // ---- the group super-diagonals
    const int pr = tid >> 2, sb4 = tid & 3, ia = sb4 & 1, ib = sb4 >> 1;
    for (int e = 1; e < ng; ++e) {
        const bool act = pr < ng - e;
        int a0 = 0, sa = 0, b0 = 0, sb = 0;
        if (act) {
            a0 = gs[pr];
            sa = gs[pr + 1] - a0;
            b0 = gs[pr + e];
            sb = gs[pr + e + 1] - b0;
            if (ia < sa && ib < sb) {
                const int a = a0 + ia, b = b0 + ib;
                // the products are summed on their own and taken from t(a, b) once: a running t(a, b) - .. would
                // round at the size of t(a, b) in every step, which is far above the products away from the diagonal
                S acc = s_zero<S>();
                for (int k = a0 + sa; k < b0; ++k) acc = add(acc, mul(sU[a + k * LD], sU[k + b * LD]));
                srhs[tid] = sub(sU[a + b * LD], acc);
            }
        }
        __syncthreads();
        if (act && sb4 == 0) {
            if constexpr (kReal) {
                const int N = sa * sb;
                double K[4][4], x[4];
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    x[u] = 0.0;
#pragma unroll
                    for (int v = 0; v < 4; ++v) K[u][v] = 0.0;
                }
                // unknown u = ua + sa ub holds y(a0 + ua, b0 + ub)
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    if (u >= N) continue;
                    const int ua = u % sa, ub = u / sa;
                    x[u] = srhs[tid + ua + 2 * ub];
#pragma unroll
                    for (int v = 0; v < 4; ++v) {
                        if (v >= N) continue;
                        const int va = v % sa, vb = v / sa;
                        double kv = 0.0;
                        if (ub == vb) kv += sU[(a0 + ua) + (a0 + va) * LD];
                        if (ua == va) kv += sU[(b0 + vb) + (b0 + ub) * LD];
                        K[u][v] = kv;
                    }
                }
                if (syl_solve4(N, K, x, smin)) pert = 1;
#pragma unroll
                for (int u = 0; u < 4; ++u)
                    if (u < N) sU[(a0 + u % sa) + (b0 + u / sa) * LD] = x[u];
            } else {
                cplx den = add(sU[a0 + a0 * LD], sU[b0 + b0 * LD]);
                if (mod_abs(den) < smin) {
                    den = cplx{smin, 0.0};
                    pert = 1;
                }
                sU[a0 + b0 * LD] = syl_cdiv(srhs[tid], den);
            }
        }
        __syncthreads();
    }
    for (int idx = tid; idx < na * na; idx += kSylThreads) {
        const int a = idx % na, k = idx / na;
        U[(r0 + a) + (int64_t)(r0 + k) * ldu] = sU[a + k * LD];
    }
    if (tid == 0) flags[blk + blk * p] = pert;
}

// U_ij <- U_ij - sum_{i < k < j} U_ik U_kj for block (i, i + s), i = blockIdx.x; U_ij holds T_ij on entry
template <class S>
__global__ __launch_bounds__(256) void sqrtm_accumulate(S* U, int64_t ldu, const int* rs, int p, int s) {
    const int i = blockIdx.x, j = i + s;
    if (j >= p) return;
    const int r0 = rs[i], na = rs[i + 1] - r0, c0 = rs[j], nb = rs[j + 1] - c0;
    for (int k = i + 1; k < j; ++k) {   // each lane reads back the entries of U_ij it stored itself
        const int k0 = rs[k], K = rs[k + 1] - k0;
        rankk_tile<S, true>(0, 0, na, nb, K, -1.0, U + r0 + (int64_t)k0 * ldu, ldu, U + k0 + (int64_t)c0 * ldu, ldu,
                            U + r0 + (int64_t)c0 * ldu, ldu);
    }
}

// A complex T from a matrix whose entries are all real: a diagonal entry left of the imaginary axis with
// |Im| <= tol is a real eigenvalue up to the factorisation's backward error; its imaginary part becomes +0, so
// that its root lies on the positive imaginary axis whatever sign the rounding left.
__global__ __launch_bounds__(256) void sqrtm_real_axis(cplx* T, int64_t n, double tol) {
    const int64_t k = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (k >= n) return;
    cplx* const t = T + k + k * n;
    if (t->re < 0.0 && fabs(t->im) <= tol) t->im = 0.0;
}

}  // namespace dev

// U <- U^(1/2) in place for the (quasi-)triangular device matrix U (leading dimension n) with the starts rs,
// stream-ordered, no host wait.  `work` receives the starts and the flags; *d_pert (device) the number of
// perturbed blocks.  Declared in sqrtm.hpp: logm.hip takes its roots with it.
template <class S>
int trsqrt_device(hipStream_t st, int64_t n, S* U, const std::vector<int>& rs, DevBuf& work, int* d_pert) {
    const int p = (int)rs.size() - 1;
    EIGSOL_TRY(work.alloc(((size_t)p + 1 + (size_t)p * p) * sizeof(int)));
    int* const d_rs = work.as<int>();
    int* const d_flags = d_rs + p + 1;
    EIGSOL_HIP(hipMemcpyAsync(d_rs, rs.data(), (size_t)(p + 1) * sizeof(int), hipMemcpyHostToDevice, st));
    EIGSOL_HIP(hipMemsetAsync(d_flags, 0, (size_t)p * p * sizeof(int), st));
    constexpr size_t lds = dev::syl_lds_bytes<S>();
    EIGSOL_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(dev::syl_block_kernel<S, true>),
                                   hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    hipLaunchKernelGGL(dev::sqrtm_diag_kernel<S>, dim3((unsigned)p), dim3(dev::kSylThreads), 0, st, U, n, d_rs, p, d_flags);
    for (int s = 1; s < p; ++s) {
        if (s > 1) hipLaunchKernelGGL(dev::sqrtm_accumulate<S>, dim3((unsigned)(p - s)), dim3(256), 0, st, U, n, d_rs, p, s);
        hipLaunchKernelGGL((dev::syl_block_kernel<S, true>), dim3((unsigned)(p - s)), dim3(dev::kSylThreads), lds, st, U, n, U, n, U, n, d_rs,
                           d_rs, p, p, p - 1 + s, s, 0, d_flags);
    }
    hipLaunchKernelGGL(dev::syl_sum_flags, dim3(1), dim3(256), 0, st, d_flags, p * p, d_pert);
    EIGSOL_HIP(hipGetLastError());
    return EIGSOL_OK;
}

template int trsqrt_device<double>(hipStream_t, int64_t, double*, const std::vector<int>&, DevBuf&, int*);
template int trsqrt_device<cplx>(hipStream_t, int64_t, cplx*, const std::vector<int>&, DevBuf&, int*);

namespace {

template <class S>
int trsqrt_host(eigsol_ctx* ctx, int64_t n, const void* T_host, void* U_out, int32_t* perturbed) {
    constexpr int NB = dev::RankKMax<S>::value;
    const char* who = "eigsol_trsqrt_dense";
    if (!all_finite<S>(T_host, n * n)) return fail(EIGSOL_E_SOLVER, std::string(who) + ": T holds a non-finite entry");
    std::vector<unsigned char> sub;
    const S* const T = static_cast<const S*>(T_host);
    if (!syl_structure_ok<S>(T, n, sub)) return fail(EIGSOL_E_INVALID, std::string(who) + ": T is not (quasi-)triangular");
    if constexpr (std::is_same_v<S, double>) {
        for (int64_t k = 0; k < n; ++k) {
            const bool lower = k + 1 < n && sub[k], upper = k > 0 && sub[k - 1];
            if (lower) {
                const double d = (T[k + k * n] - T[(k + 1) + (k + 1) * n]) / 2.0;
                if (!(d * d + T[k + (k + 1) * n] * T[(k + 1) + k * n] < 0.0))
                    return fail(EIGSOL_E_INVALID, std::string(who) + ": a 2 x 2 diagonal block of T has real eigenvalues");
            } else if (!upper && T[k + k * n] < 0.0) {
                return fail(EIGSOL_E_INVALID,
                            std::string(who) + ": a negative 1 x 1 diagonal block has no real square root; pass T as complex");
            }
        }
    }
    const std::vector<int> rs = syl_starts(n, NB, sub);
    hipStream_t st = ctx->stream;
    DevBuf dU, work, dpert;
    EIGSOL_TRY(dU.alloc((size_t)n * n * sizeof(S)));
    EIGSOL_TRY(dpert.alloc(sizeof(int)));
    EIGSOL_HIP(hipMemcpyAsync(dU.p, T_host, (size_t)n * n * sizeof(S), hipMemcpyHostToDevice, st));
    EIGSOL_TRY(trsqrt_device<S>(st, n, dU.as<S>(), rs, work, dpert.as<int>()));
    int pert = 0;
    EIGSOL_HIP(hipMemcpyAsync(U_out, dU.p, (size_t)n * n * sizeof(S), hipMemcpyDeviceToHost, st));
    EIGSOL_HIP(hipMemcpyAsync(&pert, dpert.p, sizeof(int), hipMemcpyDeviceToHost, st));
    EIGSOL_HIP(hipStreamSynchronize(st));
    if (perturbed) *perturbed = pert;
    return EIGSOL_OK;
}

template <class S>
int sqrtm_host(eigsol_ctx* ctx, int64_t n, const void* A_host, int max_iter, void* X_out, int32_t* perturbed, int32_t* converged,
               int32_t* needs_complex) {
    constexpr int NB = dev::RankKMax<S>::value;
    if (!all_finite<S>(A_host, n * n)) return fail(EIGSOL_E_SOLVER, "eigsol_sqrtm_dense: the matrix holds a non-finite entry");
    // complex storage of a real matrix (what a caller sends after *needs_complex = 1): its Frobenius norm
    double real_norm = -1.0;
    if constexpr (!std::is_same_v<S, double>) {
        const cplx* const a = static_cast<const cplx*>(A_host);
        double big = 0.0, ssq = 0.0;
        bool real_input = true;
        for (int64_t i = 0; i < n * n && real_input; ++i) {
            real_input = a[i].im == 0.0;
            big = std::max(big, std::fabs(a[i].re));
        }
        if (real_input && big > 0.0) {
            for (int64_t i = 0; i < n * n; ++i) ssq += (a[i].re / big) * (a[i].re / big);
            real_norm = big * std::sqrt(ssq);
        }
    }
    hipStream_t st = ctx->stream;
    StageClock clock, clock_s;
    EIGSOL_TRY(clock.start(3));
    EIGSOL_TRY(clock_s.start(4));
    for (int k = 0; k < 4; ++k) ctx->sqrtm_ms[k] = 0.0;
    if (perturbed) *perturbed = 0;
    if (needs_complex) *needs_complex = 0;
    SchurDevice sd;
    EIGSOL_TRY(clock.mark(0, st));
    EIGSOL_TRY(schur_device<S>(ctx, n, A_host, max_iter, true, sd, clock_s));
    sd.w.release();
    sd.rot.release();
    EIGSOL_TRY(clock.mark(1, st));
    if (sd.failed) {
        EIGSOL_HIP(hipStreamSynchronize(st));
        clock.read(ctx->sqrtm_ms, 1);
        ctx->sqrtm_ms[3] = ctx->sqrtm_ms[0];
        if (converged) *converged = 0;
        return EIGSOL_OK;
    }
    // ---- the partition and the sign of the 1 x 1 blocks (one host wait, n bytes)
    DevBuf scratch, work, dpert, dW, dX;
    std::vector<unsigned char> sub;
    bool neg = false;
    EIGSOL_TRY(syl_device_pattern<S>(st, sd.T.as<S>(), n, scratch, sub, &neg));
    if (neg) {   // a negative real eigenvalue: no real root; the caller runs the complex path
        clock.read(ctx->sqrtm_ms, 1);
        ctx->sqrtm_ms[3] = ctx->sqrtm_ms[0];
        if (converged) *converged = 1;
        if (needs_complex) *needs_complex = 1;
        return EIGSOL_OK;
    }
    const std::vector<int> rs = syl_starts(n, NB, sub);
    EIGSOL_TRY(dpert.alloc(sizeof(int)));
    EIGSOL_TRY(dW.alloc((size_t)n * n * sizeof(S)));
    EIGSOL_TRY(dX.alloc((size_t)n * n * sizeof(S)));
    // ---- U = T^(1/2) in place in T
    S* const U = sd.T.as<S>();
    if constexpr (!std::is_same_v<S, double>) {
        if (real_norm > 0.0)
            hipLaunchKernelGGL(dev::sqrtm_real_axis, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, U, n,
                               (double)n * 2.220446049250313e-16 * real_norm);
    }
    const S* const Z = sd.Z.as<S>();
    EIGSOL_TRY(trsqrt_device<S>(st, n, U, rs, work, dpert.as<int>()));
    EIGSOL_TRY(clock.mark(2, st));
    // ---- X = Z U Z^H
    EIGSOL_TRY(syl_product<S>(st, false, n, n, n, Z, n, U, n, dW.as<S>()));     // W = Z U
    EIGSOL_TRY(syl_product<S>(st, true, n, n, n, dW.as<S>(), n, Z, n, dX.as<S>()));   // X = W Z^H
    int pert = 0;
    EIGSOL_HIP(hipMemcpyAsync(X_out, dX.p, (size_t)n * n * sizeof(S), hipMemcpyDeviceToHost, st));
    EIGSOL_HIP(hipMemcpyAsync(&pert, dpert.p, sizeof(int), hipMemcpyDeviceToHost, st));
    EIGSOL_TRY(clock.mark(3, st));
    EIGSOL_HIP(hipStreamSynchronize(st));
    clock.read(ctx->sqrtm_ms, 3);
    ctx->sqrtm_ms[3] = ctx->sqrtm_ms[0] + ctx->sqrtm_ms[1] + ctx->sqrtm_ms[2];
    if (perturbed) *perturbed = pert;
    if (converged) *converged = 1;
    return EIGSOL_OK;
}

}  // namespace
}  // namespace eigsol

using namespace eigsol;

extern "C" {

int eigsol_trsqrt_dense(eigsol_ctx* ctx, int dtype, int64_t n, const void* T_colmajor, void* U_out, int32_t* perturbed) {
    if (n < 0) return fail(EIGSOL_E_INVALID, "eigsol_trsqrt_dense: negative order");
    if (!ctx) return fail(EIGSOL_E_INVALID, "eigsol_trsqrt_dense: null context");
    if (n == 0) {
        if (perturbed) *perturbed = 0;
        return EIGSOL_OK;
    }
    if (!T_colmajor || !U_out) return fail(EIGSOL_E_INVALID, "eigsol_trsqrt_dense: null pointer");
    EIGSOL_TRY(syl_check_args("eigsol_trsqrt_dense", ctx, dtype, n, n));
    return dtype == EIGSOL_C128 ? trsqrt_host<cplx>(ctx, n, T_colmajor, U_out, perturbed)
                                : trsqrt_host<double>(ctx, n, T_colmajor, U_out, perturbed);
}

int eigsol_sqrtm_dense(eigsol_ctx* ctx, int dtype, int64_t n, const void* A_colmajor, const eigsol_solver_options* opts,
                       void* X_out, int32_t* perturbed, int32_t* converged, int32_t* needs_complex) {
    const char* who = "eigsol_sqrtm_dense";
    if (n < 0) return fail(EIGSOL_E_INVALID, std::string(who) + ": negative order");
    if (!ctx) return fail(EIGSOL_E_INVALID, std::string(who) + ": null context");
    const int max_iter = opts ? opts->max_iterations : 1000;
    if (n == 0) {
        if (perturbed) *perturbed = 0;
        if (converged) *converged = 1;
        if (needs_complex) *needs_complex = 0;
        return EIGSOL_OK;
    }
    if (!A_colmajor || !X_out) return fail(EIGSOL_E_INVALID, std::string(who) + ": null pointer");
    if (max_iter < 1) return fail(EIGSOL_E_INVALID, std::string(who) + ": max_iterations < 1");
    EIGSOL_TRY(syl_check_args(who, ctx, dtype, n, n));
    return dtype == EIGSOL_C128 ? sqrtm_host<cplx>(ctx, n, A_colmajor, max_iter, X_out, perturbed, converged, needs_complex)
                                : sqrtm_host<double>(ctx, n, A_colmajor, max_iter, X_out, perturbed, converged, needs_complex);
}

int eigsol_sqrtm_stage_times(eigsol_ctx* ctx, double* ms4) {
    if (!ctx || !ms4) return fail(EIGSOL_E_INVALID, "eigsol_sqrtm_stage_times: null pointer");
    for (int q = 0; q < 4; ++q) ms4[q] = ctx->sqrtm_ms[q];
    return EIGSOL_OK;
}

}  // extern "C"
