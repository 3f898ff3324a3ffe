// The pieces of sylvester.hip that the matrix square root (sqrtm.hip) runs too: the partition rule,
// the one-workgroup block solve R_ii Y + Y op(S_jj) = F_ij, the in-order product of the transforms, the host
// checks and the sub-diagonal pattern.  See the head of sylvester.hip for the method.
#pragma once

#include <algorithm>
#include <cmath>
#include <string>
#include <vector>

#include "kernels_common.hpp"
#include "mfma_rankk.hpp"
#include "scratch.hpp"
#include "small_solve.hpp"

namespace eigsol {
namespace dev {

// a / b by Smith's method (no overflow in |b|^2)
__device__ inline cplx syl_cdiv(cplx a, cplx b) {
    if (fabs(b.re) >= fabs(b.im)) {
        const double r = b.im / b.re, den = b.re + b.im * r;
        return cplx{(a.re + a.im * r) / den, (a.im - a.re * r) / den};
    }
    const double r = b.re / b.im, den = b.re * r + b.im;
    return cplx{(a.re * r + a.im) / den, (a.im * r - a.re) / den};
}

// pat[k] (k < n): bit 0: T(k + 1, k) != 0 (k < n - 1); bit 1: T(k, k) < 0.  sylvester.hip
__global__ __launch_bounds__(256) void syl_subdiag(const double* T, int64_t n, unsigned char* pat);
__global__ __launch_bounds__(256) void syl_sum_flags(const int* flags, int cnt, int* out);

// C (m x nn) += L (m x kk) op(R): kRT: R is kk x nn; else R is nn x kk and op is the (conjugate) transpose
template <class S, bool kRT, bool kConj>
__global__ __launch_bounds__(256) void syl_gemm(int m, int nn, int kk, const S* L, int64_t ldl, const S* R, int64_t ldr, S* C,
                                                int64_t ldc) {
    constexpr int NB = RankKMax<S>::value;
    for (int k0 = 0; k0 < kk; k0 += NB)   // each lane reads back the entries of C it stored itself
        rankk_tile<S, kRT, kConj>(blockIdx.x, blockIdx.y, m, nn, min(NB, kk - k0), 1.0, L + (int64_t)k0 * ldl, ldl,
                                  kRT ? R + k0 : R + (int64_t)k0 * ldr, ldr, C, ldc);
}

// block t of wavefront d: block row i, block column j
__device__ __forceinline__ bool syl_block_of(int t, int p, int q, int d, int trans, int& i, int& j) {
    i = p - 1 - (d - t);
    j = trans ? q - 1 - t : t;
    return t >= 0 && t < q && i >= 0 && i < p;
}

constexpr int kSylThreads = 256;

template <class S> constexpr size_t syl_lds_bytes() {
    return (size_t)3 * RankKMax<S>::value * (RankKMax<S>::value + 1) * sizeof(S);
}

// One workgroup solves block t0 + blockIdx.x of wavefront d in LDS (see the head of sylvester.hip).
// kSumFirst (off for the Sylvester solvers, whose bits it leaves as they were; on for sqrtm.hip): a right-hand
// side's products are summed on their own and taken from f(a, b) once, instead of a running f(a, b) - .. that
// rounds at the size of f(a, b) in every step.  It matters where the products are far below f(a, b), as in the
// square-root recurrence away from the diagonal.
template <class S, bool kSumFirst = false>
__global__ __launch_bounds__(kSylThreads) void syl_block_kernel(const S* R, int64_t ldr, const S* Sm, int64_t lds, S* F, int64_t ldf,
                                                               const int* rs, const int* cs, int p, int q, int d, int t0,
                                                               int trans, int* flags) {
    constexpr bool kReal = std::is_same_v<S, double>;
    constexpr int NB = RankKMax<S>::value, LD = NB + 1;
    extern __shared__ __align__(16) unsigned char syl_lds[];
    S* const sR = reinterpret_cast<S*>(syl_lds);
    S* const sS = sR + NB * LD;
    S* const sF = sS + NB * LD;
    __shared__ S srhs[kSylThreads];
    __shared__ double red[kSylThreads];
    __shared__ int ga[NB + 1], gb[NB + 1];
    __shared__ int ng[2], pert;
    const int tid = threadIdx.x;
    int i, j;
    if (!syl_block_of(t0 + (int)blockIdx.x, p, q, d, trans, i, j)) return;
    const int r0 = rs[i], na = rs[i + 1] - r0, c0 = cs[j], nb = cs[j + 1] - c0;
    if (na < 1 || na > NB || nb < 1 || nb > NB) return;
    double amax = 0.0;
    for (int idx = tid; idx < na * na; idx += kSylThreads) {
        const int a = idx % na, k = idx / na;
        const S v = R[(r0 + a) + (int64_t)(r0 + k) * ldr];
        sR[a + k * LD] = v;
        amax = fmax(amax, mod_abs(v));
    }
    for (int idx = tid; idx < nb * nb; idx += kSylThreads) {
        const int a = idx % nb, k = idx / nb;
        const S v = Sm[(c0 + a) + (int64_t)(c0 + k) * lds];
        sS[a + k * LD] = v;
        amax = fmax(amax, mod_abs(v));
    }
    for (int idx = tid; idx < na * nb; idx += kSylThreads) {
        const int a = idx % na, k = idx / na;
        sF[a + k * LD] = F[(r0 + a) + (int64_t)(c0 + k) * ldf];
    }
    red[tid] = amax;
    __syncthreads();
    for (int w = kSylThreads / 2; w > 0; w >>= 1) {
        if (tid < w) red[tid] = fmax(red[tid], red[tid + w]);
        __syncthreads();
    }
    if (tid == 0 || tid == 64) {   // the groups of R_ii (lane 0) and of S_jj (lane 64)
        const S* const M = tid == 0 ? sR : sS;
        int* const gs = tid == 0 ? ga : gb;
        const int cnt = tid == 0 ? na : nb;
        int g = 0;
        for (int k = 0; k < cnt;) {
            gs[g++] = k;
            bool two = false;
            if constexpr (kReal) two = k + 1 < cnt && M[(k + 1) + k * LD] != 0.0;
            k += two ? 2 : 1;
        }
        gs[g] = cnt;
        ng[tid == 0 ? 0 : 1] = g;
        if (tid == 0) pert = 0;
    }
    __syncthreads();
    const double eps = 2.220446049250313e-16, tiny = 2.2250738585072014e-308;
    const double smin = fmax(eps * red[0], tiny / eps);
    const int nga = ng[0], ngb = ng[1];
    const int pr = tid >> 2, sb4 = tid & 3, ia = sb4 & 1, ib = sb4 >> 1;
    for (int e = 0; e < nga + ngb - 1; ++e) {
        const int lo = max(0, e - (ngb - 1)), hi = min(e, nga - 1);
        const bool act = pr <= hi - lo;
        int a0 = 0, sa = 0, b0 = 0, sb = 0;
        if (act) {
            const int gap = lo + pr, gbp = e - gap;
            const int gA = nga - 1 - gap, gB = trans ? ngb - 1 - gbp : gbp;
            a0 = ga[gA];
            sa = ga[gA + 1] - a0;
            b0 = gb[gB];
            sb = gb[gB + 1] - b0;
            if (ia < sa && ib < sb) {
                const int a = a0 + ia, b = b0 + ib;
                if constexpr (kSumFirst) {
                    S sum = s_zero<S>();
                    for (int k = a0 + sa; k < na; ++k) sum = add(sum, mul(sR[a + k * LD], sF[k + b * LD]));
                    if (!trans)
                        for (int k = 0; k < b0; ++k) sum = add(sum, mul(sF[a + k * LD], sS[k + b * LD]));
                    else
                        for (int k = b0 + sb; k < nb; ++k) sum = add(sum, mul(sF[a + k * LD], conj_c(sS[b + k * LD])));
                    srhs[tid] = sub(sF[a + b * LD], sum);
                } else {
                    S acc = sF[a + b * LD];
                    for (int k = a0 + sa; k < na; ++k) acc = sub(acc, mul(sR[a + k * LD], sF[k + b * LD]));
                    if (!trans)
                        for (int k = 0; k < b0; ++k) acc = sub(acc, mul(sF[a + k * LD], sS[k + b * LD]));
                    else
                        for (int k = b0 + sb; k < nb; ++k) acc = sub(acc, mul(sF[a + k * LD], conj_c(sS[b + k * LD])));
                    srhs[tid] = acc;
                }
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
                        if (ub == vb) kv += sR[(a0 + ua) + (a0 + va) * LD];
                        if (ua == va) kv += trans ? sS[(b0 + ub) + (b0 + vb) * LD] : sS[(b0 + vb) + (b0 + ub) * LD];
                        K[u][v] = kv;
                    }
                }
                if (syl_solve4(N, K, x, smin)) pert = 1;
#pragma unroll
                for (int u = 0; u < 4; ++u)
                    if (u < N) sF[(a0 + u % sa) + (b0 + u / sa) * LD] = x[u];
            } else {
                const cplx sbb = trans ? conj_c(sS[b0 + b0 * LD]) : sS[b0 + b0 * LD];
                cplx den = add(sR[a0 + a0 * LD], sbb);
                if (mod_abs(den) < smin) {
                    den = cplx{smin, 0.0};
                    pert = 1;
                }
                sF[a0 + b0 * LD] = syl_cdiv(srhs[tid], den);
            }
        }
        __syncthreads();
    }
    for (int idx = tid; idx < na * nb; idx += kSylThreads) {
        const int a = idx % na, k = idx / na;
        F[(r0 + a) + (int64_t)(c0 + k) * ldf] = sF[a + k * LD];
    }
    if (tid == 0) flags[i + j * p] = pert;
}

}  // namespace dev

// Block starts of an order-n matrix: s_0 = 0, s_{b+1} = min(s_b + NB, n), one less where T(s_{b+1}, s_{b+1} - 1)
// != 0 (sub[k] = T(k + 1, k) != 0; empty: triangular).  The last entry is n.
std::vector<int> syl_starts(int64_t n, int NB, const std::vector<unsigned char>& sub);

// dtype is EIGSOL_F64 or EIGSOL_C128, the orders are within schur's, and the context's device is current
int syl_check_args(const char* who, eigsol_ctx* ctx, int dtype, int64_t m, int64_t n);

// C (m x nn) = L (m x kk) R (R stored kk x nn), or L R^H (conj_right: R stored nn x kk); leading dimensions ldl,
// ldr and m
template <class S>
int syl_product(hipStream_t st, bool conj_right, int64_t m, int64_t nn, int64_t kk, const S* L, int64_t ldl, const S* R,
                int64_t ldr, S* C) {
    EIGSOL_HIP(hipMemsetAsync(C, 0, (size_t)m * nn * sizeof(S), st));
    const dim3 grid((unsigned)((m + 63) / 64), (unsigned)((nn + 63) / 64));
    if (conj_right)   // C = L R^H, R stored nn x kk
        hipLaunchKernelGGL((dev::syl_gemm<S, false, true>), grid, dim3(256), 0, st, (int)m, (int)nn, (int)kk, L, ldl, R, ldr, C, m);
    else   // C = L R, R stored kk x nn
        hipLaunchKernelGGL((dev::syl_gemm<S, true, false>), grid, dim3(256), 0, st, (int)m, (int)nn, (int)kk, L, ldl, R, ldr, C, m);
    EIGSOL_HIP(hipGetLastError());
    return EIGSOL_OK;
}

template <class S>
bool all_finite(const void* a_host, int64_t cnt_scalars) {
    const double* a = static_cast<const double*>(a_host);
    const int64_t cnt = (std::is_same_v<S, double> ? 1 : 2) * cnt_scalars;
    for (int64_t i = 0; i < cnt; ++i)
        if (!std::isfinite(a[i])) return false;
    return true;
}

// zeros below the sub-diagonal; complex: a zero sub-diagonal; real: no two consecutive non-zero sub-diagonal
// entries.  sub receives the pattern of the sub-diagonal (real only).
template <class S>
bool syl_structure_ok(const S* T, int64_t n, std::vector<unsigned char>& sub) {
    constexpr bool kReal = std::is_same_v<S, double>;
    sub.clear();
    for (int64_t j = 0; j < n; ++j)
        for (int64_t i = j + 2; i < n; ++i)
            if (mod_abs(T[i + j * n]) != 0.0) return false;
    if (kReal && n > 1) sub.assign((size_t)(n - 1), 0);
    for (int64_t k = 0; k + 1 < n; ++k) {
        const bool nz = mod_abs(T[(k + 1) + k * n]) != 0.0;
        if (!kReal && nz) return false;
        if (kReal) {
            sub[k] = nz ? 1 : 0;
            if (nz && k > 0 && sub[k - 1]) return false;
        }
    }
    return true;
}

// the sub-diagonal pattern of a real device matrix, on the host (one host wait, n bytes); complex: empty.
// neg_1x1 (may be null) receives whether a 1 x 1 diagonal block of the real matrix is negative.
template <class S>
int syl_device_pattern(hipStream_t st, const S* T, int64_t n, DevBuf& scratch, std::vector<unsigned char>& sub,
                       bool* neg_1x1 = nullptr) {
    sub.clear();
    if (neg_1x1) *neg_1x1 = false;
    if constexpr (std::is_same_v<S, double>) {
        if (n < 2 && !neg_1x1) return EIGSOL_OK;
        std::vector<unsigned char> pat((size_t)n, 0);
        EIGSOL_TRY(scratch.alloc((size_t)n));
        hipLaunchKernelGGL(dev::syl_subdiag, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, T, n, scratch.as<unsigned char>());
        EIGSOL_HIP(hipGetLastError());
        EIGSOL_HIP(hipMemcpyAsync(pat.data(), scratch.p, (size_t)n, hipMemcpyDeviceToHost, st));
        EIGSOL_HIP(hipStreamSynchronize(st));
        if (n > 1) sub.assign((size_t)(n - 1), 0);
        for (int64_t k = 0; k < n; ++k) {
            const bool lower = k + 1 < n && (pat[k] & 1), upper = k > 0 && (pat[k - 1] & 1);
            if (k + 1 < n) sub[k] = lower ? 1 : 0;
            if (neg_1x1 && (pat[k] & 2) && !lower && !upper) *neg_1x1 = true;
        }
    }
    return EIGSOL_OK;
}

}  // namespace eigsol
