// Principal matrix logarithm through the Schur form (gfx950; EIGSOL_F64 and EIGSOL_C128):
// the Schur-Pade inverse scaling and squaring method (Higham, Functions of Matrices, Alg. 11.9, with the bounds
// theta_m of Al-Mohy and Higham (2012) applied to the 1-norm),
//   A = Z T Z^H (schur_device),  L = log T on the device,  X = Z L Z^H (two syl_product calls)
// and the triangular stage on its own for an upper triangular (complex) or quasi-triangular (real, 2 x 2 blocks
// with complex eigenvalues) T.  exp(X) = A and every eigenvalue of X has its imaginary part in (-pi, pi].
//
// The triangular stage.
//   1. logm_keep_diag keeps T's diagonal, sub-diagonal and super-diagonal (3 n scalars, T0).
//   2. The root loop: R = T - I (mat_lincomb), ||R||_1 (mat_norm1), one host wait of 8 bytes (with the count of
//      perturbed blocks of the last root), logm_plan (logm_plan.hpp) decides: stop with degree m, or T <- T^(1/2)
//      in place by trsqrt_device (sqrtm.hip).  At most 64 roots.  ||R||_1 = 0: T = I and L = 0 without arithmetic.
//   3. The Pade approximant of log(I + R) through its partial fractions,
//        r_m(R) = sum_j alpha_j X_j,   (I + beta_j R) X_j = R,   j = 1 .. m <= 7,
//      beta_j and alpha_j the nodes and weights of the m-point Gauss-Legendre rule on [0, 1].  R is cut into p
//      blocks by syl_starts (NB = 64 real, 32 complex; no 2 x 2 block is split), and all m upper block triangular
//      systems are solved together by block super-diagonals d = 0 .. p - 1:
//        X_j(i, c) = W_ji (R(i, c) - beta_j sum_{i < k <= c} R(i, k) X_j(k, c)),   c = i + d,  k ascending.
//      a. logm_winv_kernel, one launch over (i, j): W_ji = (I + beta_j R_ii)^-1 in LDS.  ||R||_1 <= theta_7 = 0.288
//         bounds ||beta_j R_ii||_1 by 0.288, so cond_1(I + beta_j R_ii) <= (1 + 0.288) / (1 - 0.288) = 1.81: the
//         explicit inverse is as good as a solve here.  A real R_ii is upper Hessenberg with isolated sub-diagonal
//         entries (the 2 x 2 bumps); one elimination step per bump (no pivoting: the multiplier is at most
//         0.288 / 0.712) leaves a triangular matrix, whose inverse one lane per column takes by back substitution.
//      b. logm_solve_kernel, one launch per d with grid (p - d, m), one workgroup per block and node: the sum over
//         k through rankk_tile on the fp64 matrix cores into a scratch block F that starts at zero (each lane
//         reads back only the entries it stored itself), then F <- R(i, c) - beta_j F entry by entry, then
//         X_j(i, c) = W_ji F through rankk_tile again.  The three steps are separated by workgroup barriers; rankk_tile
//         keeps its operands in registers and uses no LDS, so the fused launch fits trivially.  Each tile has one
//         writer.
//      c. logm_combine_kernel, one launch: L = 2^s sum_j alpha_j X_j, j ascending; exact zeros below the
//         quasi-triangle; the diagonal blocks from T0 (small_log.hpp): log t for a 1 x 1 block (complex: the
//         principal logarithm, -0.0 counting as +0.0), ln|lambda| I + (atan2(mu, a) / mu) (B - a I) for a real
//         2 x 2 block; and between two 1 x 1 blocks the super-diagonal entry by Al-Mohy and Higham's formula.
// That is 2 + p launches after the roots with no host wait between them; the stage's scratch, m n^2 scalars for the
// X_j (7 n^2 at degree 7: 15 GB at n = 16384 in f64) and 2 m p NB^2 for W and F, is allocated before them.  No atomics and fixed orders throughout: two runs give
// the same bits.  The logarithm of a real T is real.
//
// A real A with a negative real eigenvalue has no real logarithm: as in sqrtm.hip the call ends with
// *needs_complex = 1 and X untouched, and the caller passes A as complex; sqrtm_real_axis then puts those
// eigenvalues on the axis with imaginary part +0, so their logarithms have imaginary part +pi (SciPy's branch).  An
// exactly zero 1 x 1 diagonal block means a singular A: EIGSOL_E_SOLVER.
//
// Not here: the alpha_p norm estimates of the 2012 algorithm, the cancellation-free recomputation of R's diagonal,
// degrees above 7, skipping the norm of the first roots from the known eigenvalues, funm, signm, fractional powers,
// Frechet derivatives and condition estimates.
#include <algorithm>
#include <cmath>
#include <cstring>
#include <string>
#include <vector>

#include "gemm.hpp"
#include "logm_plan.hpp"
#include "schur.hpp"
#include "small_log.hpp"
#include "sqrtm.hpp"
#include "sylvester.hpp"

namespace eigsol {
namespace dev {

struct LogmNodes {
    double beta[kLogmMaxDegree], alpha[kLogmMaxDegree];
};

__device__ __forceinline__ double scale_r(double b, double v) { return b * v; }
__device__ __forceinline__ cplx scale_r(double b, cplx v) { return cplx{b * v.re, b * v.im}; }
template <class S> __device__ __forceinline__ S s_one() {
    S v = s_zero<S>();
    set_re_im(v, 1.0, 0.0);
    return v;
}
template <class S> constexpr size_t logm_winv_lds_bytes() {
    return (size_t)2 * RankKMax<S>::value * (RankKMax<S>::value + 1) * sizeof(S);
}

// t0[k] = T(k, k), t0[n + k] = T(k + 1, k), t0[2 n + k] = T(k, k + 1) (zero for k = n - 1)
template <class S>
__global__ __launch_bounds__(256) void logm_keep_diag(const S* T, int64_t n, S* t0) {
    const int64_t k = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (k >= n) return;
    t0[k] = T[k + k * n];
    t0[n + k] = k + 1 < n ? T[(k + 1) + k * n] : s_zero<S>();
    t0[2 * n + k] = k + 1 < n ? T[k + (k + 1) * n] : s_zero<S>();
}

// One workgroup: W = (I + beta_j R_ii)^-1 for i = blockIdx.x, j = blockIdx.y, into Wall + (j p + i) NB^2 (leading
// dimension NB); see the head of this file.
template <class S>
__global__ __launch_bounds__(256) void logm_winv_kernel(const S* R, int64_t ldr, const int* rs, int p, LogmNodes nd, S* Wall) {
    constexpr bool kReal = std::is_same_v<S, double>;
    constexpr int NB = RankKMax<S>::value, LD = NB + 1;
    extern __shared__ __align__(16) unsigned char logm_lds[];   // 66560 bytes for double: above the static limit
    S* const sM = reinterpret_cast<S*>(logm_lds);
    S* const sV = sM + NB * LD;
    __shared__ double sl[NB];
    const int tid = threadIdx.x, i = blockIdx.x, j = blockIdx.y;
    if (i >= p) return;
    const int r0 = rs[i], na = rs[i + 1] - r0;
    if (na < 1 || na > NB) return;
    const double beta = nd.beta[j];
    for (int idx = tid; idx < na * na; idx += 256) {
        const int a = idx % na, k = idx / na;
        // below the quasi-triangle R is zero; nothing there is read
        S v = a > k + (kReal ? 1 : 0) ? s_zero<S>() : scale_r(beta, R[(r0 + a) + (int64_t)(r0 + k) * ldr]);
        if (a == k) v = add(v, s_one<S>());
        sM[a + k * LD] = v;
        sV[a + k * LD] = a == k ? s_one<S>() : s_zero<S>();
    }
    __syncthreads();
    if constexpr (kReal) {
        // the bumps: row a <- row a - l_a row (a - 1), l_a = m(a, a - 1) / m(a - 1, a - 1); the bumps share no row
        if (tid < na) sl[tid] = tid > 0 && sM[tid + (tid - 1) * LD] != 0.0 ? sM[tid + (tid - 1) * LD] / sM[(tid - 1) + (tid - 1) * LD] : 0.0;
        __syncthreads();
        for (int idx = tid; idx < na * na; idx += 256) {
            const int a = idx % na, k = idx / na;
            const double l = sl[a];
            if (l != 0.0) {
                if (k == a - 1) {
                    sM[a + k * LD] = 0.0;
                    sV[a + k * LD] = -l;
                } else if (k >= a) {
                    sM[a + k * LD] = sM[a + k * LD] - l * sM[(a - 1) + k * LD];
                }
            }
        }
        __syncthreads();
    }
    if (tid < na) {   // column tid of the inverse by back substitution, in place in sV
        const int c = tid;
        for (int a = na - 1; a >= 0; --a) {
            S acc = s_zero<S>();
            for (int k = a + 1; k < na; ++k) acc = add(acc, mul(sM[a + k * LD], sV[k + c * LD]));
            const S num = sub(sV[a + c * LD], acc);
            if constexpr (kReal) sV[a + c * LD] = num / sM[a + a * LD];
            else sV[a + c * LD] = syl_cdiv(num, sM[a + a * LD]);
        }
    }
    __syncthreads();
    S* const W = Wall + ((size_t)j * p + i) * NB * NB;
    for (int idx = tid; idx < na * na; idx += 256) {
        const int a = idx % na, k = idx / na;
        W[a + k * NB] = sV[a + k * LD];
    }
}

// One workgroup: X_j(i, c) for i = blockIdx.x, c = i + d, j = blockIdx.y; see the head of this file.  Xall holds
// the m matrices X_j (n x n each), Wall the inverses, Gall one NB x NB scratch block per (j, i).
template <class S>
__global__ __launch_bounds__(256) void logm_solve_kernel(const S* R, int64_t n, S* Xall, const S* Wall, S* Gall, const int* rs, int p,
                                                         int d, LogmNodes nd) {
    constexpr int NB = RankKMax<S>::value;
    const int tid = threadIdx.x, i = blockIdx.x, c = i + d, j = blockIdx.y;
    if (c >= p) return;
    const int r0 = rs[i], na = rs[i + 1] - r0, c0 = rs[c], nb = rs[c + 1] - c0;
    if (na < 1 || na > NB || nb < 1 || nb > NB) return;
    S* const Xj = Xall + (size_t)j * n * n;
    S* const F = Gall + ((size_t)j * p + i) * NB * NB;
    const S* const W = Wall + ((size_t)j * p + i) * NB * NB;
    const double beta = nd.beta[j];
    for (int idx = tid; idx < na * nb; idx += 256) F[(idx % na) + (idx / na) * NB] = s_zero<S>();
    __syncthreads();
    for (int k = i + 1; k <= c; ++k) {   // each lane reads back the entries of F it stored itself
        const int k0 = rs[k], K = rs[k + 1] - k0;
        rankk_tile<S, true>(0, 0, na, nb, K, 1.0, R + r0 + (int64_t)k0 * n, n, Xj + k0 + (int64_t)c0 * n, n, F, NB);
    }
    __syncthreads();
    for (int idx = tid; idx < na * nb; idx += 256) {
        const int a = idx % na, b = idx / na;
        F[a + b * NB] = sub(R[(r0 + a) + (int64_t)(c0 + b) * n], scale_r(beta, F[a + b * NB]));
        Xj[(r0 + a) + (int64_t)(c0 + b) * n] = s_zero<S>();
    }
    __syncthreads();
    rankk_tile<S, true>(0, 0, na, nb, na, 1.0, W, NB, F, NB, Xj + r0 + (int64_t)c0 * n, n);
}

__device__ __forceinline__ double logm_log1(double t) { return log(t); }
__device__ __forceinline__ cplx logm_log1(cplx t) { return log_principal(t); }

// L = scale sum_j alpha_j X_j (j ascending) on the upper triangle, zeros below the quasi-triangle, the diagonal
// blocks and the super-diagonal entries between two 1 x 1 blocks from t0; see the head of this file.
template <class S>
__global__ __launch_bounds__(256) void logm_combine_kernel(const S* Xall, int64_t n, int m, LogmNodes nd, double scale, const S* t0,
                                                           S* L) {
    constexpr bool kReal = std::is_same_v<S, double>;
    const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (idx >= n * n) return;
    const int64_t r = idx % n, q = idx / n;
    auto bump = [&](int64_t k) {   // rows k, k + 1 are a 2 x 2 block
        if constexpr (kReal) return k >= 0 && k + 1 < n && t0[n + k] != 0.0;
        else return false;
    };
    auto one = [&](int64_t k) { return !bump(k) && !bump(k - 1); };
    auto combined = [&]() {
        S acc = s_zero<S>();
        for (int j = 0; j < m; ++j) acc = add(acc, scale_r(nd.alpha[j], Xall[(size_t)j * n * n + idx]));
        return scale_r(scale, acc);
    };
    S out = s_zero<S>();
    if (r > q + 1) {
        out = s_zero<S>();
    } else if (r >= q - 1 && (bump(r < q ? r : q) || (r == q && bump(q - 1)))) {
        if constexpr (kReal) {
            const int64_t k = bump(r < q ? r : q) ? (r < q ? r : q) : q - 1;   // the block's first row
            double l[4];
            const int sel = (int)((r - k) + 2 * (q - k));   // selected without indexing l, which stays in registers
            if (log_block2(t0[k], t0[n + k], t0[2 * n + k], t0[k + 1], l)) out = sel == 0 ? l[0] : sel == 1 ? l[1] : sel == 2 ? l[2] : l[3];
            else out = r <= q ? combined() : 0.0;
        }
    } else if (r == q + 1) {
        out = s_zero<S>();
    } else if (r == q) {
        out = logm_log1(t0[q]);
    } else if (r == q - 1 && one(r) && one(q)) {
        out = log_superdiag(t0[r], t0[q], t0[2 * n + r]);
    } else {
        out = combined();
    }
    L[idx] = out;
}

}  // namespace dev

namespace {

struct LogmInfo {
    int roots = 0, degree = 0, perturbed = 0;
};

// L (device, n x n) <- log T for the (quasi-)triangular device matrix T, which is overwritten by its last root.
// rs: the starts.  t0_host (3 n scalars) receives T's three diagonals (one host wait); the caller's `check`
// refuses what it finds there before any root is taken.  clock mark `mark_roots` is recorded after the roots.
template <class S, class Check>
int trlogm_device(const char* who, hipStream_t st, int64_t n, S* T, const std::vector<int>& rs, S* L, LogmInfo& info, StageClock& clock,
                  int mark_roots, Check check) {
    constexpr int NB = dev::RankKMax<S>::value;
    const int p = (int)rs.size() - 1;
    const size_t bytes = (size_t)n * n * sizeof(S);
    DevBuf dt0, dR, dnorm, dpert, work;
    EIGSOL_TRY(dt0.alloc((size_t)3 * n * sizeof(S)));
    EIGSOL_TRY(dR.alloc(bytes));
    EIGSOL_TRY(dnorm.alloc(((size_t)n + 1) * sizeof(double)));
    EIGSOL_TRY(dpert.alloc(sizeof(int)));
    S* const t0 = dt0.as<S>();
    S* const R = dR.as<S>();
    double* const d_colsum = dnorm.as<double>();
    double* const d_norm = d_colsum + n;
    hipLaunchKernelGGL(dev::logm_keep_diag<S>, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, T, n, t0);
    EIGSOL_HIP(hipGetLastError());
    std::vector<S> t0_host((size_t)3 * n);
    EIGSOL_HIP(hipMemcpyAsync(t0_host.data(), t0, (size_t)3 * n * sizeof(S), hipMemcpyDeviceToHost, st));
    EIGSOL_HIP(hipStreamSynchronize(st));
    EIGSOL_TRY(check(t0_host));
    // ---- the roots
    info = LogmInfo{};
    int tried = 0;
    double norm = 0.0;
    for (;;) {
        const double one = 1.0;
        const S* const Tc = T;
        EIGSOL_TRY(mat_lincomb<S>(st, n, 1, &one, &Tc, -1.0, R));
        EIGSOL_TRY(mat_norm1<S>(st, n, R, false, d_colsum, d_norm));
        int pert = 0;
        EIGSOL_HIP(hipMemcpyAsync(&norm, d_norm, sizeof(double), hipMemcpyDeviceToHost, st));
        if (info.roots > 0) EIGSOL_HIP(hipMemcpyAsync(&pert, dpert.p, sizeof(int), hipMemcpyDeviceToHost, st));
        EIGSOL_HIP(hipStreamSynchronize(st));
        info.perturbed += pert;
        if (!std::isfinite(norm)) return fail(EIGSOL_E_SOLVER, std::string(who) + ": a square root of T is not finite");
        if (norm == 0.0) break;
        info.degree = logm_plan(norm, tried);
        if (info.degree) break;
        if (norm <= kLogmTheta[kLogmMaxDegree - 1]) tried = 1;
        if (info.roots == kLogmMaxRoots)
            return fail(EIGSOL_E_SOLVER, std::string(who) + ": T^(1/2^s) is not near I after " + std::to_string(kLogmMaxRoots) + " square roots");
        EIGSOL_TRY(trsqrt_device<S>(st, n, T, rs, work, dpert.as<int>()));
        ++info.roots;
    }
    if (norm == 0.0) {   // T = I
        EIGSOL_TRY(clock.mark(mark_roots, st));
        EIGSOL_HIP(hipMemsetAsync(L, 0, bytes, st));
        return EIGSOL_OK;
    }
    // ---- the Pade approximant.  Its scratch (the m matrices X_j: m n^2 scalars, and 2 m p NB^2 for W and F) is
    // allocated before the stage's mark: hipMalloc and the hipFree inside alloc wait for the device, so they count
    // in the root stage, and the launches between the two marks run without a host wait.
    const int m = info.degree;
    dev::LogmNodes nd{};
    for (int j = 0; j < m; ++j) {
        nd.beta[j] = kLogmBeta[m - 1][j];
        nd.alpha[j] = kLogmAlpha[m - 1][j];
    }
    DevBuf dX, dW, dG;
    EIGSOL_TRY(dX.alloc(bytes * m));
    EIGSOL_TRY(dW.alloc((size_t)m * p * NB * NB * sizeof(S)));
    EIGSOL_TRY(dG.alloc((size_t)m * p * NB * NB * sizeof(S)));
    EIGSOL_TRY(work.alloc(((size_t)p + 1) * sizeof(int)));
    int* const d_rs = work.as<int>();
    EIGSOL_HIP(hipMemcpyAsync(d_rs, rs.data(), (size_t)(p + 1) * sizeof(int), hipMemcpyHostToDevice, st));
    EIGSOL_TRY(clock.mark(mark_roots, st));
    constexpr size_t lds = dev::logm_winv_lds_bytes<S>();
    EIGSOL_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(dev::logm_winv_kernel<S>), hipFuncAttributeMaxDynamicSharedMemorySize,
                                   (int)lds));
    hipLaunchKernelGGL(dev::logm_winv_kernel<S>, dim3((unsigned)p, (unsigned)m), dim3(256), lds, st, R, n, d_rs, p, nd, dW.as<S>());
    for (int d = 0; d < p; ++d)
        hipLaunchKernelGGL(dev::logm_solve_kernel<S>, dim3((unsigned)(p - d), (unsigned)m), dim3(256), 0, st, R, n, dX.as<S>(), dW.as<S>(),
                           dG.as<S>(), d_rs, p, d, nd);
    hipLaunchKernelGGL(dev::logm_combine_kernel<S>, dim3((unsigned)((n * n + 255) / 256)), dim3(256), 0, st, dX.as<S>(), n, m, nd,
                       std::ldexp(1.0, info.roots), t0, L);
    EIGSOL_HIP(hipGetLastError());
    // the scratch is released by hipFree, which waits for the device
    return EIGSOL_OK;
}

// a zero 1 x 1 diagonal block in the kept diagonals (sub-diagonal at t0[n + k])
template <class S>
int logm_refuse_singular(const char* who, int64_t n, const std::vector<S>& t0) {
    for (int64_t k = 0; k < n; ++k) {
        const bool lower = k + 1 < n && mod_abs(t0[n + k]) != 0.0, upper = k > 0 && mod_abs(t0[n + k - 1]) != 0.0;
        if (!lower && !upper && mod_abs(t0[k]) == 0.0)
            return fail(EIGSOL_E_SOLVER, std::string(who) + ": the matrix is singular: the diagonal entry of row " + std::to_string(k) +
                                             " of its triangular form is zero");
    }
    return EIGSOL_OK;
}

template <class S>
int trlogm_host(eigsol_ctx* ctx, int64_t n, const void* T_host, void* L_out, int32_t* roots, int32_t* degree, int32_t* perturbed) {
    constexpr int NB = dev::RankKMax<S>::value;
    const char* who = "eigsol_trlogm_dense";
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
                            std::string(who) + ": a negative 1 x 1 diagonal block has no real logarithm; pass T as complex");
            }
        }
    }
    const std::vector<int> rs = syl_starts(n, NB, sub);
    hipStream_t st = ctx->stream;
    StageClock clock;
    EIGSOL_TRY(clock.start(1));
    DevBuf dT, dL;
    EIGSOL_TRY(dT.alloc((size_t)n * n * sizeof(S)));
    EIGSOL_TRY(dL.alloc((size_t)n * n * sizeof(S)));
    EIGSOL_HIP(hipMemcpyAsync(dT.p, T_host, (size_t)n * n * sizeof(S), hipMemcpyHostToDevice, st));
    LogmInfo info;
    EIGSOL_TRY(trlogm_device<S>(who, st, n, dT.as<S>(), rs, dL.as<S>(), info, clock, 0,
                                [&](const std::vector<S>& t0) { return logm_refuse_singular<S>(who, n, t0); }));
    EIGSOL_HIP(hipMemcpyAsync(L_out, dL.p, (size_t)n * n * sizeof(S), hipMemcpyDeviceToHost, st));
    EIGSOL_HIP(hipStreamSynchronize(st));
    if (roots) *roots = info.roots;
    if (degree) *degree = info.degree;
    if (perturbed) *perturbed = info.perturbed;
    return EIGSOL_OK;
}

template <class S>
int logm_host(eigsol_ctx* ctx, int64_t n, const void* A_host, int max_iter, void* X_out, int32_t* roots, int32_t* degree,
              int32_t* perturbed, int32_t* converged, int32_t* needs_complex) {
    constexpr int NB = dev::RankKMax<S>::value;
    const char* who = "eigsol_logm_dense";
    if (!all_finite<S>(A_host, n * n)) return fail(EIGSOL_E_SOLVER, std::string(who) + ": the matrix holds a non-finite entry");
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
    EIGSOL_TRY(clock.start(4));
    EIGSOL_TRY(clock_s.start(4));
    for (int k = 0; k < 5; ++k) ctx->logm_ms[k] = 0.0;
    if (roots) *roots = 0;
    if (degree) *degree = 0;
    if (perturbed) *perturbed = 0;
    if (needs_complex) *needs_complex = 0;
    SchurDevice sd;
    EIGSOL_TRY(clock.mark(0, st));
    EIGSOL_TRY(schur_device<S>(ctx, n, A_host, max_iter, true, sd, clock_s));
    sd.w.release();
    sd.rot.release();
    EIGSOL_TRY(clock.mark(1, st));
    auto schur_only = [&]() {
        clock.read(ctx->logm_ms, 1);
        ctx->logm_ms[4] = ctx->logm_ms[0];
    };
    if (sd.failed) {
        EIGSOL_HIP(hipStreamSynchronize(st));
        schur_only();
        if (converged) *converged = 0;
        return EIGSOL_OK;
    }
    // ---- the partition and the sign of the 1 x 1 blocks (one host wait, n bytes)
    DevBuf scratch, dW, dX, dL;
    std::vector<unsigned char> sub;
    bool neg = false;
    EIGSOL_TRY(syl_device_pattern<S>(st, sd.T.as<S>(), n, scratch, sub, &neg));
    if (neg) {   // a negative real eigenvalue: no real logarithm; the caller runs the complex path
        schur_only();
        if (converged) *converged = 1;
        if (needs_complex) *needs_complex = 1;
        return EIGSOL_OK;
    }
    const std::vector<int> rs = syl_starts(n, NB, sub);
    EIGSOL_TRY(dL.alloc((size_t)n * n * sizeof(S)));
    S* const T = sd.T.as<S>();
    if constexpr (!std::is_same_v<S, double>) {
        if (real_norm > 0.0)
            hipLaunchKernelGGL(dev::sqrtm_real_axis, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, T, n,
                               (double)n * 2.220446049250313e-16 * real_norm);
    }
    const S* const Z = sd.Z.as<S>();
    LogmInfo info;
    EIGSOL_TRY(trlogm_device<S>(who, st, n, T, rs, dL.as<S>(), info, clock, 2,
                                [&](const std::vector<S>& t0) { return logm_refuse_singular<S>(who, n, t0); }));
    EIGSOL_TRY(clock.mark(3, st));
    // ---- X = Z L Z^H
    EIGSOL_TRY(dW.alloc((size_t)n * n * sizeof(S)));
    EIGSOL_TRY(dX.alloc((size_t)n * n * sizeof(S)));
    EIGSOL_TRY(syl_product<S>(st, false, n, n, n, Z, n, dL.as<S>(), n, dW.as<S>()));    // W = Z L
    EIGSOL_TRY(syl_product<S>(st, true, n, n, n, dW.as<S>(), n, Z, n, dX.as<S>()));     // X = W Z^H
    EIGSOL_HIP(hipMemcpyAsync(X_out, dX.p, (size_t)n * n * sizeof(S), hipMemcpyDeviceToHost, st));
    EIGSOL_TRY(clock.mark(4, st));
    EIGSOL_HIP(hipStreamSynchronize(st));
    clock.read(ctx->logm_ms, 4);
    ctx->logm_ms[4] = ctx->logm_ms[0] + ctx->logm_ms[1] + ctx->logm_ms[2] + ctx->logm_ms[3];
    if (roots) *roots = info.roots;
    if (degree) *degree = info.degree;
    if (perturbed) *perturbed = info.perturbed;
    if (converged) *converged = 1;
    return EIGSOL_OK;
}

}  // namespace
}  // namespace eigsol

using namespace eigsol;

extern "C" {

int eigsol_logm_plan(double norm, int32_t tried, int32_t* degree) {
    if (!degree) return fail(EIGSOL_E_INVALID, "eigsol_logm_plan: null pointer");
    if (!(norm >= 0.0) || !std::isfinite(norm)) return fail(EIGSOL_E_INVALID, "eigsol_logm_plan: the norm must be finite and >= 0");
    *degree = logm_plan(norm, tried != 0);
    return EIGSOL_OK;
}

int eigsol_trlogm_dense(eigsol_ctx* ctx, int dtype, int64_t n, const void* T_colmajor, void* L_out, int32_t* roots, int32_t* degree,
                        int32_t* perturbed) {
    const char* who = "eigsol_trlogm_dense";
    if (n < 0) return fail(EIGSOL_E_INVALID, std::string(who) + ": negative order");
    if (!ctx) return fail(EIGSOL_E_INVALID, std::string(who) + ": null context");
    if (roots) *roots = 0;
    if (degree) *degree = 0;
    if (perturbed) *perturbed = 0;
    if (n == 0) return EIGSOL_OK;
    if (!T_colmajor || !L_out) return fail(EIGSOL_E_INVALID, std::string(who) + ": null pointer");
    EIGSOL_TRY(syl_check_args(who, ctx, dtype, n, n));
    return dtype == EIGSOL_C128 ? trlogm_host<cplx>(ctx, n, T_colmajor, L_out, roots, degree, perturbed)
                                : trlogm_host<double>(ctx, n, T_colmajor, L_out, roots, degree, perturbed);
}

int eigsol_logm_dense(eigsol_ctx* ctx, int dtype, int64_t n, const void* A_colmajor, const eigsol_solver_options* opts, void* X_out,
                      int32_t* roots, int32_t* degree, int32_t* perturbed, int32_t* converged, int32_t* needs_complex) {
    const char* who = "eigsol_logm_dense";
    if (n < 0) return fail(EIGSOL_E_INVALID, std::string(who) + ": negative order");
    if (!ctx) return fail(EIGSOL_E_INVALID, std::string(who) + ": null context");
    const int max_iter = opts ? opts->max_iterations : 1000;
    if (n == 0) {
        if (roots) *roots = 0;
        if (degree) *degree = 0;
        if (perturbed) *perturbed = 0;
        if (converged) *converged = 1;
        if (needs_complex) *needs_complex = 0;
        return EIGSOL_OK;
    }
    if (!A_colmajor || !X_out) return fail(EIGSOL_E_INVALID, std::string(who) + ": null pointer");
    if (max_iter < 1) return fail(EIGSOL_E_INVALID, std::string(who) + ": max_iterations < 1");
    EIGSOL_TRY(syl_check_args(who, ctx, dtype, n, n));
    return dtype == EIGSOL_C128 ? logm_host<cplx>(ctx, n, A_colmajor, max_iter, X_out, roots, degree, perturbed, converged, needs_complex)
                                : logm_host<double>(ctx, n, A_colmajor, max_iter, X_out, roots, degree, perturbed, converged, needs_complex);
}

int eigsol_logm_stage_times(eigsol_ctx* ctx, double* ms5) {
    if (!ctx || !ms5) return fail(EIGSOL_E_INVALID, "eigsol_logm_stage_times: null pointer");
    for (int q = 0; q < 5; ++q) ms5[q] = ctx->logm_ms[q];
    return EIGSOL_OK;
}

}  // extern "C"
