// Matrix exponential by scaling and squaring (gfx950; EIGSOL_F64 and EIGSOL_C128): Higham,
// "The scaling and squaring method for the matrix exponential revisited", SIAM J. Matrix Anal. Appl. 26 (2005),
// Algorithm 2.3; what scipy.linalg.expm computed before the 2009 refinement.
//   1. the host refuses a non-finite entry before the upload;
//   2. alpha = ||A||_1 on the device (mat_norm1, gemm.hip), one host wait for 8 bytes;
//   3. expm_plan (expm_plan.hpp): the degree m of the Pade approximant and the squarings s; A <- 2^-s A;
//   4. U (odd part) and V (even part) of the approximant's numerator p = V + U, the denominator being q = V - U:
//      the even powers A^2, A^4, A^6 (A^8) by gemm_device, the polynomials in them by mat_lincomb, U = A (..).
//      m = 13 is split so that it takes six products:
//        U = A (A6 (b13 A6 + b11 A4 + b9 A2) + b7 A6 + b5 A4 + b3 A2 + b1 I),
//        V =    A6 (b12 A6 + b10 A4 + b8 A2) + b6 A6 + b4 A4 + b2 A2 + b0 I;
//   5. (V - U) X = V + U by dense_getrf and dense_getrs (dense_lu.hip);
//   6. X <- X^2, s times, between two buffers; the download.  A device pass tells whether X is finite.
// No atomics and fixed summation orders throughout: two calls give the same bits.  A real A gives a real X;
// alpha = 0 gives I without any arithmetic.  The norm estimates, the choice of s from ||A^k||^(1/k) and the
// triangular squaring of Al-Mohy and Higham (2009) are not here: a strongly non-normal matrix is scaled by its
// 1-norm alone and may be squared more often than SciPy squares it.
#include <algorithm>
#include <cmath>
#include <string>

#include "dense_lu.hpp"
#include "expm_plan.hpp"
#include "gemm.hpp"
#include "scratch.hpp"

namespace eigsol {
namespace {

// Higham's b_k, exactly representable integers
constexpr double kPade3[4] = {120., 60., 12., 1.};
constexpr double kPade5[6] = {30240., 15120., 3360., 420., 30., 1.};
constexpr double kPade7[8] = {17297280., 8648640., 1995840., 277200., 25200., 1512., 56., 1.};
constexpr double kPade9[10] = {17643225600., 8821612800., 2075673600., 302702400., 30270240., 2162160., 110880., 3960., 90., 1.};
constexpr double kPade13[14] = {64764752532480000., 32382376266240000., 7771770303897600., 1187353796428800., 129060195264000.,
                                10559470521600.,    670442572800.,      33522128640.,      1323241920.,       40840800.,
                                960960.,            16380.,             182.,              1.};

bool finite_host(const void* a_host, int64_t cnt_doubles) {
    const double* a = static_cast<const double*>(a_host);
    for (int64_t i = 0; i < cnt_doubles; ++i)
        if (!std::isfinite(a[i])) return false;
    return true;
}

template <class S>
int lin(hipStream_t st, int64_t n, std::initializer_list<std::pair<double, const S*>> terms, double d, S* out) {
    double c[4];
    const S* M[4];
    int cnt = 0;
    for (const auto& t : terms) {
        c[cnt] = t.first;
        M[cnt++] = t.second;
    }
    return mat_lincomb<S>(st, n, cnt, c, M, d, out);
}

template <class S>
int expm_host(eigsol_ctx* ctx, int64_t n, const void* A_host, void* X_out, int32_t* degree, int32_t* squarings) {
    const char* who = "eigsol_expm_dense";
    constexpr int kDoubles = std::is_same_v<S, double> ? 1 : 2;
    if (!finite_host(A_host, n * n * kDoubles)) return fail(EIGSOL_E_SOLVER, std::string(who) + ": the matrix holds a non-finite entry");
    hipStream_t st = ctx->stream;
    const size_t bytes = (size_t)n * n * sizeof(S);
    StageClock clock;
    EIGSOL_TRY(clock.start(6));   // the five stages, then the finiteness pass with the copy to the host
    for (int q = 0; q < 6; ++q) ctx->expm_ms[q] = 0.0;
    auto finish_times = [&]() {
        double ms[6];
        clock.read(ms, 6);
        ctx->expm_ms[5] = 0.0;
        for (int q = 0; q < 6; ++q) ctx->expm_ms[5] += ms[q];
        for (int q = 0; q < 5; ++q) ctx->expm_ms[q] = ms[q];
    };
    DevBuf dA, dnorm, dpiv;
    EIGSOL_TRY(dA.alloc(bytes));
    EIGSOL_TRY(dnorm.alloc(((size_t)n + 2) * sizeof(double)));   // column sums, the norm, the finiteness word
    EIGSOL_TRY(dpiv.alloc(((size_t)n + 1) * sizeof(int32_t)));   // pivots, the zero-pivot word
    double* const d_colsum = dnorm.as<double>();
    double* const d_alpha = d_colsum + n;
    double* const d_bad = d_colsum + n + 1;
    int32_t* const d_piv = dpiv.as<int32_t>();
    int32_t* const d_zp = d_piv + n;
    S* const A = dA.as<S>();
    // ---- the norm
    EIGSOL_TRY(clock.mark(0, st));
    EIGSOL_HIP(hipMemcpyAsync(A, A_host, bytes, hipMemcpyHostToDevice, st));
    EIGSOL_TRY(mat_norm1<S>(st, n, A, false, d_colsum, d_alpha));
    double alpha = 0.0;
    EIGSOL_HIP(hipMemcpyAsync(&alpha, d_alpha, sizeof(double), hipMemcpyDeviceToHost, st));
    EIGSOL_TRY(clock.mark(1, st));
    EIGSOL_HIP(hipStreamSynchronize(st));
    if (!std::isfinite(alpha)) return fail(EIGSOL_E_SOLVER, std::string(who) + ": the 1-norm of the matrix overflows");
    int m = 3, s = 0;
    expm_plan(alpha, &m, &s);
    if (degree) *degree = m;
    if (squarings) *squarings = s;
    DevBuf d2, d4, d6, dT, dU, dV;
    EIGSOL_TRY(d2.alloc(bytes));
    EIGSOL_TRY(dU.alloc(bytes));
    EIGSOL_TRY(dV.alloc(bytes));
    S* const A2 = d2.as<S>();
    S* const U = dU.as<S>();
    S* const V = dV.as<S>();
    S* X = V;   // the result so far
    if (alpha == 0.0) {
        EIGSOL_TRY(lin<S>(st, n, {}, 1.0, X));
        for (int q = 2; q <= 5; ++q) EIGSOL_TRY(clock.mark(q, st));
    } else {
        if (m >= 5) EIGSOL_TRY(d4.alloc(bytes));
        if (m >= 7) EIGSOL_TRY(d6.alloc(bytes));
        EIGSOL_TRY(dT.alloc(bytes));
        S* const A4 = d4.as<S>();
        S* const A6 = d6.as<S>();
        S* const T = dT.as<S>();
        // ---- U and V
        if (s > 0) EIGSOL_TRY(mat_scale_pow2<S>(st, n * n, s, A, A));
        auto mm = [&](const S* L, const S* R, S* out) { return gemm_device<S>(st, n, n, n, L, n, R, n, out, n); };
        EIGSOL_TRY(mm(A, A, A2));
        if (m >= 5) EIGSOL_TRY(mm(A2, A2, A4));
        if (m >= 7) EIGSOL_TRY(mm(A4, A2, A6));
        if (m == 3) {
            const double* b = kPade3;
            EIGSOL_TRY(lin<S>(st, n, {{b[3], A2}}, b[1], T));
            EIGSOL_TRY(lin<S>(st, n, {{b[2], A2}}, b[0], V));
        } else if (m == 5) {
            const double* b = kPade5;
            EIGSOL_TRY(lin<S>(st, n, {{b[5], A4}, {b[3], A2}}, b[1], T));
            EIGSOL_TRY(lin<S>(st, n, {{b[4], A4}, {b[2], A2}}, b[0], V));
        } else if (m == 7) {
            const double* b = kPade7;
            EIGSOL_TRY(lin<S>(st, n, {{b[7], A6}, {b[5], A4}, {b[3], A2}}, b[1], T));
            EIGSOL_TRY(lin<S>(st, n, {{b[6], A6}, {b[4], A4}, {b[2], A2}}, b[0], V));
        } else if (m == 9) {
            const double* b = kPade9;
            EIGSOL_TRY(mm(A6, A2, U));   // A^8, until U itself is formed
            EIGSOL_TRY(lin<S>(st, n, {{b[9], U}, {b[7], A6}, {b[5], A4}, {b[3], A2}}, b[1], T));
            EIGSOL_TRY(lin<S>(st, n, {{b[8], U}, {b[6], A6}, {b[4], A4}, {b[2], A2}}, b[0], V));
        } else {
            const double* b = kPade13;
            EIGSOL_TRY(lin<S>(st, n, {{b[13], A6}, {b[11], A4}, {b[9], A2}}, 0.0, U));
            EIGSOL_TRY(mm(A6, U, T));
            EIGSOL_TRY(lin<S>(st, n, {{1.0, T}, {b[7], A6}, {b[5], A4}, {b[3], A2}}, b[1], T));
            EIGSOL_TRY(lin<S>(st, n, {{b[12], A6}, {b[10], A4}, {b[8], A2}}, 0.0, U));
            EIGSOL_TRY(mm(A6, U, V));
            EIGSOL_TRY(lin<S>(st, n, {{1.0, V}, {b[6], A6}, {b[4], A4}, {b[2], A2}}, b[0], V));
        }
        EIGSOL_TRY(mm(A, T, U));
        EIGSOL_TRY(lin<S>(st, n, {{1.0, V}, {-1.0, U}}, 0.0, T));   // q = V - U
        EIGSOL_TRY(lin<S>(st, n, {{1.0, V}, {1.0, U}}, 0.0, V));    // p = V + U
        EIGSOL_TRY(clock.mark(2, st));
        // ---- q X = p
        EIGSOL_HIP(hipMemsetAsync(d_zp, 0xff, sizeof(int32_t), st));
        dense_getrf<S>(st, T, n, d_piv, d_zp);
        EIGSOL_HIP(hipGetLastError());
        EIGSOL_TRY(clock.mark(3, st));
        dense_getrs<S>(st, T, n, d_piv, V, n, n);
        EIGSOL_HIP(hipGetLastError());
        EIGSOL_TRY(clock.mark(4, st));
        // ---- the squarings
        S* Y = U;
        for (int q = 0; q < s; ++q) {
            EIGSOL_TRY(mm(X, X, Y));
            std::swap(X, Y);
        }
        EIGSOL_TRY(clock.mark(5, st));
    }
    EIGSOL_TRY(mat_norm1<S>(st, n, X, true, d_colsum, d_bad));
    double bad = 0.0;
    int32_t zp = -1;
    EIGSOL_HIP(hipMemcpyAsync(&bad, d_bad, sizeof(double), hipMemcpyDeviceToHost, st));
    if (alpha != 0.0) EIGSOL_HIP(hipMemcpyAsync(&zp, d_zp, sizeof(int32_t), hipMemcpyDeviceToHost, st));
    EIGSOL_HIP(hipMemcpyAsync(X_out, X, bytes, hipMemcpyDeviceToHost, st));
    EIGSOL_TRY(clock.mark(6, st));
    EIGSOL_HIP(hipStreamSynchronize(st));
    finish_times();
    if (bad != 0.0) return fail(EIGSOL_E_SOLVER, std::string(who) + ": result overflows");
    if (zp >= 0)
        return fail(EIGSOL_E_SOLVER, std::string(who) + ": the Pade denominator is singular: the pivot of column " + std::to_string(zp) + " is zero");
    return EIGSOL_OK;
}

}  // namespace
}  // namespace eigsol

using namespace eigsol;

extern "C" {

int eigsol_expm_plan(double alpha, int32_t* degree, int32_t* squarings) {
    if (!degree || !squarings) return fail(EIGSOL_E_INVALID, "eigsol_expm_plan: null pointer");
    if (!(alpha >= 0.0) || !std::isfinite(alpha)) return fail(EIGSOL_E_INVALID, "eigsol_expm_plan: the norm must be finite and >= 0");
    int m = 0, s = 0;
    expm_plan(alpha, &m, &s);
    *degree = m;
    *squarings = s;
    return EIGSOL_OK;
}

int eigsol_expm_dense(eigsol_ctx* ctx, int dtype, int64_t n, const void* A_colmajor, void* X_out, int32_t* degree,
                      int32_t* squarings) {
    const char* who = "eigsol_expm_dense";
    if (n < 0) return fail(EIGSOL_E_INVALID, std::string(who) + ": negative order");
    if (!ctx) return fail(EIGSOL_E_INVALID, std::string(who) + ": null context");
    EIGSOL_TRY(dense_fn_check(who, ctx, dtype, n));
    if (degree) *degree = 0;
    if (squarings) *squarings = 0;
    if (n == 0) return EIGSOL_OK;
    if (!A_colmajor || !X_out) return fail(EIGSOL_E_INVALID, std::string(who) + ": null pointer");
    return dtype == EIGSOL_C128 ? expm_host<cplx>(ctx, n, A_colmajor, X_out, degree, squarings)
                                : expm_host<double>(ctx, n, A_colmajor, X_out, degree, squarings);
}

int eigsol_expm_stage_times(eigsol_ctx* ctx, double* ms6) {
    if (!ctx || !ms6) return fail(EIGSOL_E_INVALID, "eigsol_expm_stage_times: null pointer");
    for (int q = 0; q < 6; ++q) ms6[q] = ctx->expm_ms[q];
    return EIGSOL_OK;
}

}  // extern "C"
