// The square GEMM of the dense matrix functions (gemm.hip) and the plain kernels expm.hip
// runs around it.  Everything is column-major on the device and stream-ordered; S is double or cplx.
#pragma once

#include "internal.hpp"

namespace eigsol {

// C (m x n, ldc) = A (m x k, lda) B (k x n, ldb); any m, n, k >= 1.  C is written once and never read; it must not
// overlap A or B.  No split-K, no atomics: two runs give the same bits.
template <class S>
int gemm_device(hipStream_t st, int64_t m, int64_t n, int64_t k, const S* A, int64_t lda, const S* B, int64_t ldb, S* C,
                int64_t ldc);

// Out = c[0] M[0] + .. + c[cnt - 1] M[cnt - 1] + d I, summed in that order, for n x n matrices of leading dimension n
// (cnt <= 4; real coefficients).  Out may be one of the M.
template <class S>
int mat_lincomb(hipStream_t st, int64_t n, int cnt, const double* c, const S* const* M, double d, S* Out);

// Out = 2^-s A over cnt scalars (exact unless an entry underflows).  Out may be A.
template <class S>
int mat_scale_pow2(hipStream_t st, int64_t cnt, int s, const S* A, S* Out);

// *out (device) = ||A||_1 of the n x n matrix A (leading dimension n): one workgroup per column sums the moduli
// in a fixed order into colsum (device, n doubles), one workgroup takes their maximum.  A NaN column sum is
// kept.  check: each column's value is 1 where it holds a non-finite entry and else 0, so *out > 0 tells that
// A is not finite.
template <class S>
int mat_norm1(hipStream_t st, int64_t n, const S* A, bool check, double* colsum, double* out);

// the checks shared by eigsol_gemm_dense, eigsol_solve_dense and eigsol_expm_dense: dtype is EIGSOL_F64 or
// EIGSOL_C128, a matrix of the order fits the device, and the context's device is current
int dense_fn_check(const char* who, eigsol_ctx* ctx, int dtype, int64_t order);

}  // namespace eigsol
