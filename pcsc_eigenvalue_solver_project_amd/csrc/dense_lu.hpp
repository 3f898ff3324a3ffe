// The dense partial-pivot LU on its own (dense_lu.hip): the blocked factorisation the shifted solves run, and a
// blocked substitution with a matrix of right-hand sides (eigsol_solve_dense, expm.hip).  Device arrays,
// column-major, stream-ordered, no host wait.
#pragma once

#include "internal.hpp"

namespace eigsol {

// a (n x n, leading dimension n) <- its factors: P a = L U, L unit lower, by right-looking panels of RankKMax<S>
// columns (LAPACK getrf's order).  piv (device, n): row k was exchanged with row piv[k] >= k, in the order
// k = 0 .. n - 1.  *zero_pivot (device; set to -1 by the caller): the first column whose pivot is exactly zero;
// that column is left unscaled and the factorisation goes on.
template <class S>
void dense_getrf(hipStream_t st, S* a, int64_t n, int32_t* piv, int32_t* zero_pivot);

// B (n x nrhs, leading dimension ldb) <- a^-1 B from dense_getrf's lu and piv: the interchanges on B's rows,
// then forward and back substitution by block rows of RankKMax<S>: the diagonal block is solved by substitution
// from LDS, one thread per column of B, and the other block rows are updated on the matrix cores.
template <class S>
void dense_getrs(hipStream_t st, const S* lu, int64_t n, const int32_t* piv, S* B, int64_t ldb, int64_t nrhs);

}  // namespace eigsol
