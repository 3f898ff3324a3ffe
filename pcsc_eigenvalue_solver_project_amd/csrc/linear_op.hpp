// The matrix as the eigensolver drivers see it (subspace.hip, krylov.hip): a CSR or a dense handle
// behind the few operations the drivers need.  Exactly one of the two pointers is set.
#pragma once

#include "shifted.hpp"

namespace eigsol {

// Y = A X on row-major interleaved blocks, enqueued on the matrix's stream (dense_block.hip);
// arguments checked by the caller
int dense_gemm_launch(eigsol_dense* A, int m, const void* X, void* Y);

struct LinearOp {
    eigsol_csr* csr = nullptr;
    eigsol_dense* dense = nullptr;

    explicit LinearOp(eigsol_csr* A) : csr(A) {}
    explicit LinearOp(eigsol_dense* A) : dense(A) {}

    const eigsol_ctx* ctx() const { return csr ? csr->ctx : dense->ctx; }
    int64_t nrows() const { return csr ? csr->nrows : dense->nrows; }
    int dtype() const { return csr ? csr->dtype : dense->dtype; }
    // y = A x on contiguous device vectors
    int apply(const void* x, void* y) const { return csr ? eigsol_csr_spmv(csr, x, y) : eigsol_dense_gemv(dense, x, y); }
    // the factor of A - sigma I
    int factor(const void* sigma, ShiftFactor** out) const {
        return csr ? shift_factor_csr(csr, sigma, out) : shift_factor_dense(dense, sigma, out);
    }
};

}  // namespace eigsol
