// The matrix as the eigensolver drivers see it (subspace.hip, krylov.hip, svds.hip): a CSR or a dense handle
// behind the few operations the drivers need.  Exactly one of csr and dense is set; csr_h,
// the CSR handle of A^H (eigsol_csr_adjoint), is set by the drivers that apply the adjoint.
#pragma once

#include "shifted.hpp"

namespace eigsol {

// Y = A X on row-major interleaved blocks, enqueued on the matrix's stream (dense_block.hip);
// arguments checked by the caller
int dense_gemm_launch(eigsol_dense* A, int m, const void* X, void* Y);

struct LinearOp {
    eigsol_csr* csr = nullptr;
    eigsol_dense* dense = nullptr;
    eigsol_csr* csr_h = nullptr;

    explicit LinearOp(eigsol_csr* A, eigsol_csr* AH = nullptr) : csr(A), csr_h(AH) {}
    explicit LinearOp(eigsol_dense* A) : dense(A) {}

    const eigsol_ctx* ctx() const { return csr ? csr->ctx : dense->ctx; }
    int64_t nrows() const { return csr ? csr->nrows : dense->nrows; }
    int64_t ncols() const { return csr ? csr->ncols : dense->ncols; }
    int dtype() const { return csr ? csr->dtype : dense->dtype; }
    // y = A x on contiguous device vectors
    int apply(const void* x, void* y) const { return csr ? eigsol_csr_spmv(csr, x, y) : eigsol_dense_gemv(dense, x, y); }
    // y = A^H x on contiguous device vectors: the adjoint handle's SpMV, or the dense adjoint kernel
    int apply_h(const void* x, void* y) const {
        if (dense) return eigsol_dense_gemv_h(dense, x, y);
        if (!csr_h) return fail(EIGSOL_E_INVALID, "LinearOp: no adjoint handle");
        return eigsol_csr_spmv(csr_h, x, y);
    }
    // the factor of A - sigma I
    int factor(const void* sigma, ShiftFactor** out) const {
        return csr ? shift_factor_csr(csr, sigma, out) : shift_factor_dense(dense, sigma, out);
    }
};

}  // namespace eigsol
