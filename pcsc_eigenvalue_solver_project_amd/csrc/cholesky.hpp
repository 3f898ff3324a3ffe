// Shared by cholesky.hip (dense Cholesky, blocked triangular solves, the generalised symmetric-definite
// driver) and eigh.hip (the standard solver the driver ends in).
#pragma once

#include <vector>

#include "scratch.hpp"

namespace eigsol {

// eigh.hip: eigsol_eigh_dense's solver on a matrix that is already on the device.  dA (n x n, column-major;
// only its lower triangle is read) is freed once reduced.  w_out (host) receives the m selected eigenvalues;
// with `vectors`, dZ receives the orthonormal eigenvectors (n x m, device) before the phase convention,
// which eigh_fix_phase_device applies.  The stage times go to ctx->eigh_ms as in eigsol_eigh_dense.
int eigh_device(eigsol_ctx* ctx, int dtype, int64_t n, DevBuf& dA, int select, int64_t il, int64_t iu, double vl,
                double vu, double* w_out, bool vectors, DevBuf& dZ, int64_t* m_out, int64_t* not_converged);
// eigh_device with the method of the tridiagonal stage (EIGSOL_EIGH_METHOD_*); eigh_device is method 0
int eigh_device_m(eigsol_ctx* ctx, int dtype, int64_t n, DevBuf& dA, int select, int64_t il, int64_t iu, double vl,
                  double vu, int method, double* w_out, bool vectors, DevBuf& dZ, int64_t* m_out, int64_t* not_converged);
int eigh_fix_phase_device(hipStream_t st, int dtype, int64_t n, int64_t m, void* Z);

// eigh_dc.hip: every eigenpair of the real symmetric tridiagonal T = (d: n, e: n - 1; host) by divide and
// conquer, block by block (starts: the split blocks' first rows, n appended).  dQ receives the n x n
// block-diagonal vector matrix on the device: column i belongs to lam[i] (host, n; unsorted within a block)
// and is zero outside its block's rows.  *ncap: leaf eigenvalues and secular roots that hit their cap.
// Sets ctx->eigh_dc_ms[1 .. 4].
int eigh_dc_tridiag(eigsol_ctx* ctx, int64_t n, const double* d, const double* e, const std::vector<int64_t>& starts,
                    DevBuf& dQ, double* lam, int64_t* ncap);
// ZT (n x m, packed) <- the columns cols[0 .. m) of Q (n x n)
int eigh_dc_take_columns(hipStream_t st, int64_t n, int64_t m, const double* Q, const std::vector<int>& cols, double* ZT);
// the selection of eigsol_eigh_options checked against n (EIGSOL_E_INVALID with `who` in the message)
int eigh_parse_selection(const char* who, int64_t n, const eigsol_eigh_options* opts, int* select, int64_t* il,
                         int64_t* iu, double* vl, double* vu);

}  // namespace eigsol
