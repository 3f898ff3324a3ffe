// Shifted solves (shifted.hip, sptrsv.hip, tri_factor.hip, dense_lu.hip): the interface the other modules use.
#pragma once

#include <vector>

#include "internal.hpp"

namespace eigsol {

struct ShiftFactor;   // shift_factor.hpp

// one launch of the iteration: the power loop's buffers and control block (same parity convention)
struct ShiftIter {
    void *buf0, *buf1;
    PowerCtl* ctl;
    const void* rank_part;
    void *my_part, *trace;
    int parity;
};

// factor of A - sigma I (sigma: one scalar of the matrix's dtype)
int shift_factor_csr(eigsol_csr* A, const void* sigma, ShiftFactor** out);
int shift_factor_dense(eigsol_dense* A, const void* sigma, ShiftFactor** out);
// triangular factor from host CSR arrays (the ILU(0) factors of the GMRES path, gmres.hip)
int shift_factor_tri(eigsol_ctx* ctx, int dtype, int64_t n, std::vector<int32_t>& rp, std::vector<int32_t>& ci,
                     const void* vals, bool up, ShiftFactor** out);
// ... and from device CSR arrays, which stay the caller's
int shift_factor_tri_dev(eigsol_ctx* ctx, int dtype, int64_t n, int32_t* rp, int32_t* ci, void* vals, int64_t nnz,
                         bool up, ShiftFactor** out);
void shift_factor_free(ShiftFactor* f);

int shift_grid(const ShiftFactor* f);
void* shift_aux(const ShiftFactor* f, int j);
int shift_error(ShiftFactor* f);
void shift_lag_reset(ShiftFactor* f);
int shift_iter_launch(ShiftFactor* f, const ShiftIter& it, int first);
int shift_solve_launch(ShiftFactor* f, const void* b_dev, void* y_dev);
void shift_info(const ShiftFactor* f, double* bytes, int32_t* variant, int32_t* tiles);

// device primitives of the on-device triangular analysis (tri_sort.hip)
hipError_t tri_sort_rows_by_level(hipStream_t st, const int32_t* lev, int32_t* lev_out, int32_t* rows_out, int64_t n,
                                  int bits);
hipError_t tri_exclusive_scan(hipStream_t st, const int32_t* in, int32_t* out, int64_t n);

}  // namespace eigsol
