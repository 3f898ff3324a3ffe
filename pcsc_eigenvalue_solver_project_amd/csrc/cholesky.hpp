// Shared by cholesky.hip (dense Cholesky, blocked triangular solves, the generalised symmetric-definite
// driver) and eigh.hip (the standard solver the driver ends in).
#pragma once

#include <algorithm>

#include "internal.hpp"

namespace eigsol {

struct DevBuf {
    void* p = nullptr;
    DevBuf() = default;
    DevBuf(const DevBuf&) = delete;
    DevBuf& operator=(const DevBuf&) = delete;
    ~DevBuf() { release(); }
    void release() {
        if (p) (void)hipFree(p);
        p = nullptr;
    }
    template <class T> T* as() { return static_cast<T*>(p); }
    hipError_t alloc(size_t bytes) { return hipMalloc(&p, std::max<size_t>(bytes, 64)); }
};

// eigh.hip: eigsol_eigh_dense's solver on a matrix that is already on the device.  dA (n x n, column-major;
// only its lower triangle is read) is freed once reduced.  w_out (host) receives the m selected eigenvalues;
// with `vectors`, dZ receives the orthonormal eigenvectors (n x m, device) before the phase convention,
// which eigh_fix_phase_device applies.  The stage times go to ctx->eigh_ms as in eigsol_eigh_dense.
int eigh_device(eigsol_ctx* ctx, int dtype, int64_t n, DevBuf& dA, int select, int64_t il, int64_t iu, double vl,
                double vu, double* w_out, bool vectors, DevBuf& dZ, int64_t* m_out, int64_t* not_converged);
int eigh_fix_phase_device(hipStream_t st, int dtype, int64_t n, int64_t m, void* Z);
// the selection of eigsol_eigh_options checked against n (EIGSOL_E_INVALID with `who` in the message)
int eigh_parse_selection(const char* who, int64_t n, const eigsol_eigh_options* opts, int* select, int64_t* il,
                         int64_t* iu, double* vl, double* vu);

}  // namespace eigsol
