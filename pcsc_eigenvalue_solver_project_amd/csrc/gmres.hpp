// The GMRES family of the general-sparse shifted solve (gmres.hip): host interface.
#pragma once

#include "internal.hpp"

namespace eigsol {

struct GmresSolver;
// Adev: the device matrix A itself (same dtype and order), used for the products with M = A - sigma I
int gmres_create(eigsol_ctx* ctx, int dtype, int64_t n, const int32_t* rp, const int32_t* ci, const void* v,
                 double sre, double sim, GmresSolver** out, eigsol_csr* Adev = nullptr);
void gmres_free(GmresSolver* g);
int gmres_solve(GmresSolver* g, const void* b_dev, double bdiv, void* y_dev);
int gmres_can_lag(const GmresSolver* g);
int gmres_solve_lag(GmresSolver* g, const void* b_dev, double bdiv, void* y_dev);
int gmres_lag_verdict(GmresSolver* g);
void gmres_lag_reset(GmresSolver* g);
void gmres_info(const GmresSolver* g, double* bytes, int32_t* steps);
int gmres_complete(const GmresSolver* g);

}  // namespace eigsol
