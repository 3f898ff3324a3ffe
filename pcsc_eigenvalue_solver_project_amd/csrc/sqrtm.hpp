// The pieces of sqrtm.hip that the matrix logarithm (logm.hip) runs too: the triangular square root on the device
// and the pass that puts the real eigenvalues of a complex T on the real axis.  See the head of sqrtm.hip.
#pragma once

#include <vector>

#include "kernels_common.hpp"
#include "scratch.hpp"

namespace eigsol {
namespace dev {

// a diagonal entry of the complex T with Re < 0 and |Im| <= tol: its imaginary part becomes +0.  sqrtm.hip
__global__ __launch_bounds__(256) void sqrtm_real_axis(cplx* T, int64_t n, double tol);

}  // namespace dev

// U <- U^(1/2) in place for the (quasi-)triangular device matrix U (leading dimension n) with the starts rs,
// stream-ordered, no host wait.  `work` receives the starts and the flags; *d_pert (device) the number of
// perturbed blocks.  S is double or cplx.
template <class S>
int trsqrt_device(hipStream_t st, int64_t n, S* U, const std::vector<int>& rs, DevBuf& work, int* d_pert);

}  // namespace eigsol
