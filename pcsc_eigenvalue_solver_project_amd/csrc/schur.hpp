// The Schur pipeline of schur.hip between its upload and its download, for drivers that go on working with
// T and Z on the device (sylvester.hip, ordschur.hip).
#pragma once

#include "scratch.hpp"

namespace eigsol {

// What schur_device leaves on the device: T (n x n), Z (n x n, only with wantz), the eigenvalues w (n cplx;
// real matrices: re, im pairs) and the scratch of its last launches, which has to outlive them.
struct SchurDevice {
    DevBuf T, Z, w, rot;
    int32_t sweeps = 1, failed = 0;
};

// Uploads A (n x n, column-major, host) and runs steps 1 to 7 of schur.hip on ctx's stream.  The caller has
// checked A for non-finite entries and started `clock` with at least 4 stages; marks 0 to 3 are recorded here
// (upload done, reduction, forming Q, sweeps).  Nothing is downloaded; the sweeps wait for the stream.
template <class S>
int schur_device(eigsol_ctx* ctx, int64_t n, const void* A_host, int max_iter, bool wantz, SchurDevice& out,
                 StageClock& clock);

}  // namespace eigsol
