// Schur form A = Z T Z^H of a general dense matrix (gfx950; EIGSOL_F64: real Schur form, quasi-triangular T
// and orthogonal Z; EIGSOL_C128: complex Schur form, triangular T and unitary Z).  The host driver and the
// kernels that are the Schur form's own; the sweeps are francis.hip / zfrancis.hip's in Schur mode.
//
//   1. the power-of-two range guard of the Francis paths (qr_range_guard, qr.hip); T and the eigenvalues are
//      scaled back by the same power of two, exactly;
//   2. H = Q^H A Q by hessenberg_blocked_vt (n >= 3; the panels are kept), the entries below
//      the sub-diagonal cleared; Z = Q by hess_backtransform on the identity, 4096 columns at a time, before
//      the sweeps (n <= 2: H = A, Z = I);
//   3. schur_sweeps_*: the multishift sweeps with aggressive early deflation of qr_eigenvalues, every delayed
//      update widened to the whole matrix, H(s:e, e:n) <- U^H H(s:e, e:n), H(0:s, s:e) <- H(0:s, s:e) U, and
//      Z(:, s:e) <- Z(:, s:e) U as a launch of its own that T never reads; every left region before every
//      right region;
//   4. a diagonal block of at most 96 (real) / 64 (complex) rows is finished by the one-wave Schur
//      factorisation with its factor kept, which is applied to the same three ranges;
//   5. every sub-diagonal entry the deflation test accepted is stored as 0.0;
//   6. real matrices: every 2 x 2 diagonal block is standardised (LAPACK dlanv2's contract): split into two
//      1 x 1 blocks, or left with equal diagonal entries and off-diagonal entries of opposite sign.  The
//      rotations are computed from the blocks (schur_lanv2, which only reads T), the blocks are rewritten
//      (schur_put_blocks), then all row rotations run in one launch and all column rotations (T's rows above
//      the block, Z's two columns) in the next: blocks are disjoint, and a row rotation of one block meets a
//      column rotation of another in one entry of T;
//   7. the eigenvalues are read from T's diagonal blocks on the device; a pair's first member has the
//      positive imaginary part, sqrt|T(k, k+1)| sqrt|T(k+1, k)|, the second its bitwise conjugate.
// No floating-point atomics; every sum has a fixed order: two calls give the same bits, and T and the
// eigenvalues are the same bits with and without Z.  Not converged (a deflation took more than
// max_iterations sweeps): T is upper Hessenberg only, A = Z T Z^H holds all the same, the 2 x 2 blocks are
// left as they are and the eigenvalues are read from what T's diagonal blocks hold.
#include <algorithm>
#include <cmath>
#include <cstring>
#include <vector>

#include "kernels_common.hpp"
#include "schur.hpp"
#include "schur_blocks.hpp"
#include "scratch.hpp"

namespace eigsol {

int schur_sweeps_f64(eigsol_ctx* ctx, double* H, int64_t n, double* Z, int maxits, int32_t* sweeps_out,
                     int32_t* fail_out);
int schur_sweeps_c128(eigsol_ctx* ctx, cplx* H, int64_t n, cplx* Z, int maxits, int32_t* sweeps_out,
                      int32_t* fail_out);

namespace dev {

__device__ __forceinline__ double sch_one(double) { return 1.0; }
__device__ __forceinline__ cplx sch_one(cplx) { return cplx{1.0, 0.0}; }

template <class S>
__global__ __launch_bounds__(256) void schur_identity(S* Z, int64_t n) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x, j = blockIdx.y;
    if (i < n) Z[i + j * n] = i == j ? sch_one(S{}) : s_zero<S>();
}

// exact zeros below the first sub-diagonal
template <class S>
__global__ __launch_bounds__(256) void schur_clear_below(S* H, int64_t n) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x, j = blockIdx.y;
    if (i < n && i > j + 1) H[i + j * n] = s_zero<S>();
}


// rot[k] for every row k that starts a 2 x 2 block (T(k+1, k) != 0); cs = 2 marks "no rotation" (no block
// there, or the block is standard already: its bits stay).  Reads T only.
__global__ __launch_bounds__(256) void schur_lanv2(const double* T, int64_t n, Lanv2* rot) {
    const int64_t k = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (k + 1 >= n) return;
    Lanv2 r{0.0, 0.0, 0.0, 0.0, 2.0, 0.0};
    const double c = T[(k + 1) + k * n];
    if (c != 0.0) {
        r = schur_lanv2_dev(T[k + k * n], T[k + (k + 1) * n], c, T[(k + 1) + (k + 1) * n]);
        if (r.cs == 1.0 && r.sn == 0.0) r.cs = 2.0;
    }
    rot[k] = r;
}

__global__ __launch_bounds__(256) void schur_put_blocks(double* T, int64_t n, const Lanv2* rot) {
    const int64_t k = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (k + 1 >= n) return;
    const Lanv2 r = rot[k];
    if (r.cs == 2.0) return;
    T[k + k * n] = r.a;
    T[k + (k + 1) * n] = r.b;
    T[(k + 1) + k * n] = r.c;
    T[(k + 1) + (k + 1) * n] = r.d;
}

// rows k, k + 1 of block k (blockIdx.y), the columns right of the block
__global__ __launch_bounds__(256) void schur_rot_rows(double* T, int64_t n, const Lanv2* rot) {
    const int64_t k = blockIdx.y;
    const Lanv2 r = rot[k];
    if (r.cs == 2.0) return;
    const int64_t j = k + 2 + (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (j >= n) return;
    const double x = T[k + j * n], y = T[(k + 1) + j * n];
    T[k + j * n] = r.cs * x + r.sn * y;
    T[(k + 1) + j * n] = r.cs * y - r.sn * x;
}

// columns k, k + 1 of block k (blockIdx.y): T's rows above the block, every row of Z (null: none)
__global__ __launch_bounds__(256) void schur_rot_cols(double* T, int64_t n, const Lanv2* rot, double* Z) {
    const int64_t k = blockIdx.y;
    const Lanv2 r = rot[k];
    if (r.cs == 2.0) return;
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i < k) {
        const double x = T[i + k * n], y = T[i + (k + 1) * n];
        T[i + k * n] = r.cs * x + r.sn * y;
        T[i + (k + 1) * n] = r.cs * y - r.sn * x;
    }
    if (Z && i < n) {
        const double x = Z[i + k * n], y = Z[i + (k + 1) * n];
        Z[i + k * n] = r.cs * x + r.sn * y;
        Z[i + (k + 1) * n] = r.cs * y - r.sn * x;
    }
}


}  // namespace dev

namespace {

template <class S> struct SchurOps;
template <> struct SchurOps<double> {
    static int reduce(hipStream_t st, double* A, int64_t n, double* V, double* T) { return hessenberg_blocked_vt_f64(st, A, n, V, T); }
    static int back(hipStream_t st, int64_t n, int64_t m, const double* V, const double* T, double* Z) {
        return hess_backtransform_f64(st, n, m, V, T, Z, n);
    }
    static int sweeps(eigsol_ctx* ctx, double* H, int64_t n, double* Z, int maxits, int32_t* sw, int32_t* failed) {
        return schur_sweeps_f64(ctx, H, n, Z, maxits, sw, failed);
    }
    static int nb() { return hess_panel_width_f64(); }
};
template <> struct SchurOps<cplx> {
    static int reduce(hipStream_t st, cplx* A, int64_t n, cplx* V, cplx* T) { return hessenberg_blocked_vt_c128(st, A, n, V, T); }
    static int back(hipStream_t st, int64_t n, int64_t m, const cplx* V, const cplx* T, cplx* Z) {
        return hess_backtransform_c128(st, n, m, V, T, Z, n);
    }
    static int sweeps(eigsol_ctx* ctx, cplx* H, int64_t n, cplx* Z, int maxits, int32_t* sw, int32_t* failed) {
        return schur_sweeps_c128(ctx, H, n, Z, maxits, sw, failed);
    }
    static int nb() { return hess_panel_width_c128(); }
};

constexpr int64_t kQChunk = 4096;   // columns per application of Q, as eig.hip's back-transformation

}  // namespace

template <class S>
int schur_device(eigsol_ctx* ctx, int64_t n, const void* A_host, int max_iter, bool wantz, SchurDevice& out,
                 StageClock& clock) {
    constexpr bool kReal = std::is_same_v<S, double>;
    using Ops = SchurOps<S>;
    hipStream_t st = ctx->stream;
    const int NB = Ops::nb();
    const int64_t npan = n >= 3 ? (n - 2 + NB - 1) / NB : 0;
    DevBuf &dH = out.T, &dZ = out.Z, &dw = out.w, &drot = out.rot;
    DevBuf dV, dT;
    EIGSOL_TRY(dH.alloc((size_t)n * n * sizeof(S)));
    EIGSOL_TRY(dw.alloc((size_t)n * sizeof(cplx)));
    if (wantz) EIGSOL_TRY(dZ.alloc((size_t)n * n * sizeof(S)));
    if (npan) {   // kept with and without Z: one reduction path, the same bits of H either way
        EIGSOL_TRY(dV.alloc((size_t)npan * n * NB * sizeof(S)));
        EIGSOL_TRY(dT.alloc((size_t)npan * NB * NB * sizeof(S)));
    }
    const dim3 gfull((unsigned)((n + 255) / 256), (unsigned)n);
    const unsigned grow = (unsigned)((n + 255) / 256);
    EIGSOL_HIP(hipMemcpyAsync(dH.p, A_host, (size_t)n * n * sizeof(S), hipMemcpyHostToDevice, st));
    EIGSOL_TRY(clock.mark(0, st));
    // ---- 1. range guard; 2. reduction
    int escale = 0;
    EIGSOL_TRY(qr_range_guard(st, dH.as<double>(), (kReal ? 1 : 2) * n * n, &escale));
    if (n >= 3) {
        EIGSOL_TRY(Ops::reduce(st, dH.as<S>(), n, dV.as<S>(), dT.as<S>()));
        hipLaunchKernelGGL(dev::schur_clear_below<S>, gfull, dim3(256), 0, st, dH.as<S>(), n);
    }
    EIGSOL_TRY(clock.mark(1, st));
    if (wantz) {
        hipLaunchKernelGGL(dev::schur_identity<S>, gfull, dim3(256), 0, st, dZ.as<S>(), n);
        if (npan)
            for (int64_t c0 = 0; c0 < n; c0 += kQChunk)
                EIGSOL_TRY(Ops::back(st, n, std::min(kQChunk, n - c0), dV.as<S>(), dT.as<S>(), dZ.as<S>() + (size_t)c0 * n));
    }
    EIGSOL_HIP(hipGetLastError());
    EIGSOL_TRY(clock.mark(2, st));
    // ---- 3. - 5. the sweeps in Schur mode
    int32_t sweeps = 1, failed = 0;
    if (n >= 2) EIGSOL_TRY(Ops::sweeps(ctx, dH.as<S>(), n, wantz ? dZ.as<S>() : nullptr, max_iter, &sweeps, &failed));
    dV.release();
    dT.release();
    EIGSOL_TRY(clock.mark(3, st));
    // ---- 6. standard 2 x 2 blocks; scaling back; 7. eigenvalues
    if constexpr (kReal) {
        if (n >= 2 && !failed) {
            EIGSOL_TRY(drot.alloc((size_t)n * sizeof(dev::Lanv2)));
            dev::Lanv2* const rot = drot.as<dev::Lanv2>();
            const dim3 gblk(grow, (unsigned)(n - 1));
            hipLaunchKernelGGL(dev::schur_lanv2, dim3(grow), dim3(256), 0, st, dH.as<double>(), n, rot);
            hipLaunchKernelGGL(dev::schur_put_blocks, dim3(grow), dim3(256), 0, st, dH.as<double>(), n, rot);
            hipLaunchKernelGGL(dev::schur_rot_rows, gblk, dim3(256), 0, st, dH.as<double>(), n, rot);
            hipLaunchKernelGGL(dev::schur_rot_cols, gblk, dim3(256), 0, st, dH.as<double>(), n, rot,
                               wantz ? dZ.as<double>() : nullptr);
        }
    }
    if (escale != 0)
        qr_scale_pow2(st, dH.as<double>(), (kReal ? 1 : 2) * n * n, -escale);
    if constexpr (kReal)
        hipLaunchKernelGGL(dev::schur_eigs_real, dim3(grow), dim3(256), 0, st, dH.as<double>(), n, dw.as<double>());
    else
        hipLaunchKernelGGL(dev::schur_eigs_cplx, dim3(grow), dim3(256), 0, st, dH.as<cplx>(), n, dw.as<cplx>());
    EIGSOL_HIP(hipGetLastError());
    out.sweeps = sweeps;
    out.failed = failed;
    return EIGSOL_OK;
}

template int schur_device<double>(eigsol_ctx*, int64_t, const void*, int, bool, SchurDevice&, StageClock&);
template int schur_device<cplx>(eigsol_ctx*, int64_t, const void*, int, bool, SchurDevice&, StageClock&);

namespace {

template <class S>
int schur_host(eigsol_ctx* ctx, int64_t n, const void* A_host, int max_iter, void* T_out, void* Z_out, void* eig_re_or_c,
               double* eig_im, int32_t* iterations, int32_t* converged) {
    constexpr bool kReal = std::is_same_v<S, double>;
    {
        const double* a = static_cast<const double*>(A_host);
        const int64_t cnt = (kReal ? 1 : 2) * n * n;
        for (int64_t i = 0; i < cnt; ++i)
            if (!std::isfinite(a[i])) return fail(EIGSOL_E_SOLVER, "eigsol_schur_dense: the matrix holds a non-finite entry");
    }
    hipStream_t st = ctx->stream;
    const bool wantz = Z_out != nullptr;
    StageClock clock;
    EIGSOL_TRY(clock.start(4));
    SchurDevice sd;
    EIGSOL_TRY(schur_device<S>(ctx, n, A_host, max_iter, wantz, sd, clock));
    DevBuf &dH = sd.T, &dZ = sd.Z, &dw = sd.w;
    const int32_t sweeps = sd.sweeps, failed = sd.failed;
    std::vector<cplx> w(n);
    EIGSOL_HIP(hipMemcpyAsync(w.data(), dw.p, (size_t)n * sizeof(cplx), hipMemcpyDeviceToHost, st));
    EIGSOL_HIP(hipMemcpyAsync(T_out, dH.p, (size_t)n * n * sizeof(S), hipMemcpyDeviceToHost, st));
    if (wantz) EIGSOL_HIP(hipMemcpyAsync(Z_out, dZ.p, (size_t)n * n * sizeof(S), hipMemcpyDeviceToHost, st));
    EIGSOL_TRY(clock.mark(4, st));
    EIGSOL_HIP(hipStreamSynchronize(st));
    clock.read(ctx->schur_ms, 4);
    if constexpr (kReal) {
        double* re = static_cast<double*>(eig_re_or_c);
        for (int64_t i = 0; i < n; ++i) {
            re[i] = w[i].re;
            if (eig_im) eig_im[i] = w[i].im;
        }
    } else {
        std::memcpy(eig_re_or_c, w.data(), (size_t)n * sizeof(cplx));
    }
    if (iterations) *iterations = sweeps;
    if (converged) *converged = failed ? 0 : 1;
    return EIGSOL_OK;
}

}  // namespace
}  // namespace eigsol

using namespace eigsol;

extern "C" {

int eigsol_schur_dense(eigsol_ctx* ctx, int dtype, int64_t n, const void* A_colmajor, const eigsol_solver_options* opts,
                       void* T_out, void* Z_out, void* eig_re_or_c, double* eig_im, int32_t* iterations,
                       int32_t* converged) {
    if (n < 0) return fail(EIGSOL_E_INVALID, "eigsol_schur_dense: negative order");
    if (!ctx) return fail(EIGSOL_E_INVALID, "eigsol_schur_dense: null context");
    const int max_iter = opts ? opts->max_iterations : 1000;
    if (n == 0) {
        if (iterations) *iterations = 0;
        if (converged) *converged = 1;
        return EIGSOL_OK;
    }
    if (!A_colmajor || !T_out || !eig_re_or_c) return fail(EIGSOL_E_INVALID, "eigsol_schur_dense: null pointer");
    if (max_iter < 1) return fail(EIGSOL_E_INVALID, "eigsol_schur_dense: max_iterations < 1");
    if (dtype_wide(dtype) || dtype_single(dtype))
        return fail(EIGSOL_E_UNSUPPORTED, "eigsol_schur_dense: double and complex double matrices only");
    if (!dtype_valid(dtype)) return fail(EIGSOL_E_INVALID, "eigsol_schur_dense: unknown dtype");
    if (dtype == EIGSOL_F64 && !eig_im) return fail(EIGSOL_E_INVALID, "eigsol_schur_dense: null eig_im for a real matrix");
    if (n > (dtype == EIGSOL_C128 ? hess_max_order_c128() : hess_max_order_f64()))
        return fail(EIGSOL_E_UNSUPPORTED, "eigsol_schur_dense: n above the order the blocked Hessenberg reduction accepts");
    EIGSOL_HIP(hipSetDevice(ctx->device));
    return dtype == EIGSOL_C128
               ? schur_host<cplx>(ctx, n, A_colmajor, max_iter, T_out, Z_out, eig_re_or_c, eig_im, iterations, converged)
               : schur_host<double>(ctx, n, A_colmajor, max_iter, T_out, Z_out, eig_re_or_c, eig_im, iterations,
                                    converged);
}

int eigsol_schur_stage_times(eigsol_ctx* ctx, double* ms4) {
    if (!ctx || !ms4) return fail(EIGSOL_E_INVALID, "eigsol_schur_stage_times: null pointer");
    for (int q = 0; q < 4; ++q) ms4[q] = ctx->schur_ms[q];
    return EIGSOL_OK;
}

}  // extern "C"
