// Shifted inverse iteration and solve_shifted on gfx950: factor once, solve per iteration.
//
// Replaces the numeric core of shiftedInversePowerMethod<S>
// (src/power_method/shifted_inverse_power_solver.hpp:112-125, impl :21-79) and solve_shifted<S>
// (src/matrix/solve_shifted.hpp:48-118).  The reference refactors A - sigma I on every iteration
// (SparseLU with COLAMD, or dense PartialPivLU); the factorisation does not depend on the
// iterate, so the device path factors once per (A, sigma) and runs ONE solve launch per
// iteration.  The Rayleigh quotient on A (:62) needs no product with A:
// A y = x + sigma y, see shift_prologue (kernels_common.hpp).
//
// Factor kinds (FactorKind, shift_factor.hpp), one file each
//   * Tri: triangular CSR, upper or lower (config 5) - sptrsv.hip, tri_factor.hip;
//   * Dense: Matrix::Dense and non-triangular sparse matrices densified on the device - dense_lu.hip;
//   * Band: RCM + banded partial-pivot LU - band_lu.hip;
//   * Gmres: exact no-pivot LU, nested-dissection multifrontal LU, or ILU(0) + GMRES - gmres.hip,
//     multifrontal.hip.
//
// This file holds the factor's lifetime, the public entry points of shifted.hpp, the general-sparse dispatch
// between band, LU and the GMRES family with its fallbacks (factor_csr_t, gmres_dense_fallback), the GMRES
// family's host-driven iteration (gmres_iter) and the dispatch of a launch to the factor's kind.
#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "shift_factor.hpp"

namespace eigsol {
namespace dev {

template <class S, class W>
__global__ __launch_bounds__(256) void convert_kernel(const S* __restrict__ in, W* __restrict__ out, int64_t n) {
    for (int64_t i = blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
        if constexpr (is_real_v<S>) out[i] = static_cast<W>(in[i]);
        else out[i] = W{static_cast<decltype(W{}.re)>(in[i].re), static_cast<decltype(W{}.im)>(in[i].im)};
    }
}

}  // namespace dev

// the GMRES family's factors are built in double
template <class S> inline constexpr bool kGmres = std::is_same_v<S, double> || std::is_same_v<S, cplx>;
// single-precision matrices take the GMRES family (exact / multifrontal LU, ILU(0) + GMRES) on their
// values widened to double: the factor, the residual checks and the refinement run in double, the
// iterate stays in the matrix's precision (dtype >= the reference's SparseLU<float>)
template <class S> using GmresScalar = std::conditional_t<is_real_v<S>, double, cplx>;

void shift_factor_free(ShiftFactor* f) {
    if (!f) return;
    hipSetDevice(f->ctx->device);
    hipStreamSynchronize(f->ctx->stream);
    f->gmres.release();
    if (f->band) band_free(f->band);
    f->tri.release();
    f->dense.release();
    if (f->hpin) hipHostFree(f->hpin);
    ctx_release(f->ctx);
    delete f;
}

// an empty factor of A - sigma I (A: n x n, nnz stored entries) holding a reference to its context
ShiftFactor* shift_factor_new(eigsol_ctx* ctx, int dtype, int64_t n, double sre, double sim, int64_t nnz) {
    auto* f = new ShiftFactor();
    f->ctx = ctx;
    ctx_retain(f->ctx);
    f->dtype = dtype;
    f->n = n;
    f->sig_re = sre;
    f->sig_im = sim;
    f->nnz_total = nnz;
    return f;
}

int shift_factor_dense(eigsol_dense* A, const void* sigma, ShiftFactor** out) {
    double s[2] = {0.0, 0.0};
    load_scalar(sigma, A->dtype, s[0], s[1]);   // a real dtype leaves s[1] = 0
    EIGSOL_HIP(hipSetDevice(A->ctx->device));
    EIGSOL_TRY(dense_limits(A->dtype, A->nrows, "shifted solve"));
    ShiftFactor* f = shift_factor_new(A->ctx, A->dtype, A->nrows, s[0], s[1], 0);
    const int rc = dense_from_matrix(f, A->a, f->dense);
    if (rc != EIGSOL_OK) { shift_factor_free(f); return rc; }
    f->kind = FactorKind::Dense;
    *out = f;
    return EIGSOL_OK;
}

// General (non-triangular) sparse solver choice; EIGSOL_SPARSE_SOLVER=band|lu|gmres forces one.
//   band  - RCM + banded partial-pivot LU (band_lu.hip): a direct factor, like the reference's
//           SparseLU, chosen when the RCM band fits the solve kernel's LDS window and the device,
//           and (up to n = 16384) is smaller than the dense matrix;
//   lu    - the densified partial-pivot LU, up to n = 16384;
//   gmres - ILU(0) + GMRES for larger patterns whose RCM band is too wide.  A GMRES that stalls
//           (or an ILU(0) zero pivot) falls back to the densified LU wherever the dense factor fits
//           the device (EIGSOL_GMRES_FALLBACK=0 disables it); otherwise the solve fails with
//           EIGSOL_E_SOLVER, as SparseLU reports a failed solve (solve_shifted.hpp:112-114).
enum SparseSolver { kSolverBand, kSolverLU, kSolverGMRES };

static double device_free_bytes() {
    size_t fr = 0, tot = 0;
    if (hipMemGetInfo(&fr, &tot) != hipSuccess) return 0.0;
    return (double)fr;
}

static bool general_sparse_forced(SparseSolver& out) {
    if (const char* e = std::getenv("EIGSOL_SPARSE_SOLVER")) {
        if (!std::strcmp(e, "gmres")) { out = kSolverGMRES; return true; }
        if (!std::strcmp(e, "lu")) { out = kSolverLU; return true; }
        if (!std::strcmp(e, "band")) { out = kSolverBand; return true; }
    }
    return false;
}

static SparseSolver general_sparse_solver(int64_t n, size_t sb, const BandPlan& plan, bool& forced) {
    forced = false;
    SparseSolver fs;
    if (general_sparse_forced(fs)) {
        forced = true;
        return fs;
    }
    const double dense = (double)n * (double)n * (double)sb;
    const bool band_fits = plan.ok && plan.bytes <= 0.6 * device_free_bytes();
    if (band_fits && (n > 16384 || plan.bytes < dense)) return kSolverBand;
    return n > 16384 ? kSolverGMRES : kSolverLU;
}

static bool gmres_fallback_enabled() {
    const char* e = std::getenv("EIGSOL_GMRES_FALLBACK");
    return !(e && !std::strcmp(e, "0"));
}


// GMRES failed (stalled solve, or ILU(0) zero pivot): switch the factor to the densified LU of A
// (retained in f->gmres.src) when it fits the device; otherwise keep GMRES's error.
static int gmres_dense_fallback(ShiftFactor* f, int rc_gmres) {
    const int64_t n = f->n;
    const double bytes = (double)n * (double)n * (double)scalar_bytes(f->dtype);
    if (!gmres_fallback_enabled() || !f->gmres.src || n > INT32_MAX / 2 || bytes > 0.8 * device_free_bytes())
        return rc_gmres;
    EIGSOL_HIP(hipStreamSynchronize(f->ctx->stream));
    // The densified LU is built in a local factor and moved into f only once it exists: a failed
    // allocation or a zero pivot leaves f a working GMRES factor (later launches and shift_info
    // still see f->gmres) and frees the local one.
    DenseFactor d;
    const int rc = dense_from_csr(f, f->gmres.src, d);
    if (rc != EIGSOL_OK) {
        d.release();
        return rc;
    }
    f->dense = d;   // its buffers now belong to f
    f->gmres.release();
    f->kind = FactorKind::Dense;
    f->fell_back = 1;
    return EIGSOL_OK;
}

template <class S>
static int factor_csr_t(eigsol_csr* A, double sre, double sim, ShiftFactor** out) {
    hipStream_t st = A->ctx->stream;
    const int64_t n = A->nrows, nnz = A->nnz;
    // triangular matrices: the level-ordered factor (tri_factor.hip); any other pattern comes back
    // downloaded, for the dispatch below
    TriHostCsr<S> h;
    *out = nullptr;
    EIGSOL_TRY(tri_build<S>(TriCsrView{A->ctx, A->dtype, n, nnz, A->rowptr, A->col, A->val}, sre, sim, -1, h, out));
    if (*out) return EIGSOL_OK;
    const std::vector<int32_t>&rp = h.rp_own, &ci = h.ci_own;
    const std::vector<S>& v = h.v_own;
    ShiftFactor* f = shift_factor_new(A->ctx, A->dtype, n, sre, sim, nnz);
    int rc = EIGSOL_OK;
    // past n = 16384 the double / complex<double> factors take the GMRES family's direct
    // factors (exact no-pivot LU where the fill stays within 3 x nnz, else the nested-dissection
    // multifrontal LU, gmres.hip / multifrontal.hip; ILU(0) + GMRES when neither fits): the band
    // factor runs one panel kernel per 64 columns on one workgroup (round 5, config5_convdiff_1M:
    // 13.8 s, 1.37 s per solve).  Single precision takes the same family on values widened to
    // double (gm_solve_s).  The band stays for smaller orders, or forced.
    BandPlan plan;
    SparseSolver fs = kSolverBand;
    const bool pre_forced = general_sparse_forced(fs);
    // from n = 1024 (EIGSOL_SPARSE_FAMILY_MIN_N) too: on a 2-D stencil the band solve (one workgroup
    // walking the band) took 0.50 ms per iteration at n = 1024, 2.2 ms at 4096 and 9.5 ms at 16384, the
    // multifrontal LU 0.11 / 0.15 / 0.21 ms with a shorter set-up (round 6, tools/r06_small_sparse_paths.py,
    // profiles/r06_small_sparse_paths.log); the band LU stays the fallback for zero pivots
    static const int64_t family_min = [] {
        const char* e = std::getenv("EIGSOL_SPARSE_FAMILY_MIN_N");
        return e ? (int64_t)std::atoll(e) : (int64_t)1024;
    }();
    const bool large_gmres = !pre_forced && (n > 16384 || n >= family_min);
    if (!large_gmres && !(pre_forced && fs != kSolverBand)) band_plan(A->dtype, n, rp.data(), ci.data(), plan);
    bool forced = false;
    const SparseSolver solver = large_gmres ? kSolverGMRES : general_sparse_solver(n, sizeof(S), plan, forced);
    if (solver == kSolverBand) {
        if (!plan.ok) {
            shift_factor_free(f);
            return fail(EIGSOL_E_UNSUPPORTED, "solve_shifted: the RCM band (kl " + std::to_string(plan.kl) +
                                                  ", ku " + std::to_string(plan.ku) +
                                                  ") is too wide for the band solve");
        }
        rc = band_create(A->ctx, A->dtype, n, rp.data(), ci.data(), v.data(), sre, sim, plan, &f->band);
        if (rc != EIGSOL_OK) { shift_factor_free(f); return rc; }
        f->kind = FactorKind::Band;
        *out = f;
        return EIGSOL_OK;
    }
    if (solver == kSolverGMRES) {
        if constexpr (kGmres<S>) {
            rc = gmres_create(A->ctx, A->dtype, n, rp.data(), ci.data(), v.data(), sre, sim, &f->gmres.gm, A);
        } else {
            using W = GmresScalar<S>;
            std::vector<W> vw(v.size());
            for (size_t e = 0; e < v.size(); ++e) {
                if constexpr (is_real_v<S>) vw[e] = static_cast<double>(v[e]);
                else vw[e] = W{static_cast<double>(v[e].re), static_cast<double>(v[e].im)};
            }
            rc = gmres_create(A->ctx, dtype_complex(A->dtype) ? EIGSOL_C128 : EIGSOL_F64, n, rp.data(), ci.data(),
                              vw.data(), sre, sim, &f->gmres.gm);
            if (rc == EIGSOL_OK && hipMalloc(&f->gmres.promo, 2 * (size_t)n * sizeof(W)) != hipSuccess)
                rc = fail(EIGSOL_E_HIP, "solve_shifted: hipMalloc(single-precision GMRES vectors)");
        }
        GmresState& g = f->gmres;
        g.red_grid = (int)std::max<int64_t>(1, std::min<int64_t>(1024, (n + 1023) / 1024));
        if (rc == EIGSOL_OK && (hipMalloc(&g.work, 64) != hipSuccess ||
                                hipMalloc(&g.wave_part, (size_t)g.red_grid * sizeof(dev::part4)) != hipSuccess ||
                                hipMemsetAsync(g.work, 0, 64, st) != hipSuccess))
            rc = fail(EIGSOL_E_HIP, "solve_shifted: GMRES work buffers");
        f->kind = FactorKind::Gmres;
        g.src = A;
        csr_retain(A);
        if (rc == EIGSOL_E_SOLVER && large_gmres) {
            // every factor of the family met a zero pivot (the no-pivot exact LU, the
            // multifrontal LU's front pivoting, ILU(0)): the partial-pivoting RCM band LU where
            // its band fits, as the reference's pivoting SparseLU would (solve_shifted.hpp:104-106)
            const std::string why = eigsol_last_error();
            BandPlan bp;
            band_plan(A->dtype, n, rp.data(), ci.data(), bp);
            if (bp.ok) {
                ShiftFactor* fb = shift_factor_new(A->ctx, A->dtype, n, sre, sim, nnz);
                if (band_create(A->ctx, A->dtype, n, rp.data(), ci.data(), v.data(), sre, sim, bp, &fb->band) ==
                    EIGSOL_OK) {
                    fb->kind = FactorKind::Band;
                    shift_factor_free(f);
                    *out = fb;
                    return EIGSOL_OK;
                }
                shift_factor_free(fb);
                (void)hipGetLastError();
            }
            rc = fail(EIGSOL_E_SOLVER, why);
        }
        if (rc == EIGSOL_E_SOLVER) rc = gmres_dense_fallback(f, rc);   // ILU(0) zero pivot
        if (rc != EIGSOL_OK) { shift_factor_free(f); return rc; }
        *out = f;
        return EIGSOL_OK;
    }
    // general sparse pattern: densify on the device and LU it (the reference's SparseLU)
    rc = dense_limits(A->dtype, n, "solve_shifted (non-triangular sparse)");
    if (rc == EIGSOL_OK) rc = dense_from_csr(f, A, f->dense);
    if (rc != EIGSOL_OK) { shift_factor_free(f); return rc; }
    f->kind = FactorKind::Dense;
    *out = f;
    return EIGSOL_OK;
}

int shift_factor_csr(eigsol_csr* A, const void* sigma, ShiftFactor** out) {
    if (A->dist) return fail(EIGSOL_E_UNSUPPORTED, "shifted inverse iteration: row-sharded matrices are not supported");
    double s[2] = {0.0, 0.0};
    load_scalar(sigma, A->dtype, s[0], s[1]);   // a real dtype leaves s[1] = 0
    EIGSOL_HIP(hipSetDevice(A->ctx->device));
    return by_dtype(A->dtype, [&](auto tag) { return factor_csr_t<decltype(tag)>(A, s[0], s[1], out); });
}

// the kinds whose kernels wait on each other (cooperative launches): their grid and sticky error word
static bool dense_multi(const ShiftFactor* f) { return f->kind == FactorKind::Dense && f->dense.multi; }

int shift_grid(const ShiftFactor* f) {
    return f->kind == FactorKind::Tri ? f->tri.grid : dense_multi(f) ? f->dense.grid : 1;
}

// a new run of the iteration (session begin): no lagged check of the previous run is carried over
void shift_lag_reset(ShiftFactor* f) {
    f->gmres.lag_prev = false;
    if (f->gmres.gm) gmres_lag_reset(f->gmres.gm);
}

static int pin_scratch(ShiftFactor* f) {
    if (!f->hpin) EIGSOL_HIP(hipHostMalloc(&f->hpin, kPinBytes, hipHostMallocDefault));
    return EIGSOL_OK;
}

int shift_error(ShiftFactor* f) {
    const int32_t* err = f->kind == FactorKind::Tri ? f->tri.err : dense_multi(f) ? f->dense.err : nullptr;
    if (!err) return EIGSOL_OK;
    EIGSOL_TRY(pin_scratch(f));
    int32_t* he = static_cast<int32_t*>(f->hpin);
    EIGSOL_HIP(hipMemcpyAsync(he, err, 4, hipMemcpyDeviceToHost, f->ctx->stream));
    EIGSOL_HIP(stream_wait(f->ctx->stream));
    const int32_t e = *he;
    if (e) return fail(EIGSOL_E_SOLVER, "triangular solve: dependency wait exceeded its bound (internal error)");
    return EIGSOL_OK;
}

// x = M^-1 (b / bdiv) by the GMRES family; single precision through gmres.promo (widen, solve, narrow)
template <class S>
static int gm_solve_s(ShiftFactor* f, const void* b, double bdiv, void* y, bool lag = false) {
    GmresSolver* gm = f->gmres.gm;
    if constexpr (kGmres<S>) {
        return lag ? gmres_solve_lag(gm, b, bdiv, y) : gmres_solve(gm, b, bdiv, y);
    } else {
        using W = GmresScalar<S>;
        hipStream_t st = f->ctx->stream;
        W* wb = static_cast<W*>(f->gmres.promo);
        W* wy = wb + f->n;
        const int grid = (int)std::max<int64_t>(1, std::min<int64_t>(4096, (f->n + 255) / 256));
        hipLaunchKernelGGL((dev::convert_kernel<S, W>), dim3(grid), dim3(256), 0, st, static_cast<const S*>(b), wb, f->n);
        EIGSOL_HIP(hipGetLastError());
        const int rc = lag ? gmres_solve_lag(gm, wb, bdiv, wy) : gmres_solve(gm, wb, bdiv, wy);
        if (rc != EIGSOL_OK) return rc;
        hipLaunchKernelGGL((dev::convert_kernel<W, S>), dim3(grid), dim3(256), 0, st, wy, static_cast<S*>(y), f->n);
        EIGSOL_HIP(hipGetLastError());
        return EIGSOL_OK;
    }
}

// the stop decision of launch it.parity (shift_decide_kernel) and the carry it read, back on the host
struct Decision {
    PowerCarry cr;
    int32_t done;
};
static_assert(sizeof(Decision) <= kPinBytes, "pinned scratch");

static int iter_decide(ShiftFactor* f, const ShiftIter& it, Decision* hd) {
    hipStream_t st = f->ctx->stream;
    EIGSOL_TRY(iter_decide_launch(f, it));
    EIGSOL_HIP(hipMemcpyAsync(&hd->done, &it.ctl->done, sizeof(int32_t), hipMemcpyDeviceToHost, st));
    EIGSOL_HIP(hipMemcpyAsync(&hd->cr, &it.ctl->st[it.parity ^ 1], sizeof(PowerCarry), hipMemcpyDeviceToHost, st));
    EIGSOL_HIP(stream_wait(st));
    return EIGSOL_OK;
}

// One iteration launch on the GMRES family: host-driven (one sync per Arnoldi step), so the iteration is
// prologue launch -> host reads the stop decision -> solve -> partials launch.  A solve the family cannot
// do switches f to the densified LU (gmres_dense_fallback); the caller sees f->kind changed and redoes the
// launch on it - and, with *redo_prev set, the previous launch first.
template <class S>
static int gmres_iter(ShiftFactor* f, const ShiftIter& it, bool* redo_prev) {
    hipStream_t st = f->ctx->stream;
    GmresState& g = f->gmres;
    const int parity = it.parity;
    EIGSOL_TRY(pin_scratch(f));
    Decision* hd = static_cast<Decision*>(f->hpin);
    EIGSOL_TRY(iter_decide(f, it, hd));
    if (g.lag_prev) {
        // the previous launch's direct solve was checked without a host wait (gmres_solve_lag): read
        // the check now; a miss redoes that iteration with the checked solve (and GMRES refinement),
        // its partials, and this launch's decision.  The previous launch read B[parity] and wrote
        // B[parity ^ 1]... in its own parity: it solved from buffer (parity ? buf1 : buf0) into
        // (parity ? buf0 : buf1), and neither has been touched since.
        g.lag_prev = false;
        const int v = gmres_lag_verdict(g.gm);
        if (v != EIGSOL_OK && v != EIGSOL_E_SOLVER) return v;
        if (v == EIGSOL_E_SOLVER) {
            ShiftIter prev = it;
            prev.parity = parity ^ 1;
            const int pp = prev.parity;
            const int rc = gm_solve_s<S>(f, pp ? it.buf0 : it.buf1, g.lag_bdiv, pp ? it.buf1 : it.buf0);
            if (rc == EIGSOL_E_SOLVER) {
                // the checked solve failed too: the densified LU redoes the previous launch (its
                // prologue re-takes that launch's decision from the same carry), then this one
                EIGSOL_TRY(gmres_dense_fallback(f, rc));
                EIGSOL_HIP(hipMemsetAsync(&it.ctl->done, 0, sizeof(int32_t), st));
                *redo_prev = true;
                return EIGSOL_OK;
            }
            EIGSOL_TRY(rc);
            EIGSOL_TRY(iter_part_launch(f, prev));
            // this launch's decision again, from the corrected partials (the prologue writes the
            // same carry slot and trace entry; a stop it had decided is undone first)
            EIGSOL_HIP(hipMemsetAsync(&it.ctl->done, 0, sizeof(int32_t), st));
            EIGSOL_TRY(iter_decide(f, it, hd));
        }
    }
    const int32_t done = hd->done;
    const PowerCarry cr = hd->cr;
    if (done) return EIGSOL_OK;
    // Every solve starts from x0 = 0.  A warm start from the latest eigenvalue estimate,
    // y ~ x / (lambda - sigma), was tried in round 4 on config 5's matrix made general and removed:
    // 54 against 55 Arnoldi steps over the run and 9.1 against 8.9 ms per iteration - the guess
    // only beats x0 = 0 once the iterate's residual is below |lambda - sigma|, i.e. in the last
    // one or two iterations
    // the direct solve's check is read at the next launch's decision wait (one host wait per
    // iteration instead of two) where the factor is complete and needs no refinement by design
    const bool lag = gmres_can_lag(g.gm);
    const int rc = gm_solve_s<S>(f, parity ? it.buf0 : it.buf1, cr.nrm, parity ? it.buf1 : it.buf0, lag);
    if (lag && rc == EIGSOL_OK) {
        g.lag_prev = true;
        g.lag_bdiv = cr.nrm;
    }
    // a failed solve switches to the densified LU, which redoes this launch: the dense kernel's prologue
    // re-evaluates the same decision from the same carry record (idempotent)
    if (rc == EIGSOL_E_SOLVER) return gmres_dense_fallback(f, rc);
    EIGSOL_TRY(rc);
    return iter_part_launch(f, it);
}

// a plain solve on the GMRES family; a failed one switches f to the densified LU for the caller to redo it
template <class S>
static int gmres_solve_once(ShiftFactor* f, const void* b, void* y) {
    const int rc = gm_solve_s<S>(f, b, 0.0, y);
    return rc == EIGSOL_E_SOLVER ? gmres_dense_fallback(f, rc) : rc;
}

static int shift_launch(ShiftFactor* f, bool iter, const void* b, void* y, const ShiftIter& it, bool first) {
    switch (f->kind) {
        case FactorKind::Tri: return tri_launch(f, iter, b, y, it, first);
        case FactorKind::Band: return band_launch(f->band, iter, b, y, it);
        case FactorKind::Gmres: {
            bool redo_prev = false;
            EIGSOL_TRY(by_dtype(f->dtype, [&](auto tag) -> int {
                using S = decltype(tag);
                return iter ? gmres_iter<S>(f, it, &redo_prev) : gmres_solve_once<S>(f, b, y);
            }));
            if (f->kind == FactorKind::Gmres) return EIGSOL_OK;
            if (redo_prev) {   // fell back to the densified LU after a failed lagged check
                ShiftIter prev = it;
                prev.parity ^= 1;
                EIGSOL_TRY(dense_launch(f, iter, b, y, prev));
            }
        }   // fell back: the launch on the densified LU
        [[fallthrough]];
        case FactorKind::Dense: return dense_launch(f, iter, b, y, it);
    }
    return fail(EIGSOL_E_INVALID, "shifted solve: unknown factor kind");
}

int shift_iter_launch(ShiftFactor* f, const ShiftIter& it, int first) {
    return shift_launch(f, true, nullptr, nullptr, it, first != 0);
}

int shift_solve_launch(ShiftFactor* f, const void* b_dev, void* y_dev) {
    return shift_launch(f, false, b_dev, y_dev, ShiftIter{}, false);
}

// algorithmic bytes of one solve (the SpTRSV counts like the SpMV) and variant
void shift_info(const ShiftFactor* f, double* bytes, int32_t* variant, int32_t* tiles) {
    const double sb = (double)scalar_bytes(f->dtype), n = (double)f->n;
    switch (f->kind) {
        case FactorKind::Gmres:
            gmres_info(f->gmres.gm, bytes, tiles);
            if (variant) {
                const int c = gmres_complete(f->gmres.gm);
                *variant = c == 2 ? 19 : c ? 18 : 7;   // 19: nested-dissection multifrontal LU
            }
            break;
        case FactorKind::Band:
            band_info(f->band, bytes, tiles);
            if (variant) *variant = 8;
            break;
        case FactorKind::Tri:
            if (bytes) *bytes = (sb + 4.0) * (double)f->nnz_total + 4.0 * (n + 1.0) + 2.0 * sb * n;
            if (variant) *variant = f->tri.multi > 1 ? 10 + f->tri.multi : 3;   // 12/13/14: 2/3/4 iterations per launch
            if (tiles) *tiles = f->tri.nlevels;
            break;
        case FactorKind::Dense:
            if (bytes) *bytes = sb * n * n + 2.0 * sb * n;
            if (variant) *variant = (f->dense.multi && f->dense.version == 1) ? 20 : 4;   // 20: dense_trsv_kernel
            if (tiles) *tiles = 0;
            break;
    }
}

}  // namespace eigsol
