// Reordering of a Schur form A = Z T Z^H so that a selected set of eigenvalues leads T (gfx950; EIGSOL_F64:
// quasi-triangular T with schur's standard 2 x 2 blocks; EIGSOL_C128: triangular T).  DESIGN.md section 23.
//
//   1. qr_range_guard on T; T is scaled back by the same power of two, exactly, at the end;
//   2. one flag byte per row on the device: from the caller's mask (real: a flag on either row of a 2 x 2
//      block selects the pair) or, for a sort code, from the eigenvalues schur left on the device.  A flag
//      moves with its row in every swap;
//   3. rounds of disjoint windows, odd-even merge-split over half-windows of h rows (47 real, 32 complex):
//      round r takes the nominal windows [(2 k + (r & 1)) h, (2 k + (r & 1) + 2) h).  A real window moves its
//      own ends on the device: a 2 x 2 block that straddles a nominal boundary belongs to the window above
//      it (the one with the smaller rows), so a window starts one row later where T(a, a - 1) != 0 and ends
//      one row later where T(b, b - 1) != 0: at most 2 h + 1 = 95 rows.  The host never learns where the
//      blocks are.
//        ord_bounds fixes the windows' ends in a launch of its own.  ord_window_kernel, one wave per window:
//      the window of T, its flags and U = I in LDS (2 x 96 x 97 doubles / 2 x 64 x 65 complex); every selected
//      block is moved to the window's top by swaps of adjacent blocks (ordschur.hpp: LAPACK dlaexc / ztrexc),
//      every lane computing the swap's few scalars from the same LDS words and the lanes sharing the rows and
//      columns it touches.  A window with nothing to move writes nothing.  A rejected swap ends the window's
//      work and is reported in its descriptor by a plain store.
//        ord_update<left>, ord_update<right>, ord_update<Z>: T(s:e, e:n) <- U^H T(s:e, e:n), then
//      T(0:s, s:e) <- T(0:s, s:e) U, then Z(:, s:e) <- Z(:, s:e) U for every window that worked, on the
//      fp64 matrix cores (window_update_tile of mfma_window.hpp, shared with the QR sweeps), the
//      window descriptors read from device memory; the tiles of an idle window leave at once.  All lefts
//      before all rights; Z is a launch T never reads;
//        the host reads three words per round (windows that worked, rejected swaps, swaps) and stops after
//      two successive rounds, one of each parity, without work;
//   4. the eigenvalues are read from T's blocks (schur.hip's kernels), the selected rows are counted.
// No atomics and every sum in a fixed order: two runs give the same bits, and T and the eigenvalues have the
// same bits with and without Z.
#include <algorithm>
#include <cmath>
#include <cstring>
#include <vector>

#include "kernels_common.hpp"
#include "mfma_window.hpp"
#include "ordschur.hpp"
#include "scratch.hpp"

namespace eigsol {
namespace dev {

struct OrdWin {
    int s, W, active, swaps, failed, pad0, pad1, pad2;
};

// the pair rule of LAPACK xTRSEN: a flag on either row of a 2 x 2 block selects both
__global__ __launch_bounds__(256) void ord_flags_mask(const double* T, int64_t n, const unsigned char* sel, unsigned char* flags,
                                                      int real) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    bool f = sel[i] != 0;
    if (real) {
        if (i + 1 < n && T[(i + 1) + i * n] != 0.0) f = f || sel[i + 1] != 0;
        if (i > 0 && T[i + (i - 1) * n] != 0.0) f = f || sel[i - 1] != 0;
    }
    flags[i] = f ? 1 : 0;
}

// w: (re, im) per row; the two members of a pair give the same answer
__global__ __launch_bounds__(256) void ord_flags_sort(const double* w, int64_t n, int sort, unsigned char* flags) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const double re = w[2 * i], im = w[2 * i + 1];
    bool f;
    if (sort == EIGSOL_SORT_LHP) f = re < 0.0;
    else if (sort == EIGSOL_SORT_RHP) f = re >= 0.0;
    else if (sort == EIGSOL_SORT_IUC) f = re * re + im * im <= 1.0;   // as the host's mask, rounding for rounding
    else f = re * re + im * im > 1.0;
    flags[i] = f ? 1 : 0;
}

__global__ __launch_bounds__(256) void ord_count(const unsigned char* flags, int64_t n, long long* out) {
    __shared__ long long part[256];
    long long s = 0;
    for (int64_t k = threadIdx.x; k < n; k += 256) s += flags[k];
    part[threadIdx.x] = s;
    __syncthreads();
    for (int w = 128; w > 0; w >>= 1) {
        if ((int)threadIdx.x < w) part[threadIdx.x] += part[threadIdx.x + w];
        __syncthreads();
    }
    if (threadIdx.x == 0) *out = part[0];
}

// word[0..2] = windows that worked, windows with a rejected swap, swaps
__global__ __launch_bounds__(64) void ord_round_summary(const OrdWin* wins, int nwin, int* word) {
    if (threadIdx.x != 0) return;
    int a = 0, f = 0, s = 0;
    for (int g = 0; g < nwin; ++g) {
        a += wins[g].active;
        f += wins[g].failed;
        s += wins[g].swaps;
    }
    word[0] = a;
    word[1] = f;
    word[2] = s;
}

__device__ __forceinline__ bool ord_nz(double a) { return a != 0.0; }
__device__ __forceinline__ bool ord_nz(cplx) { return false; }   // triangular: no block straddles
__device__ __forceinline__ double ord_one(double) { return 1.0; }
__device__ __forceinline__ cplx ord_one(cplx) { return cplx{1.0, 0.0}; }

template <class S> constexpr size_t ord_lds_bytes() {
    return (size_t)2 * OrdDims<S>::wmax * OrdDims<S>::ld * sizeof(S) + 128;
}

// The windows of round `phase`: window g's rows [s, s + W) from its nominal ends and T's sub-diagonal, in a
// launch of its own, because a window rewrites the sub-diagonal entry its neighbour below looks at.
template <class S>
__global__ __launch_bounds__(256) void ord_bounds(const S* T, int64_t n, int phase, int nwin, OrdWin* wins) {
    constexpr int h = OrdDims<S>::h;
    const int g = blockIdx.x * 256 + threadIdx.x;
    if (g >= nwin) return;
    OrdWin me{0, 0, 0, 0, 0, 0, 0, 0};
    const int64_t a = (int64_t)(2 * g + phase) * h, b = min<int64_t>(a + 2 * h, n);
    if (a < n) {
        const int64_t s = a + ((a > 0 && ord_nz(T[a + (a - 1) * n])) ? 1 : 0);
        const int64_t e = b + ((b < n && ord_nz(T[b + (b - 1) * n])) ? 1 : 0);
        me.s = (int)s;
        me.W = (int)(e - s);
    }
    wins[g] = me;
}

// One wave per window (see the head of this file).
template <class S>
__global__ __launch_bounds__(64) void ord_window_kernel(S* T, int64_t n, unsigned char* flags, OrdWin* wins, S* Us) {
    constexpr int WM = OrdDims<S>::wmax, LD = OrdDims<S>::ld;
    extern __shared__ __align__(16) unsigned char ord_lds[];
    S* const t = reinterpret_cast<S*>(ord_lds);
    S* const u = t + WM * LD;
    unsigned char* const f = reinterpret_cast<unsigned char*>(u + WM * LD);
    const int lane = threadIdx.x, g = blockIdx.x;
    OrdWin me = wins[g];   // s and W from ord_bounds
    const int64_t s = me.s;
    const int W = me.W;
    if (W > WM) {   // cannot happen (2 h + 1 <= WM); if it ever did, the host must not report an ordered T
        me.failed = 1;
        if (lane == 0) wins[g] = me;
        return;
    }
    if (W < 2) return;
    for (int i = lane; i < W; i += 64) f[i] = flags[s + i];
    __syncthreads();
    bool work = false, gap = false;
    for (int i = 0; i < W; ++i) {
        if (!f[i]) gap = true;
        else if (gap) work = true;
    }
    if (!work) return;
    for (int idx = lane; idx < W * W; idx += 64) {
        const int i = idx % W, j = idx / W;
        t[i + j * LD] = T[(s + i) + (s + j) * n];
        u[i + j * LD] = i == j ? ord_one(S{}) : s_zero<S>();
    }
    __syncthreads();
    int failed = 0;
    const int swaps = ord_window<S>(t, u, f, W, LD, lane, 64, failed);
    __syncthreads();
    for (int idx = lane; idx < W * W; idx += 64) {
        const int i = idx % W, j = idx / W;
        if (i <= j + 1) T[(s + i) + (s + j) * n] = t[i + j * LD];
        Us[(size_t)g * WM * WM + i + j * WM] = u[i + j * LD];
    }
    for (int i = lane; i < W; i += 64) flags[s + i] = f[i];
    me.active = 1;
    me.swaps = swaps;
    me.failed = failed;
    if (lane == 0) wins[g] = me;
}

// The delayed updates of one round's windows, window blockIdx.y, 64 columns (left) or rows (right) per
// workgroup, on the fp64 matrix cores (mfma_window.hpp): kKind 0: M = T, T(s:e, e:n) <- U^H T(s:e, e:n);
// 1: M = T, T(0:s, s:e) <- T(0:s, s:e) U; 2: M = Z, Z(:, s:e) <- Z(:, s:e) U.  The tiles of an idle window
// and the tiles past a region's end leave at once.
template <class S, int kKind>
__global__ __launch_bounds__(256) void ord_update(S* M, int64_t n, const OrdWin* wins, const S* Us) {
    constexpr int kWin = OrdDims<S>::wmax;
    const OrdWin w = wins[blockIdx.y];
    if (!w.active) return;
    const int64_t lo = kKind == 0 ? (int64_t)w.s + w.W : 0, hi = kKind == 1 ? (int64_t)w.s : n;
    const int64_t base = lo + (int64_t)blockIdx.x * 64;
    if (base >= hi) return;
    window_update_tile<S, kWin, kKind == 0>(M, n, w.s, w.W, base, (int)min<int64_t>(64, hi - base),
                                            Us + (size_t)blockIdx.y * kWin * kWin, kWin);
}

}  // namespace dev

namespace {

template <int kKind, class S>
void ord_launch_update(hipStream_t st, dim3 grid, S* M, int64_t n, const dev::OrdWin* wins, const S* Us) {
    hipLaunchKernelGGL((dev::ord_update<S, kKind>), grid, dim3(256), 0, st, M, n, wins, Us);
}

}  // namespace

template <class S>
int ordschur_device(eigsol_ctx* ctx, int64_t n, SchurDevice& sd, bool wantz, const unsigned char* select_host, int sort,
                    int64_t* sdim, int32_t* ordered, OrdStats* stats) {
    constexpr bool kReal = std::is_same_v<S, double>;
    constexpr int h = OrdDims<S>::h, WM = OrdDims<S>::wmax;
    hipStream_t st = ctx->stream;
    S* const T = sd.T.as<S>();
    S* const Z = wantz ? sd.Z.as<S>() : nullptr;
    const unsigned grow = (unsigned)((n + 255) / 256);
    const int nhalf = (int)((n + h - 1) / h), nwmax = (nhalf + 1) / 2;
    DevBuf dflags, dsel, dwins, dU, dword, dcount;
    StageClock clock;
    EIGSOL_TRY(clock.start(1));
    EIGSOL_TRY(dflags.alloc((size_t)n));
    EIGSOL_TRY(dwins.alloc((size_t)nwmax * sizeof(dev::OrdWin)));
    EIGSOL_TRY(dU.alloc((size_t)nwmax * WM * WM * sizeof(S)));
    EIGSOL_TRY(dword.alloc(4 * sizeof(int)));
    EIGSOL_TRY(dcount.alloc(sizeof(long long)));
    EIGSOL_TRY(clock.mark(0, st));
    unsigned char* const flags = dflags.as<unsigned char>();
    if (select_host) {
        EIGSOL_TRY(dsel.alloc((size_t)n));
        EIGSOL_HIP(hipMemcpyAsync(dsel.p, select_host, (size_t)n, hipMemcpyHostToDevice, st));
        hipLaunchKernelGGL(dev::ord_flags_mask, dim3(grow), dim3(256), 0, st, sd.T.as<double>(), n, dsel.as<unsigned char>(), flags,
                           kReal ? 1 : 0);
    } else {
        hipLaunchKernelGGL(dev::ord_flags_sort, dim3(grow), dim3(256), 0, st, sd.w.as<double>(), n, sort, flags);
    }
    EIGSOL_HIP(hipGetLastError());
    int escale = 0;
    EIGSOL_TRY(qr_range_guard(st, sd.T.as<double>(), (kReal ? 1 : 2) * n * n, &escale));
    constexpr size_t lds = dev::ord_lds_bytes<S>();
    EIGSOL_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(dev::ord_window_kernel<S>),
                                   hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    dev::OrdWin* const wins = dwins.as<dev::OrdWin>();
    const unsigned tiles = (unsigned)((n + 63) / 64);
    OrdStats os;
    bool failed = false, done = false;
    int idle = 0;
    const int maxr = 2 * nhalf + 8;
    for (int r = 0; r < maxr && !done && !failed; ++r) {
        const int phase = r & 1;
        const int nwin = n > (int64_t)phase * h ? (int)((n - (int64_t)phase * h + 2 * h - 1) / (2 * h)) : 0;
        int word[4] = {0, 0, 0, 0};
        if (nwin > 0) {
            hipLaunchKernelGGL(dev::ord_bounds<S>, dim3((unsigned)((nwin + 255) / 256)), dim3(256), 0, st, T, n, phase, nwin, wins);
            hipLaunchKernelGGL(dev::ord_window_kernel<S>, dim3((unsigned)nwin), dim3(64), lds, st, T, n, flags, wins, dU.as<S>());
            hipLaunchKernelGGL(dev::ord_round_summary, dim3(1), dim3(64), 0, st, wins, nwin, dword.as<int>());
            const dim3 grid(tiles, (unsigned)nwin);
            ord_launch_update<0>(st, grid, T, n, wins, dU.as<S>());
            ord_launch_update<1>(st, grid, T, n, wins, dU.as<S>());
            if (Z) ord_launch_update<2>(st, grid, Z, n, wins, dU.as<S>());
            EIGSOL_HIP(hipGetLastError());
            EIGSOL_HIP(hipMemcpyAsync(word, dword.p, 3 * sizeof(int), hipMemcpyDeviceToHost, st));
            EIGSOL_HIP(hipStreamSynchronize(st));
        }
        if (word[0] > 0) {
            idle = 0;
            ++os.rounds;
            os.windows += word[0];
            os.swaps += word[2];
        } else if (++idle == 2) {
            done = true;
        }
        if (word[1] > 0) failed = true;
    }
    if (escale != 0)
        qr_scale_pow2(st, sd.T.as<double>(), (kReal ? 1 : 2) * n * n, -escale);
    if constexpr (kReal)
        hipLaunchKernelGGL(dev::schur_eigs_real, dim3(grow), dim3(256), 0, st, sd.T.as<double>(), n, sd.w.as<double>());
    else
        hipLaunchKernelGGL(dev::schur_eigs_cplx, dim3(grow), dim3(256), 0, st, sd.T.as<cplx>(), n, sd.w.as<cplx>());
    hipLaunchKernelGGL(dev::ord_count, dim3(1), dim3(256), 0, st, flags, n, dcount.as<long long>());
    EIGSOL_HIP(hipGetLastError());
    long long cnt = 0;
    EIGSOL_HIP(hipMemcpyAsync(&cnt, dcount.p, sizeof(long long), hipMemcpyDeviceToHost, st));
    EIGSOL_TRY(clock.mark(1, st));
    EIGSOL_HIP(hipStreamSynchronize(st));
    clock.read(&os.ms, 1);
    if (sdim) *sdim = cnt;
    if (ordered) *ordered = (done && !failed) ? 1 : 0;
    if (stats) *stats = os;
    return EIGSOL_OK;
}

template int ordschur_device<double>(eigsol_ctx*, int64_t, SchurDevice&, bool, const unsigned char*, int, int64_t*, int32_t*,
                                     OrdStats*);
template int ordschur_device<cplx>(eigsol_ctx*, int64_t, SchurDevice&, bool, const unsigned char*, int, int64_t*, int32_t*,
                                   OrdStats*);

namespace {

void ord_store_stats(eigsol_ctx* ctx, const OrdStats& os) {
    ctx->ordschur_ms = os.ms;
    ctx->ordschur_counts[0] = os.rounds;
    ctx->ordschur_counts[1] = os.windows;
    ctx->ordschur_counts[2] = os.swaps;
}

template <class S>
void ord_eigs_out(const std::vector<cplx>& w, int64_t n, void* eig_re_or_c, double* eig_im) {
    if constexpr (std::is_same_v<S, double>) {
        double* re = static_cast<double*>(eig_re_or_c);
        for (int64_t i = 0; i < n; ++i) {
            re[i] = w[i].re;
            if (eig_im) eig_im[i] = w[i].im;
        }
    } else {
        std::memcpy(eig_re_or_c, w.data(), (size_t)n * sizeof(cplx));
    }
}

// 0: a Schur form; 1: not (quasi-)triangular or a 2 x 2 block not in schur's standard form; 2: non-finite
template <class S>
int ord_check_T(const S* T, int64_t n) {
    constexpr bool kReal = std::is_same_v<S, double>;
    const double* a = reinterpret_cast<const double*>(T);
    const int64_t cnt = (kReal ? 1 : 2) * n * n;
    for (int64_t i = 0; i < cnt; ++i)
        if (!std::isfinite(a[i])) return 2;
    for (int64_t j = 0; j < n; ++j)
        for (int64_t i = j + 2; i < n; ++i)
            if (mod_abs(T[i + j * n]) != 0.0) return 1;
    bool prev = false;
    for (int64_t k = 0; k + 1 < n; ++k) {
        const bool nz = mod_abs(T[(k + 1) + k * n]) != 0.0;
        if (!kReal && nz) return 1;
        if (nz && prev) return 1;
        if constexpr (kReal) {
            if (nz) {
                const double b = T[k + (k + 1) * n], c = T[(k + 1) + k * n];
                if (T[k + k * n] != T[(k + 1) + (k + 1) * n] || b == 0.0 || std::signbit(b) == std::signbit(c)) return 1;
            }
        }
        prev = nz;
    }
    return 0;
}

template <class S>
int ordschur_host(eigsol_ctx* ctx, int64_t n, void* T_inout, void* Z_inout, const uint8_t* select, void* eig_re_or_c,
                  double* eig_im, int64_t* sdim, int32_t* ordered) {
    const int bad = ord_check_T<S>(static_cast<const S*>(T_inout), n);
    if (bad == 2) return fail(EIGSOL_E_SOLVER, "eigsol_ordschur_dense: T holds a non-finite entry");
    if (bad == 1) return fail(EIGSOL_E_INVALID, "eigsol_ordschur_dense: T is not a Schur form with standard 2 x 2 blocks");
    if (Z_inout) {
        const double* z = static_cast<const double*>(Z_inout);
        const int64_t cnt = (std::is_same_v<S, double> ? 1 : 2) * n * n;
        for (int64_t i = 0; i < cnt; ++i)
            if (!std::isfinite(z[i])) return fail(EIGSOL_E_SOLVER, "eigsol_ordschur_dense: Z holds a non-finite entry");
    }
    hipStream_t st = ctx->stream;
    const bool wantz = Z_inout != nullptr;
    SchurDevice sd;
    EIGSOL_TRY(sd.T.alloc((size_t)n * n * sizeof(S)));
    EIGSOL_TRY(sd.w.alloc((size_t)n * sizeof(cplx)));
    if (wantz) EIGSOL_TRY(sd.Z.alloc((size_t)n * n * sizeof(S)));
    EIGSOL_HIP(hipMemcpyAsync(sd.T.p, T_inout, (size_t)n * n * sizeof(S), hipMemcpyHostToDevice, st));
    if (wantz) EIGSOL_HIP(hipMemcpyAsync(sd.Z.p, Z_inout, (size_t)n * n * sizeof(S), hipMemcpyHostToDevice, st));
    OrdStats os;
    int64_t cnt = 0;
    int32_t ok = 0;
    EIGSOL_TRY(ordschur_device<S>(ctx, n, sd, wantz, select, 0, &cnt, &ok, &os));
    std::vector<cplx> w(n);
    EIGSOL_HIP(hipMemcpyAsync(w.data(), sd.w.p, (size_t)n * sizeof(cplx), hipMemcpyDeviceToHost, st));
    EIGSOL_HIP(hipMemcpyAsync(T_inout, sd.T.p, (size_t)n * n * sizeof(S), hipMemcpyDeviceToHost, st));
    if (wantz) EIGSOL_HIP(hipMemcpyAsync(Z_inout, sd.Z.p, (size_t)n * n * sizeof(S), hipMemcpyDeviceToHost, st));
    EIGSOL_HIP(hipStreamSynchronize(st));
    ord_store_stats(ctx, os);
    ord_eigs_out<S>(w, n, eig_re_or_c, eig_im);
    if (sdim) *sdim = cnt;
    if (ordered) *ordered = ok;
    return EIGSOL_OK;
}

template <class S>
int schur_sorted_host(eigsol_ctx* ctx, int64_t n, const void* A_host, int max_iter, int sort, void* T_out, void* Z_out,
                      void* eig_re_or_c, double* eig_im, int64_t* sdim, int32_t* iterations, int32_t* converged,
                      int32_t* ordered) {
    {
        const double* a = static_cast<const double*>(A_host);
        const int64_t cnt = (std::is_same_v<S, double> ? 1 : 2) * n * n;
        for (int64_t i = 0; i < cnt; ++i)
            if (!std::isfinite(a[i])) return fail(EIGSOL_E_SOLVER, "eigsol_schur_sorted_dense: the matrix holds a non-finite entry");
    }
    hipStream_t st = ctx->stream;
    const bool wantz = Z_out != nullptr;
    StageClock clock;
    EIGSOL_TRY(clock.start(4));
    SchurDevice sd;
    EIGSOL_TRY(schur_device<S>(ctx, n, A_host, max_iter, wantz, sd, clock));
    OrdStats os;
    int64_t cnt = 0;
    int32_t ok = 0;
    if (!sd.failed) EIGSOL_TRY(ordschur_device<S>(ctx, n, sd, wantz, nullptr, sort, &cnt, &ok, &os));   // T and Z stay on the device
    std::vector<cplx> w(n);
    EIGSOL_HIP(hipMemcpyAsync(w.data(), sd.w.p, (size_t)n * sizeof(cplx), hipMemcpyDeviceToHost, st));
    EIGSOL_HIP(hipMemcpyAsync(T_out, sd.T.p, (size_t)n * n * sizeof(S), hipMemcpyDeviceToHost, st));
    if (wantz) EIGSOL_HIP(hipMemcpyAsync(Z_out, sd.Z.p, (size_t)n * n * sizeof(S), hipMemcpyDeviceToHost, st));
    EIGSOL_TRY(clock.mark(4, st));
    EIGSOL_HIP(hipStreamSynchronize(st));
    clock.read(ctx->schur_ms, 4);
    ord_store_stats(ctx, os);
    ord_eigs_out<S>(w, n, eig_re_or_c, eig_im);
    if (sdim) *sdim = cnt;
    if (iterations) *iterations = sd.sweeps;
    if (converged) *converged = sd.failed ? 0 : 1;
    if (ordered) *ordered = ok;
    return EIGSOL_OK;
}

int ord_check_args(const char* who, eigsol_ctx* ctx, int dtype, int64_t n) {
    if (dtype_wide(dtype) || dtype_single(dtype))
        return fail(EIGSOL_E_UNSUPPORTED, std::string(who) + ": double and complex double matrices only");
    if (!dtype_valid(dtype)) return fail(EIGSOL_E_INVALID, std::string(who) + ": unknown dtype");
    if (n > (dtype == EIGSOL_C128 ? hess_max_order_c128() : hess_max_order_f64()))
        return fail(EIGSOL_E_UNSUPPORTED, std::string(who) + ": n above the order the blocked Hessenberg reduction accepts");
    EIGSOL_HIP(hipSetDevice(ctx->device));
    return EIGSOL_OK;
}

}  // namespace
}  // namespace eigsol

using namespace eigsol;

extern "C" {

int eigsol_ordschur_dense(eigsol_ctx* ctx, int dtype, int64_t n, void* T_inout, void* Z_inout, const uint8_t* select,
                          void* eig_re_or_c, double* eig_im, int64_t* sdim, int32_t* ordered) {
    const char* who = "eigsol_ordschur_dense";
    if (n < 0) return fail(EIGSOL_E_INVALID, std::string(who) + ": negative order");
    if (!ctx) return fail(EIGSOL_E_INVALID, std::string(who) + ": null context");
    if (n == 0) {
        if (sdim) *sdim = 0;
        if (ordered) *ordered = 1;
        return EIGSOL_OK;
    }
    if (!T_inout || !select || !eig_re_or_c) return fail(EIGSOL_E_INVALID, std::string(who) + ": null pointer");
    EIGSOL_TRY(ord_check_args(who, ctx, dtype, n));
    if (dtype == EIGSOL_F64 && !eig_im) return fail(EIGSOL_E_INVALID, std::string(who) + ": null eig_im for a real matrix");
    return dtype == EIGSOL_C128 ? ordschur_host<cplx>(ctx, n, T_inout, Z_inout, select, eig_re_or_c, eig_im, sdim, ordered)
                                : ordschur_host<double>(ctx, n, T_inout, Z_inout, select, eig_re_or_c, eig_im, sdim, ordered);
}

int eigsol_schur_sorted_dense(eigsol_ctx* ctx, int dtype, int64_t n, const void* A_colmajor, const eigsol_solver_options* opts,
                              int sort, void* T_out, void* Z_out, void* eig_re_or_c, double* eig_im, int64_t* sdim,
                              int32_t* iterations, int32_t* converged, int32_t* ordered) {
    const char* who = "eigsol_schur_sorted_dense";
    if (n < 0) return fail(EIGSOL_E_INVALID, std::string(who) + ": negative order");
    if (!ctx) return fail(EIGSOL_E_INVALID, std::string(who) + ": null context");
    if (sort < EIGSOL_SORT_LHP || sort > EIGSOL_SORT_OUC) return fail(EIGSOL_E_INVALID, std::string(who) + ": unknown sort code");
    const int max_iter = opts ? opts->max_iterations : 1000;
    if (n == 0) {
        if (sdim) *sdim = 0;
        if (iterations) *iterations = 0;
        if (converged) *converged = 1;
        if (ordered) *ordered = 1;
        return EIGSOL_OK;
    }
    if (!A_colmajor || !T_out || !eig_re_or_c) return fail(EIGSOL_E_INVALID, std::string(who) + ": null pointer");
    if (max_iter < 1) return fail(EIGSOL_E_INVALID, std::string(who) + ": max_iterations < 1");
    EIGSOL_TRY(ord_check_args(who, ctx, dtype, n));
    if (dtype == EIGSOL_F64 && !eig_im) return fail(EIGSOL_E_INVALID, std::string(who) + ": null eig_im for a real matrix");
    return dtype == EIGSOL_C128 ? schur_sorted_host<cplx>(ctx, n, A_colmajor, max_iter, sort, T_out, Z_out, eig_re_or_c, eig_im, sdim,
                                                          iterations, converged, ordered)
                                : schur_sorted_host<double>(ctx, n, A_colmajor, max_iter, sort, T_out, Z_out, eig_re_or_c, eig_im,
                                                            sdim, iterations, converged, ordered);
}

int eigsol_ordschur_stats(eigsol_ctx* ctx, double* ms, int32_t* rounds, int32_t* windows, int32_t* swaps) {
    if (!ctx) return fail(EIGSOL_E_INVALID, "eigsol_ordschur_stats: null context");
    if (ms) *ms = ctx->ordschur_ms;
    if (rounds) *rounds = ctx->ordschur_counts[0];
    if (windows) *windows = ctx->ordschur_counts[1];
    if (swaps) *swaps = ctx->ordschur_counts[2];
    return EIGSOL_OK;
}

}  // extern "C"
