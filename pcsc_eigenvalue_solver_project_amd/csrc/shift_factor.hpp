// The shifted-solve factor (ShiftFactor): one sub-struct per factor kind, each owning its buffers and its launch
// state, and what the family's translation units share.  sptrsv.hip: the level-ordered triangular solve (TriFactor);
// tri_factor.hip: that factor's analysis and layout; dense_lu.hip: the dense partial-pivot LU (DenseFactor);
// shifted.hip: the factor's lifetime, the general-sparse dispatch and the GMRES family's iteration (GmresState).
// Private to those files; other modules see shifted.hpp.
#pragma once

#include <type_traits>
#include <vector>

#include "band_lu.hpp"
#include "gmres.hpp"
#include "kernels_common.hpp"
#include "shifted.hpp"

namespace eigsol {

namespace dev {
constexpr int kMaxMulti = 4;      // solves per multi-solve launch (one head wave each)
}

constexpr size_t kPinBytes = 256;   // ShiftFactor::hpin

enum class FactorKind { Tri, Dense, Gmres, Band };

template <class T>
static void free_null(T*& p) {
    if (p) hipFree(p);
    p = nullptr;
}

// level-ordered triangular CSR: everything indexed by solve position (rows sorted by level, levels padded)
struct TriFactor {
    int upper = 1;
    int64_t nnz_off = 0;
    int32_t* order = nullptr;     // head position -> row (-1: level padding)
    void* z[2] = {nullptr, nullptr};   // solve values polled by readers; sentinel = not yet solved
    int32_t npos = 0, nchunks = 0, nlevels = 0;
    void* hval = nullptr;         // head, pass-major entries / columns / pivots
    int32_t* hcol = nullptr;
    void* hpiv = nullptr;
    int2* passes = nullptr;       // head passes {first position, end | barrier}
    int32_t npass = 0, hpos = 0, hlevels = 0;
    int wave_head = 1;            // head kernel: 1 one-wave (sptrsv_whead_kernel), 0 one workgroup
    void* wval = nullptr;         // one-wave head, pass-major (see sptrsv_whead_kernel)
    int32_t* wcol = nullptr;
    void* wrp = nullptr;
    int32_t* wdst = nullptr;
    int32_t nwpass = 0;
    int red_grid = 0;             // blocks of the partials reduction
    int2* smeta = nullptr;        // tail slices (see sptrsv_slice_kernel)
    int32_t* trow = nullptr;
    void* tpiv = nullptr;
    int32_t* tcol = nullptr;
    void* tval = nullptr;
    int32_t nslices = 0;
    int slice_b = 16;             // entries per lane held in registers (4, 8 or 16)
    int tail_chunks = 0;          // tail variant: 1 chunk kernel, 0 slice kernel
    int chunk_two = 0;            // chunk kernel with two entries per lane (tail rows longer than 16)
    int32_t* porder = nullptr;    // chunk variant (see sptrsv_chunk_kernel)
    int32_t* pptr = nullptr;
    int32_t* pcol = nullptr;
    void* pval = nullptr;
    void* ppiv = nullptr;
    int32_t chunk0 = 0;
    // tail polls without back-off (EIGSOL_TRSV_POLL_FAST, low 16 bits) and the back-off schedule
    // (EIGSOL_TRSV_POLL_SLOW, bits 16-18; poll_backoff).  Round 6 (tools/r06_trsv_backoff_ab.sh,
    // profiles/r06_trsv_backoff_ab.log, config 5 at K = 4): sleeps of 2 / 8 / 32 x 64 cycles
    // (growing with the spins) 0.4127-0.4134 ms per iteration; a constant 4 / 6 / 8 / 12 / 16:
    // 0.4072-0.4083 (the long sleeps woke late); 32: 0.415.  Default: a constant 8
    int poll_fast = 4 << 16;
    int poll_mode = 2;            // EIGSOL_TRSV_POLL_MODE (bit 0: slice tail, one re-poll per lane; bit 1: chunk tails, the second chunk's first polls after the first chunk: config 5 0.698 -> 0.674 ms, K = 4 0.419 -> 0.414)
    // multi-solve launches (sptrsv_chunk_role_kernel; EIGSOL_TRSV_MULTI=K, 1 disables): K reference
    // iterations per launch, solve j one dependency round behind solve j - 1
    int multi = 1;
    int grid_multi = 0;
    int hconc = 0;                // multi head: every solve's values fit the LDS (sptrsv_whead_kernel)
    void* aux[dev::kMaxMulti - 1] = {};           // w_0 .. w_{K-2} (n scalars each)
    void* zm[dev::kMaxMulti][2] = {};             // solve j >= 1: polled values (zm[0] unused: z)
    int32_t epoch_m = 0;
    void* kpart = nullptr;        // part4 per solve j >= 1: {||w_j||^2, w_{j-1}^H w_j}
    void* kblk = nullptr;         // part4 per block of those reductions
    uint32_t* work = nullptr;     // [2]: last-arriver ticket of the partials reduction
    int32_t* err = nullptr;
    void* wave_part = nullptr;    // part4 per wave
    int32_t epoch = 0;
    int grid = 0;                 // tail grid: one residency round (cooperative launch)

    void release() {
        free_null(order), free_null(z[0]), free_null(z[1]);
        free_null(hval), free_null(hcol), free_null(hpiv), free_null(passes);
        free_null(wval), free_null(wcol), free_null(wrp), free_null(wdst);
        free_null(smeta), free_null(trow), free_null(tpiv), free_null(tcol), free_null(tval);
        free_null(porder), free_null(pptr), free_null(pcol), free_null(pval), free_null(ppiv);
        for (void*& p : aux) free_null(p);
        for (auto& zj : zm) free_null(zj[0]), free_null(zj[1]);
        free_null(kpart), free_null(kblk), free_null(work), free_null(err), free_null(wave_part);
    }
};

// dense partial-pivot LU (Matrix::Dense, densified sparse matrices, the GMRES family's fallback)
struct DenseFactor {
    void* lu = nullptr;           // column-major n x n, L (unit) below, U on and above the diagonal
    int32_t* perm = nullptr;      // P b: b_perm[i] = b[perm[i]]
    int32_t* zero_pivot = nullptr;
    size_t lds_bytes = 0;
    // multi-CU substitution (large n): epoch flags per block row, forward results
    int multi = 0;
    int nblk = 0;                 // block rows of 64
    int32_t* flag_f = nullptr;
    int32_t* flag_b = nullptr;
    void* zf = nullptr;
    void* tinv = nullptr;         // [nblk][2] inverted diagonal blocks inv(L_kk), inv(U_kk), 64 x 64 column-major
    void* tmul = nullptr;         // [nblk][2] premultiplied next-to-diagonal tiles (dense_tmul_kernel)
    int version = 2;              // substitution kernel: 2 = dense_trsv2_kernel, 1 = dense_trsv_kernel (ill-conditioned
                                  // diagonal blocks, or EIGSOL_DENSE_TRSV=1; see dense_lu_factor)
    int32_t epoch = 0;
    int grid = 0;                 // persistent block-row workgroups, all resident (cooperative launch)
    uint32_t* work = nullptr;
    int32_t* err = nullptr;
    void* wave_part = nullptr;    // part4 per workgroup

    void release() {
        free_null(lu), free_null(perm), free_null(zero_pivot), free_null(flag_f), free_null(flag_b);
        free_null(zf), free_null(tinv), free_null(tmul), free_null(work), free_null(err), free_null(wave_part);
    }
};

// the GMRES family (exact / multifrontal LU, ILU(0) + GMRES; gmres.hip) and its host-driven iteration
struct GmresState {
    GmresSolver* gm = nullptr;
    bool lag_prev = false;        // the previous launch's solve check is still to be read
    double lag_bdiv = 0.0;        // ... and that solve's divisor (||y_{t-1}||)
    void* promo = nullptr;        // single precision: [2][n] double-precision right-hand side and solution of
                                  // the family's solve (its factors are built in double)
    eigsol_csr* src = nullptr;    // A, retained for the densified-LU fallback
    int red_grid = 0;             // blocks of the partials reduction
    uint32_t* work = nullptr;
    void* wave_part = nullptr;

    void release() {
        if (gm) gmres_free(gm);
        if (src) csr_release(src);
        gm = nullptr, src = nullptr;
        free_null(promo), free_null(work), free_null(wave_part);
    }
};

struct ShiftFactor {
    eigsol_ctx* ctx = nullptr;
    int dtype = EIGSOL_F64;
    int64_t n = 0;
    double sig_re = 0.0, sig_im = 0.0;
    int64_t nnz_total = 0;        // nonzeros of A (diagonal included), for roofline accounting
    FactorKind kind = FactorKind::Tri;
    int fell_back = 0;            // Dense reached through the GMRES fallback
    void* hpin = nullptr;         // pinned host scratch for per-solve readbacks (pageable copies sleep ~1 ms)
    TriFactor tri;
    DenseFactor dense;
    GmresState gmres;
    BandFactor* band = nullptr;   // band_lu.hip
};

// the launch fields every solve kernel's argument struct shares (TriArgs, DenseSolveArgs, DenseTriArgs)
template <class Args>
static void fill_iter(Args& a, const ShiftFactor* f, const void* b, void* y, const ShiftIter& it) {
    using S = std::remove_pointer_t<decltype(a.buf0)>;
    a.n = f->n;
    a.b_plain = static_cast<const S*>(b);
    a.y_plain = static_cast<S*>(y);
    a.buf0 = static_cast<S*>(it.buf0);
    a.buf1 = static_cast<S*>(it.buf1);
    a.ctl = it.ctl;
    a.rank_part = static_cast<const dev::part4*>(it.rank_part);
    a.my_part = static_cast<dev::part4*>(it.my_part);
    a.trace = static_cast<S*>(it.trace);
    a.sig_re = f->sig_re;
    a.sig_im = f->sig_im;
}

namespace dev {

constexpr int kRowLanes = 16;   // lanes per row: one row per 16-lane group
constexpr int kWaveRows = 64 / kRowLanes;          // positions per wave round (one chunk): levels are padded to this
// An unsolved entry of z holds this NaN in every 8-byte word.  A solved value never does: the
// producer maps it to the default quiet NaN (sanitize), so the value itself is the ready flag.
constexpr unsigned long long kSent = 0x7FF4DEAD7FF4DEADull;
// one-workgroup head (sptrsv_head_kernel)
constexpr int kHeadThreads = 1024;
constexpr int kHeadRows = kHeadThreads / kRowLanes;    // rows per pass
constexpr int kHeadDepth = 8;                          // passes in flight
constexpr int32_t kPassBarrier = 1 << 30;
// one-wave head (sptrsv_whead_kernel)
constexpr int kWHeadDepth = 8;
constexpr int kWHeadRows = 16;   // rows per pass

}  // namespace dev

template <class F>
static int by_dtype(int dtype, F&& fn) {
    switch (dtype) {
        case EIGSOL_C128: return fn(cplx{});
        case EIGSOL_F32: return fn(0.0f);
        case EIGSOL_C64: return fn(cplxf{});
        default: return fn(0.0);
    }
}

template <class S>
static S make_sigma(double re, double im) {
    if constexpr (std::is_same_v<S, double>) { (void)im; return re; }
    else if constexpr (std::is_same_v<S, cplx>) return cplx{re, im};
    else if constexpr (std::is_same_v<S, float>) { (void)im; return (float)re; }
    else return cplxf{(float)re, (float)im};
}
// host arithmetic of the factor set-up (pivots d_i - sigma) in the scalar's own precision
template <class S> static S h_add(S a, S b) {
    if constexpr (is_real_v<S>) return a + b;
    else return S{a.re + b.re, a.im + b.im};
}
template <class S> static S h_sub(S a, S b) {
    if constexpr (is_real_v<S>) return a - b;
    else return S{a.re - b.re, a.im - b.im};
}
template <class S> static bool h_zero(S a) {
    if constexpr (is_real_v<S>) return a == 0;
    else return a.re == 0 && a.im == 0;
}

// shifted.hip
ShiftFactor* shift_factor_new(eigsol_ctx* ctx, int dtype, int64_t n, double sre, double sim, int64_t nnz);

// sptrsv.hip.  Each __global__ template of the family is defined, and its address taken, in one file only
// (cooperative launches, attributes and occupancy queries must name the instantiation that is launched).
int tri_launch_setup(ShiftFactor* f);
int tri_launch(ShiftFactor* f, bool iter, const void* b, void* y, const ShiftIter& it, bool first);
// the GMRES family's iteration: the stop decision of launch it.parity, and the norm / Rayleigh partials of y
int iter_decide_launch(ShiftFactor* f, const ShiftIter& it);
int iter_part_launch(ShiftFactor* f, const ShiftIter& it);

// dense_lu.hip
int dense_limits(int dtype, int64_t n, const char* who);
// factor a copy of the column-major device matrix a, or the densified A, shifted by f's sigma, into d
int dense_from_matrix(const ShiftFactor* f, const void* a, DenseFactor& d);
int dense_from_csr(const ShiftFactor* f, const eigsol_csr* A, DenseFactor& d);
int dense_launch(ShiftFactor* f, bool iter, const void* b, void* y, const ShiftIter& it);

// tri_factor.hip
// a CSR matrix held in three device arrays that stay their owner's
struct TriCsrView {
    eigsol_ctx* ctx;
    int dtype;
    int64_t n, nnz;
    const int32_t* rowptr;
    const int32_t* col;
    const void* val;
};
// the same matrix on the host, for the host build: the caller's arrays (rp set), or tri_build's download
template <class S>
struct TriHostCsr {
    const int32_t* rp = nullptr;
    const int32_t* ci = nullptr;
    const S* v = nullptr;
    std::vector<int32_t> rp_own, ci_own;
    std::vector<S> v_own;
};
// The level-ordered factor of A - sigma I for a triangular A: built on the device, or on the host when
// the host build is forced (tri_host_forced) or the device build declines (h is downloaded then, unless the caller
// filled it).  up: 1 upper, 0 lower, -1 decide from the pattern; *out stays null for a pattern that is
// not triangular, which h then holds for the caller.
template <class S>
int tri_build(const TriCsrView& A, double sre, double sim, int up, TriHostCsr<S>& h, ShiftFactor** out);
}  // namespace eigsol
