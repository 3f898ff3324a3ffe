// Delayed window update on the fp64 matrix cores (gfx950, v_mfma_f64_16x16x4_f64), shared by the
// multishift QR sweeps (francis.hip, zfrancis.hip) and the Schur reordering (ordschur.hip): a small
// accumulated transformation U (W x W, W <= kWin) applied to a strip of a big column-major matrix M,
//
//   left : M(s:s+W, base:base+cnt) <- U^H M(s:s+W, base:base+cnt)     (U^T for double)
//   right: M(base:base+cnt, s:s+W) <- M(base:base+cnt, s:s+W) U
//
// by one 256-thread workgroup; 1 <= cnt <= kTile (the callers leave before the call where a
// workgroup has nothing to do; loads are clamped into the strip and every store is masked by cnt
// and W).  S = double (kWin = 96) or cplx (kWin = 64).
//
// U (and, left, the panel of M) is staged in LDS at the odd-word pitch kWin + 2 ((k + 2 i) mod 32
// is distinct for 32 lanes), zero-padded to kWin, so the k-steps past W add exact zeros; the right
// panel stays in registers, loaded before anything else and consumed last.  Every global load of a
// thread is issued before its first LDS store.  A complex operand is split into re / im planes and a
// complex tile product is four real MFMAs:
//   left : re += Xr Ur + Xi Ui,  im += Xi Ur - Xr Ui        (X conj(U))
//   right: re += Ur Xr - Ui Xi,  im += Ur Xi + Ui Xr
//
// kTile = 64: wave w owns outputs 16 w .. 16 w + 15 of the tile and all kWin / 16 row tiles of U.
// kTile = 32 (double only): waves (w & 1) own 16 outputs and (w >> 1) half of U's row tiles, so twice
// as many workgroups share a launch's MFMA work.  The k order of every output element is the same for
// both tilings: bitwise the same update.
//
// Fragment layout of the f64 MFMA (cdna_hip_programming.md): A operand lane l holds A[l & 15][l >> 4],
// B operand lane l holds B[l >> 4][l & 15], D lane l register r holds D[(l >> 4) + 4 r][l & 15].  D's
// column index is put on the output's row, so 16 lanes store contiguous bytes of one column of M.
#pragma once

#include "kernels_common.hpp"
#include "mfma_rankk.hpp"

namespace eigsol {
namespace dev {

// One side of the delayed updates of up to kMaxW windows in one launch (the QR sweeps).  Left
// regions of different windows own disjoint rows and right regions disjoint columns, so a launch is
// race-free; a left region of a window meets the right region of a window further down the chain,
// hence lefts and rights are two launches (U_g^H X U_h = (U_g^H X) U_h).
template <class S>
struct WindowRegion {
    int s, W;          // window rows/columns [s, s + W)
    int64_t lo, hi;    // left: columns [lo, hi); right: rows [lo, hi)
    int blk0;          // first workgroup of this window
    const S* U;        // W x W, column-major
};
template <class S, int kMaxW>
struct WindowBatch {
    S* H;
    int64_t n;
    int nw;
    WindowRegion<S> w[kMaxW];
};

template <class S, int kWin, bool kLeft, int kTile = 64>
__device__ __forceinline__ void window_update_tile(S* M, int64_t ldm, int s, int W, int64_t base, int cnt, const S* U,
                                                   int ldu) {
    constexpr bool kC = std::is_same_v<S, cplx>;
    static_assert(kC || std::is_same_v<S, double>, "window_update_tile: double or cplx");
    static_assert(kTile == 64 || (kTile == 32 && !kC && kWin == 96), "the 32-wide tiling is the real kernel's");
    constexpr int kUP = kWin + 2;                                    // LDS pitch
    constexpr int kT = kTile == 64 ? kWin / 16 : kWin / 32;          // U row tiles per wave
    constexpr int kKs = kWin / 4;
    constexpr int kXs = kLeft ? kTile * kUP : 1;
    __shared__ double ur_s[kWin * kUP], ui_s[kC ? kWin * kUP : 1];   // u*_s[k + rho * kUP] = U(k, rho), re and im
    __shared__ double xr_s[kXs], xi_s[kC ? kXs : 1];                 // left: x*_s[k + c * kUP] = M(s + k, base + c)
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int li = lane & 15, lk = lane >> 4;
    const int ct = kTile == 64 ? wave : (wave & 1);                  // this wave's 16 columns / rows of the tile
    const int t0 = kTile == 64 ? 0 : kT * (wave >> 1);               // ... and its first U row tile
    // right: this lane's X(r_j, k) for k = lk, lk + 4, ... (issued first, consumed last)
    S xv[kLeft ? 1 : kKs];
    const int rj = 16 * ct + li;
    const bool rv = rj < cnt;
    if constexpr (!kLeft) {
        const S* xr = M + (base + min(rj, max(cnt - 1, 0))) + (int64_t)s * ldm;
#pragma unroll
        for (int q = 0; q < kKs; ++q) xv[q] = xr[(int64_t)min(4 * q + lk, W - 1) * ldm];
    }
    {
        // U (and the left panel) into LDS: every global load of the thread issued before any store
        constexpr int kPU = kWin * kWin / 256;
        S tu[kPU];
#pragma unroll
        for (int q = 0; q < kPU; ++q) {
            const int idx = threadIdx.x + 256 * q;
            const int k = idx % kWin, rho = idx / kWin;
            tu[q] = U[min(k, W - 1) + min(rho, W - 1) * ldu];
        }
        if constexpr (kLeft) {
            constexpr int kPX = kWin * kTile / 256;
            S tx[kPX];
#pragma unroll
            for (int q = 0; q < kPX; ++q) {
                const int idx = threadIdx.x + 256 * q;
                const int k = idx % kWin, c = idx / kWin;
                tx[q] = M[(s + min(k, W - 1)) + (base + min(c, max(cnt - 1, 0))) * ldm];
            }
#pragma unroll
            for (int q = 0; q < kPX; ++q) {
                const int idx = threadIdx.x + 256 * q;
                const int k = idx % kWin, c = idx / kWin;
                const bool ok = k < W && c < cnt;
                xr_s[k + c * kUP] = ok ? re_of(tx[q]) : 0.0;
                if constexpr (kC) xi_s[k + c * kUP] = ok ? im_of(tx[q]) : 0.0;
            }
        }
#pragma unroll
        for (int q = 0; q < kPU; ++q) {
            const int idx = threadIdx.x + 256 * q;
            const int k = idx % kWin, rho = idx / kWin;
            const bool ok = k < W && rho < W;
            ur_s[k + rho * kUP] = ok ? re_of(tu[q]) : 0.0;
            if constexpr (kC) ui_s[k + rho * kUP] = ok ? im_of(tu[q]) : 0.0;
        }
    }
    __syncthreads();
    auto mfma = [](double a, double b, mfma_d4 c) { return __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, c, 0, 0, 0); };
    mfma_d4 aR[kT], aI[kC ? kT : 1];
#pragma unroll
    for (int t = 0; t < kT; ++t) {
        aR[t] = mfma_d4{0.0, 0.0, 0.0, 0.0};
        if constexpr (kC) aI[t] = mfma_d4{0.0, 0.0, 0.0, 0.0};
    }
    // left : D[i][j] = sum_k X(k, c_i) conj(U(k, rho_j)): i = column 16 ct + i, j = row 16 (t0 + t) + j
    // right: D[i][j] = sum_k U(k, rho_i) X(r_j, k):       i = output column rho, j = row 16 ct + j
    const int co = (16 * ct + li) * kUP;
#pragma unroll
    for (int q = 0; q < kKs; ++q) {     // rows k >= W of both LDS images are zero
        const int k = 4 * q + lk;
        double xr, xi = 0.0;
        if constexpr (kLeft) {
            xr = xr_s[co + k];
            if constexpr (kC) xi = xi_s[co + k];
        } else {
            const bool ok = rv && k < W;
            xr = ok ? re_of(xv[q]) : 0.0;
            if constexpr (kC) xi = ok ? im_of(xv[q]) : 0.0;
        }
        double ur[kT], ui[kC ? kT : 1];
#pragma unroll
        for (int t = 0; t < kT; ++t) {
            ur[t] = ur_s[k + (16 * (t0 + t) + li) * kUP];
            if constexpr (kC) ui[t] = ui_s[k + (16 * (t0 + t) + li) * kUP];
        }
#pragma unroll
        for (int t = 0; t < kT; ++t) {
            if constexpr (kLeft) {
                aR[t] = mfma(xr, ur[t], aR[t]);
                if constexpr (kC) {
                    aR[t] = mfma(xi, ui[t], aR[t]);
                    aI[t] = mfma(xi, ur[t], aI[t]);
                    aI[t] = mfma(-xr, ui[t], aI[t]);
                }
            } else {
                aR[t] = mfma(ur[t], xr, aR[t]);
                if constexpr (kC) {
                    aR[t] = mfma(-ui[t], xi, aR[t]);
                    aI[t] = mfma(ur[t], xi, aI[t]);
                    aI[t] = mfma(ui[t], xr, aI[t]);
                }
            }
        }
    }
#pragma unroll
    for (int t = 0; t < kT; ++t)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            S v;
            if constexpr (kC) v = cplx{aR[t][r], aI[t][r]};
            else v = aR[t][r];
            if constexpr (kLeft) {
                const int c = 16 * ct + lk + 4 * r, rho = 16 * (t0 + t) + li;
                if (c < cnt && rho < W) M[(s + rho) + (base + c) * ldm] = v;
            } else {
                const int rho = 16 * (t0 + t) + lk + 4 * r;
                if (rv && rho < W) M[(base + rj) + (int64_t)(s + rho) * ldm] = v;
            }
        }
}

// The sweeps' launches: workgroup blockIdx.x finds its window by blk0 and takes kTile columns (left) or
// rows (right) of its region.
template <class S, int kWin, bool kLeft, int kTile, int kMaxW>
__device__ __forceinline__ void window_update_batch(const WindowBatch<S, kMaxW>& b) {
    int g = 0;
#pragma unroll
    for (int q = 1; q < kMaxW; ++q)
        if (q < b.nw && (int)blockIdx.x >= b.w[q].blk0) g = q;
    const WindowRegion<S> w = b.w[g];
    const int64_t base = w.lo + (int64_t)((int)blockIdx.x - w.blk0) * kTile;
    const int cnt = (int)min<int64_t>(kTile, w.hi - base);
    window_update_tile<S, kWin, kLeft, kTile>(b.H, b.n, w.s, w.W, base, cnt, w.U, w.W);
}

}  // namespace dev
}  // namespace eigsol
