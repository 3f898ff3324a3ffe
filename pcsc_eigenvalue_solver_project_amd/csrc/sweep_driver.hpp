// The host skeleton shared by the real and complex multishift QR sweeps (francis.hip, zfrancis.hip; DESIGN.md
// §24): the chase descriptors, the deflation scan and the search for the active block, the chase loop over the
// rounds of chase_schedule.hpp with the delayed window updates after each round, and Schur mode's widened
// updates.  The two .hip files keep what differs per type and hand the launches over as a traits struct Tr:
//   S, kWin, kMaxGroups          scalar, window order and most windows per round (the chase kernel's)
//   kMaxRegions, kName           capacity of the update kernels' WindowBatch; prefix of the error messages
//   chase(st, nwin, batch)       launches the chase kernel, one workgroup per window
//   update<kLeft>(st, tile, grid, batch)   launches the window-update kernel, tile outputs per workgroup
//   update_tile(span, num_cus)   tile of a round's left and right batches: 64, or 32 where the type has it
#pragma once

#include <algorithm>
#include <cmath>
#include <string>

#include "chase_schedule.hpp"
#include "kernels_common.hpp"
#include "mfma_window.hpp"
#include "scratch.hpp"

namespace eigsol {
namespace dev {

// One window of a chase round: group g's bulges j = 0..nb-1 sit at rows k = l + t - 3 j for the
// group-local steps t in [t0, t1); the window [s, e) holds them for the whole round.
template <class S>
struct ChaseWin {
    int s, e;          // window [s, e)
    int t0, t1;        // group-local chase steps of this round
    int nb;            // bulges of the group
    const S* shifts;   // two values per bulge (real: xs (= ys) and ws of the shift pair; complex: s1, s2)
    S* U;              // out: (e - s)^2 accumulated factor, column-major
};
template <class S, int kMaxGroups>
struct ChaseBatch {    // one workgroup per window; the windows are disjoint
    S* H;
    int64_t n;         // leading dimension
    int l, ihi;        // active block
    ChaseWin<S> w[kMaxGroups];   // window of workgroup blockIdx.x
};

}  // namespace dev

// |a| of the deflation test: |Re a| + |Im a| (ZLAHQR's cabs1)
inline double abs1(double a) { return std::fabs(a); }
inline double abs1(const cplx& a) { return std::fabs(a.re) + std::fabs(a.im); }

// kSchur = false: the eigenvalue-only iteration.  kSchur = true: the same sweeps, shifts and launches of the chase,
// with every delayed update widened to the whole matrix (left regions to column n - 1, right regions from row 0),
// the window factors also applied to Z and accepted sub-diagonal entries stored as zeros.
template <class Tr, bool kSchur>
struct SweepDriver {
    using S = typename Tr::S;
    using Batch = dev::WindowBatch<S, Tr::kMaxRegions>;
    using Region = dev::WindowRegion<S>;
    static constexpr double eps = 2.220446049250313e-16;

    hipStream_t st;
    S *H, *Z;      // the matrix and the Schur vectors (null: none), n x n with leading dimension n
    int64_t n;
    int num_cus;
    DevBuf bds, bU;
    PinBuf bhs;
    S* ds = nullptr;    // pinned: the latest deflation scan, diagonal [0, n), subdiagonal [n, 2n) (device: bds)
    S* dU = nullptr;    // kMaxGroups window factors of kWin^2
    bool scanned = false;   // the previous sweep's closing scan is still current (nothing ran since)
    // `sweeps` tracks the largest number of sweeps any single deflation needed; stall: sweeps on the
    // current bottom block without a deflation
    int sweeps = 0, failed = 0, stall = 0;
    int st_windows = 0;
    long long st_steps = 0;

    int alloc() {
        EIGSOL_TRY(bds.alloc(2 * n * sizeof(S)));
        EIGSOL_TRY(bU.alloc((size_t)Tr::kMaxGroups * Tr::kWin * Tr::kWin * sizeof(S)));
        // every per-sweep transfer goes through pinned host memory: a pageable hipMemcpyAsync is staged by the
        // runtime and waited for with a sleeping wait, ~1 ms per copy (round-4 kernel trace of 4096^2: 1.12 s of
        // 2.8 s idle after such copies, tools/gap_analysis.py), more than a sweep's kernels at the iteration's end
        EIGSOL_TRY(bhs.alloc(2 * n * sizeof(S)));
        dU = bU.template as<S>();
        ds = bhs.template as<S>();
        return EIGSOL_OK;
    }
    static int error(int status, const char* what) { return fail(status, std::string(Tr::kName) + ": " + what); }

    void deflated() {
        sweeps = std::max(sweeps, stall);
        stall = 0;
    }
    // deflation scan of [0, ihi]: diagonal and subdiagonal into pinned host memory (only the
    // ihi + 1 leading entries of each half travel)
    int scan(int ihi) {
        S* const dds = bds.template as<S>();
        hipLaunchKernelGGL(dev::diag_sub_kernel<S>, dim3((ihi + 256) / 256), dim3(256), 0, st, H, n, ihi, dds);
        if (hipMemcpyAsync(ds, dds, (ihi + 1) * sizeof(S), hipMemcpyDeviceToHost, st) != hipSuccess ||
            hipMemcpyAsync(ds + n, dds + n, (ihi + 1) * sizeof(S), hipMemcpyDeviceToHost, st) != hipSuccess ||
            stream_wait(st) != hipSuccess)
            return error(EIGSOL_E_HIP, "deflation scan");
        return EIGSOL_OK;
    }
    bool negligible(int k) const { return abs1(ds[n + k]) <= eps * (abs1(ds[k - 1]) + abs1(ds[k])); }
    // the active block [*l, ihi] that ends at ihi, from a current scan
    int next_block(int ihi, int* l_out) {
        if (!scanned) EIGSOL_TRY(scan(ihi));
        scanned = false;
        int l = ihi;
        while (l > 0 && !negligible(l) && abs1(ds[n + l]) != 0.0) --l;
        if constexpr (kSchur) {   // the accepted sub-diagonal entry becomes an exact zero
            if (l > 0 && abs1(ds[n + l]) != 0.0)
                hipLaunchKernelGGL(dev::zero_entry_kernel<S>, dim3(1), dim3(1), 0, st, H, n, l, l - 1);
        }
        *l_out = l;
        return EIGSOL_OK;
    }
    // after a sweep on [l, ihi]: a deflation anywhere in the block resets the stall counter; the scan
    // also serves the next pass
    int close_sweep(int l, int ihi) {
        if (hipGetLastError() != hipSuccess) return error(EIGSOL_E_HIP, "launch");
        EIGSOL_TRY(scan(ihi));
        scanned = true;
        for (int k = ihi; k > l; --k)
            if (negligible(k)) {
                deflated();
                break;
            }
        return EIGSOL_OK;
    }
    // iterations reported: sweeps spent on the slowest deflation (>= 1, the final check), so that
    // iterations <= maxIterations exactly when the iteration converged
    void report(int32_t* sweeps_out, int32_t* fail_out) const {
        *sweeps_out = std::max(1, sweeps);
        *fail_out = failed;
    }

    template <bool kLeft>
    void update_one(S* M, int s, int W, int64_t lo, int64_t hi, const S* U) {
        Batch b{M, n, 1, {}};
        b.w[0] = Region{s, W, lo, hi, 0, U};
        Tr::template update<kLeft>(st, 64, (int)((hi - lo + 63) / 64), b);
    }
    // Schur mode: the factor U (W x W) of the rows / columns [s, s + W) applied outside them: U^H to the
    // columns [e, n), U to the rows [0, rhi) and to Z's columns
    void apply_outside(int s, int W, int64_t rhi, const S* U) {
        const int e = s + W;
        if (e < n) update_one<true>(H, s, W, e, n, U);
        if (rhi > 0) update_one<false>(H, s, W, 0, rhi, U);
        if (Z) update_one<false>(Z, s, W, 0, n, U);
    }
    // the factor V of an AED window [kw, kw + nw) of the active block [l, .] that deflated
    void apply_aed(int l, int kw, int nw, const S* V) {
        if constexpr (kSchur) {   // V on the columns right of the window, the rows above it and Z
            apply_outside(kw, nw, kw, V);
        } else if (kw > l) {   // rows of the block above the window: H[l, kw) x [kw, kw + nw) V
            update_one<false>(H, kw, nw, l, kw, V);
        }
    }
    // delayed updates of a round: every left region, then every right region (U_a^H X U_b = (U_a^H X) U_b); tiles
    // of 64 columns / rows per workgroup, or the type's narrower one.  Schur mode: right regions from row 0 (the
    // chase updated the window's own rows from max(l, s) on), and Z's columns [s, e) as one more right batch
    void launch_updates(const dev::ChaseWin<S>* wins, int nwin, int l, int ihi) {
        Batch lb{H, n, 0, {}}, rb{H, n, 0, {}}, zb{Z, n, 0, {}};
        const int lend = kSchur ? (int)n : ihi + 1;   // left regions: columns [e, lend)
        const int rlo = kSchur ? 0 : l;               // right regions: rows [rlo, rhi)
        auto rhi = [&](const dev::ChaseWin<S>& w) { return kSchur ? std::max(l, w.s) : w.s; };
        int nlb = 0, nrb = 0, nzb = 0, span = 0;
        for (int q = 0; q < nwin; ++q) {
            const dev::ChaseWin<S>& w = wins[q];
            if (w.e < lend) span += lend - w.e;
            if (rhi(w) > rlo) span += rhi(w) - rlo;
        }
        const int tile = Tr::update_tile(span, num_cus);
        for (int q = 0; q < nwin; ++q) {
            const dev::ChaseWin<S>& w = wins[q];
            const int W = w.e - w.s;
            if (w.e < lend) {
                lb.w[lb.nw++] = Region{w.s, W, (int64_t)w.e, (int64_t)lend, nlb, w.U};
                nlb += (lend - w.e + tile - 1) / tile;
            }
            if (rhi(w) > rlo) {
                rb.w[rb.nw++] = Region{w.s, W, (int64_t)rlo, (int64_t)rhi(w), nrb, w.U};
                nrb += (rhi(w) - rlo + tile - 1) / tile;
            }
            if (kSchur && Z) {
                zb.w[zb.nw++] = Region{w.s, W, 0, n, nzb, w.U};
                nzb += (int)((n + 63) / 64);
            }
        }
        if (nlb > 0) Tr::template update<true>(st, tile, nlb, lb);
        if (nrb > 0) Tr::template update<false>(st, tile, nrb, rb);
        if (nzb > 0) Tr::template update<false>(st, 64, nzb, zb);
    }

    // one sweep on [l, ihi]: p.C groups of p.nbg bulges (group g's shifts at dsh + 2 g nbg), each group in
    // its own LDS window; a round advances every started group's window by the same number of steps
    int run_chase(int l, int ihi, ChasePlan p, const S* dsh) {
        const ChaseGeometry geo{l, ihi, p.C, p.nbg, Tr::kWin};
        const int T = geo.T();
        ChaseRoundWin rw[Tr::kMaxGroups];
        for (int t0 = 0; t0 < T;) {
            int nwin = 0;
            const int t1 = chase_next_round(geo, t0, rw, &nwin);
            if (t1 == kChaseNoAdvance) return error(EIGSOL_E_SOLVER, "window did not advance (internal error)");
            if (t1 == kChaseOverlap) return error(EIGSOL_E_SOLVER, "windows overlap (internal error)");
            if (nwin > 0) {
                dev::ChaseBatch<S, Tr::kMaxGroups> cb{H, n, l, ihi, {}};
                for (int q = 0; q < nwin; ++q)
                    cb.w[q] = dev::ChaseWin<S>{rw[q].s, rw[q].e, rw[q].t0, rw[q].t1, p.nbg, dsh + 2 * rw[q].g * p.nbg,
                                               dU + (size_t)q * Tr::kWin * Tr::kWin};
                st_windows += nwin;
                st_steps += t1 - t0;
                Tr::chase(st, nwin, cb);
                launch_updates(cb.w, nwin, l, ihi);
            }
            t0 = t1;
        }
        return EIGSOL_OK;
    }
};

}  // namespace eigsol
