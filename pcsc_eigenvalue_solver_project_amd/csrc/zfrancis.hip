// Complex multishift QR sweeps (eigenvalues only) for std::complex<double> Hessenberg matrices.
//
// The reference's qr_eigenvalues_dense<std::complex<double>> (qr_eigenvalues.hpp:40-108) runs the
// unshifted iteration H <- R Q, which does not converge on general input (a complex N(0,1) matrix
// has eigenvalues of equal modulus).  This is the complex counterpart of francis.hip: the same
// small-bulge chase geometry, with complex arithmetic and shifts that need not come in conjugate
// pairs (LAPACK ZLAQR5's bulges):
//   * a bulge carries two shifts (s1, s2); its first column is (H - s1)(H - s2) e_l (scaled as in
//     ZLAQR1), and it is chased down by 3 x 3 complex Householder reflectors Q = I - tau v v^H
//     (ZLARFG's convention: Q^H (alpha, x) = (beta, 0) with beta real), the last step by a 2 x 2;
//   * bulges sit 3 rows apart and move together: every bulge's left update (Q^H on rows k..k+2)
//     runs before any right update (Q on columns k..k+2), which touch disjoint words within a
//     phase, and associativity makes the simultaneous step the product of the sequential ones;
//   * the chain is chased inside an LDS window [s, e) of at most 64 rows/columns (complex: H and
//     its accumulated unitary U take 2 x 64 KiB of LDS), one wave per bulge; the window's updates
//     outside it are applied afterwards as complex GEMMs over the columns right of the window
//     (U^H X) and the rows above it (X U), on the fp64 matrix cores (window_update_tile of
//     mfma_window.hpp, the tile francis.hip and ordschur.hip use too);
//   * shifts: eigenvalues of the trailing 2 nb x 2 nb block; every 6th sweep without a deflation
//     uses exceptional shifts; active blocks of at most 64 rows are finished in LDS by a one-wave
//     single-shift QR (the ZLAHQR iteration: Wilkinson shift, exceptional shifts at iterations 10
//     and 20, Ahues-Tisseur deflation test).
// Deflation: |h(k,k-1)| <= eps (|h(k,k)| + |h(k-1,k-1)|) with |z| = |Re z| + |Im z| (ZLAHQR's cabs1).
#include <algorithm>
#include <cstdio>
#include <cstdlib>

#include "sweep_driver.hpp"

namespace eigsol {
namespace dev {

constexpr int kZWin = 64;         // window rows/columns
constexpr int kZSmall = 64;       // blocks finished by the one-wave solver
constexpr int kZMaxBulges = 32;   // per sweep (shifts from a <= 64 block); per window <= 16, one wave each
constexpr int kZMaxGroups = 4;    // bulge chains chased concurrently, one window (workgroup) each

__device__ __forceinline__ cplx cconj(cplx a) { return cplx{a.re, -a.im}; }
__device__ __forceinline__ double cabs1(cplx a) { return fabs(a.re) + fabs(a.im); }
__device__ __forceinline__ cplx cscale(cplx a, double s) { return cplx{a.re * s, a.im * s}; }
__device__ __forceinline__ cplx cmul_conj(cplx a, cplx b) {   // conj(a) * b
    return cplx{a.re * b.re + a.im * b.im, a.re * b.im - a.im * b.re};
}
__device__ __forceinline__ cplx csqrt_(cplx z) {
    const double r = hypot(z.re, z.im);
    if (r == 0.0) return cplx{0.0, 0.0};
    const double t = sqrt(0.5 * (r + fabs(z.re)));
    return z.re >= 0.0 ? cplx{t, z.im / (2.0 * t)} : cplx{fabs(z.im) / (2.0 * t), copysign(t, z.im)};
}
// robust quotient (Smith's algorithm)
__device__ __forceinline__ cplx cdiv_s(cplx a, cplx b) {
    if (fabs(b.re) >= fabs(b.im)) {
        const double r = b.im / b.re, d = b.re + b.im * r;
        return cplx{(a.re + a.im * r) / d, (a.im - a.re * r) / d};
    }
    const double r = b.re / b.im, d = b.re * r + b.im;
    return cplx{(a.re * r + a.im) / d, (a.im * r - a.re) / d};
}

// ZLARFG on (alpha, x1, x2) (x2 ignored when !three): Q = I - tau v v^H, v = (1, v1, v2),
// Q^H (alpha, x1, x2) = (beta, 0, 0).  tau = 0 (Q = I) when x = 0 and alpha is real.  The caller
// scales the input to O(1).
__device__ __forceinline__ void zhouse(cplx a, cplx x1, cplx x2, bool three, double& beta, cplx& tau, cplx& v1,
                                       cplx& v2) {
    const double xn2 = sq_abs(x1) + (three ? sq_abs(x2) : 0.0);
    if (xn2 == 0.0 && a.im == 0.0) {
        beta = a.re;
        tau = cplx{0.0, 0.0};
        v1 = v2 = cplx{0.0, 0.0};
        return;
    }
    const double an = sqrt(a.re * a.re + a.im * a.im + xn2);
    beta = a.re >= 0.0 ? -an : an;
    // the step's serial chain: reciprocals (v_rcp_f64 + two Newton steps, within an ulp or two)
    // instead of IEEE divisions; x / d by Smith's scaling with one reciprocal of the denominator
    const double ib = rcp_nr(beta);
    tau = cplx{(beta - a.re) * ib, -a.im * ib};
    const cplx d = cplx{a.re - beta, a.im};   // |d| >= |beta| > 0
    const bool re_big = fabs(d.re) >= fabs(d.im);
    const double r = re_big ? d.im * rcp_nr(d.re) : d.re * rcp_nr(d.im);
    const double id = rcp_nr(re_big ? __builtin_fma(d.im, r, d.re) : __builtin_fma(d.re, r, d.im));
    auto qt = [&](cplx x) -> cplx {
        return re_big ? cplx{__builtin_fma(x.im, r, x.re) * id, __builtin_fma(-x.re, r, x.im) * id}
                      : cplx{__builtin_fma(x.re, r, x.im) * id, __builtin_fma(x.im, r, -x.re) * id};
    };
    v1 = qt(x1);
    v2 = three ? qt(x2) : cplx{0.0, 0.0};
}

// zhouse for the 2 x 2 reflectors of the one-wave QR, on any scale: (alpha, x1) is scaled by a power
// of two (exact) so that its largest component lies in [1/2, 1), which puts the norm's square in
// [1/4, 4] and lets the hardware square root seed replace the IEEE sequence; tau and v are
// scale-free, beta is scaled back.  The same reflector as zhouse up to the rounding of the square
// root and reciprocals.
__device__ __forceinline__ void zhouse2_scaled(cplx a, cplx x1, double& beta, cplx& tau, cplx& v1) {
    const double m = fmax(fmax(fabs(a.re), fabs(a.im)), fmax(fabs(x1.re), fabs(x1.im)));
    const int ex = m > 0.0 ? __builtin_amdgcn_frexp_exp(m) : 0;
    const cplx as{__builtin_amdgcn_ldexp(a.re, -ex), __builtin_amdgcn_ldexp(a.im, -ex)};
    const cplx xs{__builtin_amdgcn_ldexp(x1.re, -ex), __builtin_amdgcn_ldexp(x1.im, -ex)};
    const double xn2 = sq_abs(xs);
    if (xn2 == 0.0 && as.im == 0.0) {
        beta = a.re;
        tau = cplx{0.0, 0.0};
        v1 = cplx{0.0, 0.0};
        return;
    }
    const double an = sqrt_nr(__builtin_fma(as.re, as.re, __builtin_fma(as.im, as.im, xn2)));
    const double bs = as.re >= 0.0 ? -an : an;
    const double ib = rcp_nr(bs);
    tau = cplx{(bs - as.re) * ib, -as.im * ib};
    const cplx d = cplx{as.re - bs, as.im};   // |d| >= |bs| > 0
    const bool re_big = fabs(d.re) >= fabs(d.im);
    const double r = re_big ? d.im * rcp_nr(d.re) : d.re * rcp_nr(d.im);
    const double id = rcp_nr(re_big ? __builtin_fma(d.im, r, d.re) : __builtin_fma(d.re, r, d.im));
    v1 = re_big ? cplx{__builtin_fma(xs.im, r, xs.re) * id, __builtin_fma(-xs.re, r, xs.im) * id}
                : cplx{__builtin_fma(xs.re, r, xs.im) * id, __builtin_fma(xs.im, r, -xs.re) * id};
    beta = __builtin_amdgcn_ldexp(bs, ex);
}

// ---------------------------------------------------------------- one-wave single-shift QR (n <= 64)
// Eigenvalues of an n x n Hessenberg block (ZLAHQR without Schur vectors; updates confined to the
// active block).  info[0] = 1 if some eigenvalue needed more than 30 max(10, n) iterations,
// info[1] = most iterations any eigenvalue took.
// One wave, so no barriers: a wave's LDS operations complete in program order, and the compiler
// fence keeps the program order.
#define EIGSOL_ZWAVE_ORDER() asm volatile("" ::: "memory")
// kSchur = false: eigenvalues only, updates confined to the active block (ZLAHQR with WANTT =
// WANTZ = false).  kSchur = true: the full Schur form T = V^H H V of the n x n block (left updates
// to column n-1, right updates from row 0, V accumulated: WANTT = WANTZ = true), for the AED.
// w[i] = the eigenvalue deflated at row i; failed / maxits / steps as for the kernel below.
// AED early stop (kSchur, spk >= 0 = cabs1 of the window's spike): when an eigenvalue deflates at
// the bottom row i its Schur vector column V(:, i) is final (later sweeps touch columns < i only),
// so the AED spike test is taken right there; the first eigenvalue that fails it ends the
// factorisation (stop = i; the rows above stay unreduced).  stop = -1: ran to completion.
// dtol: relative subdiagonal at which the block splits (ulp: ZLAHQR's test; the sweeps' shifts are
// could be computed with a looser one)
template <bool kSchur>
__device__ void zwave_hqr(cplx* h, cplx* v, int n, cplx* w, int& failed, int& maxits, int& steps,
                          double spk = -1.0, int* stop = nullptr, double dtol = 2.220446049250313e-16) {
    constexpr int lh = kZSmall + 1;
    const int ln = threadIdx.x;
    auto H = [&](int i, int j) -> cplx& { return h[i + j * lh]; };
    auto V = [&](int i, int j) -> cplx& { return v[i + j * lh]; };
    const double ulp = 2.220446049250313e-16, smlnum = 2.2250738585072014e-308 * ((double)n / ulp);
    const int itmax = 30 * max(10, n);
    int i = n - 1;
    failed = 0;
    maxits = 0;
    steps = 0;
    while (i >= 0) {
        int l = 0, its = 0;
        for (; its <= itmax; ++its) {
            // the largest k in (l, i] with a negligible subdiagonal (l if none): the serial downward
            // scan's answer, one k per lane, then a wave max
            int kf = l;
            for (int k = i - ln; k > l; k -= 64) {
                const cplx hk = H(k, k - 1);
                bool neg = cabs1(hk) <= smlnum;
                if (!neg) {
                    double tst = cabs1(H(k - 1, k - 1)) + cabs1(H(k, k));
                    if (tst == 0.0) {
                        if (k - 2 >= l) tst += fabs(H(k - 1, k - 2).re);
                        if (k + 1 <= i) tst += fabs(H(k + 1, k).re);
                    }
                    if (cabs1(hk) <= dtol * tst) {
                        const double ab = fmax(cabs1(hk), cabs1(H(k - 1, k))), ba = fmin(cabs1(hk), cabs1(H(k - 1, k)));
                        const cplx dd = sub(H(k - 1, k - 1), H(k, k));
                        const double aa = fmax(cabs1(H(k, k)), cabs1(dd)), bb = fmin(cabs1(H(k, k)), cabs1(dd));
                        const double s = aa + ab;
                        neg = ba * (ab / s) <= fmax(smlnum, dtol * (bb * (aa / s)));
                    }
                }
                if (neg) { kf = k; break; }
            }
#pragma unroll
            for (int off = 32; off > 0; off >>= 1) kf = max(kf, __shfl_xor(kf, off, 64));
            l = __builtin_amdgcn_readfirstlane(kf);
            EIGSOL_ZWAVE_ORDER();
            if (l > 0 && ln == 0) H(l, l - 1) = cplx{0.0, 0.0};
            EIGSOL_ZWAVE_ORDER();
            if (l >= i) break;
            // shift
            cplx t;
            if (its == 10) {
                t = add(cplx{0.75 * fabs(H(l + 1, l).re), 0.0}, H(l, l));
            } else if (its == 20) {
                t = add(cplx{0.75 * fabs(H(i, i - 1).re), 0.0}, H(i, i));
            } else {
                t = H(i, i);
                const cplx u = mul(csqrt_(H(i - 1, i)), csqrt_(H(i, i - 1)));
                double s = cabs1(u);
                if (s != 0.0) {
                    const cplx x = cscale(sub(H(i - 1, i - 1), t), 0.5);
                    const double sx = cabs1(x);
                    s = fmax(s, sx);
                    const cplx xs = cscale(x, 1.0 / s), us = cscale(u, 1.0 / s);
                    cplx y = cscale(csqrt_(add(mul(xs, xs), mul(us, us))), s);
                    if (sx > 0.0) {
                        const cplx xn = cscale(x, 1.0 / sx);
                        if (xn.re * y.re + xn.im * y.im < 0.0) y = cplx{-y.re, -y.im};
                    }
                    t = sub(t, mul(u, cdiv_s(u, add(x, y))));
                }
            }
            // single-shift sweep from l
            steps += i - l;
            for (int kk = l; kk < i; ++kk) {
                // the left update's rows kk, kk+1 (columns >= kk: this step's own stores go to
                // column kk-1) and V's columns kk, kk+1 are loaded first, so their LDS latency
                // overlaps the reflector's chain; the reflector is zhouse2_scaled's.  (Round 5's step
                // loaded them where they are used and took zhouse's reflector; removed.)
                const int c = kk + ln;
                const bool cl = c <= (kSchur ? n - 1 : i);
                cplx a0{0.0, 0.0}, a1{0.0, 0.0}, w0{0.0, 0.0}, w1{0.0, 0.0};
                if (cl) { a0 = H(kk, c); a1 = H(kk + 1, c); }
                if (kSchur && ln < n) { w0 = V(ln, kk); w1 = V(ln, kk + 1); }
                cplx v0, v1;
                if (kk == l) {
                    const cplx h11s = sub(H(l, l), t);
                    const cplx h21 = H(l + 1, l);
                    const double s = cabs1(h11s) + cabs1(h21);
                    v0 = s > 0.0 ? cscale(h11s, 1.0 / s) : h11s;
                    v1 = s > 0.0 ? cscale(h21, 1.0 / s) : h21;
                } else {
                    v0 = H(kk, kk - 1);
                    v1 = H(kk + 1, kk - 1);
                }
                double beta;
                cplx tau, vv;
                zhouse2_scaled(v0, v1, beta, tau, vv);
                EIGSOL_ZWAVE_ORDER();
                if (kk > l && ln == 0) {
                    H(kk, kk - 1) = cplx{beta, 0.0};
                    H(kk + 1, kk - 1) = cplx{0.0, 0.0};
                }
                const cplx ct = cconj(tau);
                {   // left: rows kk, kk+1, columns kk..i (Schur: ..n-1)
                    if (cl) {
                        const cplx s = mul(ct, add(a0, cmul_conj(vv, a1)));
                        H(kk, c) = sub(a0, s);
                        H(kk + 1, c) = sub(a1, mul(s, vv));
                    }
                }
                EIGSOL_ZWAVE_ORDER();
                {   // right: columns kk, kk+1, rows l..min(kk+2, i) (Schur: from row 0; and V)
                    const int r = (kSchur ? 0 : l) + ln;
                    if (r <= min(kk + 2, i)) {
                        const cplx b0 = H(r, kk), b1 = H(r, kk + 1);
                        const cplx s = mul(tau, add(b0, mul(b1, vv)));
                        H(r, kk) = sub(b0, s);
                        H(r, kk + 1) = sub(b1, mul(s, cconj(vv)));
                    }
                    if (kSchur && ln < n) {
                        const cplx s = mul(tau, add(w0, mul(w1, vv)));
                        V(ln, kk) = sub(w0, s);
                        V(ln, kk + 1) = sub(w1, mul(s, cconj(vv)));
                    }
                }
                EIGSOL_ZWAVE_ORDER();
            }
        }
        if (its > itmax) {
            failed = 1;
            break;
        }
        maxits = max(maxits, its);
        // H(l..i) has deflated to a single eigenvalue at i (l == i)
        if (ln == 0) w[i] = H(i, i);
        if (kSchur && spk >= 0.0) {
            double foo = cabs1(H(i, i));
            if (foo == 0.0) foo = spk;
            if (spk * cabs1(V(0, i)) > fmax(smlnum, ulp * foo)) {
                *stop = i;
                return;
            }
        }
        i = l - 1;
    }
    if (stop) *stop = -1;
    if (failed) {
        for (int r = ln; r <= i; r += 64) w[r] = H(r, r);   // best effort, flagged as failed
    }
}

// Eigenvalues of an n x n Hessenberg block (n <= 64) in LDS.
__global__ __launch_bounds__(64) void zhqr_wave_kernel(const cplx* Hin, int64_t ld, int n, cplx* w, int* info,
                                                       double dtol) {
    __shared__ cplx h[kZSmall * (kZSmall + 1)];
    constexpr int lh = kZSmall + 1;
    const int ln = threadIdx.x;
    for (int idx = ln; idx < n * n; idx += 64) h[(idx % n) + (idx / n) * lh] = Hin[(idx % n) + (int64_t)(idx / n) * ld];
    __syncthreads();
    int failed, maxits, steps;
    zwave_hqr<false>(h, nullptr, n, w, failed, maxits, steps, -1.0, nullptr, dtol);
    if (ln == 0) {
        info[0] = failed;
        info[1] = maxits;
    }
}

// ---------------------------------------------------------------- complex aggressive early deflation
// (ZLAQR3's idea, restated for one wave, as francis.hip's aed_kernel is for the real case.)  The
// trailing nw x nw window T = H[kw:kw+nw, kw:kw+nw] of the active block is brought to complex
// Schur form T = V S V^H (zwave_hqr<true>).  The window is coupled to the rest of the block only
// through the spike s = H(kw, kw-1), which the similarity turns into the column s conj(V(0, :))^T;
// trailing eigenvalues whose spike entry is negligible (cabs1(s) cabs1(V(0, j)) <=
// max(smlnum, ulp cabs1(S(j, j))), ZLAQR3's test; no reordering) deflate outright, scanning from
// the bottom to the first that does not.  When some deflate, the undeflated top part with its
// spike is reduced back to Hessenberg form by complex Householder reflectors (ZLARFG convention,
// accumulated into V), the window and the new spike are written back, and the caller applies V to
// the rows of the block above the window (H[l:kw, kw:kw+nw] V).  w[kw + i] = S(i, i): the
// deflated eigenvalues are final.  The factorisation stops at the first eigenvalue that does not
// deflate (zwave_hqr's early stop), so the next sweep's shifts come from the trailing block.
// info = {fail, deflated, iterations, undeflated, steps}.
struct ZAedCtl {
    cplx tau, spike;
    double beta;
    int fail, maxsw, steps, nd;
};
// 256 threads: wave 0 runs the one-wave Schur factorisation, the spike test and the Householder
// vectors; the reflector applications of the back-reduction take four lanes per row / column (each
// sums every fourth term, the four partial sums meet as (s0 + s1) + (s2 + s3)).  Round 4: the
// one-wave version summed each dot product in one chain.
constexpr int kZAedThreads = 256;
__device__ __forceinline__ cplx quad_sum(cplx sq, int q) {   // (s0 + s1) + (s2 + s3) over the 4-lane group
    const cplx o1{__shfl_xor(sq.re, 1, 64), __shfl_xor(sq.im, 1, 64)};
    const cplx pr = (q & 1) ? add(o1, sq) : add(sq, o1);
    const cplx o2{__shfl_xor(pr.re, 2, 64), __shfl_xor(pr.im, 2, 64)};
    return (q & 2) ? add(o2, pr) : add(pr, o2);
}
// Concurrent shifts (round 5, as francis.hip's ShiftJob: a second workgroup of the launch solving
// the pre-AED trailing block for the next sweep's shifts) were measured and removed: a launch ends
// with its slower workgroup, and the 64 x 64 complex shift QR (~2.5 ms) outlasts the AED (~1 ms),
// so every AED - also the 70 % after which the sweep is skipped - waited for it: 4096^2 1.569 s ->
// 2.285 s (used only when the AED deflates nothing: same 122 sweeps, bitwise the same eigenvalues),
// 2.085 s (also after a deflation, 131 sweeps).
__global__ __launch_bounds__(kZAedThreads) void zaed_kernel(cplx* Hg, int64_t n, int kw, int nw, int spike_valid,
                                                            cplx* w, cplx* Vout, int* info) {
    constexpr int lh = kZSmall + 1;
    constexpr int NT = kZAedThreads;
    __shared__ cplx t[kZSmall * lh];
    __shared__ cplx v[kZSmall * lh];
    __shared__ cplx hv[kZSmall];
    __shared__ cplx sp[kZSmall];
    __shared__ ZAedCtl c;
    const int tid = threadIdx.x, ln = tid & 63, wv0 = tid < 64;
    const int grp = tid >> 2, q = tid & 3;   // 64 groups of four lanes
    auto T = [&](int i, int j) -> cplx& { return t[i + j * lh]; };
    auto V = [&](int i, int j) -> cplx& { return v[i + j * lh]; };
    for (int e = tid; e < nw * nw; e += NT) {
        const int i = e % nw, j = e / nw;
        T(i, j) = Hg[(kw + i) + (int64_t)(kw + j) * n];
        V(i, j) = i == j ? cplx{1.0, 0.0} : cplx{0.0, 0.0};
    }
    const cplx spike = (spike_valid && kw > 0) ? Hg[kw + (int64_t)(kw - 1) * n] : cplx{0.0, 0.0};
    __syncthreads();
    if (wv0) {
        int fail, maxsw, steps, stop = -1;
        zwave_hqr<true>(t, v, nw, w + kw, fail, maxsw, steps, cabs1(spike), &stop);
        // deflated = the trailing run of negligible spike entries (the spike test ran inside the
        // factorisation, which stopped at the first eigenvalue that failed it)
        const int nd = fail ? 0 : nw - 1 - stop;
        if (ln == 0) {
            c.fail = fail;
            c.maxsw = maxsw;
            c.steps = steps;
            c.nd = nd;
        }
    }
    __syncthreads();
    const int nd = c.nd;
    const int m = nw - nd;
    // undeflated part + spike back to Hessenberg form.  Q = I - tau hv hv^H (hv[0] = 1) applied
    // as Q^H T on rows [o, o + len) (columns [jlo, nw)), then T Q on T's rows [0, m) and V Q
    auto reflect = [&](int o, int len, int jlo) {
        const cplx tau = c.tau, ctau = cconj(tau);
        for (int j = jlo + grp; j < nw; j += NT / 4) {
            cplx sq{0.0, 0.0};
            for (int i = q; i < len; i += 4) sq = add(sq, cmul_conj(hv[i], T(o + i, j)));
            const cplx wv = mul(ctau, quad_sum(sq, q));
            for (int i = q; i < len; i += 4) T(o + i, j) = sub(T(o + i, j), mul(hv[i], wv));
        }
        __syncthreads();
        if (grp < nw) {
            cplx sq{0.0, 0.0};
            for (int jj = q; jj < len; jj += 4) sq = add(sq, mul(V(grp, o + jj), hv[jj]));
            const cplx wv = mul(tau, quad_sum(sq, q));
            for (int jj = q; jj < len; jj += 4) V(grp, o + jj) = sub(V(grp, o + jj), mul(wv, cconj(hv[jj])));
        }
        if (grp < m) {
            cplx sq{0.0, 0.0};
            for (int jj = q; jj < len; jj += 4) sq = add(sq, mul(T(grp, o + jj), hv[jj]));
            const cplx wv = mul(tau, quad_sum(sq, q));
            for (int jj = q; jj < len; jj += 4) T(grp, o + jj) = sub(T(grp, o + jj), mul(wv, cconj(hv[jj])));
        }
        __syncthreads();
    };
    // ZLARFG of x[0..len) by wave 0: hv, c.tau (0: Q = I), c.beta (real); every thread calls it
    auto house = [&](const cplx* x, int len) {
        cplx tau{0.0, 0.0}, sc{0.0, 0.0};
        double beta = 0.0;
        if (wv0) {
            const cplx alpha = x[0];
            double part = 0.0;
            for (int i = 1 + ln; i < len; i += 64) part += sq_abs(x[i]);
            const double xn2 = wave_sum(part);
            beta = alpha.re;
            if (xn2 != 0.0 || alpha.im != 0.0) {
                beta = -copysign(sqrt(sq_abs(alpha) + xn2), alpha.re);
                tau = cplx{(beta - alpha.re) / beta, -alpha.im / beta};
                sc = cdiv_s(cplx{1.0, 0.0}, cplx{alpha.re - beta, alpha.im});
            }
        }
        __syncthreads();   // x may alias a T column the stores below do not touch; order the reads
        if (wv0) {
            for (int i = 1 + ln; i < len; i += 64) hv[i] = mul(x[i], sc);
            if (ln == 0) {
                hv[0] = cplx{1.0, 0.0};
                c.tau = tau;
                c.beta = beta;
            }
        }
        __syncthreads();
    };
    if (nd > 0 && m > 0) {
        for (int i = tid; i < m; i += NT) sp[i] = mul(spike, cconj(V(0, i)));
        __syncthreads();
        if (m > 1) {
            house(sp, m);
            if (tid == 0) c.spike = cplx{c.beta, 0.0};
            __syncthreads();
            if (c.tau.re != 0.0 || c.tau.im != 0.0) reflect(0, m, 0);
        } else {
            if (tid == 0) c.spike = sp[0];
            __syncthreads();
        }
        for (int col = 0; col + 2 < m; ++col) {
            house(&T(col + 1, col), m - col - 1);
            if (tid == 0) T(col + 1, col) = cplx{c.beta, 0.0};
            for (int i = col + 2 + tid; i < m; i += NT) T(i, col) = cplx{0.0, 0.0};
            __syncthreads();
            if (c.tau.re != 0.0 || c.tau.im != 0.0) reflect(col + 1, m - col - 1, col + 1);
        }
    } else if (tid == 0) {
        c.spike = cplx{0.0, 0.0};
    }
    __syncthreads();
    if (nd > 0) {
        for (int e = tid; e < nw * nw; e += NT) {
            const int i = e % nw, j = e / nw;
            Hg[(kw + i) + (int64_t)(kw + j) * n] = i > j + 1 ? cplx{0.0, 0.0} : T(i, j);
            Vout[e] = V(i, j);
        }
        if (tid == 0 && spike_valid && kw > 0) Hg[kw + (int64_t)(kw - 1) * n] = c.spike;
    }
    if (tid == 0) {
        info[0] = c.fail;
        info[1] = nd;
        info[2] = c.maxsw;
        info[3] = m;
        info[4] = c.steps;
    }
}

// ---------------------------------------------------------------- windowed multishift chase
__global__ __launch_bounds__(1024) void zchase_kernel(ChaseBatch<cplx, kZMaxGroups> b) {
    const ChaseWin<cplx> a = b.w[blockIdx.x];
    __shared__ cplx h[kZWin * (kZWin + 1)];
    __shared__ cplx u[kZWin * kZWin];
    constexpr int lh = kZWin + 1, lu = kZWin;
    const int W = a.e - a.s;
    const int tid = threadIdx.x;
    auto Hw = [&](int i, int j) -> cplx& { return h[(i - a.s) + (j - a.s) * lh]; };
    for (int idx = tid; idx < W * W; idx += 1024) {
        const int i = idx % W, j = idx / W;
        h[i + j * lh] = b.H[(a.s + i) + (int64_t)(a.s + j) * b.n];
        u[i + j * lu] = (i == j) ? cplx{1.0, 0.0} : cplx{0.0, 0.0};
    }
    __syncthreads();
    const int l = b.l, ihi = b.ihi;
    const int wv = tid >> 6, ln = tid & 63;
    const int rlo = max(l, a.s);
    for (int t = a.t0; t < a.t1; ++t) {
        const int k = l + t - 3 * wv;
        const bool live = wv < a.nb && k >= l && k <= ihi - 1;
        const bool three = k != ihi - 1;
        double beta = 0.0;
        cplx tau{0.0, 0.0}, v1{0.0, 0.0}, v2{0.0, 0.0};
        bool act = false;
        if (live) {
            cplx p, q, r;
            int ex = 0;
            if (k == l) {
                const cplx s1 = a.shifts[2 * wv], s2 = a.shifts[2 * wv + 1];
                const cplx h11 = Hw(l, l), h21 = Hw(l + 1, l), h12 = Hw(l, l + 1), h22 = Hw(l + 1, l + 1);
                const double s = cabs1(sub(h11, s2)) + cabs1(h21);
                if (s == 0.0) {
                    p = q = r = cplx{0.0, 0.0};
                } else {
                    const cplx h21s = cscale(h21, 1.0 / s);
                    p = add(mul(h21s, h12), mul(sub(h11, s1), cscale(sub(h11, s2), 1.0 / s)));
                    q = mul(h21s, sub(add(h11, h22), add(s1, s2)));
                    r = three ? mul(h21s, Hw(l + 2, l + 1)) : cplx{0.0, 0.0};
                }
            } else {
                p = Hw(k, k - 1);
                q = Hw(k + 1, k - 1);
                r = three ? Hw(k + 2, k - 1) : cplx{0.0, 0.0};
            }
            const double mx = fmax(fmax(cabs1(p), cabs1(q)), cabs1(r));
            if (mx > 0.0) {
                ex = __builtin_amdgcn_frexp_exp(mx);   // exact power-of-two scaling into [1/2, 1)
                p = cplx{ldexp(p.re, -ex), ldexp(p.im, -ex)};
                q = cplx{ldexp(q.re, -ex), ldexp(q.im, -ex)};
                r = cplx{ldexp(r.re, -ex), ldexp(r.im, -ex)};
                zhouse(p, q, r, three, beta, tau, v1, v2);
                act = true;
                if (k != l && ln == 0) {
                    Hw(k, k - 1) = cplx{ldexp(beta, ex), 0.0};
                    Hw(k + 1, k - 1) = cplx{0.0, 0.0};
                    if (three) Hw(k + 2, k - 1) = cplx{0.0, 0.0};
                }
                const cplx ct = cconj(tau);
                // phase A: left update (Q^H on rows k..k+2), columns [k, e)
                const int c = k + ln;
                if (c < a.e) {
                    const cplx x0 = Hw(k, c), x1 = Hw(k + 1, c);
                    const cplx x2 = three ? Hw(k + 2, c) : cplx{0.0, 0.0};
                    cplx wsum = add(x0, cmul_conj(v1, x1));
                    if (three) wsum = add(wsum, cmul_conj(v2, x2));
                    const cplx s = mul(ct, wsum);
                    Hw(k, c) = sub(x0, s);
                    Hw(k + 1, c) = sub(x1, mul(s, v1));
                    if (three) Hw(k + 2, c) = sub(x2, mul(s, v2));
                }
                // U <- U Q on columns k..k+2 (window-relative), every row
                if (ln < W) {
                    const int kk = k - a.s;
                    const cplx y0 = u[ln + kk * lu], y1 = u[ln + (kk + 1) * lu];
                    const cplx y2 = three ? u[ln + (kk + 2) * lu] : cplx{0.0, 0.0};
                    cplx wsum = add(y0, mul(y1, v1));
                    if (three) wsum = add(wsum, mul(y2, v2));
                    const cplx s = mul(tau, wsum);
                    u[ln + kk * lu] = sub(y0, s);
                    u[ln + (kk + 1) * lu] = sub(y1, mul(s, cconj(v1)));
                    if (three) u[ln + (kk + 2) * lu] = sub(y2, mul(s, cconj(v2)));
                }
            }
        }
        __syncthreads();
        if (act) {   // phase B: right update (Q on columns k..k+2), rows [rlo, min(k + 3, ihi)]
            const int r = rlo + ln;
            if (r <= min(k + 3, ihi)) {
                const cplx y0 = Hw(r, k), y1 = Hw(r, k + 1);
                const cplx y2 = three ? Hw(r, k + 2) : cplx{0.0, 0.0};
                cplx wsum = add(y0, mul(y1, v1));
                if (three) wsum = add(wsum, mul(y2, v2));
                const cplx s = mul(tau, wsum);
                Hw(r, k) = sub(y0, s);
                Hw(r, k + 1) = sub(y1, mul(s, cconj(v1)));
                if (three) Hw(r, k + 2) = sub(y2, mul(s, cconj(v2)));
            }
        }
        __syncthreads();
    }
    for (int idx = tid; idx < W * W; idx += 1024) {
        const int i = idx % W, j = idx / W;
        b.H[(a.s + i) + (int64_t)(a.s + j) * b.n] = h[i + j * lh];
        a.U[idx] = u[i + j * lu];
    }
}

// Delayed window updates on the fp64 matrix cores (mfma_window.hpp; the VALU kernel that preceded it,
// 8 output columns per 128-thread workgroup, was removed).  left: H(s:s+W, cols) <- U^H H(s:s+W, cols)
// for the columns [lo, hi); right: H(rows, s:s+W) <- H(rows, s:s+W) U for the rows [lo, hi); 64
// columns / rows per workgroup of 4 waves.
using ZWinGemmBatch = WindowBatch<cplx, kZMaxGroups>;
constexpr int kZMG = 64;   // outputs per workgroup
constexpr int kZMT = 4 * kZMG;   // threads: one wave per 16 outputs
template <bool kLeft>
__global__ __launch_bounds__(kZMT) void zwin_gemm_mfma(ZWinGemmBatch bt) {
    window_update_batch<cplx, kZWin, kLeft, kZMG>(bt);
}

// Schur mode: the diagonal block H[l:l+m, l:l+m] (m <= kZSmall) finished in one piece: complex Schur form
// T = V^H H V by the one-wave factorisation with V kept.  T goes back in place (exact zeros below the
// diagonal once it converged, below the sub-diagonal otherwise), V to Vout (m x m, column-major); the
// caller applies V to the columns right of the block, the rows above it and Z.  info = {fail, most sweeps}.
__global__ __launch_bounds__(kZAedThreads) void zschur_block_kernel(cplx* Hg, int64_t n, int l, int m, cplx* w,
                                                                    cplx* Vout, int* info) {
    constexpr int lh = kZSmall + 1;
    constexpr int NT = kZAedThreads;
    __shared__ cplx t[kZSmall * lh];
    __shared__ cplx v[kZSmall * lh];
    __shared__ int sfail;
    const int tid = threadIdx.x;
    for (int e = tid; e < m * m; e += NT) {
        const int i = e % m, j = e / m;
        t[i + j * lh] = Hg[(l + i) + (int64_t)(l + j) * n];
        v[i + j * lh] = i == j ? cplx{1.0, 0.0} : cplx{0.0, 0.0};
    }
    __syncthreads();
    if (tid < 64) {
        int fail, maxsw, steps;
        zwave_hqr<true>(t, v, m, w, fail, maxsw, steps);
        if (tid == 0) {
            sfail = fail;
            info[0] = fail;
            info[1] = maxsw;
        }
    }
    __syncthreads();
    const int below = sfail ? 1 : 0;   // converged: triangular, the accepted sub-diagonal entries exact zeros
    for (int e = tid; e < m * m; e += NT) {
        const int i = e % m, j = e / m;
        Hg[(l + i) + (int64_t)(l + j) * n] = i > j + below ? cplx{0.0, 0.0} : t[i + j * lh];
        Vout[e] = v[i + j * lh];
    }
}

}  // namespace dev

// AED window.  Early-stop AED, 32 bulges in 4 chains: window
// 32 / 48 / 64 at 1024^2 0.292 / 0.287 / 0.320 s; 48 vs 64 at 4096^2 2.65 / 2.75 s.  Without the
// AED: 1024^2 0.37-0.42 s, 4096^2 4.4 s; an AED over the window's whole Schur form (LAPACK's, the
// undeflated eigenvalues becoming the shifts) 0.54 / 4.4 s.  Both were removed.
static constexpr int kZAedWin = 48;

// the complex sweeps' side of sweep_driver.hpp
struct ComplexSweep {
    using S = cplx;
    static constexpr int kWin = dev::kZWin, kMaxGroups = dev::kZMaxGroups, kMaxRegions = dev::kZMaxGroups;
    static constexpr const char* kName = "complex QR";
    static void chase(hipStream_t st, int nwin, const dev::ChaseBatch<cplx, dev::kZMaxGroups>& b) {
        hipLaunchKernelGGL(dev::zchase_kernel, dim3(nwin), dim3(1024), 0, st, b);
    }
    template <bool kLeft>
    static void update(hipStream_t st, int, int grid, const dev::ZWinGemmBatch& b) {
        hipLaunchKernelGGL(dev::zwin_gemm_mfma<kLeft>, dim3(grid), dim3(dev::kZMT), 0, st, b);
    }
    static int update_tile(int, int) { return dev::kZMG; }
};

// eigenvalues of the complex Hessenberg matrix H (device, n x n, leading dimension n; destroyed).  kSchur = true
// (schur_sweeps_c128): Schur mode (sweep_driver.hpp), blocks <= kZSmall finished by zschur_block_kernel; no w_host.
template <bool kSchur>
static int zfrancis_impl(eigsol_ctx* ctx, cplx* H, int64_t n, int maxits, cplx* w_host, int32_t* sweeps_out,
                         int32_t* fail_out, cplx* Z) {
    hipStream_t st = ctx->stream;
    SweepDriver<ComplexSweep, kSchur> sd{st, H, Z, n, ctx->num_cus};
    EIGSOL_TRY(sd.alloc());
    DevBuf bw, bsh, binfo, bV;
    EIGSOL_TRY(bw.alloc(n * sizeof(cplx)));
    EIGSOL_TRY(bsh.alloc(2 * dev::kZMaxBulges * sizeof(cplx)));
    EIGSOL_TRY(binfo.alloc(64));
    EIGSOL_TRY(bV.alloc((size_t)dev::kZSmall * dev::kZSmall * sizeof(cplx)));   // the AED window's unitary factor
    cplx *const dw = bw.as<cplx>(), *const dsh = bsh.as<cplx>(), *const dV = bV.as<cplx>();
    int* const dinfo = binfo.as<int>();
    int rc = EIGSOL_OK;
    // the per-sweep transfers' pinned staging (sweep_driver.hpp: why pinned)
    struct Staging {
        int info[8];
        cplx sh[2 * dev::kZMaxBulges];
    };
    PinBuf bhp;
    EIGSOL_TRY(bhp.alloc(sizeof(Staging)));
    Staging* const hp = bhp.as<Staging>();
    const cplx* const ds = sd.ds;   // the latest deflation scan: diagonal [0, n), subdiagonal [n, 2n)
    int &sweeps = sd.sweeps, &failed = sd.failed, &stall = sd.stall;
    int st_sweeps = 0, st_aed = 0, st_aed_defl = 0, st_small = 0;
    static const bool stats = std::getenv("EIGSOL_QR_STATS") != nullptr;
    int ihi = (int)n - 1;
    const int max_stall = std::max(1, maxits);
    // the shifts' QR splits at the eigenvalues' own relative subdiagonal (the real path's round-4
    // grid, francis.hip, put its optimum at a looser 1e-4; not adopted here)
    constexpr double shift_tol = 2.220446049250313e-16;
    auto small = [&](int l, int hi, cplx* wdst, int info[2], double dtol = 2.220446049250313e-16) -> int {
        hipLaunchKernelGGL(dev::zhqr_wave_kernel, dim3(1), dim3(64), 0, st, H + l + (int64_t)l * n, (int64_t)n,
                           hi - l + 1, wdst, dinfo, dtol);
        EIGSOL_HIP(hipMemcpyAsync(hp->info, dinfo, 2 * sizeof(int), hipMemcpyDeviceToHost, st));
        EIGSOL_HIP(stream_wait(st));
        info[0] = hp->info[0];
        info[1] = hp->info[1];
        return EIGSOL_OK;
    };
    while (rc == EIGSOL_OK && ihi >= 0) {
        int l;
        if ((rc = sd.next_block(ihi, &l)) != EIGSOL_OK) break;
        const int N = ihi - l + 1;
        if (N <= dev::kZSmall) {
            int info[2] = {0, 0};
            ++st_small;
            if constexpr (kSchur) {
                if (N > 1) {   // a 1 x 1 block is its own Schur form
                    hipLaunchKernelGGL(dev::zschur_block_kernel, dim3(1), dim3(dev::kZAedThreads), 0, st, H, (int64_t)n, l, N,
                                       dw + l, dV, dinfo);
                    sd.apply_outside(l, N, l, dV);
                    if (hipGetLastError() != hipSuccess ||
                        hipMemcpyAsync(hp->info, dinfo, 2 * sizeof(int), hipMemcpyDeviceToHost, st) != hipSuccess ||
                        stream_wait(st) != hipSuccess) {
                        rc = fail(EIGSOL_E_HIP, "complex QR: Schur block");
                        break;
                    }
                    info[0] = hp->info[0];
                    info[1] = hp->info[1];
                }
            } else if ((rc = small(l, ihi, dw + l, info)) != EIGSOL_OK) break;
            if (info[0]) failed = 1;
            sweeps = std::max({sweeps, stall, info[1]});
            if (kSchur && failed) break;   // the block stays unreduced: T is upper Hessenberg there
            stall = 0;
            ihi = l - 1;
            continue;
        }
        if (++stall > max_stall) { failed = 1; sweeps = std::max(sweeps, stall); break; }
        // aggressive early deflation on the trailing window, stopped at the first undeflatable
        // eigenvalue; the shifts come from the trailing block afterwards
        constexpr int aed_win = kZAedWin;
        constexpr int nibble = 14;   // % of the window deflated that skips the sweep (LAPACK's NIBBLE)
        {
            const int nw = std::min(aed_win, N);
            const int kw = ihi - nw + 1;
            hipLaunchKernelGGL(dev::zaed_kernel, dim3(1), dim3(dev::kZAedThreads), 0, st, H, (int64_t)n, kw, nw,
                               kw > l ? 1 : 0, dw, dV, dinfo);
            int* info = hp->info;
            if (hipMemcpyAsync(info, dinfo, 5 * sizeof(int), hipMemcpyDeviceToHost, st) != hipSuccess ||
                stream_wait(st) != hipSuccess) {
                rc = fail(EIGSOL_E_HIP, "complex QR: aed");
                break;
            }
            ++st_aed;
            if (!info[0]) {
                const int nd = info[1];
                if (nd > 0) {
                    st_aed_defl += nd;
                    sd.apply_aed(l, kw, nw, dV);
                    const int m = info[3];
                    ihi = kw + m - 1;
                    sd.deflated();
                    if (100 * nd >= nibble * nw || m < 2 || ihi - l + 1 <= dev::kZSmall) continue;
                }
            }
        }
        // bulges of the sweep on the block as the AED's deflations left it (C chains of nbg): the shift count 2 nb
        const ChasePlan plan = chase_plan_c128(ihi - l + 1);
        const int nb = plan.C * plan.nbg;
        const int ns = 2 * nb;
        cplx* const sh = hp->sh;   // ns values; the chase reads them from dsh
        // every 6th sweep without a deflation: exceptional shifts (LAPACK's KEXSH; stall is 0 right
        // after the AED deflated, and such a sweep takes the regular shifts; round 3's test also took
        // stall == 0, i.e. ad hoc shifts after every partial deflation: a bug, fixed in round 4)
        bool exceptional = stall > 0 && stall % 6 == 0;
        if (!exceptional) {
            int info[2];
            if ((rc = small(ihi - ns + 1, ihi, dsh, info, shift_tol)) != EIGSOL_OK) break;   // shifts written to dsh
            if (info[0]) exceptional = true;
        }
        if (exceptional) {
            for (int b = 0; b < nb; ++b) {
                const cplx d = ds[ihi - b];
                const double sc = abs1(ds[n + ihi - b]) + abs1(d) * 1e-3 + 1e-300;
                sh[2 * b] = cplx{d.re + 0.75 * sc, d.im};
                sh[2 * b + 1] = cplx{d.re - 0.75 * sc, d.im};
            }
            if (hipMemcpyAsync(dsh, sh, ns * sizeof(cplx), hipMemcpyHostToDevice, st) != hipSuccess) {
                rc = fail(EIGSOL_E_HIP, "complex QR: shift upload");
                break;
            }
        }
        ++st_sweeps;
        if ((rc = sd.run_chase(l, ihi, plan, dsh)) != EIGSOL_OK) break;
        if ((rc = sd.close_sweep(l, ihi)) != EIGSOL_OK) break;
    }
    if (rc == EIGSOL_OK && !kSchur) {
        if (hipMemcpyAsync(w_host, dw, n * sizeof(cplx), hipMemcpyDeviceToHost, st) != hipSuccess ||
            stream_wait(st) != hipSuccess)
            rc = fail(EIGSOL_E_HIP, "complex QR: download");
    }
    if (stats)
        std::fprintf(stderr, "complex francis: n=%lld sweeps=%d small_blocks=%d aed=%d aed_deflated=%d\n",
                     (long long)n, st_sweeps, st_small, st_aed, st_aed_defl);
    sd.report(sweeps_out, fail_out);
    return rc;
}

int francis_large_c128(eigsol_ctx* ctx, cplx* H, int64_t n, int maxits, cplx* w_host, int32_t* sweeps_out,
                       int32_t* fail_out) {
    return zfrancis_impl<false>(ctx, H, n, maxits, w_host, sweeps_out, fail_out, nullptr);
}

// The sweeps in Schur mode (schur.hip): H (upper Hessenberg, exact zeros below the sub-diagonal) becomes the
// upper triangular T, Z (null: none) becomes Z U for the unitary U with T = U^H H U.  *fail_out: T is upper
// Hessenberg only; the similarity holds all the same.
int schur_sweeps_c128(eigsol_ctx* ctx, cplx* H, int64_t n, cplx* Z, int maxits, int32_t* sweeps_out,
                      int32_t* fail_out) {
    return zfrancis_impl<true>(ctx, H, n, maxits, nullptr, sweeps_out, fail_out, Z);
}

}  // namespace eigsol
