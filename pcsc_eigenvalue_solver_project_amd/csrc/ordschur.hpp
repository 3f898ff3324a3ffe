// Reordering of a Schur form on the device (ordschur.hip): the driver's interface and the
// work of one window, which is plain C++ on a window of T and its factor U so that a host program can run it
// with one lane (tests/cpp/ordschur_window_host.cpp, tests/test_ordschur_window_cpu.py).
#pragma once

#include "schur.hpp"
#include "schur_blocks.hpp"
#include "small_solve.hpp"

namespace eigsol {

// Half-window rows h and the largest window: real 2 h + 1 = 95 <= 96 (a window takes the pair that straddles
// its lower end), complex 2 h = 64.
template <class S> struct OrdDims;
template <> struct OrdDims<double> {
    static constexpr int h = 47, wmax = 96, ld = 97;
};
template <> struct OrdDims<cplx> {
    static constexpr int h = 32, wmax = 64, ld = 65;
};

struct OrdStats {
    double ms = 0.0;
    int32_t rounds = 0, windows = 0, swaps = 0;
};

// Reorders sd.T (and sd.Z where wantz) in place on ctx's stream so that the selected eigenvalues lead, and
// rewrites sd.w.  select_host: one byte per row (host), or null with sort = EIGSOL_SORT_*: the flags are then
// built on the device from sd.w.  Waits for the stream once per round.  *ordered = 0: a swap was rejected;
// T is a Schur form and A = Z T Z^H holds all the same.
template <class S>
int ordschur_device(eigsol_ctx* ctx, int64_t n, SchurDevice& sd, bool wantz, const unsigned char* select_host, int sort,
                    int64_t* sdim, int32_t* ordered, OrdStats* stats);

namespace dev {

#if defined(__HIP_DEVICE_COMPILE__)
#define EIGSOL_ORD_SYNC() __syncthreads()
#else
#define EIGSOL_ORD_SYNC() ((void)0)
#endif

// What one swap of adjacent diagonal blocks does to a vector of the n1 + n2 rows (or columns) it spans; the
// same sequence serves T's rows right of the blocks, T's columns above them and U's columns.
//   kind 0: the rotation of two 1 x 1 blocks;  1: n1 = 1, n2 = 2;  2: n1 = 2, n2 = 1;  3: two 2 x 2 blocks
// followed by the rotations that standardise the new leading (r1) and trailing (r2, at position p2) 2 x 2 block.
struct OrdOp {
    int kind, r1, r2, p2;
    double cs, sn;
    double v1[3], tau1, v2[3], tau2;
    double c1, s1, c2, s2;
};

__host__ __device__ inline void ord_rot(double& x, double& y, double c, double s) {
    const double a = c * x + s * y;
    y = c * y - s * x;
    x = a;
}
// (a, b, c) <- (I - tau v v^T) (a, b, c)
__host__ __device__ inline void ord_refl3(const double (&v)[3], double tau, double& a, double& b, double& c) {
    const double sum = (v[0] * a + v[1] * b + v[2] * c) * tau;
    a -= sum * v[0];
    b -= sum * v[1];
    c -= sum * v[2];
}
__host__ __device__ inline void ord_apply(const OrdOp& o, double (&x)[4]) {
    if (o.kind == 0) {
        ord_rot(x[0], x[1], o.cs, o.sn);
        return;
    }
    ord_refl3(o.v1, o.tau1, x[0], x[1], x[2]);
    if (o.kind == 3) ord_refl3(o.v2, o.tau2, x[1], x[2], x[3]);
    if (o.r1) ord_rot(x[0], x[1], o.c1, o.s1);
    if (o.r2) {
        if (o.p2 == 1) ord_rot(x[1], x[2], o.c2, o.s2);
        else ord_rot(x[2], x[3], o.c2, o.s2);
    }
}

// LAPACK dlarfg for three entries, alpha at position ia, without its rescaling loop (the range guard):
// v[ia] = 1, H = I - tau v v^T maps the vector onto a multiple of e_ia.
__host__ __device__ inline void ord_larfg3(double (&u)[3], int ia, double (&v)[3], double& tau) {
    const double alpha = u[ia];
    double xn = 0.0;
    if (ia == 0) xn = hypot(u[1], u[2]);
    else xn = hypot(u[0], u[1]);
    if (xn == 0.0) {
        tau = 0.0;
        v[0] = v[1] = v[2] = 0.0;
        v[ia] = 1.0;
        return;
    }
    const double beta = -copysign(hypot(alpha, xn), alpha);
    tau = (beta - alpha) / beta;
    const double sc = 1.0 / (alpha - beta);
#pragma unroll
    for (int k = 0; k < 3; ++k) v[k] = u[k] * sc;
    v[ia] = 1.0;
}

// The swap of the blocks D(0:n1, 0:n1) and D(n1:nd, n1:nd) of the local copy D (LAPACK dlaexc); the block sizes
// are template arguments so that every index into the 4 x 4 arrays is a constant and they stay in registers.
// On success D holds the swapped, standardised blocks and o the sequence for everything outside D; false: the
// swap was rejected by dlaexc's test, D and the window are untouched.
template <int n1, int n2>
__host__ __device__ inline bool ord_swap_local(double (&D)[4][4], OrdOp& o) {
    const double eps = 2.220446049250313e-16, smlnum = 2.2250738585072014e-308 / eps;
    constexpr int nd = n1 + n2;
    o.r1 = o.r2 = 0;
    o.p2 = n2;
    if constexpr (nd == 2) {
        const double t11 = D[0][0], t22 = D[1][1];
        const double f = D[0][1], g = t22 - t11;
        o.kind = 0;
        if (g == 0.0) {
            o.cs = 1.0;
            o.sn = 0.0;
        } else if (f == 0.0) {
            o.cs = 0.0;
            o.sn = 1.0;
        } else {
            const double d = hypot(f, g), r = copysign(d, f);
            o.cs = fabs(f) / d;
            o.sn = g / r;
        }
        D[0][0] = t22;
        D[1][1] = t11;
        return true;
    }
    double dnorm = 0.0, tmax = 0.0;
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j)
            if (i < nd && j < nd) {
                dnorm = fmax(dnorm, fabs(D[i][j]));
                if ((i < n1) == (j < n1)) tmax = fmax(tmax, fabs(D[i][j]));
            }
    const double thresh = fmax(10.0 * eps * dnorm, smlnum);
    const double smin = fmax(eps * tmax, smlnum);
    // T11 X - X T22 = T12: unknown u = ua + n1 ub holds X(ua, ub)
    constexpr int N = n1 * n2;
    double K[4][4], x[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
        x[u] = 0.0;
#pragma unroll
        for (int v = 0; v < 4; ++v) K[u][v] = 0.0;
    }
#pragma unroll
    for (int u = 0; u < 4; ++u) {
        if (u >= N) continue;
        const int ua = u % n1, ub = u / n1;
        x[u] = D[ua][n1 + ub];
#pragma unroll
        for (int v = 0; v < 4; ++v) {
            if (v >= N) continue;
            const int va = v % n1, vb = v / n1;
            double kv = 0.0;
            if (ub == vb) kv += D[ua][va];
            if (ua == va) kv -= D[n1 + vb][n1 + ub];
            K[u][v] = kv;
        }
    }
    (void)syl_solve4(N, K, x, smin);
    double E[4][4];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) E[i][j] = D[i][j];
    if constexpr (n1 == 1 && n2 == 2) {
        o.kind = 1;
        double u[3] = {1.0, x[0], x[1]};
        ord_larfg3(u, 2, o.v1, o.tau1);
        const double t11 = E[0][0];
#pragma unroll
        for (int j = 0; j < 3; ++j) ord_refl3(o.v1, o.tau1, E[0][j], E[1][j], E[2][j]);
#pragma unroll
        for (int i = 0; i < 3; ++i) ord_refl3(o.v1, o.tau1, E[i][0], E[i][1], E[i][2]);
        if (fmax(fmax(fabs(E[2][0]), fabs(E[2][1])), fabs(E[2][2] - t11)) > thresh) return false;
        E[2][0] = 0.0;
        E[2][1] = 0.0;
        E[2][2] = t11;
    } else if constexpr (n1 == 2 && n2 == 1) {
        o.kind = 2;
        double u[3] = {-x[0], -x[1], 1.0};
        ord_larfg3(u, 0, o.v1, o.tau1);
        const double t33 = E[2][2];
#pragma unroll
        for (int j = 0; j < 3; ++j) ord_refl3(o.v1, o.tau1, E[0][j], E[1][j], E[2][j]);
#pragma unroll
        for (int i = 0; i < 3; ++i) ord_refl3(o.v1, o.tau1, E[i][0], E[i][1], E[i][2]);
        if (fmax(fmax(fabs(E[1][0]), fabs(E[2][0])), fabs(E[0][0] - t33)) > thresh) return false;
        E[0][0] = t33;
        E[1][0] = 0.0;
        E[2][0] = 0.0;
    } else {
        o.kind = 3;
        double u1[3] = {-x[0], -x[1], 1.0};
        ord_larfg3(u1, 0, o.v1, o.tau1);
        const double temp = -o.tau1 * (x[2] + o.v1[1] * x[3]);
        double u2[3] = {-temp * o.v1[1] - x[3], -temp * o.v1[2], 1.0};
        ord_larfg3(u2, 0, o.v2, o.tau2);
#pragma unroll
        for (int j = 0; j < 4; ++j) ord_refl3(o.v1, o.tau1, E[0][j], E[1][j], E[2][j]);
#pragma unroll
        for (int i = 0; i < 4; ++i) ord_refl3(o.v1, o.tau1, E[i][0], E[i][1], E[i][2]);
#pragma unroll
        for (int j = 0; j < 4; ++j) ord_refl3(o.v2, o.tau2, E[1][j], E[2][j], E[3][j]);
#pragma unroll
        for (int i = 0; i < 4; ++i) ord_refl3(o.v2, o.tau2, E[i][1], E[i][2], E[i][3]);
        if (fmax(fmax(fabs(E[2][0]), fabs(E[2][1])), fmax(fabs(E[3][0]), fabs(E[3][1]))) > thresh) return false;
        E[2][0] = 0.0;
        E[2][1] = 0.0;
        E[3][0] = 0.0;
        E[3][1] = 0.0;
    }
    if constexpr (n2 == 2) {   // the new leading block, rows 0 and 1
        const Lanv2 r = schur_lanv2_dev(E[0][0], E[0][1], E[1][0], E[1][1]);
        E[0][0] = r.a;
        E[0][1] = r.b;
        E[1][0] = r.c;
        E[1][1] = r.d;
        if (!(r.cs == 1.0 && r.sn == 0.0)) {
            o.r1 = 1;
            o.c1 = r.cs;
            o.s1 = r.sn;
#pragma unroll
            for (int j = 2; j < 4; ++j)
                if (j < nd) ord_rot(E[0][j], E[1][j], r.cs, r.sn);
        }
    }
    if constexpr (n1 == 2) {   // the new trailing block, rows n2 and n2 + 1
        if constexpr (n2 == 1) {
            const Lanv2 r = schur_lanv2_dev(E[1][1], E[1][2], E[2][1], E[2][2]);
            E[1][1] = r.a;
            E[1][2] = r.b;
            E[2][1] = r.c;
            E[2][2] = r.d;
            if (!(r.cs == 1.0 && r.sn == 0.0)) {
                o.r2 = 1;
                o.c2 = r.cs;
                o.s2 = r.sn;
                ord_rot(E[0][1], E[0][2], r.cs, r.sn);
            }
        } else {
            const Lanv2 r = schur_lanv2_dev(E[2][2], E[2][3], E[3][2], E[3][3]);
            E[2][2] = r.a;
            E[2][3] = r.b;
            E[3][2] = r.c;
            E[3][3] = r.d;
            if (!(r.cs == 1.0 && r.sn == 0.0)) {
                o.r2 = 1;
                o.c2 = r.cs;
                o.s2 = r.sn;
                ord_rot(E[0][2], E[0][3], r.cs, r.sn);
                ord_rot(E[1][2], E[1][3], r.cs, r.sn);
            }
        }
    }
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) D[i][j] = E[i][j];
    return true;
}

// One swap inside the window: blocks of n1 and n2 rows at row j1.  t, u: W x W at pitch LD; every lane takes
// the same path.  False: rejected, nothing written.
__host__ __device__ inline bool ord_swap(double* t, double* u, unsigned char* f, int W, int LD, int j1, int n1, int n2, int lane,
                                         int nl) {
    const int nd = n1 + n2;
    double D[4][4];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) D[i][j] = (i < nd && j < nd) ? t[(j1 + i) + (j1 + j) * LD] : 0.0;
    OrdOp o;
    bool ok;
    if (n1 == 1) ok = n2 == 1 ? ord_swap_local<1, 1>(D, o) : ord_swap_local<1, 2>(D, o);
    else ok = n2 == 1 ? ord_swap_local<2, 1>(D, o) : ord_swap_local<2, 2>(D, o);
    const unsigned char fa = f[j1], fb = f[j1 + n1];
    EIGSOL_ORD_SYNC();
    if (!ok) return false;
    // items: the columns right of the blocks, T's rows above them, every row of U
    const int ncol = W - (j1 + nd), nitem = ncol + j1 + W;
    for (int it = lane; it < nitem; it += nl) {
        double x[4] = {0.0, 0.0, 0.0, 0.0};
        double* p;
        int step;
        if (it < ncol) {
            p = t + j1 + (j1 + nd + it) * LD;
            step = 1;
        } else if (it < ncol + j1) {
            p = t + (it - ncol) + j1 * LD;
            step = LD;
        } else {
            p = u + (it - ncol - j1) + j1 * LD;
            step = LD;
        }
#pragma unroll
        for (int k = 0; k < 4; ++k)
            if (k < nd) x[k] = p[k * step];
        ord_apply(o, x);
#pragma unroll
        for (int k = 0; k < 4; ++k)
            if (k < nd) p[k * step] = x[k];
    }
    if (lane == 0) {
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int j = 0; j < 4; ++j)
                if (i < nd && j < nd) t[(j1 + i) + (j1 + j) * LD] = D[i][j];
        for (int k = 0; k < nd; ++k) f[j1 + k] = k < n2 ? fb : fa;
    }
    EIGSOL_ORD_SYNC();
    return true;
}

// ztrexc's swap of the diagonal entries at rows j1 and j1 + 1: one rotation, the diagonal exchanged exactly
__host__ __device__ inline bool ord_swap(cplx* t, cplx* u, unsigned char* f, int W, int LD, int j1, int, int, int lane, int nl) {
    const cplx t11 = t[j1 + j1 * LD], t22 = t[(j1 + 1) + (j1 + 1) * LD];
    const cplx fv = t[j1 + (j1 + 1) * LD], g = cplx{t22.re - t11.re, t22.im - t11.im};
    const double fa = cabs_(fv.re, fv.im), ga = cabs_(g.re, g.im);
    double cs;
    cplx sn;   // [cs sn; -conj(sn) cs] (f; g) = (r; 0)
    if (ga == 0.0) {
        cs = 1.0;
        sn = cplx{0.0, 0.0};
    } else if (fa == 0.0) {
        cs = 0.0;
        sn = cplx{g.re / ga, -g.im / ga};
    } else {
        const double d = hypot(fa, ga);
        cs = fa / d;
        const cplx ph{fv.re / fa, fv.im / fa};   // f / |f|; sn = ph conj(g) / d
        sn = cplx{(ph.re * g.re + ph.im * g.im) / d, (ph.im * g.re - ph.re * g.im) / d};
    }
    const unsigned char f0 = f[j1], f1 = f[j1 + 1];
    EIGSOL_ORD_SYNC();
    const int ncol = W - (j1 + 2), nitem = ncol + j1 + W;
    for (int it = lane; it < nitem; it += nl) {
        cplx *px, *py;
        cplx s = sn;
        if (it < ncol) {   // rows: x' = cs x + sn y, y' = cs y - conj(sn) x
            px = t + j1 + (j1 + 2 + it) * LD;
            py = px + 1;
        } else {   // columns: the same with conj(sn)
            cplx* const base = it < ncol + j1 ? t + (it - ncol) : u + (it - ncol - j1);
            px = base + j1 * LD;
            py = px + LD;
            s.im = -s.im;
        }
        const cplx x = *px, y = *py;
        *px = cplx{cs * x.re + (s.re * y.re - s.im * y.im), cs * x.im + (s.re * y.im + s.im * y.re)};
        *py = cplx{cs * y.re - (s.re * x.re + s.im * x.im), cs * y.im - (s.re * x.im - s.im * x.re)};
    }
    if (lane == 0) {
        t[j1 + j1 * LD] = t22;
        t[(j1 + 1) + (j1 + 1) * LD] = t11;
        f[j1] = f1;
        f[j1 + 1] = f0;
    }
    EIGSOL_ORD_SYNC();
    return true;
}

__host__ __device__ inline bool ord_is_pair(const double* t, int LD, int W, int k) {
    return k + 1 < W && t[(k + 1) + k * LD] != 0.0;
}
__host__ __device__ inline bool ord_is_pair(const cplx*, int, int, int) { return false; }

// Moves every selected block of the window to its top by swaps of adjacent blocks, in order, so that the
// selected and the unselected blocks each keep their order (LAPACK xTRSEN's order).  Returns the number of
// swaps; failed = 1 where one was rejected, which ends the window's work.
template <class S>
__host__ __device__ inline int ord_window(S* t, S* u, unsigned char* f, int W, int LD, int lane, int nl, int& failed) {
    int swaps = 0, pos = 0, k = 0;
    failed = 0;
    while (k < W) {
        const int bk = ord_is_pair(t, LD, W, k) ? 2 : 1;
        if (!f[k]) {
            k += bk;
            continue;
        }
        int here = k, cur = bk;
        bool split = false;
        while (here > pos) {
            const int na = (here >= 2 && ord_is_pair(t, LD, W, here - 2)) ? 2 : 1;
            if (!ord_swap(t, u, f, W, LD, here - na, na, cur, lane, nl)) {
                failed = 1;
                return swaps;
            }
            ++swaps;
            here -= na;
            if (cur == 2 && !ord_is_pair(t, LD, W, here)) {   // the pair split: its first half goes on alone
                cur = 1;
                split = true;
            }
        }
        pos += cur;
        k = split ? pos : k + bk;
    }
    return swaps;
}

}  // namespace dev
}  // namespace eigsol
