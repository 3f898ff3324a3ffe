// The scalar logarithms behind the diagonal of the triangular logarithm (logm.hip): the principal logarithm of a
// complex number, of a real 2 x 2 block with a complex pair of eigenvalues, and the super-diagonal entry of the
// logarithm of an upper triangular 2 x 2 matrix (Al-Mohy and Higham 2012, eq. 5.6).  Plain C++ so that a host
// program can run them (tests/cpp/small_log_host.cpp, tests/test_logm_cpu.py).
#pragma once

#include <cmath>

#include "kernels_common.hpp"

namespace eigsol {
namespace dev {

constexpr double kLogPi = 3.141592653589793238462643383279502884;

// ln sqrt(x^2 + y^2), x^2 + y^2 > 0: through log1p where the modulus is near 1, so that the logarithm of a number
// near the unit circle keeps its relative accuracy
__host__ __device__ inline double log_modulus(double x, double y) {
    const double ax = fabs(x), ay = fabs(y);
    const double big = ax > ay ? ax : ay, small = ax > ay ? ay : ax;
    if (big > 0.5 && big < 2.0 && small < 2.0) {
        const double d = (big - 1.0) * (big + 1.0) + small * small;   // |z|^2 - 1; big - 1 is exact
        if (d > -0.5 && d < 1.0) return 0.5 * log1p(d);
    }
    return log(hypot(x, y));
}

// Principal logarithm of x + i y != 0: ln|z| + i atan2(y, x), the imaginary part in (-pi, pi]; an imaginary part
// of -0.0 counts as +0.0, so both zeros on the negative real axis give +i pi.
__host__ __device__ inline cplx log_principal(cplx z) {
    const double y = z.im == 0.0 ? 0.0 : z.im;
    return cplx{log_modulus(z.re, y), atan2(y, z.re)};
}

// L = log B for the real 2 x 2 block B = [b11 b12; b21 b22] with eigenvalues a +- i mu, mu > 0: with M = B - a I,
//   L = ln(|lambda|) I + (atan2(mu, a) / mu) M.
// l receives l11, l21, l12, l22 (column-major).  False: the eigenvalues are real, l is not written.
__host__ __device__ inline bool log_block2(double b11, double b21, double b12, double b22, double (&l)[4]) {
    const double a = (b11 + b22) / 2.0, d = (b11 - b22) / 2.0;
    const double mu2 = -(d * d + b12 * b21);
    if (!(mu2 > 0.0)) return false;
    const double mu = sqrt(mu2);
    const double lm = log_modulus(a, mu), f = atan2(mu, a) / mu;
    l[0] = lm + f * d;
    l[1] = f * b21;
    l[2] = f * b12;
    l[3] = lm - f * d;
    return true;
}

// atanh z for |z| <= 1 / 2 or so (Kahan's formulas; no cancellation near 0)
__host__ __device__ inline cplx atanh_small(cplx z) {
    const double x = z.re, y = z.im;
    const double om = 1.0 - x;
    const double re = 0.25 * log1p(4.0 * x / (om * om + y * y));
    const double im = 0.5 * atan2(2.0 * y, om * (1.0 + x) - y * y);
    return cplx{re, im};
}

__host__ __device__ inline cplx log_cdiv(cplx a, cplx b) {   // Smith's method
    if (fabs(b.re) >= fabs(b.im)) {
        const double r = b.im / b.re, den = b.re + b.im * r;
        return cplx{(a.re + a.im * r) / den, (a.im - a.re * r) / den};
    }
    const double r = b.re / b.im, den = b.re * r + b.im;
    return cplx{(a.re * r + a.im) / den, (a.im * r - a.re) / den};
}

// The (1, 2) entry of log [l1 t12; 0 l2], l1, l2 > 0:
//   l1 == l2: t12 / l1;  far apart (|l2 - l1| > |l1 + l2| / 2): t12 (ln l2 - ln l1) / (l2 - l1);
//   else t12 2 atanh((l2 - l1) / (l2 + l1)) / (l2 - l1).
__host__ __device__ inline double log_superdiag(double l1, double l2, double t12) {
    if (l1 == l2) return t12 / l1;
    const double df = l2 - l1;
    if (fabs(df) > fabs(l1 + l2) / 2.0) return t12 * (log(l2) - log(l1)) / df;
    return t12 * 2.0 * atanh(df / (l2 + l1)) / df;
}

// The same for complex l1, l2 != 0: the atanh form carries the unwinding number u of ln l2 - ln l1,
//   t12 2 (atanh(z) + i pi u) / (l2 - l1),  u = ceil((Im(ln l2 - ln l1) - pi) / (2 pi)).
__host__ __device__ inline cplx log_superdiag(cplx l1, cplx l2, cplx t12) {
    auto cmul = [](cplx a, cplx b) { return cplx{a.re * b.re - a.im * b.im, a.re * b.im + a.im * b.re}; };
    if (l1.re == l2.re && l1.im == l2.im) return log_cdiv(t12, l1);
    const cplx df{l2.re - l1.re, l2.im - l1.im}, sm{l2.re + l1.re, l2.im + l1.im};
    const cplx g1 = log_principal(l1), g2 = log_principal(l2);
    const cplx w{g2.re - g1.re, g2.im - g1.im};
    if (hypot(df.re, df.im) > hypot(sm.re, sm.im) / 2.0) return log_cdiv(cmul(t12, w), df);
    const double u = ceil((w.im - kLogPi) / (2.0 * kLogPi));
    cplx at = atanh_small(log_cdiv(df, sm));
    at.im += kLogPi * u;
    return log_cdiv(cmul(t12, cplx{2.0 * at.re, 2.0 * at.im}), df);
}

}  // namespace dev
}  // namespace eigsol
