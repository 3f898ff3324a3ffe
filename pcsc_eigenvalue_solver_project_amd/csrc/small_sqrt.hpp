// The scalar square roots behind the diagonal groups of the triangular square root (sqrtm.hip): the principal
// root of a complex number and of a real 2 x 2 block with a complex pair of eigenvalues.  Plain C++ so that a
// host program can run them (tests/cpp/small_sqrt_host.cpp, tests/test_small_sqrt_cpu.py).
//
// Both take an even power of two 2^(2 h) out of their operands first, so that the largest of them lies in
// [1, 4), work on the scaled operands with products, sums, quotients and sqrt only (no library hypot), and
// scale the result by 2^h.  The scaled operands of 4^e z are the bits of those of z, so the root of 4^e z is
// 2^e times the root of z, bit for bit (away from overflow and underflow of the operands themselves).
#pragma once

#include <cmath>

#include "kernels_common.hpp"

namespace eigsol {
namespace dev {

// the even exponent 2 h with 2^(2 h) <= m < 2^(2 h + 2); m > 0, finite
__host__ __device__ inline int sqrt_even_exp(double m) {
    const int e = (int)ilogb(m);
    return e - (e & 1);   // floor to even, also for negative e (two's complement)
}

// Principal square root of x + i y: real part >= 0; on the negative real axis the root lies on the positive
// imaginary axis, and an imaginary part of -0.0 counts as +0.0.
//   x >= 0: a = sqrt((|z| + x) / 2), b = y / (2 a);   x < 0: |b| = sqrt((|z| - x) / 2), a = |y| / (2 |b|)
// so that neither sum cancels.
__host__ __device__ inline cplx sqrt_principal(cplx z) {
    const double ax = z.re < 0 ? -z.re : z.re, ay = z.im < 0 ? -z.im : z.im;
    const double m = ax > ay ? ax : ay;
    if (!(m > 0.0)) return cplx{m, m == 0.0 ? 0.0 : m};   // 0 -> 0; nan -> nan
    const int e2 = sqrt_even_exp(m);
    const double x = ldexp(z.re, -e2), y = ldexp(z.im, -e2);
    const double r = sqrt(x * x + y * y);
    double a, b;
    if (x >= 0.0) {
        a = sqrt((r + x) / 2.0);
        b = y == 0.0 ? 0.0 : y / (2.0 * a);
    } else {
        const double bm = sqrt((r - x) / 2.0);
        a = ay == 0.0 ? 0.0 : (y < 0 ? -y : y) / (2.0 * bm);
        b = y < 0.0 ? -bm : bm;
    }
    return cplx{ldexp(a, e2 / 2), ldexp(b, e2 / 2)};
}

// U = B^(1/2) for the real 2 x 2 block B = [b11 b12; b21 b22] with eigenvalues theta +- i mu, mu > 0 (any such
// block, not only schur's standard form): U = alpha I + (B - theta I) / (2 alpha), alpha = Re sqrt(theta + i mu),
//   alpha = sqrt((|lambda| + theta) / 2)                  theta >= 0
//   alpha = mu / (2 sqrt((|lambda| - theta) / 2))         theta < 0
// u receives u11, u21, u12, u22 (column-major).  False: the eigenvalues are real (mu^2 <= 0), u is not written.
__host__ __device__ inline bool sqrt_block2(double b11, double b21, double b12, double b22, double (&u)[4]) {
    double m = fabs(b11);
    m = fmax(m, fabs(b21));
    m = fmax(m, fabs(b12));
    m = fmax(m, fabs(b22));
    if (!(m > 0.0)) return false;
    const int e2 = sqrt_even_exp(m);
    const double s11 = ldexp(b11, -e2), s21 = ldexp(b21, -e2), s12 = ldexp(b12, -e2), s22 = ldexp(b22, -e2);
    const double theta = (s11 + s22) / 2.0, d = (s11 - s22) / 2.0;
    const double mu2 = -(d * d + s12 * s21);
    if (!(mu2 > 0.0)) return false;
    const double mu = sqrt(mu2), lam = sqrt(theta * theta + mu2);
    const double alpha = theta >= 0.0 ? sqrt((lam + theta) / 2.0) : mu / (2.0 * sqrt((lam - theta) / 2.0));
    const double t = 2.0 * alpha;
    const int h = e2 / 2;
    u[0] = ldexp(alpha + d / t, h);
    u[1] = ldexp(s21 / t, h);
    u[2] = ldexp(s12 / t, h);
    u[3] = ldexp(alpha - d / t, h);
    return true;
}

}  // namespace dev
}  // namespace eigsol
