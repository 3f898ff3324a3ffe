// Pieces of schur.hip that the drivers working on a Schur form on the device share (ordschur.hip): the
// standardisation of one 2 x 2 block and the eigenvalues of T's blocks.
#pragma once

#include <cmath>

#include "kernels_common.hpp"

namespace eigsol {
namespace dev {

// One 2 x 2 block [a b; c d] to its standard form by the rotation [cs sn; -sn cs] (LAPACK dlanv2 without
// its rescaling loop: the range guard has put the matrix inside [smlnum, 1 / smlnum]).
struct Lanv2 {
    double a, b, c, d, cs, sn;
};
__host__ __device__ inline double sch_sign(double x, double s) { return copysign(fabs(x), s); }
__host__ __device__ inline Lanv2 schur_lanv2_dev(double a, double b, double c, double d) {
    using std::signbit;   // the host build takes <cmath>'s
    const double eps = 2.220446049250313e-16, multpl = 4.0;
    double cs, sn;
    if (c == 0.0) {
        cs = 1.0;
        sn = 0.0;
    } else if (b == 0.0) {   // swap rows and columns
        cs = 0.0;
        sn = 1.0;
        const double tmp = d;
        d = a;
        a = tmp;
        b = -c;
        c = 0.0;
    } else if (a - d == 0.0 && signbit(b) != signbit(c)) {
        cs = 1.0;
        sn = 0.0;
    } else {
        double temp = a - d;
        double p = 0.5 * temp;
        const double bcmax = fmax(fabs(b), fabs(c));
        const double bcmis = fmin(fabs(b), fabs(c)) * sch_sign(1.0, b) * sch_sign(1.0, c);
        const double scale = fmax(fabs(p), bcmax);
        double z = p / scale * p + bcmax / scale * bcmis;
        if (z >= multpl * eps) {   // real eigenvalues: a or d becomes one of them
            z = p + sch_sign(sqrt(scale) * sqrt(z), p);
            a = d + z;
            d = d - bcmax / z * bcmis;
            const double tau = hypot(c, z);
            cs = z / tau;
            sn = c / tau;
            b = b - c;
            c = 0.0;
        } else {   // complex or nearly equal real eigenvalues: equal diagonal entries first
            const double sigma = b + c;
            const double tau = hypot(sigma, temp);
            cs = sqrt(0.5 * (1.0 + fabs(sigma) / tau));
            sn = -(p / (tau * cs)) * sch_sign(1.0, sigma);
            const double aa = a * cs + b * sn, bb = -a * sn + b * cs;
            const double cc = c * cs + d * sn, dd = -c * sn + d * cs;
            a = aa * cs + cc * sn;
            b = bb * cs + dd * sn;
            c = -aa * sn + cc * cs;
            d = -bb * sn + dd * cs;
            temp = 0.5 * (a + d);
            a = temp;
            d = temp;
            if (c != 0.0) {
                if (b != 0.0) {
                    if (signbit(b) == signbit(c)) {   // real eigenvalues after all: to upper triangular
                        const double sab = sqrt(fabs(b)), sac = sqrt(fabs(c));
                        p = sch_sign(sab * sac, c);
                        const double tau2 = 1.0 / sqrt(fabs(b + c));
                        a = temp + p;
                        d = temp - p;
                        b = b - c;
                        c = 0.0;
                        const double cs1 = sab * tau2, sn1 = sac * tau2;
                        const double t2 = cs * cs1 - sn * sn1;
                        sn = cs * sn1 + sn * cs1;
                        cs = t2;
                    }
                } else {
                    b = -c;
                    c = 0.0;
                    const double t2 = cs;
                    cs = -sn;
                    sn = t2;
                }
            }
        }
    }
    return Lanv2{a, b, c, d, cs, sn};
}

// eigenvalues of the quasi-triangular T: w[2 i], w[2 i + 1] = Re, Im of the eigenvalue at row i
static __global__ __launch_bounds__(256) void schur_eigs_real(const double* T, int64_t n, double* w) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const double lower = i + 1 < n ? T[(i + 1) + i * n] : 0.0;
    const double upper = i > 0 ? T[i + (i - 1) * n] : 0.0;
    double im = 0.0;
    if (lower != 0.0) im = sqrt(fabs(T[i + (i + 1) * n])) * sqrt(fabs(lower));
    else if (upper != 0.0) im = -(sqrt(fabs(T[(i - 1) + i * n])) * sqrt(fabs(upper)));
    w[2 * i] = T[i + i * n];
    w[2 * i + 1] = im;
}

static __global__ __launch_bounds__(256) void schur_eigs_cplx(const cplx* T, int64_t n, cplx* w) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i < n) w[i] = T[i + i * n];
}

}  // namespace dev
}  // namespace eigsol
