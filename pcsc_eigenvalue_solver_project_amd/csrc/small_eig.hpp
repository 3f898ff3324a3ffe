// Host-side eigen-decomposition of a small complex matrix and the Ritz-value order, shared by the
// block subspace iteration (subspace.hip, m <= 32) and the Krylov-Schur solver (krylov.hip,
// m <= 64).
#pragma once

#include <algorithm>
#include <cmath>
#include <complex>
#include <vector>

#include "internal.hpp"

namespace eigsol {
namespace smalleig {

using cd = std::complex<double>;

// ---------------------------------------------------------------- eig of a small complex matrix
// H: m x m row-major (destroyed).  Hessenberg reduction by reflectors, single-shift QR with the
// Schur vectors accumulated, eigenvectors of the triangle by back substitution.  w[k]: eigenvalue,
// column k of Y (row-major m x m): its unit eigenvector.  false: the QR iteration did not converge.
inline bool small_eig(int m, std::vector<cd>& H, std::vector<cd>& w, std::vector<cd>& Y) {
    const double eps = 0x1p-52;
    auto h = [&](int i, int j) -> cd& { return H[(size_t)i * m + j]; };
    std::vector<cd> V((size_t)m * m, cd(0));
    auto v = [&](int i, int j) -> cd& { return V[(size_t)i * m + j]; };
    for (int i = 0; i < m; ++i) v(i, i) = 1.0;
    std::vector<cd> u(m);
    for (int k = 0; k + 2 < m; ++k) {
        double alpha = 0.0;
        for (int i = k + 1; i < m; ++i) alpha += std::norm(h(i, k));
        alpha = std::sqrt(alpha);
        if (alpha == 0.0) continue;
        const cd x0 = h(k + 1, k);
        const cd phase = std::abs(x0) > 0.0 ? x0 / std::abs(x0) : cd(1.0);
        double un2 = 0.0;
        for (int i = k + 1; i < m; ++i) {
            u[i] = h(i, k);
            if (i == k + 1) u[i] += phase * alpha;
            un2 += std::norm(u[i]);
        }
        if (un2 == 0.0) continue;
        const double beta = 2.0 / un2;
        for (int j = 0; j < m; ++j) {              // H <- P H
            cd s = 0.0;
            for (int i = k + 1; i < m; ++i) s += std::conj(u[i]) * h(i, j);
            s *= beta;
            for (int i = k + 1; i < m; ++i) h(i, j) -= u[i] * s;
        }
        for (int i = 0; i < m; ++i) {              // H <- H P, V <- V P
            cd s = 0.0, sv = 0.0;
            for (int j = k + 1; j < m; ++j) {
                s += h(i, j) * u[j];
                sv += v(i, j) * u[j];
            }
            s *= beta;
            sv *= beta;
            for (int j = k + 1; j < m; ++j) {
                h(i, j) -= s * std::conj(u[j]);
                v(i, j) -= sv * std::conj(u[j]);
            }
        }
        for (int i = k + 2; i < m; ++i) h(i, k) = 0.0;
    }
    double hn = 0.0;
    for (const cd& z : H) hn += std::norm(z);
    hn = std::sqrt(hn);
    std::vector<cd> gc(m), gs(m);
    int hi = m - 1, iter = 0;
    while (hi >= 0) {
        int l = hi;
        for (; l > 0; --l) {
            double s = std::abs(h(l - 1, l - 1)) + std::abs(h(l, l));
            if (s == 0.0) s = hn;
            if (std::abs(h(l, l - 1)) <= eps * s) {
                h(l, l - 1) = 0.0;
                break;
            }
        }
        if (l == hi) {
            --hi;
            iter = 0;
            continue;
        }
        if (++iter > 100) return false;
        cd mu;
        if (iter == 10 || iter == 20 || iter == 40) {
            mu = h(hi, hi) + cd(0.75 * std::abs(h(hi, hi - 1)), 0.0);
        } else {
            const cd a = h(hi - 1, hi - 1), b = h(hi - 1, hi), c = h(hi, hi - 1), d = h(hi, hi);
            const cd half = 0.5 * (a - d);
            const cd disc = std::sqrt(half * half + b * c);
            const cd m1 = 0.5 * (a + d) + disc, m2 = 0.5 * (a + d) - disc;
            mu = std::abs(m1 - d) <= std::abs(m2 - d) ? m1 : m2;
        }
        for (int i = l; i <= hi; ++i) h(i, i) -= mu;
        for (int i = l; i < hi; ++i) {             // rows i, i+1 <- G_i rows
            const cd a = h(i, i), b = h(i + 1, i);
            const double r = std::hypot(std::abs(a), std::abs(b));
            cd c = 1.0, s = 0.0;
            if (r > 0.0) {
                c = a / r;
                s = b / r;
            }
            gc[i] = c;
            gs[i] = s;
            for (int j = i; j < m; ++j) {
                const cd p = h(i, j), q = h(i + 1, j);
                h(i, j) = std::conj(c) * p + std::conj(s) * q;
                h(i + 1, j) = -s * p + c * q;
            }
            h(i + 1, i) = 0.0;
        }
        for (int i = l; i < hi; ++i) {             // columns i, i+1 <- columns G_i^H
            const cd c = gc[i], s = gs[i];
            for (int r = 0; r <= i + 1; ++r) {
                const cd p = h(r, i), q = h(r, i + 1);
                h(r, i) = p * c + q * s;
                h(r, i + 1) = -std::conj(s) * p + std::conj(c) * q;
            }
            for (int r = 0; r < m; ++r) {
                const cd p = v(r, i), q = v(r, i + 1);
                v(r, i) = p * c + q * s;
                v(r, i + 1) = -std::conj(s) * p + std::conj(c) * q;
            }
        }
        for (int i = l; i <= hi; ++i) h(i, i) += mu;
    }
    double tn = 0.0;
    for (int i = 0; i < m; ++i)
        for (int j = i; j < m; ++j) tn = std::max(tn, std::abs(h(i, j)));
    const double small = std::max(eps * tn, 1e-300);
    w.assign(m, cd(0));
    Y.assign((size_t)m * m, cd(0));
    std::vector<cd> x(m);
    for (int k = 0; k < m; ++k) {
        w[k] = h(k, k);
        x[k] = 1.0;
        for (int i = k - 1; i >= 0; --i) {
            cd s = 0.0;
            for (int j = i + 1; j <= k; ++j) s += h(i, j) * x[j];
            cd d = h(i, i) - h(k, k);
            if (std::abs(d) < small) d = small;
            x[i] = -s / d;
        }
        double nn = 0.0;
        for (int i = 0; i < m; ++i) {
            cd s = 0.0;
            for (int j = 0; j <= k; ++j) s += v(i, j) * x[j];
            Y[(size_t)i * m + k] = s;
            nn += std::norm(s);
        }
        nn = std::sqrt(nn);
        if (nn > 0.0 && std::isfinite(nn))
            for (int i = 0; i < m; ++i) Y[(size_t)i * m + k] /= nn;
    }
    return true;
}

// |theta| descending; inside a run of neighbours whose moduli agree to 1e-12 relative, the larger
// imaginary part first (a conjugate pair comes out +imag first)
inline std::vector<int> ritz_order(const std::vector<cd>& w) {
    const int m = (int)w.size();
    std::vector<int> p(m);
    for (int i = 0; i < m; ++i) p[i] = i;
    std::stable_sort(p.begin(), p.end(), [&](int a, int b) { return std::abs(w[a]) > std::abs(w[b]); });
    int i = 0;
    while (i < m) {
        int j = i + 1;
        while (j < m && std::abs(w[p[j - 1]]) - std::abs(w[p[j]]) <= 1e-12 * std::abs(w[p[j - 1]])) ++j;
        std::stable_sort(p.begin() + i, p.begin() + j, [&](int a, int b) { return w[a].imag() > w[b].imag(); });
        i = j;
    }
    return p;
}

template <class T> struct host_of { using type = double; };
template <> struct host_of<cplx> { using type = cd; };

}  // namespace smalleig
}  // namespace eigsol
