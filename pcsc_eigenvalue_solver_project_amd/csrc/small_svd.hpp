// Host SVD of the small projected matrix of the Golub-Kahan-Lanczos driver (svds.hip): one-sided
// Jacobi (Hestenes) on a matrix of order <= 65, real or complex.  Host code only.
#pragma once

#include <algorithm>
#include <cmath>
#include <complex>
#include <numeric>
#include <vector>

namespace eigsol {
namespace smallsvd {

using cd = std::complex<double>;

inline double conj_s(double v) { return v; }
inline cd conj_s(cd v) { return std::conj(v); }
inline double abs2_s(double v) { return v * v; }
inline double abs2_s(cd v) { return std::norm(v); }

// G = L diag(s) R^H for G (r x c, column-major, r >= c; destroyed): s descending, L (r x c) with
// orthonormal columns, R (c x c) unitary.  Column pairs are rotated until every pair satisfies
// |g_p^H g_q| <= sqrt(r) 2^-52 ||g_p|| ||g_q||; then s_i = ||g_i|| and l_i = g_i / s_i.  A column whose norm is
// at most 2^-52 r s_0 (a singular value that is zero to working precision) gets a unit vector
// orthogonal to the other columns of L, so that L is orthonormal for a rank-deficient G too.
// false: the sweeps did not converge, or G is not finite.
template <class T>
bool jacobi_svd(int r, int c, std::vector<T>& G, std::vector<double>& s, std::vector<T>& L, std::vector<T>& R) {
    const double eps = 0x1p-52, tol = std::sqrt((double)r) * eps;
    std::vector<T> J((size_t)c * c, T(0));
    for (int i = 0; i < c; ++i) J[(size_t)i * c + i] = T(1);
    for (const T& g : G)
        if (!std::isfinite(std::abs(g))) return false;
    bool done = false;
    for (int sweep = 0; sweep < 60 && !done; ++sweep) {
        done = true;
        for (int p = 0; p + 1 < c; ++p)
            for (int q = p + 1; q < c; ++q) {
                T* gp = &G[(size_t)p * r];
                T* gq = &G[(size_t)q * r];
                double a = 0.0, b = 0.0;
                T g = T(0);
                for (int i = 0; i < r; ++i) {
                    a += abs2_s(gp[i]);
                    b += abs2_s(gq[i]);
                    g += conj_s(gp[i]) * gq[i];
                }
                const double ag = std::abs(g);
                if (!(ag > tol * std::sqrt(a) * std::sqrt(b)) || ag == 0.0) continue;
                done = false;
                const T ph = conj_s(g) / ag;          // g_q ph: the inner product with g_p becomes |g|
                const double zeta = (b - a) / (2.0 * ag);
                const double t = (zeta >= 0.0 ? 1.0 : -1.0) / (std::abs(zeta) + std::hypot(1.0, zeta));
                const double cs = 1.0 / std::hypot(1.0, t), sn = cs * t;
                for (int i = 0; i < r; ++i) {
                    const T x = gp[i], y = gq[i] * ph;
                    gp[i] = cs * x - sn * y;
                    gq[i] = sn * x + cs * y;
                }
                T* jp = &J[(size_t)p * c];
                T* jq = &J[(size_t)q * c];
                for (int i = 0; i < c; ++i) {
                    const T x = jp[i], y = jq[i] * ph;
                    jp[i] = cs * x - sn * y;
                    jq[i] = sn * x + cs * y;
                }
            }
    }
    if (!done) return false;
    std::vector<double> nrm(c);
    for (int j = 0; j < c; ++j) {
        double mx = 0.0;
        for (int i = 0; i < r; ++i) mx = std::max(mx, std::abs(G[(size_t)j * r + i]));
        double a = 0.0;
        if (mx > 0.0)
            for (int i = 0; i < r; ++i) a += abs2_s(G[(size_t)j * r + i] / mx);
        nrm[j] = mx * std::sqrt(a);
    }
    std::vector<int> perm(c);
    std::iota(perm.begin(), perm.end(), 0);
    std::stable_sort(perm.begin(), perm.end(), [&](int x, int y) { return nrm[x] > nrm[y]; });
    s.assign(c, 0.0);
    L.assign((size_t)r * c, T(0));
    R.assign((size_t)c * c, T(0));
    const double floor = eps * r * (c ? nrm[perm[0]] : 0.0);
    for (int j = 0; j < c; ++j) {
        const int src = perm[j];
        s[j] = nrm[src];
        for (int i = 0; i < c; ++i) R[(size_t)j * c + i] = J[(size_t)src * c + i];
        if (nrm[src] > floor)
            for (int i = 0; i < r; ++i) L[(size_t)j * r + i] = G[(size_t)src * r + i] / nrm[src];
    }
    // complete L over the columns at or below the floor: the unit vector least represented so far
    for (int j = 0; j < c; ++j) {
        if (s[j] > floor) continue;
        T* lj = &L[(size_t)j * r];
        bool ok = false;
        for (int e = 0; e < r && !ok; ++e) {
            for (int i = 0; i < r; ++i) lj[i] = T(i == e ? 1 : 0);
            for (int pass = 0; pass < 2; ++pass)
                for (int o = 0; o < c; ++o) {
                    if (o == j || (o > j && !(s[o] > floor))) continue;   // later completed columns are not set yet
                    const T* lo = &L[(size_t)o * r];
                    T d = T(0);
                    for (int i = 0; i < r; ++i) d += conj_s(lo[i]) * lj[i];
                    for (int i = 0; i < r; ++i) lj[i] -= lo[i] * d;
                }
            double a = 0.0;
            for (int i = 0; i < r; ++i) a += abs2_s(lj[i]);
            a = std::sqrt(a);
            if (a > 0.5 / std::sqrt((double)r)) {
                for (int i = 0; i < r; ++i) lj[i] /= a;
                ok = true;
            }
        }
        if (!ok) return false;
    }
    return true;
}

}  // namespace smallsvd
}  // namespace eigsol
