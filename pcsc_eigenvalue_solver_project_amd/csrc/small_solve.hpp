// The dense solve of order 1, 2 or 4 behind the small Sylvester equations (LAPACK dlasy2's method), shared by
// sylvester.hip and ordschur.hip.
#pragma once

#include "kernels_common.hpp"

namespace eigsol {
namespace dev {

// x <- K^-1 x for the leading N x N part (N = 1, 2 or 4) by complete pivoting; a pivot below smin in
// modulus is replaced by smin (returns true).  Every index is a compile-time constant after unrolling.
__host__ __device__ __forceinline__ bool syl_solve4(int N, double (&K)[4][4], double (&x)[4], double smin) {
    bool pert = false;
    int perm[4] = {0, 1, 2, 3};
#pragma unroll
    for (int s = 0; s < 4; ++s) {
        if (s >= N) continue;
        double best = -1.0;
        int pi = s, pj = s;
#pragma unroll
        for (int u = 0; u < 4; ++u)
#pragma unroll
            for (int v = 0; v < 4; ++v)
                if (u >= s && v >= s && u < N && v < N) {
                    const double a = fabs(K[u][v]);
                    if (a > best) {
                        best = a;
                        pi = u;
                        pj = v;
                    }
                }
#pragma unroll
        for (int u = 0; u < 4; ++u)
            if (u > s && u == pi) {
#pragma unroll
                for (int v = 0; v < 4; ++v) {
                    const double tmp = K[s][v];
                    K[s][v] = K[u][v];
                    K[u][v] = tmp;
                }
                const double tmp = x[s];
                x[s] = x[u];
                x[u] = tmp;
            }
#pragma unroll
        for (int v = 0; v < 4; ++v)
            if (v > s && v == pj) {
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    const double tmp = K[u][s];
                    K[u][s] = K[u][v];
                    K[u][v] = tmp;
                }
                const int tp = perm[s];
                perm[s] = perm[v];
                perm[v] = tp;
            }
        if (fabs(K[s][s]) < smin) {
            K[s][s] = smin;
            pert = true;
        }
#pragma unroll
        for (int u = 0; u < 4; ++u)
            if (u > s && u < N) {
                const double f = K[u][s] / K[s][s];
#pragma unroll
                for (int v = 0; v < 4; ++v)
                    if (v > s) K[u][v] -= f * K[s][v];
                x[u] -= f * x[s];
            }
    }
#pragma unroll
    for (int s = 3; s >= 0; --s) {
        if (s >= N) continue;
        double acc = x[s];
#pragma unroll
        for (int v = 0; v < 4; ++v)
            if (v > s && v < N) acc -= K[s][v] * x[v];
        x[s] = acc / K[s][s];
    }
    double y[4] = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
    for (int s = 0; s < 4; ++s)
#pragma unroll
        for (int u = 0; u < 4; ++u)
            if (s < N && perm[s] == u) y[u] = x[s];
#pragma unroll
    for (int u = 0; u < 4; ++u) x[u] = y[u];
    return pert;
}

}  // namespace dev
}  // namespace eigsol
