// Host build of syl_solve4 (csrc/small_solve.hpp), for tests/test_small_solve_cpu.py.  Compiled as HIP for the
// host only; needs no device.
//   input : one system per record: N (1, 2 or 4), smin, the N * N entries of K row by row, the N entries of x
//   output: one line per record: the flag (1: a pivot was replaced by smin), then the N entries of the solution
#include <cstdio>

#include "small_solve.hpp"

using namespace eigsol;

int main() {
    int N;
    double smin;
    while (std::scanf("%d %lf", &N, &smin) == 2) {
        if (N != 1 && N != 2 && N != 4) return 2;
        double K[4][4] = {{0.0}}, x[4] = {0.0, 0.0, 0.0, 0.0};
        for (int u = 0; u < N; ++u)
            for (int v = 0; v < N; ++v)
                if (std::scanf("%lf", &K[u][v]) != 1) return 2;
        for (int u = 0; u < N; ++u)
            if (std::scanf("%lf", &x[u]) != 1) return 2;
        const bool pert = dev::syl_solve4(N, K, x, smin);
        std::printf("%d", pert ? 1 : 0);
        for (int u = 0; u < N; ++u) std::printf(" %.17g", x[u]);
        std::printf("\n");
    }
    return 0;
}
