// Host build of the scalar logarithms of csrc/small_log.hpp and of the plan of csrc/logm_plan.hpp, for
// tests/test_logm_cpu.py.  Compiled as HIP for the host only; needs no device.
//   input : one record per line:
//             "s re im"                        log_principal
//             "b b11 b21 b12 b22"              log_block2
//             "r l1 l2 t12"                    log_superdiag, real
//             "c l1re l1im l2re l2im t12re t12im"   log_superdiag, complex
//             "p norm tried"                   logm_plan
//             "n m"                            the nodes and weights of degree m
//   output: one line per record: "s": re im;  "b": ok l11 l21 l12 l22 (zeros where ok = 0);  "r": value;
//           "c": re im;  "p": degree;  "n": beta_1 .. beta_m alpha_1 .. alpha_m
#include <cstdio>

#include "logm_plan.hpp"
#include "small_log.hpp"

using namespace eigsol;

int main() {
    char kind;
    while (std::scanf(" %c", &kind) == 1) {
        if (kind == 's') {
            double re, im;
            if (std::scanf("%la %la", &re, &im) != 2) return 2;
            const cplx r = dev::log_principal(cplx{re, im});
            std::printf("%a %a\n", r.re, r.im);
        } else if (kind == 'b') {
            double b[4], l[4] = {0.0, 0.0, 0.0, 0.0};
            if (std::scanf("%la %la %la %la", &b[0], &b[1], &b[2], &b[3]) != 4) return 2;
            const bool ok = dev::log_block2(b[0], b[1], b[2], b[3], l);
            std::printf("%d %a %a %a %a\n", ok ? 1 : 0, l[0], l[1], l[2], l[3]);
        } else if (kind == 'r') {
            double v[3];
            if (std::scanf("%la %la %la", &v[0], &v[1], &v[2]) != 3) return 2;
            std::printf("%a\n", dev::log_superdiag(v[0], v[1], v[2]));
        } else if (kind == 'c') {
            double v[6];
            if (std::scanf("%la %la %la %la %la %la", &v[0], &v[1], &v[2], &v[3], &v[4], &v[5]) != 6) return 2;
            const cplx r = dev::log_superdiag(cplx{v[0], v[1]}, cplx{v[2], v[3]}, cplx{v[4], v[5]});
            std::printf("%a %a\n", r.re, r.im);
        } else if (kind == 'p') {
            double norm;
            int tried;
            if (std::scanf("%la %d", &norm, &tried) != 2) return 2;
            std::printf("%d\n", logm_plan(norm, tried));
        } else if (kind == 'n') {
            int m;
            if (std::scanf("%d", &m) != 1 || m < 1 || m > kLogmMaxDegree) return 2;
            for (int j = 0; j < m; ++j) std::printf("%a ", kLogmBeta[m - 1][j]);
            for (int j = 0; j < m; ++j) std::printf("%a%c", kLogmAlpha[m - 1][j], j + 1 < m ? ' ' : '\n');
        } else {
            return 2;
        }
    }
    return 0;
}
