// Host build of the scalar roots of csrc/small_sqrt.hpp, for tests/test_small_sqrt_cpu.py.  Compiled as HIP for
// the host only; needs no device.
//   input : one record per line: "s re im" (sqrt_principal) or "b b11 b21 b12 b22" (sqrt_block2)
//   output: one line per record: "s": re im;  "b": ok u11 u21 u12 u22 (zeros where ok = 0)
#include <cstdio>

#include "small_sqrt.hpp"

using namespace eigsol;

int main() {
    char kind;
    while (std::scanf(" %c", &kind) == 1) {
        if (kind == 's') {
            double re, im;
            if (std::scanf("%la %la", &re, &im) != 2) return 2;
            const cplx r = dev::sqrt_principal(cplx{re, im});
            std::printf("%a %a\n", r.re, r.im);
        } else if (kind == 'b') {
            double b[4], u[4] = {0.0, 0.0, 0.0, 0.0};
            if (std::scanf("%la %la %la %la", &b[0], &b[1], &b[2], &b[3]) != 4) return 2;
            const bool ok = dev::sqrt_block2(b[0], b[1], b[2], b[3], u);
            std::printf("%d %a %a %a %a\n", ok ? 1 : 0, u[0], u[1], u[2], u[3]);
        } else {
            return 2;
        }
    }
    return 0;
}
