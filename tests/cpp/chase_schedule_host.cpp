// Host build of the chase schedule (csrc/chase_schedule.hpp), for tests/test_chase_schedule_cpu.py.  Compiled as
// HIP for the host only; needs no device.
//   input : one geometry per line:
//             real N l          the real driver's own plan for an active block of N rows that starts at row l
//             cplx N l          the complex driver's
//             free kWin N l C nbg
//   output: per geometry one line "geo l ihi C nbg kWin", then one line per round with "g s e t0 t1" for each of
//           its windows, then "end STATUS" (0, or the negative internal error of chase_next_round)
#include <cstdio>
#include <cstring>

#include "chase_schedule.hpp"

using namespace eigsol;

int main() {
    char kind[8];
    int N, l;
    while (std::scanf("%7s", kind) == 1) {
        ChaseGeometry c{};
        if (!std::strcmp(kind, "free")) {
            if (std::scanf("%d %d %d %d %d", &c.kWin, &N, &l, &c.C, &c.nbg) != 5) return 2;
        } else {
            if (std::scanf("%d %d", &N, &l) != 2) return 2;
            const bool real = !std::strcmp(kind, "real");
            if (!real && std::strcmp(kind, "cplx")) return 2;
            const ChasePlan p = real ? chase_plan_f64(chase_bulges_f64(N), N) : chase_plan_c128(N);
            c.C = p.C;
            c.nbg = p.nbg;
            c.kWin = real ? 96 : 64;
        }
        c.l = l;
        c.ihi = l + N - 1;
        if (c.C < 1 || c.C > 8) return 2;
        std::printf("geo %d %d %d %d %d\n", c.l, c.ihi, c.C, c.nbg, c.kWin);
        int status = 0;
        for (int t0 = 0; t0 < c.T();) {
            ChaseRoundWin w[8];
            int nwin = 0;
            const int t1 = chase_next_round(c, t0, w, &nwin);
            if (t1 < 0) {
                status = t1;
                break;
            }
            if (nwin > 0) {
                for (int q = 0; q < nwin; ++q)
                    std::printf("%s%d %d %d %d %d", q ? " " : "", w[q].g, w[q].s, w[q].e, w[q].t0, w[q].t1);
                std::printf("\n");
            }
            t0 = t1;
        }
        std::printf("end %d\n", status);
    }
    return 0;
}
