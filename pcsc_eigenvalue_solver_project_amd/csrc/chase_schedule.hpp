// The chase schedule of the multishift QR sweeps (francis.hip, zfrancis.hip; run by sweep_driver.hpp): plain
// host integer arithmetic, no HIP, checked round by round in tests/test_chase_schedule_cpu.py.
// A sweep on the active block [l, ihi] chases C groups of nbg bulges.  Bulge j of a group sits at row
// k = l + t - 3 j at the group-local step t in [0, Tg); group g runs G global steps behind group g - 1.  A round
// takes every started group through the same number of steps inside one LDS window [s, e) of at most kWin rows
// per group.  A step on the bulge at row k touches the rows and columns max(k - 1, l - 1) .. min(k + 3, ihi), so
// a round ends before the leading live bulge passes kmax.  The spacing G keeps a round's windows disjoint.
#pragma once

#include <algorithm>

namespace eigsol {

struct ChaseGeometry {
    int l, ihi;   // active block
    int C, nbg;   // groups, bulges per group
    int kWin;     // window rows/columns
    int G() const { return kWin + 3 * nbg; }                        // group spacing in steps
    int Tg() const { return (ihi - 1 - l) + 3 * (nbg - 1) + 1; }    // steps of one group
    int T() const { return (C - 1) * G() + Tg(); }                  // steps of the sweep
};

// One window of a round: group g's window [s, e) and its group-local steps [t0, t1).
struct ChaseRoundWin {
    int s, e, t0, t1, g;
};

enum : int { kChaseNoAdvance = -1, kChaseOverlap = -2 };   // internal errors of chase_next_round

// The round that starts at the global step t0 < T(): fills out[0 .. *nwin) (at most C entries, the leading group
// first) and returns the round's end step t1 > t0.  *nwin == 0: every started group is done and the next is not
// yet due; the caller moves on to t1.  A negative value is an internal error.
inline int chase_next_round(const ChaseGeometry& c, int t0, ChaseRoundWin* out, int* nwin) {
    const int G = c.G(), Tg = c.Tg(), l = c.l, ihi = c.ihi, nbg = c.nbg;
    int t1 = c.T(), nw = 0;
    for (int g = 0; g < c.C; ++g) {
        const int tl = t0 - g * G;
        if (tl < 0) { t1 = std::min(t1, g * G); break; }    // later groups start at a round boundary
        if (tl >= Tg) continue;                              // group done
        const int s = tl <= 3 * (nbg - 1) ? std::max(0, l - 1) : std::max(0, l + tl - 3 * (nbg - 1) - 1);
        const int e = std::min(s + c.kWin, ihi + 1);
        const int kmax = (e == ihi + 1) ? ihi - 1 : e - 4;
        int tl1 = tl;
        while (tl1 < Tg) {
            const int blead = std::max(0, (l + tl1 - (ihi - 1) + 2) / 3);   // first bulge not past ihi-1
            if (blead >= nbg) { tl1 = Tg; break; }
            if (l + tl1 - 3 * blead > kmax) break;
            ++tl1;
        }
        t1 = std::min(t1, tl1 + g * G);
        out[nw++] = ChaseRoundWin{s, e, tl, 0, g};
    }
    *nwin = nw;
    if (nw == 0 && t1 > t0) return t1;
    if (t1 <= t0 || nw == 0) return kChaseNoAdvance;
    for (int q = 0; q < nw; ++q) {
        out[q].t1 = t1 - out[q].g * G;
        if (q > 0 && out[q].e > out[q - 1].s) return kChaseOverlap;
    }
    return t1;
}

// The drivers' (C, nbg) plans.
struct ChasePlan {
    int C, nbg;
};

// real (kWin = 96, at most 8 groups): nb bulges whose shifts are at hand, an active block of Nact rows.
// groups of >= 4 bulges; the spacing costs (C - 1) G extra steps, kept below N / 4
inline ChasePlan chase_plan_f64(int nb, int Nact) {
    constexpr int max_groups = 8, kWin = 96;
    const int C = std::max(1, std::min({max_groups, nb / 4, 1 + Nact / (4 * (kWin + 12))}));
    const int nbg = std::min(nb / C, 16);   // one wave per bulge: at most 16 per window
    return ChasePlan{C, nbg};
}
// the real driver's bulge count of a sweep on an active block of N rows (2 nb shifts)
inline int chase_bulges_f64(int N) {
    constexpr int max_bulges = 32;   // bulges per chain
    return std::min(max_bulges, std::max(1, N / 8));
}

// complex (kWin = 64): up to 32 bulges per sweep (64 shifts) in C chains of at most 8 (a chain's 3 nb
// rows must leave its 64-row window room to advance), the chains chased concurrently in disjoint
// windows.  With the AED (round 3) 32 bulges in 4 chains beat 16 in 2: 1024^2 0.31 -> 0.29 s,
// 2048^2 0.93 -> 0.77 s, 4096^2 3.28 -> 2.65 s.  The sweep's shift count is 2 C nbg.
inline ChasePlan chase_plan_c128(int Nact) {
    constexpr int max_nb = 32, max_groups = 4, kWin = 64;
    const int nb = std::min(max_nb, std::max(1, Nact / 16));
    const int C = std::max(1, std::min({max_groups, (nb + 7) / 8, 1 + Nact / (4 * (kWin + 12))}));
    const int nbg = std::max(1, std::min(8, nb / C));
    return ChasePlan{C, nbg};
}

}  // namespace eigsol
