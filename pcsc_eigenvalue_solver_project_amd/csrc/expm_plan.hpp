// Degree and scaling of the matrix exponential (expm.hip; Higham 2005, Table 2.3): host code.
#pragma once

#include <cmath>

namespace eigsol {

constexpr int kExpmDegrees[5] = {3, 5, 7, 9, 13};
// theta_m: the largest ||A||_1 for which the degree-m Pade approximant has backward error below 2^-53
constexpr double kExpmTheta[5] = {1.495585217958292e-2, 2.539398330063230e-1, 9.504178996162932e-1, 2.097847961257068,
                                  5.371920351148152};

// alpha = ||A||_1 >= 0, finite.  The first degree m with alpha <= theta_m and no squaring; else m = 13 and the
// smallest s with alpha 2^-s <= theta_13.  With alpha = f 2^e and theta_13 = g 2^3, f and g in [1/2, 1), that is
// s = e - 3 where f <= g and e - 2 otherwise: a comparison of two doubles, no logarithm to round.
inline void expm_plan(double alpha, int* degree, int* squarings) {
    *squarings = 0;
    for (int q = 0; q < 5; ++q)
        if (alpha <= kExpmTheta[q]) {
            *degree = kExpmDegrees[q];
            return;
        }
    *degree = 13;
    int e = 0, e13 = 0;
    const double f = std::frexp(alpha, &e), g = std::frexp(kExpmTheta[4], &e13);
    *squarings = f <= g ? e - e13 : e - e13 + 1;
}

}  // namespace eigsol
