// When the root loop of the matrix logarithm stops, and the Pade degree it stops with (logm.hip; Higham, Functions
// of Matrices, Alg. 11.9, with the bounds of Al-Mohy and Higham (2012) applied to the 1-norm): host code.
#pragma once

namespace eigsol {

constexpr int kLogmMaxDegree = 7;
constexpr int kLogmMaxRoots = 64;
// theta_m: the largest ||R|| for which the degree-m Pade approximant of log(I + R) has backward error below 2^-53
constexpr double kLogmTheta[kLogmMaxDegree] = {1.59e-5, 2.31e-3, 1.94e-2, 6.21e-2, 1.28e-1, 2.06e-1, 2.88e-1};

// norm = ||R||_1 >= 0 with R = T^(1/2^s) - I.  Returns the degree m to stop with, or 0: take another root.
//   norm > theta_7 (or NaN): another root;
//   else j1 = min{m : norm <= theta_m}, j2 = min{m : norm / 2 <= theta_m}: one more root would about halve the
//   norm; it pays only if it saves more than one degree.  Stop with j1 if j1 - j2 <= 1, or if this test was
//   reached before (tried != 0); else another root.
inline int logm_plan(double norm, int tried) {
    if (!(norm <= kLogmTheta[kLogmMaxDegree - 1])) return 0;
    int j1 = 1, j2 = 1;
    while (norm > kLogmTheta[j1 - 1]) ++j1;
    while (norm / 2.0 > kLogmTheta[j2 - 1]) ++j2;
    return (j1 - j2 <= 1 || tried) ? j1 : 0;
}

// beta_j (nodes) and alpha_j (weights) of the m-point Gauss-Legendre rule on [0, 1], m = 1 .. 7, row m - 1:
//   r_m(x) = sum_j alpha_j x / (1 + beta_j x)  is the [m / m] Pade approximant of log(1 + x).
constexpr double kLogmBeta[kLogmMaxDegree][kLogmMaxDegree] = {
    {0.5},
    {0.21132486540518712, 0.78867513459481288},
    {0.11270166537925831, 0.5, 0.88729833462074169},
    {0.069431844202973712, 0.33000947820757187, 0.66999052179242813, 0.93056815579702629},
    {0.046910077030668004, 0.23076534494715845, 0.5, 0.76923465505284155, 0.953089922969332},
    {0.033765242898423986, 0.16939530676686774, 0.38069040695840155, 0.61930959304159845, 0.83060469323313226,
     0.96623475710157601},
    {0.025446043828620738, 0.12923440720030278, 0.29707742431130142, 0.5, 0.70292257568869858, 0.87076559279969722,
     0.97455395617137926}};
constexpr double kLogmAlpha[kLogmMaxDegree][kLogmMaxDegree] = {
    {1.0},
    {0.5, 0.5},
    {0.27777777777777778, 0.44444444444444444, 0.27777777777777778},
    {0.17392742256872693, 0.32607257743127307, 0.32607257743127307, 0.17392742256872693},
    {0.11846344252809454, 0.23931433524968323, 0.28444444444444444, 0.23931433524968323, 0.11846344252809454},
    {0.085662246189585173, 0.1803807865240693, 0.23395696728634552, 0.23395696728634552, 0.1803807865240693,
     0.085662246189585173},
    {0.064742483084434847, 0.13985269574463833, 0.19091502525255947, 0.20897959183673469, 0.19091502525255947,
     0.13985269574463833, 0.064742483084434847}};

}  // namespace eigsol
