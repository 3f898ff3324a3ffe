// C++ façade test of EigSol::sqrtm on a real case with a real root, a complex case, a real case with negative real
// eigenvalues (the root comes back complex) and the first case rounded to float (promoted to fp64): the figure
//   r = ||X^2 - A||_F / (n eps ||X||_F^2)
// against the bounds tests/test_gpu_sqrtm_facade.py passes in a file.  Same minimal harness as test_sylvester.cpp.
// Needs a gfx950 device.
#include <eigsol/eigsol.hpp>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <fstream>
#include <limits>
#include <string>
#include <vector>

static int g_fail = 0, g_checks = 0;
#define EXPECT_TRUE(c)                                                                   \
    do {                                                                                 \
        ++g_checks;                                                                      \
        if (!(c)) { ++g_fail; std::printf("  FAIL %s:%d: %s\n", __FILE__, __LINE__, #c); } \
    } while (0)

using C = std::complex<double>;

// argv: the real case, the complex case, the real case whose root is complex, the bounds.  A case file holds "n",
// then A (n * n lines "re im", column-major).  The bounds file holds max(2, 3 r_SciPy) of the three cases.
static const char* g_argv[5];
static double g_bound[3];

template <typename S>
static EigSol::DenseMatrix<S> read_case(const char* path) {
    std::ifstream in(path);
    std::int64_t n = 0;
    in >> n;
    EigSol::DenseMatrix<S> A(n, n);
    for (std::int64_t j = 0; j < n; ++j)
        for (std::int64_t i = 0; i < n; ++i) {
            double re, im;
            in >> re >> im;
            if constexpr (std::is_same_v<S, C>) A(i, j) = C(re, im);
            else A(i, j) = static_cast<S>(re);
        }
    if (!in || n == 0) throw std::runtime_error(std::string("cannot read ") + path);
    return A;
}

// ||X^2 - A||_F / ||X||_F^2, accumulated in double
template <typename S, typename X>
static double residual(const EigSol::DenseMatrix<S>& A, const EigSol::DenseMatrix<X>& Xm) {
    const std::int64_t n = A.rows();
    double s = 0, fx = 0;
    for (std::int64_t j = 0; j < n; ++j)
        for (std::int64_t i = 0; i < n; ++i) {
            C acc = -C(A(i, j));
            for (std::int64_t k = 0; k < n; ++k) acc += C(Xm(i, k)) * C(Xm(k, j));
            s += std::norm(acc);
            fx += std::norm(C(Xm(i, j)));
        }
    return std::sqrt(s) / fx;
}

template <typename M>
static bool all_finite(const M& Xm) {
    bool finite = true;
    for (std::int64_t i = 0; i < Xm.size(); ++i) finite = finite && std::isfinite(std::abs(C(Xm.data()[i])));
    return finite;
}

template <typename S>
static void root_in_place(const char* path, double bound) {
    const EigSol::DenseMatrix<S> A = read_case<S>(path);
    const std::int64_t n = A.rows();
    const double eps = std::numeric_limits<double>::epsilon();
    const auto res = EigSol::sqrtm<S>(A);
    EXPECT_TRUE(!res.isComplex && res.Xc.size() == 0);
    EXPECT_TRUE(res.X.rows() == n && res.X.cols() == n);
    EXPECT_TRUE(res.converged && res.perturbed == 0);
    EXPECT_TRUE(all_finite(res.X));
    const double r = residual(A, res.X) / (static_cast<double>(n) * eps);
    std::printf("  order %lld r=%.4f (<= %.3f)\n", static_cast<long long>(n), r, bound);
    EXPECT_TRUE(r <= bound);
    const auto again = EigSol::sqrtm<S>(A);   // the same call again: the same bits
    bool same = true;
    for (std::int64_t i = 0; i < res.X.size(); ++i) same = same && res.X.data()[i] == again.X.data()[i];
    EXPECT_TRUE(same);
}

static void real_case() { root_in_place<double>(g_argv[1], g_bound[0]); }
static void complex_case() { root_in_place<C>(g_argv[2], g_bound[1]); }

// a real matrix with negative real eigenvalues: the root is complex and equals the root of A passed as complex
static void real_case_complex_root() {
    const EigSol::DenseMatrix<double> A = read_case<double>(g_argv[3]);
    const std::int64_t n = A.rows();
    const double eps = std::numeric_limits<double>::epsilon();
    const auto res = EigSol::sqrtm<double>(A);
    EXPECT_TRUE(res.isComplex && res.X.size() == 0);
    EXPECT_TRUE(res.Xc.rows() == n && res.Xc.cols() == n);
    EXPECT_TRUE(res.converged && res.perturbed == 0);
    EXPECT_TRUE(all_finite(res.Xc));
    const double r = residual(A, res.Xc) / (static_cast<double>(n) * eps);
    std::printf("  order %lld r=%.4f (<= %.3f), complex root\n", static_cast<long long>(n), r, g_bound[2]);
    EXPECT_TRUE(r <= g_bound[2]);
    const auto rc = EigSol::sqrtm<C>(EigSol::detail::convert_dense<C>(A));
    bool same = !rc.isComplex && rc.X.size() == res.Xc.size();
    for (std::int64_t i = 0; same && i < res.Xc.size(); ++i) same = res.Xc.data()[i] == rc.X.data()[i];
    EXPECT_TRUE(same);
}

// The real case rounded to float: the root of the fp64 promotion, rounded back.  X_f = X + E with
// |E| <= (eps_f / 2) |X| entry by entry, so ||X_f^2 - A||_F <= ||X^2 - A||_F + eps_f (1 + eps_f / 4) ||X||_F^2 and
// ||X_f||_F >= (1 - eps_f / 2) ||X||_F: the residual over ||X_f||_F^2 is at most eps_f (1 + 2 eps_f) plus the fp64
// root's own part, which the real case's bound covers.
static void real_case_float() {
    const EigSol::DenseMatrix<float> A = read_case<float>(g_argv[1]);
    const std::int64_t n = A.rows();
    const double epsf = std::numeric_limits<float>::epsilon(), eps = std::numeric_limits<double>::epsilon();
    const auto res = EigSol::sqrtm<float>(A);
    EXPECT_TRUE(!res.isComplex && res.X.rows() == n && res.X.cols() == n && res.converged && res.perturbed == 0);
    const double rr = residual(A, res.X);
    const double bound = epsf * (1.0 + 2.0 * epsf) + g_bound[0] * static_cast<double>(n) * eps * (1.0 + 2.0 * epsf);
    std::printf("  float residual figure %.3e (<= %.3e)\n", rr, bound);
    EXPECT_TRUE(rr <= bound);
    const auto rd = EigSol::sqrtm<double>(EigSol::detail::convert_dense<double>(A));   // the promoted root, rounded: the same values
    bool same = !rd.isComplex;
    for (std::int64_t i = 0; same && i < res.X.size(); ++i) same = res.X.data()[i] == static_cast<float>(rd.X.data()[i]);
    EXPECT_TRUE(same);
}

static void refusals() {
    bool threw = false;
    try {
        (void)EigSol::sqrtm<double>(EigSol::DenseMatrix<double>(3, 4));
    } catch (const std::runtime_error&) {
        threw = true;
    }
    EXPECT_TRUE(threw);
    threw = false;
    try {
        (void)EigSol::sqrtm<long double>(EigSol::DenseMatrix<long double>(3, 3));
    } catch (const std::runtime_error&) {
        threw = true;
    }
    EXPECT_TRUE(threw);
}

int main(int argc, char** argv) {
    if (argc != 5) {
        std::printf("usage: test_sqrtm real.txt complex.txt real_complex_root.txt bounds.txt\n");
        return 2;
    }
    for (int i = 0; i < 5; ++i) g_argv[i] = argv[i];
    {
        std::ifstream in(argv[4]);
        in >> g_bound[0] >> g_bound[1] >> g_bound[2];
        if (!in) {
            std::printf("cannot read %s\n", argv[4]);
            return 2;
        }
    }
    const std::pair<const char*, void (*)()> tests[] = {{"real_case", real_case},
                                                        {"complex_case", complex_case},
                                                        {"real_case_complex_root", real_case_complex_root},
                                                        {"real_case_float", real_case_float},
                                                        {"refusals", refusals}};
    for (const auto& [name, fn] : tests) {
        const int before = g_fail;
        try {
            fn();
        } catch (const std::exception& e) {
            ++g_fail;
            std::printf("  FAIL %s: unexpected exception: %s\n", name, e.what());
        }
        std::printf("%s %s\n", g_fail == before ? "[ OK ]" : "[FAIL]", name);
    }
    std::printf("%d checks, %d failures\n", g_checks, g_fail);
    if (g_fail == 0) std::printf("ALL PASSED\n");
    return g_fail == 0 ? 0 : 1;
}
