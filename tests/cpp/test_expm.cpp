// C++ façade test of EigSol::expm and EigSol::solve on one real and one complex case, and on the real case rounded
// to float (promoted to fp64).  tests/test_gpu_expm_facade.py passes, per case, A, the exponential to compare with
// (scipy.linalg.expm) and the bound on g = ||X - X_ref||_F / ||X_ref||_F; solve is checked by its residual.  Same
// minimal harness as test_sqrtm.cpp.  Needs a gfx950 device.
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

// argv: the real case, the complex case.  A case file holds "n degree squarings bound solve_bound", then A and X_ref
// (each n * n lines "re im", column-major).
static const char* g_argv[3];

template <typename S>
struct Case {
    EigSol::DenseMatrix<S> A, Xref;
    int degree = 0, squarings = 0;
    double bound = 0, solve_bound = 0;
};

template <typename S>
static Case<S> read_case(const char* path) {
    std::ifstream in(path);
    std::int64_t n = 0;
    Case<S> c;
    in >> n >> c.degree >> c.squarings >> c.bound >> c.solve_bound;
    c.A = EigSol::DenseMatrix<S>(n, n);
    c.Xref = EigSol::DenseMatrix<S>(n, n);
    for (EigSol::DenseMatrix<S>* M : {&c.A, &c.Xref})
        for (std::int64_t j = 0; j < n; ++j)
            for (std::int64_t i = 0; i < n; ++i) {
                double re, im;
                in >> re >> im;
                if constexpr (std::is_same_v<S, C>) (*M)(i, j) = C(re, im);
                else (*M)(i, j) = static_cast<S>(re);
            }
    if (!in || n == 0) throw std::runtime_error(std::string("cannot read ") + path);
    return c;
}

template <typename M1, typename M2>
static double gap(const M1& Xm, const M2& Ref) {
    double s = 0, f = 0;
    for (std::int64_t i = 0; i < Ref.size(); ++i) {
        s += std::norm(C(Xm.data()[i]) - C(Ref.data()[i]));
        f += std::norm(C(Ref.data()[i]));
    }
    return std::sqrt(s / f);
}

template <typename S>
static void expm_case(const char* path) {
    const Case<S> c = read_case<S>(path);
    const std::int64_t n = c.A.rows();
    const auto res = EigSol::expm<S>(c.A);
    EXPECT_TRUE(res.X.rows() == n && res.X.cols() == n);
    EXPECT_TRUE(res.degree == c.degree && res.squarings == c.squarings);
    const double g = gap(res.X, c.Xref);
    std::printf("  order %lld g=%.3e (<= %.3e), degree %d, squarings %d\n", static_cast<long long>(n), g, c.bound, res.degree,
                res.squarings);
    EXPECT_TRUE(std::isfinite(g) && g <= c.bound);
    const auto again = EigSol::expm<S>(c.A);   // the same call again: the same bits
    bool same = true;
    for (std::int64_t i = 0; i < res.X.size(); ++i) same = same && res.X.data()[i] == again.X.data()[i];
    EXPECT_TRUE(same);
}

// A Y = exp(A): the figure of tests/test_gpu_solve.py, max_j ||A y_j - b_j||_inf / ((||A||_inf ||y_j||_inf +
// ||b_j||_inf) n eps) with the residual in long double, against the bound the case file carries
template <typename S>
static void solve_case(const char* path) {
    const Case<S> c = read_case<S>(path);
    const std::int64_t n = c.A.rows();
    const auto X = EigSol::solve<S>(c.A, c.Xref);
    EXPECT_TRUE(X.rows() == n && X.cols() == n);
    double an = 0;
    for (std::int64_t i = 0; i < n; ++i) {
        double r = 0;
        for (std::int64_t j = 0; j < n; ++j) r += std::abs(C(c.A(i, j)));
        an = std::max(an, r);
    }
    double worst = 0;
    for (std::int64_t j = 0; j < n; ++j) {
        double res = 0, xn = 0, bn = 0;
        for (std::int64_t i = 0; i < n; ++i) {
            std::complex<long double> acc = -std::complex<long double>(C(c.Xref(i, j)));
            for (std::int64_t k = 0; k < n; ++k) acc += std::complex<long double>(C(c.A(i, k))) * std::complex<long double>(C(X(k, j)));
            res = std::max(res, static_cast<double>(std::abs(acc)));
            xn = std::max(xn, std::abs(C(X(i, j))));
            bn = std::max(bn, std::abs(C(c.Xref(i, j))));
        }
        worst = std::max(worst, res / ((an * xn + bn) * static_cast<double>(n) * std::numeric_limits<double>::epsilon()));
    }
    std::printf("  solve order %lld figure %.3f (<= %.3f)\n", static_cast<long long>(n), worst, c.solve_bound);
    EXPECT_TRUE(worst <= c.solve_bound);
}

static void real_case() { expm_case<double>(g_argv[1]); }
static void complex_case() { expm_case<C>(g_argv[2]); }
static void real_solve() { solve_case<double>(g_argv[1]); }
static void complex_solve() { solve_case<C>(g_argv[2]); }

// The real case rounded to float: the results are those of the fp64 promotion, rounded back.
static void float_promotion() {
    const Case<float> c = read_case<float>(g_argv[1]);
    const auto res = EigSol::expm<float>(c.A);
    const auto rd = EigSol::expm<double>(EigSol::detail::convert_dense<double>(c.A));
    EXPECT_TRUE(res.degree == rd.degree && res.squarings == rd.squarings);
    bool same = res.X.size() == rd.X.size();
    for (std::int64_t i = 0; same && i < res.X.size(); ++i) same = res.X.data()[i] == static_cast<float>(rd.X.data()[i]);
    EXPECT_TRUE(same);
    const auto xs = EigSol::solve<float>(c.A, c.Xref);
    const auto xd = EigSol::solve<double>(EigSol::detail::convert_dense<double>(c.A), EigSol::detail::convert_dense<double>(c.Xref));
    same = xs.size() == xd.size();
    for (std::int64_t i = 0; same && i < xs.size(); ++i) same = xs.data()[i] == static_cast<float>(xd.data()[i]);
    EXPECT_TRUE(same);
}

static void refusals() {
    auto throws = [](auto&& fn) {
        try {
            fn();
        } catch (const std::runtime_error&) {
            return true;
        }
        return false;
    };
    EXPECT_TRUE(throws([] { (void)EigSol::expm<double>(EigSol::DenseMatrix<double>(3, 4)); }));
    EXPECT_TRUE(throws([] { (void)EigSol::expm<long double>(EigSol::DenseMatrix<long double>(3, 3)); }));
    EXPECT_TRUE(throws([] { (void)EigSol::solve<double>(EigSol::DenseMatrix<double>(3, 3), EigSol::DenseMatrix<double>(4, 1)); }));
    EigSol::DenseMatrix<double> Z(3, 3), B(3, 1);   // the zero matrix is singular: the pivot of column 0
    bool named = false;
    try {
        (void)EigSol::solve<double>(Z, B);
    } catch (const std::runtime_error& e) {
        named = std::string(e.what()).find("column 0 ") != std::string::npos;
    }
    EXPECT_TRUE(named);
}

int main(int argc, char** argv) {
    if (argc != 3) {
        std::printf("usage: test_expm real.txt complex.txt\n");
        return 2;
    }
    for (int i = 0; i < 3; ++i) g_argv[i] = argv[i];
    const std::pair<const char*, void (*)()> tests[] = {{"real_case", real_case},         {"complex_case", complex_case},
                                                        {"real_solve", real_solve},       {"complex_solve", complex_solve},
                                                        {"float_promotion", float_promotion}, {"refusals", refusals}};
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
