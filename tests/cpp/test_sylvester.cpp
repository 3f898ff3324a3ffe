// C++ façade test of EigSol::solve_sylvester on a real case, a complex case and the real case rounded to float
// (promoted to fp64), and of EigSol::solve_lyapunov on one real case: the figure
//   r = ||A X + X op(B) - C||_F / (max(m, n) eps ((||A||_F + ||B||_F) ||X||_F + ||C||_F))
// against the bounds tests/test_gpu_sylvester_facade.py passes in a file.  Same minimal harness as test_schur.cpp.
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

// argv: the real case, the complex case, the Lyapunov case, the bounds.  A case file holds "m n", then A (m * m
// lines "re im", column-major), B (n * n lines; a Lyapunov case has n = 0 and no B) and C (m * n lines; Lyapunov:
// Q, m * m lines).  The bounds file holds three numbers, max(2, 3 r_LAPACK) of the three cases in that order.
static const char* g_argv[5];
static double g_bound[3];

template <typename S>
static EigSol::DenseMatrix<S> read_block(std::ifstream& in, std::int64_t rows, std::int64_t cols) {
    EigSol::DenseMatrix<S> A(rows, cols);
    for (std::int64_t j = 0; j < cols; ++j)
        for (std::int64_t i = 0; i < rows; ++i) {
            double re, im;
            in >> re >> im;
            if constexpr (std::is_same_v<S, C>) A(i, j) = C(re, im);
            else A(i, j) = static_cast<S>(re);
        }
    return A;
}

template <typename S>
struct Case {
    EigSol::DenseMatrix<S> A, B, Cm;
    bool lyapunov = false;
};

template <typename S>
static Case<S> read_case(const char* path) {
    std::ifstream in(path);
    std::int64_t m = 0, n = 0;
    in >> m >> n;
    Case<S> c;
    c.lyapunov = n == 0;
    c.A = read_block<S>(in, m, m);
    if (!c.lyapunov) c.B = read_block<S>(in, n, n);
    c.Cm = read_block<S>(in, m, c.lyapunov ? m : n);
    if (!in || m == 0) throw std::runtime_error(std::string("cannot read ") + path);
    return c;
}

// ||A X + X op(B) - C||_F / ((||A||_F + ||B||_F) ||X||_F + ||C||_F), accumulated in double; op(B) = A^H for Lyapunov
template <typename S>
static double residual(const Case<S>& c, const EigSol::DenseMatrix<S>& X) {
    const std::int64_t m = c.A.rows(), n = X.cols();
    auto opb = [&](std::int64_t k, std::int64_t j) { return c.lyapunov ? std::conj(C(c.A(j, k))) : C(c.B(k, j)); };
    double s = 0, fa = 0, fb = 0, fx = 0, fc = 0;
    for (std::int64_t j = 0; j < n; ++j)
        for (std::int64_t i = 0; i < m; ++i) {
            C acc = -C(c.Cm(i, j));
            for (std::int64_t k = 0; k < m; ++k) acc += C(c.A(i, k)) * C(X(k, j));
            for (std::int64_t k = 0; k < n; ++k) acc += C(X(i, k)) * opb(k, j);
            s += std::norm(acc);
            fx += std::norm(C(X(i, j)));
            fc += std::norm(C(c.Cm(i, j)));
        }
    for (std::int64_t j = 0; j < m; ++j)
        for (std::int64_t i = 0; i < m; ++i) fa += std::norm(C(c.A(i, j)));
    for (std::int64_t j = 0; j < n; ++j)
        for (std::int64_t i = 0; i < n; ++i) fb += std::norm(opb(i, j));
    return std::sqrt(s) / ((std::sqrt(fa) + std::sqrt(fb)) * std::sqrt(fx) + std::sqrt(fc));
}

template <typename S>
static void solve(const char* path, double bound) {
    const Case<S> c = read_case<S>(path);
    const std::int64_t m = c.A.rows(), n = c.Cm.cols();
    const double eps = std::numeric_limits<double>::epsilon();
    const auto res = c.lyapunov ? EigSol::solve_lyapunov<S>(c.A, c.Cm) : EigSol::solve_sylvester<S>(c.A, c.B, c.Cm);
    EXPECT_TRUE(res.X.rows() == m && res.X.cols() == n);
    EXPECT_TRUE(res.converged && res.perturbed == 0);
    bool finite = true;
    for (std::int64_t i = 0; i < res.X.size(); ++i) finite = finite && std::isfinite(std::abs(C(res.X.data()[i])));
    EXPECT_TRUE(finite);
    const double r = residual(c, res.X) / (static_cast<double>(std::max(m, n)) * eps);
    std::printf("  %lld x %lld r=%.4f (<= %.3f)\n", static_cast<long long>(m), static_cast<long long>(n), r, bound);
    EXPECT_TRUE(r <= bound);
    // the same call again: the same bits
    const auto again = c.lyapunov ? EigSol::solve_lyapunov<S>(c.A, c.Cm) : EigSol::solve_sylvester<S>(c.A, c.B, c.Cm);
    bool same = true;
    for (std::int64_t i = 0; i < res.X.size(); ++i) same = same && res.X.data()[i] == again.X.data()[i];
    EXPECT_TRUE(same);
}

static void real_case() { solve<double>(g_argv[1], g_bound[0]); }
static void complex_case() { solve<C>(g_argv[2], g_bound[1]); }
static void lyapunov_case() { solve<double>(g_argv[3], g_bound[2]); }

// The real case rounded to float: solved on the fp64 promotion, X rounded back.  X_f = X + E with
// |E| <= (eps_f / 2) |X| entry by entry, so ||A E + E B||_F <= (eps_f / 2) (||A||_F + ||B||_F) ||X||_F, and
// ||X_f||_F >= (1 - eps_f / 2) ||X||_F: the residual over its denominator is at most (eps_f / 2) (1 + eps_f) plus
// the fp64 solve's own part, which the real case's bound covers.
static void real_case_float() {
    const Case<float> c = read_case<float>(g_argv[1]);
    const std::int64_t m = c.A.rows(), n = c.Cm.cols();
    const double epsf = std::numeric_limits<float>::epsilon(), eps = std::numeric_limits<double>::epsilon();
    const auto res = EigSol::solve_sylvester<float>(c.A, c.B, c.Cm);
    EXPECT_TRUE(res.X.rows() == m && res.X.cols() == n && res.converged && res.perturbed == 0);
    const double rr = residual(c, res.X);
    const double bound = 0.5 * epsf * (1.0 + epsf) + g_bound[0] * static_cast<double>(std::max(m, n)) * eps;
    std::printf("  float residual figure %.3e (<= %.3e)\n", rr, bound);
    EXPECT_TRUE(rr <= bound);
    // the fp64 solve of the promoted matrices, rounded: the same values
    const auto rd = EigSol::solve_sylvester<double>(EigSol::detail::convert_dense<double>(c.A), EigSol::detail::convert_dense<double>(c.B),
                                                    EigSol::detail::convert_dense<double>(c.Cm));
    bool same = true;
    for (std::int64_t i = 0; i < res.X.size(); ++i) same = same && res.X.data()[i] == static_cast<float>(rd.X.data()[i]);
    EXPECT_TRUE(same);
}

static void refusals() {
    const Case<double> c = read_case<double>(g_argv[1]);
    bool threw = false;
    try {
        (void)EigSol::solve_sylvester<double>(c.A, c.B, c.A);   // C of the wrong shape
    } catch (const std::runtime_error&) {
        threw = true;
    }
    EXPECT_TRUE(threw);
    threw = false;
    try {
        (void)EigSol::solve_lyapunov<double>(c.A, c.Cm);
    } catch (const std::runtime_error&) {
        threw = true;
    }
    EXPECT_TRUE(threw);
}

int main(int argc, char** argv) {
    if (argc != 5) {
        std::printf("usage: test_sylvester real.txt complex.txt lyapunov.txt bounds.txt\n");
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
                                                        {"lyapunov_case", lyapunov_case},
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
