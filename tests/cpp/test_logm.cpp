// C++ façade test of EigSol::logm on a real case with a real logarithm, a complex case, a real case with negative
// real eigenvalues (the logarithm comes back complex) and the first case rounded to float (promoted to fp64).  The
// test writes every logarithm to a file; tests/test_gpu_logm_facade.py forms the figure e of tests/logm_ref.py from
// them.  Here: shapes, flags, the same bits from a second call, the complex rerun against the complex call, the
// float result against the rounded fp64 one, and the refusals.  Same minimal harness as test_sqrtm.cpp.
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

// argv: the real case, the complex case, the real case whose logarithm is complex, the output prefix.  A case file
// holds "n", then A (n * n lines "re im", column-major); an output file has the same layout.
static const char* g_argv[5];

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

template <typename M>
static void write_result(const std::string& path, const M& X) {
    std::FILE* f = std::fopen(path.c_str(), "w");
    if (!f) throw std::runtime_error("cannot write " + path);
    std::fprintf(f, "%lld\n", static_cast<long long>(X.rows()));
    for (std::int64_t i = 0; i < X.size(); ++i) {
        const C v(X.data()[i]);
        std::fprintf(f, "%.17g %.17g\n", v.real(), v.imag());
    }
    std::fclose(f);
}

template <typename M>
static bool all_finite(const M& Xm) {
    bool finite = true;
    for (std::int64_t i = 0; i < Xm.size(); ++i) finite = finite && std::isfinite(std::abs(C(Xm.data()[i])));
    return finite;
}

template <typename S>
static void log_in_place(const char* path, const char* tag) {
    const EigSol::DenseMatrix<S> A = read_case<S>(path);
    const std::int64_t n = A.rows();
    const auto res = EigSol::logm<S>(A);
    EXPECT_TRUE(!res.isComplex && res.Xc.size() == 0);
    EXPECT_TRUE(res.X.rows() == n && res.X.cols() == n);
    EXPECT_TRUE(res.converged && res.perturbed == 0);
    EXPECT_TRUE(res.roots >= 1 && res.roots <= 64 && res.degree >= 1 && res.degree <= 7);
    EXPECT_TRUE(all_finite(res.X));
    std::printf("  order %lld roots %d degree %d\n", static_cast<long long>(n), res.roots, res.degree);
    write_result(std::string(g_argv[4]) + tag, res.X);
    const auto again = EigSol::logm<S>(A);   // the same call again: the same bits
    bool same = again.roots == res.roots && again.degree == res.degree;
    for (std::int64_t i = 0; i < res.X.size(); ++i) same = same && res.X.data()[i] == again.X.data()[i];
    EXPECT_TRUE(same);
}

static void real_case() { log_in_place<double>(g_argv[1], "real.txt"); }
static void complex_case() { log_in_place<C>(g_argv[2], "complex.txt"); }

// a real matrix with negative real eigenvalues: the logarithm is complex and equals that of A passed as complex
static void real_case_complex_log() {
    const EigSol::DenseMatrix<double> A = read_case<double>(g_argv[3]);
    const std::int64_t n = A.rows();
    const auto res = EigSol::logm<double>(A);
    EXPECT_TRUE(res.isComplex && res.X.size() == 0);
    EXPECT_TRUE(res.Xc.rows() == n && res.Xc.cols() == n);
    EXPECT_TRUE(res.converged && res.perturbed == 0);
    EXPECT_TRUE(all_finite(res.Xc));
    write_result(std::string(g_argv[4]) + "real_complex_log.txt", res.Xc);
    const auto rc = EigSol::logm<C>(EigSol::detail::convert_dense<C>(A));
    bool same = !rc.isComplex && rc.X.size() == res.Xc.size() && rc.roots == res.roots && rc.degree == res.degree;
    for (std::int64_t i = 0; same && i < res.Xc.size(); ++i) same = res.Xc.data()[i] == rc.X.data()[i];
    EXPECT_TRUE(same);
}

// The real case rounded to float: the logarithm of the fp64 promotion, rounded back
static void real_case_float() {
    const EigSol::DenseMatrix<float> A = read_case<float>(g_argv[1]);
    const std::int64_t n = A.rows();
    const auto res = EigSol::logm<float>(A);
    EXPECT_TRUE(!res.isComplex && res.X.rows() == n && res.X.cols() == n && res.converged && res.perturbed == 0);
    const auto rd = EigSol::logm<double>(EigSol::detail::convert_dense<double>(A));
    bool same = !rd.isComplex && rd.roots == res.roots && rd.degree == res.degree;
    for (std::int64_t i = 0; same && i < res.X.size(); ++i) same = res.X.data()[i] == static_cast<float>(rd.X.data()[i]);
    EXPECT_TRUE(same);
}

static void refusals() {
    bool threw = false;
    try {
        (void)EigSol::logm<double>(EigSol::DenseMatrix<double>(3, 4));
    } catch (const std::runtime_error&) {
        threw = true;
    }
    EXPECT_TRUE(threw);
    threw = false;
    try {
        (void)EigSol::logm<long double>(EigSol::DenseMatrix<long double>(3, 3));
    } catch (const std::runtime_error&) {
        threw = true;
    }
    EXPECT_TRUE(threw);
    threw = false;
    try {   // singular
        EigSol::DenseMatrix<double> Z(2, 2);
        Z(0, 0) = 2.0;
        Z(0, 1) = Z(1, 0) = Z(1, 1) = 0.0;
        (void)EigSol::logm<double>(Z);
    } catch (const std::runtime_error&) {
        threw = true;
    }
    EXPECT_TRUE(threw);
}

int main(int argc, char** argv) {
    if (argc != 5) {
        std::printf("usage: test_logm real.txt complex.txt real_complex_log.txt output_prefix\n");
        return 2;
    }
    for (int i = 0; i < 5; ++i) g_argv[i] = argv[i];
    const std::pair<const char*, void (*)()> tests[] = {{"real_case", real_case},
                                                        {"complex_case", complex_case},
                                                        {"real_case_complex_log", real_case_complex_log},
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
