// C++ façade test of EigSol::svd and EigSol::svdvals on a real and on a complex matrix: shapes, the order of
// s, the phase convention of V, unit columns, svdvals against svd bit for bit, and the argument checks.  U, s
// and V are written out for the caller, which forms the residual, orthogonality and singular value figures.
// Same minimal harness as test_eig.cpp.  Needs a gfx950 device.
#include <eigsol/eigsol.hpp>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
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

// argv: rand97 matrix, where its result goes; the same two for crand65 (tests/test_gpu_svd_facade.py writes
// and reads them).  A matrix file holds "n", then n * n lines "re im", column-major.  A result file holds
// "n sweeps", n lines of s, then U and V as n * n lines "re im" each, column-major.
static const char* g_argv[5];

template <typename S>
static EigSol::DenseMatrix<S> read_dense(const char* path) {
    std::ifstream in(path);
    std::int64_t n = 0;
    in >> n;
    EigSol::DenseMatrix<S> A(n, n);
    for (std::int64_t j = 0; j < n; ++j)
        for (std::int64_t i = 0; i < n; ++i) {
            double re, im;
            in >> re >> im;
            if constexpr (std::is_same_v<S, C>) A(i, j) = C(re, im);
            else A(i, j) = re;
        }
    if (!in || n == 0) throw std::runtime_error(std::string("cannot read ") + path);
    return A;
}

template <typename S>
static void triplets(const char* mpath, const char* opath) {
    const auto A = read_dense<S>(mpath);
    const std::int64_t n = A.rows();
    const double eps = std::numeric_limits<double>::epsilon();
    const auto res = EigSol::svd<S>(A);
    EXPECT_TRUE(static_cast<std::int64_t>(res.s.size()) == n);
    EXPECT_TRUE(res.U.rows() == n && res.U.cols() == n && res.V.rows() == n && res.V.cols() == n);
    EXPECT_TRUE(res.not_converged == 0 && res.sweeps >= 1);
    for (std::int64_t j = 0; j + 1 < n; ++j) EXPECT_TRUE(res.s[static_cast<std::size_t>(j)] >= res.s[static_cast<std::size_t>(j + 1)]);
    for (std::int64_t j = 0; j < n; ++j) {
        double nu = 0, nv = 0, big = 0;
        std::int64_t at = 0;
        for (std::int64_t i = 0; i < n; ++i) {
            nu += std::norm(C(res.U(i, j)));
            nv += std::norm(C(res.V(i, j)));
            if (std::abs(C(res.V(i, j))) > big) { big = std::abs(C(res.V(i, j))); at = i; }
        }
        EXPECT_TRUE(std::abs(std::sqrt(nu) - 1.0) <= 8 * eps * std::sqrt(static_cast<double>(n)));
        EXPECT_TRUE(std::abs(std::sqrt(nv) - 1.0) <= 8 * eps * std::sqrt(static_cast<double>(n)));
        EXPECT_TRUE(C(res.V(at, j)).imag() == 0.0 && C(res.V(at, j)).real() > 0.0);
    }
    // the singular values alone: the same bits
    const auto only = EigSol::svdvals<S>(A);
    EXPECT_TRUE(only.size() == res.s.size() && std::memcmp(only.data(), res.s.data(), only.size() * sizeof(double)) == 0);
    // one sweep is not enough: the result so far comes back with the pairs that were still rotating
    EigSol::SvdOptions one;
    one.maxSweeps = 1;
    const auto part = EigSol::svd<S>(A, one);
    EXPECT_TRUE(part.sweeps == 1 && part.not_converged > 0);
    std::printf("  n=%lld sweeps=%d s_1=%.6g s_n=%.6g\n", static_cast<long long>(n), res.sweeps, res.s.front(), res.s.back());
    std::ofstream out(opath);
    out.precision(17);
    out << n << " " << res.sweeps << "\n";
    for (double v : res.s) out << v << "\n";
    for (const auto* M : {&res.U, &res.V})
        for (std::int64_t j = 0; j < n; ++j)
            for (std::int64_t i = 0; i < n; ++i) out << C((*M)(i, j)).real() << " " << C((*M)(i, j)).imag() << "\n";
    EXPECT_TRUE(static_cast<bool>(out));
}

static void rand97() { triplets<double>(g_argv[1], g_argv[2]); }
static void crand65() { triplets<C>(g_argv[3], g_argv[4]); }

static void arguments() {
    bool threw = false;
    try {
        (void)EigSol::svd<double>(EigSol::DenseMatrix<double>(0, 3));
    } catch (const std::runtime_error& e) {
        threw = std::string(e.what()).find("svd: matrix has zero size") != std::string::npos;
    }
    EXPECT_TRUE(threw);
    threw = false;
    try {
        EigSol::SvdOptions o;
        o.maxSweeps = 0;
        EigSol::DenseMatrix<double> A(2, 2);
        A(0, 0) = A(1, 1) = 1.0;
        (void)EigSol::svdvals<double>(A, o);
    } catch (const std::exception&) {
        threw = true;
    }
    EXPECT_TRUE(threw);
    // a rectangular matrix: shapes of the thin factors
    EigSol::DenseMatrix<double> B(5, 3);
    for (std::int64_t j = 0; j < 3; ++j) B(j, j) = static_cast<double>(j + 1);
    const auto r = EigSol::svd<double>(B);
    EXPECT_TRUE(r.U.rows() == 5 && r.U.cols() == 3 && r.V.rows() == 3 && r.V.cols() == 3);
    EXPECT_TRUE(r.s.size() == 3 && r.s[0] == 3.0 && r.s[1] == 2.0 && r.s[2] == 1.0);
}

int main(int argc, char** argv) {
    if (argc != 5) {
        std::printf("usage: test_svd rand97.txt rand97_out.txt crand65.txt crand65_out.txt\n");
        return 2;
    }
    for (int i = 0; i < 5; ++i) g_argv[i] = argv[i];
    const std::pair<const char*, void (*)()> tests[] = {{"rand97", rand97}, {"crand65", crand65}, {"arguments", arguments}};
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
