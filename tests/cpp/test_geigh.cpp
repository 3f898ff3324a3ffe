// C++ façade tests of EigSol::eigh(A, B), EigSol::eigvalsh(A, B) and EigSol::cholesky(B) (the generalised
// symmetric-definite eigensolver; no counterpart in the reference).  Same minimal harness as test_eigh.cpp.
// Needs a gfx950 device at run time.
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
// stmt must throw std::runtime_error whose message is exactly msg
#define EXPECT_MESSAGE(stmt, msg)                                                        \
    do {                                                                                 \
        std::string got_ = "(nothing thrown)";                                           \
        try { stmt; } catch (const std::runtime_error& e) { got_ = e.what(); }           \
        ++g_checks;                                                                      \
        if (got_ != (msg)) { ++g_fail; std::printf("  FAIL %s:%d: got \"%s\"\n", __FILE__, __LINE__, got_.c_str()); } \
    } while (0)

using C = std::complex<double>;

// argv: gsym97 A, B, expectations, gherm70 A, B, expectations (tests/test_gpu_geigh_facade.py writes them from
// tests/geigh_ref.py).  A matrix file holds "n", then n * n lines "re im", column-major.  An expectation file
// holds one line "value_bound r_bound o_bound c_bound cond_B" (the conditions of tests/test_gpu_geigh.py and
// tests/test_gpu_cholesky.py), then the reference eigenvalues, ascending, one per line.
static const char* g_argv[7];

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

struct Expect {
    double value_bound = 0, r_bound = 0, o_bound = 0, c_bound = 0, cond_b = 0;
    std::vector<double> w;
};
static Expect read_expect(const char* path) {
    std::ifstream in(path);
    Expect e;
    in >> e.value_bound >> e.r_bound >> e.o_bound >> e.c_bound >> e.cond_b;
    double v;
    while (in >> v) e.w.push_back(v);
    if (e.w.empty()) throw std::runtime_error(std::string("cannot read ") + path);
    return e;
}

template <typename S>
static double fro(const EigSol::DenseMatrix<S>& A) {
    double s = 0;
    for (std::int64_t j = 0; j < A.cols(); ++j)
        for (std::int64_t i = 0; i < A.rows(); ++i) s += std::norm(C(A(i, j)));
    return std::sqrt(s);
}

// r = ||A X - B X L||_F / (n eps (||A||_F + max|w| ||B||_F) ||X||_F), o = ||X^H B X - I||_F / (n eps cond_2(B))
template <typename S>
static void figures(const EigSol::DenseMatrix<S>& A, const EigSol::DenseMatrix<S>& B, double cond_b,
                    const std::vector<double>& w, const EigSol::DenseMatrix<S>& X, double& r, double& o) {
    const double n = static_cast<double>(A.rows()), eps = std::numeric_limits<double>::epsilon();
    EigSol::DenseMatrix<S> R = A * X, BX = B * X;
    double wmax = 0;
    for (double v : w) wmax = std::max(wmax, std::abs(v));
    for (std::int64_t j = 0; j < X.cols(); ++j)
        for (std::int64_t i = 0; i < X.rows(); ++i) R(i, j) -= BX(i, j) * w[static_cast<std::size_t>(j)];
    EigSol::DenseMatrix<S> G = X.adjoint() * BX;
    for (std::int64_t j = 0; j < G.cols(); ++j) G(j, j) -= S(1);
    r = fro(R) / (n * eps * (fro(A) + wmax * fro(B)) * fro(X));
    o = fro(G) / (n * eps * cond_b);
}

template <typename S>
static void all_pairs(const char* apath, const char* bpath, const char* epath) {
    const auto A = read_dense<S>(apath);
    const auto B = read_dense<S>(bpath);
    const Expect e = read_expect(epath);
    const std::int64_t n = A.rows();
    const auto res = EigSol::eigh<S>(A, B);
    EXPECT_TRUE(static_cast<std::int64_t>(res.eigenvalues.size()) == n && e.w.size() == res.eigenvalues.size());
    EXPECT_TRUE(res.eigenvectors.rows() == n && res.eigenvectors.cols() == n);
    EXPECT_TRUE(res.notConverged == 0);
    double dw = 0;
    for (std::size_t i = 0; i < e.w.size() && i < res.eigenvalues.size(); ++i) {
        dw = std::max(dw, std::abs(res.eigenvalues[i] - e.w[i]));
        if (i) EXPECT_TRUE(res.eigenvalues[i] >= res.eigenvalues[i - 1]);
    }
    double r = 0, o = 0;
    figures(A, B, e.cond_b, res.eigenvalues, res.eigenvectors, r, o);
    std::printf("  n=%lld r=%.4f (<= %.3f) o=%.4f (<= %.3f) |w - w_ref|=%.3e (<= %.3e)\n", static_cast<long long>(n), r,
                e.r_bound, o, e.o_bound, dw, e.value_bound);
    EXPECT_TRUE(dw <= e.value_bound);
    EXPECT_TRUE(r <= e.r_bound);
    EXPECT_TRUE(o <= e.o_bound);
    // eigvalsh: the same values, bit for bit
    const std::vector<double> w = EigSol::eigvalsh<S>(A, B);
    EXPECT_TRUE(w.size() == res.eigenvalues.size() &&
                std::memcmp(w.data(), res.eigenvalues.data(), w.size() * sizeof(double)) == 0);
    // index selection: the same places of the full run
    EigSol::EighOptions sel;
    sel.select = EigSol::EighOptions::Select::Index;
    sel.il = 10;
    sel.iu = 19;
    const auto part = EigSol::eigh<S>(A, B, sel);
    EXPECT_TRUE(part.eigenvalues.size() == 10 && part.eigenvectors.rows() == n && part.eigenvectors.cols() == 10);
    EXPECT_TRUE(part.eigenvalues.size() == 10 &&
                std::memcmp(part.eigenvalues.data(), res.eigenvalues.data() + 10, 10 * sizeof(double)) == 0);
    EXPECT_TRUE(EigSol::eigvalsh<S>(A, B, sel) == part.eigenvalues);
    // cholesky: c = ||L L^H - B||_F / (n eps ||B||_F), zero strict upper triangle, real positive diagonal
    const auto L = EigSol::cholesky<S>(B);
    EigSol::DenseMatrix<S> D = L * L.adjoint();
    bool shape = true;
    for (std::int64_t j = 0; j < n; ++j)
        for (std::int64_t i = 0; i < n; ++i) {
            D(i, j) -= B(i, j);
            if (i < j && L(i, j) != S(0)) shape = false;
            if (i == j && !(std::real(C(L(i, j))) > 0 && std::imag(C(L(i, j))) == 0)) shape = false;
        }
    const double c = fro(D) / (static_cast<double>(n) * std::numeric_limits<double>::epsilon() * fro(B));
    std::printf("  cholesky c=%.4f (<= %.3f)\n", c, e.c_bound);
    EXPECT_TRUE(shape);
    EXPECT_TRUE(c <= e.c_bound);
}

static void gsym97() { all_pairs<double>(g_argv[1], g_argv[2], g_argv[3]); }
static void gherm70() { all_pairs<C>(g_argv[4], g_argv[5], g_argv[6]); }

static void throw_messages() {
    using D = EigSol::DenseMatrix<double>;
    const D A = D::Identity(5, 5);
    EXPECT_MESSAGE(EigSol::eigh<double>(A, D::Identity(4, 4)), "eigh: B must be square and of A's order");
    EXPECT_MESSAGE(EigSol::eigvalsh<double>(A, D(5, 4)), "eigvalsh: B must be square and of A's order");
    D Bad = D::Identity(5, 5);
    Bad(3, 3) = -1.0;
    EXPECT_MESSAGE(EigSol::eigh<double>(A, Bad),
                   "eigsol_geigh_dense: B is not positive definite: the pivot of column 3 is not > 0");
    EXPECT_MESSAGE(EigSol::cholesky<double>(Bad),
                   "eigsol_cholesky_dense: B is not positive definite: the pivot of column 3 is not > 0");
    EXPECT_MESSAGE(EigSol::cholesky<double>(D(2, 3)), "cholesky: matrix must be square");
    const EigSol::DenseMatrix<float> F = EigSol::DenseMatrix<float>::Identity(6, 6);
    EXPECT_MESSAGE(EigSol::eigh<float>(F, F),
                   "eigh: scalar type not supported by the device path (double, std::complex<double>)");
    EXPECT_MESSAGE(EigSol::cholesky<float>(F),
                   "cholesky: scalar type not supported by the device path (double, std::complex<double>)");
    // the context still solves after the failures
    const std::vector<double> w = EigSol::eigvalsh<double>(A, A);
    EXPECT_TRUE(w.size() == 5 && w.front() == 1.0 && w.back() == 1.0);
}

int main(int argc, char** argv) {
    if (argc != 7) {
        std::printf("usage: test_geigh gsym97_A gsym97_B gsym97_expect gherm70_A gherm70_B gherm70_expect\n");
        return 2;
    }
    for (int i = 0; i < 7; ++i) g_argv[i] = argv[i];
    const std::pair<const char*, void (*)()> tests[] = {{"gsym97", gsym97}, {"gherm70", gherm70}, {"throw_messages", throw_messages}};
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
