// C++ façade test of EigSol::eigh with EighOptions::Method::DC (divide and conquer on the tridiagonal matrix) on
// a real and on a complex matrix: residual, orthogonality, eigenvalues against LAPACK's, a selection against the
// full run, and the default method unchanged.  Same minimal harness as test_eigh.cpp.  Needs a gfx950 device.
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

// argv: sym97 matrix, its expectations, herm70 matrix, its expectations (tests/test_gpu_eigh_dc_facade.py writes
// them).  A matrix file holds "n", then n * n lines "re im", column-major.  An expectation file holds one line
// "value_bound r_bound o_bound" (2 n eps ||A||_F, max(2, 3 r_evd), max(2, 3 o_evd) of LAPACK's divide and
// conquer), then LAPACK's eigenvalues, ascending, one per line.
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

struct Expect {
    double value_bound = 0, r_bound = 0, o_bound = 0;
    std::vector<double> w;
};
static Expect read_expect(const char* path) {
    std::ifstream in(path);
    Expect e;
    in >> e.value_bound >> e.r_bound >> e.o_bound;
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

// r = ||A Z - Z L||_F / (n eps ||A||_F) and o = ||Z^H Z - I||_F / (n eps)
template <typename S>
static void figures(const EigSol::DenseMatrix<S>& A, const std::vector<double>& w, const EigSol::DenseMatrix<S>& Z,
                    double& r, double& o) {
    const double n = static_cast<double>(A.rows()), eps = std::numeric_limits<double>::epsilon();
    EigSol::DenseMatrix<S> R = A * Z;
    for (std::int64_t j = 0; j < Z.cols(); ++j)
        for (std::int64_t i = 0; i < Z.rows(); ++i) R(i, j) -= Z(i, j) * w[static_cast<std::size_t>(j)];
    EigSol::DenseMatrix<S> G = Z.adjoint() * Z;
    for (std::int64_t j = 0; j < G.cols(); ++j) G(j, j) -= S(1);
    r = fro(R) / (n * eps * fro(A));
    o = fro(G) / (n * eps);
}

template <typename S>
static bool same_bits(const EigSol::DenseMatrix<S>& X, std::int64_t xj, const EigSol::DenseMatrix<S>& Y, std::int64_t yj) {
    for (std::int64_t i = 0; i < X.rows(); ++i) {
        const S a = X(i, xj), b = Y(i, yj);
        if (std::memcmp(&a, &b, sizeof(S)) != 0) return false;
    }
    return true;
}

template <typename S>
static void all_pairs(const char* mpath, const char* epath) {
    const auto A = read_dense<S>(mpath);
    const Expect e = read_expect(epath);
    const std::int64_t n = A.rows();
    EigSol::EighOptions dc;
    dc.method = EigSol::EighOptions::Method::DC;
    const auto res = EigSol::eigh<S>(A, dc);
    EXPECT_TRUE(static_cast<std::int64_t>(res.eigenvalues.size()) == n && e.w.size() == res.eigenvalues.size());
    EXPECT_TRUE(res.eigenvectors.rows() == n && res.eigenvectors.cols() == n);
    EXPECT_TRUE(res.notConverged == 0);
    double dw = 0;
    for (std::size_t i = 0; i < e.w.size() && i < res.eigenvalues.size(); ++i) {
        dw = std::max(dw, std::abs(res.eigenvalues[i] - e.w[i]));
        if (i) EXPECT_TRUE(res.eigenvalues[i] >= res.eigenvalues[i - 1]);
    }
    double r = 0, o = 0;
    figures(A, res.eigenvalues, res.eigenvectors, r, o);
    std::printf("  n=%lld r=%.3f (<= %.3f) o=%.3f (<= %.3f) |w - w_lapack|=%.3e (<= %.3e)\n", static_cast<long long>(n), r,
                e.r_bound, o, e.o_bound, dw, e.value_bound);
    EXPECT_TRUE(dw <= e.value_bound);
    EXPECT_TRUE(r <= e.r_bound);
    EXPECT_TRUE(o <= e.o_bound);
    // an index selection returns the full run's places, values and vectors, bit for bit
    EigSol::EighOptions sel = dc;
    sel.select = EigSol::EighOptions::Select::Index;
    sel.il = 10;
    sel.iu = 19;
    const auto part = EigSol::eigh<S>(A, sel);
    EXPECT_TRUE(part.eigenvalues.size() == 10 && part.eigenvectors.rows() == n && part.eigenvectors.cols() == 10);
    EXPECT_TRUE(part.eigenvalues.size() == 10 &&
                std::memcmp(part.eigenvalues.data(), res.eigenvalues.data() + 10, 10 * sizeof(double)) == 0);
    for (std::int64_t j = 0; j < part.eigenvectors.cols(); ++j) EXPECT_TRUE(same_bits(part.eigenvectors, j, res.eigenvectors, 10 + j));
    // eigvalsh ignores the method: the default call's values
    EXPECT_TRUE(EigSol::eigvalsh<S>(A, dc) == EigSol::eigvalsh<S>(A));
    // the default method is Stein, and naming it changes nothing
    EigSol::EighOptions st;
    st.method = EigSol::EighOptions::Method::Stein;
    const auto a = EigSol::eigh<S>(A), b = EigSol::eigh<S>(A, st);
    EXPECT_TRUE(EigSol::EighOptions{}.method == EigSol::EighOptions::Method::Stein);
    EXPECT_TRUE(a.eigenvalues == b.eigenvalues);
    for (std::int64_t j = 0; j < n; ++j) EXPECT_TRUE(same_bits(a.eigenvectors, j, b.eigenvectors, j));
}

static void sym97() { all_pairs<double>(g_argv[1], g_argv[2]); }
static void herm70() { all_pairs<C>(g_argv[3], g_argv[4]); }

int main(int argc, char** argv) {
    if (argc != 5) {
        std::printf("usage: test_eigh_dc sym97.txt sym97_expect.txt herm70.txt herm70_expect.txt\n");
        return 2;
    }
    for (int i = 0; i < 5; ++i) g_argv[i] = argv[i];
    const std::pair<const char*, void (*)()> tests[] = {{"sym97", sym97}, {"herm70", herm70}};
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
