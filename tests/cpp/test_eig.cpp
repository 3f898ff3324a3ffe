// C++ façade test of EigSol::eig (general dense eigenpairs) on a real and on a complex matrix: residual,
// eigenvalues against NumPy's one to one, the conventions of the vectors, a selection against the full run, and
// the eigenvalues against qr_eigenvalues bit for bit.  The vectors are written out for the caller, which
// forms cond(V).  Same minimal harness as test_eigh.cpp.  Needs a gfx950 device.
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

// argv: gen97 matrix, its expectations, where its vectors go; the same three for cgen70
// (tests/test_gpu_eig_facade.py writes and reads them).  A matrix file holds "n", then n * n lines "re im",
// column-major; the vectors are written the same way (n, then n * n lines).  An expectation file holds one line
// "value_bound r_bound" (2 n eps ||A||_F and max(2, 3 r_restatement)), then NumPy's eigenvalues "re im".
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
    double value_bound = 0, r_bound = 0;
    std::vector<C> w;
};
static Expect read_expect(const char* path) {
    std::ifstream in(path);
    Expect e;
    in >> e.value_bound >> e.r_bound;
    double re, im;
    while (in >> re >> im) e.w.emplace_back(re, im);
    if (e.w.empty()) throw std::runtime_error(std::string("cannot read ") + path);
    return e;
}

static bool same_bits(const EigSol::DenseMatrix<C>& X, std::int64_t xj, const EigSol::DenseMatrix<C>& Y, std::int64_t yj) {
    for (std::int64_t i = 0; i < X.rows(); ++i) {
        const C a = X(i, xj), b = Y(i, yj);
        if (std::memcmp(&a, &b, sizeof(C)) != 0) return false;
    }
    return true;
}

template <typename S>
static void all_pairs(const char* mpath, const char* epath, const char* vpath) {
    const auto A = read_dense<S>(mpath);
    const Expect e = read_expect(epath);
    const std::int64_t n = A.rows();
    const double eps = std::numeric_limits<double>::epsilon();
    const auto res = EigSol::eig<S>(A);
    EXPECT_TRUE(static_cast<std::int64_t>(res.eigenvalues.size()) == n && e.w.size() == res.eigenvalues.size());
    EXPECT_TRUE(res.eigenvectors.rows() == n && res.eigenvectors.cols() == n);
    EXPECT_TRUE(res.converged && res.notConverged == 0);
    // r = max_j ||A v_j - w_j v_j||_2 / (n eps ||A||_F)
    double fro = 0, worst = 0;
    for (std::int64_t j = 0; j < n; ++j)
        for (std::int64_t i = 0; i < n; ++i) fro += std::norm(C(A(i, j)));
    fro = std::sqrt(fro);
    for (std::int64_t j = 0; j < n; ++j) {
        double s = 0, nrm = 0, big = 0;
        std::int64_t at = 0;
        for (std::int64_t i = 0; i < n; ++i) {
            C acc = -res.eigenvalues[static_cast<std::size_t>(j)] * res.eigenvectors(i, j);
            for (std::int64_t k = 0; k < n; ++k) acc += C(A(i, k)) * res.eigenvectors(k, j);
            s += std::norm(acc);
            nrm += std::norm(res.eigenvectors(i, j));
            if (std::abs(res.eigenvectors(i, j)) > big) { big = std::abs(res.eigenvectors(i, j)); at = i; }
        }
        worst = std::max(worst, std::sqrt(s));
        EXPECT_TRUE(std::abs(std::sqrt(nrm) - 1.0) <= 8 * eps);
        EXPECT_TRUE(res.eigenvectors(at, j).imag() == 0.0 && res.eigenvectors(at, j).real() > 0.0);
        if constexpr (std::is_same_v<S, double>) {
            if (res.eigenvalues[static_cast<std::size_t>(j)].imag() == 0.0) {
                bool real = true;
                for (std::int64_t i = 0; i < n; ++i) real = real && res.eigenvectors(i, j).imag() == 0.0;
                EXPECT_TRUE(real);
            }
        }
    }
    const double r = worst / (static_cast<double>(n) * eps * fro);
    // every eigenvalue against NumPy's, one to one (greedy nearest pairing)
    std::vector<C> left = e.w;
    double dw = 0;
    for (const C& x : res.eigenvalues) {
        std::size_t best = 0;
        for (std::size_t k = 1; k < left.size(); ++k)
            if (std::abs(left[k] - x) < std::abs(left[best] - x)) best = k;
        if (left.empty()) break;
        dw = std::max(dw, std::abs(left[best] - x));
        left.erase(left.begin() + static_cast<std::ptrdiff_t>(best));
    }
    std::printf("  n=%lld r=%.3f (<= %.3f) |w - w_numpy|=%.3e (<= %.3e)\n", static_cast<long long>(n), r, e.r_bound, dw,
                e.value_bound);
    EXPECT_TRUE(r <= e.r_bound);
    EXPECT_TRUE(dw <= e.value_bound);
    // the eigenvalues are qr_eigenvalues' (n >= 64), bit for bit
    const auto q = EigSol::qr_eigenvalues_dense<S>(A, EigSol::SolverOptions{});
    EXPECT_TRUE(q.eigenvalues_complex.size() == res.eigenvalues.size() &&
                std::memcmp(q.eigenvalues_complex.data(), res.eigenvalues.data(), res.eigenvalues.size() * sizeof(C)) == 0);
    // a selection, and the eigenvalues alone
    EigSol::EigOptions sel;
    sel.select = {0, 5, n - 1};
    sel.batch = 2;
    const auto part = EigSol::eig<S>(A, sel);
    EXPECT_TRUE(part.eigenvectors.rows() == n && part.eigenvectors.cols() == 3 && part.notConverged == 0);
    EXPECT_TRUE(part.eigenvalues == res.eigenvalues);
    for (std::int64_t j = 0; j < part.eigenvectors.cols(); ++j)
        EXPECT_TRUE(same_bits(part.eigenvectors, j, res.eigenvectors, sel.select[static_cast<std::size_t>(j)]));
    EigSol::EigOptions vals;
    vals.vectors = false;
    const auto only = EigSol::eig<S>(A, vals);
    EXPECT_TRUE(only.eigenvalues == res.eigenvalues && only.eigenvectors.cols() == 0);
    std::ofstream out(vpath);
    out.precision(17);
    out << n << "\n";
    for (std::int64_t j = 0; j < n; ++j)
        for (std::int64_t i = 0; i < n; ++i) out << res.eigenvectors(i, j).real() << " " << res.eigenvectors(i, j).imag() << "\n";
    EXPECT_TRUE(static_cast<bool>(out));
}

static void gen97() { all_pairs<double>(g_argv[1], g_argv[2], g_argv[3]); }
static void cgen70() { all_pairs<C>(g_argv[4], g_argv[5], g_argv[6]); }

int main(int argc, char** argv) {
    if (argc != 7) {
        std::printf("usage: test_eig gen97.txt gen97_expect.txt gen97_vectors.txt cgen70.txt cgen70_expect.txt cgen70_vectors.txt\n");
        return 2;
    }
    for (int i = 0; i < 7; ++i) g_argv[i] = argv[i];
    const std::pair<const char*, void (*)()> tests[] = {{"gen97", gen97}, {"cgen70", cgen70}};
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
