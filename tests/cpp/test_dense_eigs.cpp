// C++ façade tests of EigSol::subspaceIteration_dense and EigSol::krylovSchur_dense (the k-eigenpair
// solvers on a DenseMatrix<S>; no counterpart in the reference).  Same minimal harness as
// test_krylov.cpp.  Needs a gfx950 device at run time.
#include <eigsol/eigsol.hpp>

#include <algorithm>
#include <cstdio>
#include <fstream>
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

// The matrices and numpy's eigenvalues come from the caller (tests/test_gpu_dense_eigs_facade.py writes
// them from tests/krylov_ref.py): argv = case a, its 4 dominant eigenvalues, lap, its 4 eigenvalues
// nearest 0, case c, its 4 dominant eigenvalues.  A matrix file holds "n nnz", then "row col re im"
// per entry; the test fills a DenseMatrix from it.  Eigenvalues are "re im" lines.
static const char* g_argv[7];

template <typename S>
static EigSol::DenseMatrix<S> read_dense(const char* path) {
    std::ifstream in(path);
    std::int64_t n = 0, nnz = 0;
    in >> n >> nnz;
    EigSol::DenseMatrix<S> A(n, n);
    for (std::int64_t e = 0; e < nnz; ++e) {
        std::int64_t r, c;
        double re, im;
        in >> r >> c >> re >> im;
        if constexpr (std::is_same_v<S, C>) A(r, c) = C(re, im);
        else A(r, c) = static_cast<S>(re);
    }
    if (!in || n == 0) throw std::runtime_error(std::string("cannot read ") + path);
    return A;
}

static std::vector<C> read_values(const char* path) {
    std::ifstream in(path);
    std::vector<C> v;
    double re, im;
    while (in >> re >> im) v.emplace_back(re, im);
    return v;
}

// every wanted value within 1e-9 (1 + |lambda|) of a returned one, as the Python tests ask
static void expect_match(const std::vector<C>& got, const std::vector<C>& want) {
    EXPECT_TRUE(got.size() == want.size() && !want.empty());
    for (const C& z : want) {
        double best = 1e300;
        for (const C& g : got) best = std::min(best, std::abs(g - z));
        EXPECT_TRUE(best <= 1e-9 * (1 + std::abs(z)));
    }
}

static void case_a_subspace() {
    const auto A = read_dense<double>(g_argv[1]);
    EigSol::SubspaceOptions o;
    o.nev = 4;
    o.maxIterations = 500;
    o.tolerance = 1e-12;
    o.residualTolerance = 1e-9;
    EigSol::set_random_seed(5);
    const auto r = EigSol::subspaceIteration_dense<double>(A, o);   // default block: 2 nev = 8
    EXPECT_TRUE(r.converged && r.iterations >= 2);
    EXPECT_TRUE(r.eigenvalues.size() == 4 && r.residuals.size() == 4);
    EXPECT_TRUE(r.eigenvectors.rows() == A.rows() && r.eigenvectors.cols() == 4);
    expect_match(r.eigenvalues, read_values(g_argv[2]));
    for (int j = 0; j < 4; ++j) {
        EXPECT_TRUE(r.residuals[j] <= 1e-9 * (1 + std::abs(r.eigenvalues[j])));
        if (j) EXPECT_TRUE(std::abs(r.eigenvalues[j]) <= std::abs(r.eigenvalues[j - 1]));
    }
    EXPECT_MESSAGE(EigSol::subspaceIteration_dense<double>(A, o, EigSol::DenseMatrix<double>(7, 8)),
                   "subspaceIteration_dense: start block size mismatch");
}

static void lap_shift_invert() {
    const auto A = read_dense<double>(g_argv[3]);
    const std::int64_t n = A.rows();
    EigSol::KrylovOptions<double> s;
    s.nev = 4;
    s.ncv = 20;
    s.shiftInvert = true;
    s.shift = 0.0;
    EigSol::Vector<double> v0(static_cast<std::size_t>(n));
    for (std::int64_t i = 0; i < n; ++i) v0(static_cast<std::size_t>(i)) = 1.0 + 0.37 * static_cast<double>(i % 11);
    const auto q = EigSol::krylovSchur_dense<double>(A, s, v0);
    EXPECT_TRUE(q.converged);
    expect_match(q.eigenvalues, read_values(g_argv[4]));
    for (int j = 1; j < 4; ++j) EXPECT_TRUE(std::abs(q.eigenvalues[j]) >= std::abs(q.eigenvalues[j - 1]));   // nearest 0 first
    EXPECT_MESSAGE(EigSol::krylovSchur_dense<double>(A, s, EigSol::Vector<double>(7)),
                   "krylovSchur_dense: start vector size mismatch");
}

static void case_c_complex_largest_modulus() {
    const auto A = read_dense<C>(g_argv[5]);
    EigSol::KrylovOptions<C> o;
    o.nev = 4;
    EigSol::set_random_seed(7);
    const auto r = EigSol::krylovSchur_dense<C>(A, o);
    EXPECT_TRUE(r.converged);
    EXPECT_TRUE(r.restarts >= 1 && r.applications >= 20);   // the default ncv is 20
    EXPECT_TRUE(r.eigenvectors.rows() == A.rows() && r.eigenvectors.cols() == 4);
    expect_match(r.eigenvalues, read_values(g_argv[6]));
    for (int j = 0; j < 4; ++j) {
        // the stopping test: ||A x - theta x|| <= tol |theta|, doubled for the reductions' rounding
        EXPECT_TRUE(r.residuals[j] <= 2e-10 * std::abs(r.eigenvalues[j]));
        if (j) EXPECT_TRUE(std::abs(r.eigenvalues[j]) <= std::abs(r.eigenvalues[j - 1]));
    }
}

static void throw_messages() {
    EigSol::DenseMatrix<float> F = EigSol::DenseMatrix<float>::Identity(30, 30);
    EXPECT_MESSAGE(EigSol::subspaceIteration_dense<float>(F),
                   "subspaceIteration_dense: scalar type not supported by the device path (double, std::complex<double>)");
    EXPECT_MESSAGE(EigSol::krylovSchur_dense<float>(F),
                   "krylovSchur_dense: scalar type not supported by the device path (double, std::complex<double>)");
    EXPECT_MESSAGE(EigSol::krylovSchur_dense<double>(EigSol::DenseMatrix<double>(2, 3)),
                   "krylovSchur_dense: matrix must be square");
    EXPECT_MESSAGE(EigSol::subspaceIteration_dense<double>(EigSol::DenseMatrix<double>(0, 0)),
                   "subspaceIteration_dense: matrix has zero size");
    // library-side validation surfaces the library's message (and the uploaded handle is released)
    EigSol::DenseMatrix<double> D = EigSol::DenseMatrix<double>::Identity(30, 30);
    EigSol::KrylovOptions<double> o;
    o.nev = 3;
    o.ncv = 4;
    EXPECT_MESSAGE(EigSol::krylovSchur_dense<double>(D, o), "krylov_schur: ncv must be at least nev + 2");
    EigSol::SubspaceOptions so;
    so.nev = 3;
    so.block = 2;
    EXPECT_MESSAGE(EigSol::subspaceIteration_dense<double>(D, so), "subspace_iteration: block must be at least nev");
}

int main(int argc, char** argv) {
    if (argc != 7) {
        std::printf("usage: test_dense_eigs a.txt a_eigs.txt lap.txt lap_eigs.txt c.txt c_eigs.txt\n");
        return 2;
    }
    for (int i = 0; i < 7; ++i) g_argv[i] = argv[i];
    const std::pair<const char*, void (*)()> tests[] = {{"case_a_subspace", case_a_subspace},
                                                        {"lap_shift_invert", lap_shift_invert},
                                                        {"case_c_complex_largest_modulus", case_c_complex_largest_modulus},
                                                        {"throw_messages", throw_messages}};
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
