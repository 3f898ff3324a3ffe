// C++ façade tests of EigSol::krylovSchur (Krylov-Schur; no counterpart in the reference).  Same
// minimal harness as test_subspace.cpp.  Needs a gfx950 device at run time.
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
#define EXPECT_NEAR(a, b, t) EXPECT_TRUE(std::abs((a) - (b)) <= (t))
// stmt must throw std::runtime_error whose message is exactly msg
#define EXPECT_MESSAGE(stmt, msg)                                                        \
    do {                                                                                 \
        std::string got_ = "(nothing thrown)";                                           \
        try { stmt; } catch (const std::runtime_error& e) { got_ = e.what(); }           \
        ++g_checks;                                                                      \
        if (got_ != (msg)) { ++g_fail; std::printf("  FAIL %s:%d: got \"%s\"\n", __FILE__, __LINE__, got_.c_str()); } \
    } while (0)

using SparseMat = EigSol::Matrix::Sparse<double>;
using DenseMat = EigSol::Matrix::Dense<double>;
using C = std::complex<double>;

// The matrices and numpy's eigenvalues come from the caller (tests/test_gpu_krylov_facade.py writes
// them from tests/krylov_ref.py): argv = case a, its 4 dominant eigenvalues, lap, its 4 eigenvalues
// nearest 0.  Matrices in the reader's "sparse" format, eigenvalues as "re im" lines.
static const char* g_argv[5];

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

static void case_a_largest_modulus() {
    const auto M = EigSol::readMatrixFromFile<double>(g_argv[1]);
    EigSol::KrylovOptions<double> o;
    o.nev = 4;
    EigSol::set_random_seed(5);
    const auto r = EigSol::krylovSchur<double>(M, o);
    EXPECT_TRUE(r.converged);
    EXPECT_TRUE(r.restarts >= 1 && r.applications >= 20);   // the default ncv is 20
    EXPECT_TRUE(r.eigenvalues.size() == 4 && r.residuals.size() == 4);
    EXPECT_TRUE(r.eigenvectors.rows() == M.rows() && r.eigenvectors.cols() == 4);
    expect_match(r.eigenvalues, read_values(g_argv[2]));
    for (int j = 0; j < 4; ++j) {
        // the stopping test: ||A x - theta x|| <= tol |theta|, doubled for the reductions' rounding
        EXPECT_TRUE(r.residuals[j] <= 2e-10 * std::abs(r.eigenvalues[j]));
        if (j) EXPECT_TRUE(std::abs(r.eigenvalues[j]) <= std::abs(r.eigenvalues[j - 1]));
    }
    EXPECT_MESSAGE(EigSol::krylovSchur<double>(M, o, EigSol::Vector<double>(7)), "krylovSchur: start vector size mismatch");
}

static void lap_shift_invert() {
    const auto M = EigSol::readMatrixFromFile<double>(g_argv[3]);
    const std::int64_t n = M.rows();
    EigSol::KrylovOptions<double> s;
    s.nev = 4;
    s.ncv = 20;
    s.shiftInvert = true;
    s.shift = 0.0;
    EigSol::Vector<double> v0(static_cast<std::size_t>(n));
    for (std::int64_t i = 0; i < n; ++i) v0(static_cast<std::size_t>(i)) = 1.0 + 0.37 * static_cast<double>(i % 11);
    const auto q = EigSol::krylovSchur<double>(M, s, v0);
    EXPECT_TRUE(q.converged);
    expect_match(q.eigenvalues, read_values(g_argv[4]));
    for (int j = 1; j < 4; ++j) EXPECT_TRUE(std::abs(q.eigenvalues[j]) >= std::abs(q.eigenvalues[j - 1]));   // nearest 0 first
}

static void throw_messages() {
    EigSol::KrylovOptions<double> o;
    SparseMat T(30, 30);
    for (int i = 0; i < 30; ++i) T.insert(i, i) = 1.0 + i;
    T.makeCompressed();
    EigSol::Matrix S(T);
    EXPECT_MESSAGE(EigSol::krylovSchur<C>(S, EigSol::KrylovOptions<C>{}), "krylovSchur: scalar type mismatch");
    SparseMat R(2, 3);
    R.insert(0, 0) = 1.0;
    R.makeCompressed();
    EXPECT_MESSAGE(EigSol::krylovSchur<double>(EigSol::Matrix(R), o), "krylovSchur: matrix must be square");
    EXPECT_MESSAGE(EigSol::krylovSchur<double>(EigSol::Matrix(SparseMat(0, 0)), o), "krylovSchur: matrix has zero size");
    DenseMat D(2, 2);
    D << 2.0, 0.0, 0.0, 1.0;
    EXPECT_MESSAGE(EigSol::krylovSchur<double>(EigSol::Matrix(D), o), "krylovSchur: only sparse matrices are supported");
    // library-side validation surfaces the library's message
    o.nev = 3;
    o.ncv = 4;
    EXPECT_MESSAGE(EigSol::krylovSchur<double>(S, o), "krylov_schur: ncv must be at least nev + 2");
}

int main(int argc, char** argv) {
    if (argc != 5) {
        std::printf("usage: test_krylov case_a.txt case_a_eigs.txt lap.txt lap_eigs.txt\n");
        return 2;
    }
    for (int i = 0; i < 5; ++i) g_argv[i] = argv[i];
    const std::pair<const char*, void (*)()> tests[] = {{"case_a_largest_modulus", case_a_largest_modulus},
                                                        {"lap_shift_invert", lap_shift_invert},
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
