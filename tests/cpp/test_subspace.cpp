// C++ façade tests of EigSol::subspaceIteration (block subspace iteration; no counterpart in the
// reference).  Same minimal harness as test_facade.cpp.  Needs a gfx950 device at run time.
#include <eigsol/eigsol.hpp>

#include <cstdio>
#include <string>

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

static SparseMat coupled_diagonal() {
    SparseMat S(3, 3);
    S.insert(0, 0) = 1.0;
    S.insert(1, 1) = 3.0;
    S.insert(2, 2) = 10.0;
    S.insert(0, 1) = 1e-3;
    S.insert(1, 0) = 1e-3;
    S.insert(1, 2) = 1e-3;
    S.insert(2, 1) = 1e-3;
    S.makeCompressed();
    return S;
}

static void two_dominant_pairs() {
    EigSol::Matrix M(coupled_diagonal());
    EigSol::SubspaceOptions o;
    o.nev = 2;
    o.block = 3;
    o.tolerance = 1e-13;
    o.residualTolerance = 1e-10;
    const auto r = EigSol::subspaceIteration<double>(M, o);
    EXPECT_TRUE(r.converged);
    EXPECT_TRUE(r.iterations >= 2 && r.iterations <= o.maxIterations);
    EXPECT_TRUE(r.eigenvalues.size() == 2 && r.residuals.size() == 2);
    EXPECT_TRUE(r.eigenvectors.rows() == 3 && r.eigenvectors.cols() == 2);
    // second-order perturbation of diag(1, 3, 10) by couplings of 1e-3: below 1e-6
    EXPECT_NEAR(r.eigenvalues[0], C(10.0), 1e-6);
    EXPECT_NEAR(r.eigenvalues[1], C(3.0), 1e-6);
    const DenseMat A = coupled_diagonal().toDense();
    for (int j = 0; j < 2; ++j) {
        double nn = 0.0, rr = 0.0;
        for (int i = 0; i < 3; ++i) {
            C s = 0.0;
            for (int l = 0; l < 3; ++l) s += A(i, l) * r.eigenvectors(l, j);
            rr += std::norm(s - r.eigenvalues[j] * r.eigenvectors(i, j));
            nn += std::norm(r.eigenvectors(i, j));
        }
        EXPECT_NEAR(std::sqrt(nn), 1.0, 1e-13);
        EXPECT_TRUE(std::sqrt(rr) <= 1e-10 * (1 + std::abs(r.eigenvalues[j])));
        EXPECT_TRUE(r.residuals[j] <= 1e-10 * (1 + std::abs(r.eigenvalues[j])));
    }
    // explicit start block and default block width (min(n, 32, 2 nev) = 3 here)
    DenseMat X0(3, 3);
    X0 << 1.0, 0.5, 0.0, 0.0, 1.0, 0.5, 0.5, 0.0, 1.0;
    EigSol::SubspaceOptions d;
    d.nev = 2;
    const auto r2 = EigSol::subspaceIteration<double>(M, d, X0);
    EXPECT_TRUE(r2.converged);
    EXPECT_NEAR(r2.eigenvalues[0], C(10.0), 1e-6);
    EXPECT_NEAR(r2.eigenvalues[1], C(3.0), 1e-6);
    EXPECT_MESSAGE(EigSol::subspaceIteration<double>(M, d, DenseMat(2, 3)), "subspaceIteration: start block size mismatch");
}

static void complex_matrix() {
    EigSol::Matrix::Sparse<C> S(3, 3);
    S.insert(0, 0) = C(0.0, 5.0);
    S.insert(1, 1) = C(2.0, 0.0);
    S.insert(2, 2) = C(-1.0, 0.0);
    S.insert(0, 2) = C(0.5, 0.5);
    S.makeCompressed();
    EigSol::Matrix M(S);
    EigSol::SubspaceOptions o;
    o.nev = 1;
    o.block = 2;
    const auto r = EigSol::subspaceIteration<C>(M, o);
    EXPECT_TRUE(r.converged);
    EXPECT_NEAR(r.eigenvalues[0], C(0.0, 5.0), 1e-8);   // upper triangular: the diagonal, to the stopping tolerance
}

static void throw_messages() {
    EigSol::SubspaceOptions o;
    EigSol::Matrix S(coupled_diagonal());
    EXPECT_MESSAGE(EigSol::subspaceIteration<C>(S, o), "subspaceIteration: scalar type mismatch");
    SparseMat R(2, 3);
    R.insert(0, 0) = 1.0;
    R.makeCompressed();
    EXPECT_MESSAGE(EigSol::subspaceIteration<double>(EigSol::Matrix(R), o), "subspaceIteration: matrix must be square");
    EXPECT_MESSAGE(EigSol::subspaceIteration<double>(EigSol::Matrix(SparseMat(0, 0)), o),
                   "subspaceIteration: matrix has zero size");
    DenseMat D(2, 2);
    D << 2.0, 0.0, 0.0, 1.0;
    EXPECT_MESSAGE(EigSol::subspaceIteration<double>(EigSol::Matrix(D), o),
                   "subspaceIteration: only sparse matrices are supported");
    EigSol::Matrix::Sparse<float> F(2, 2);
    F.insert(0, 0) = 1.0f;
    F.insert(1, 1) = 2.0f;
    F.makeCompressed();
    std::string msg;
    try {
        EigSol::subspaceIteration<float>(EigSol::Matrix(F), o);
    } catch (const std::runtime_error& e) {
        msg = e.what();
    }
    EXPECT_TRUE(msg.rfind("subspaceIteration: scalar type not supported by the device path", 0) == 0);
    // library-side validation surfaces the library's message
    o.nev = 3;
    o.block = 2;
    EXPECT_MESSAGE(EigSol::subspaceIteration<double>(S, o), "subspace_iteration: block must be at least nev");
}

static void seed_governs_default_start() {
    EigSol::Matrix M(coupled_diagonal());
    EigSol::SubspaceOptions o;
    o.nev = 2;
    o.block = 2;
    o.maxIterations = 6;
    o.tolerance = -1.0;   // never converges: six products from the drawn start block
    EigSol::set_random_seed(77);
    const auto a = EigSol::subspaceIteration<double>(M, o);
    EigSol::set_random_seed(77);
    const auto b = EigSol::subspaceIteration<double>(M, o);
    EigSol::set_random_seed(78);
    const auto c = EigSol::subspaceIteration<double>(M, o);
    EXPECT_TRUE(a.iterations == 6 && !a.converged);
    bool same = a.eigenvalues == b.eigenvalues && a.residuals == b.residuals, differs = false;
    for (std::int64_t i = 0; i < a.eigenvectors.size(); ++i) {
        same = same && a.eigenvectors.data()[i] == b.eigenvectors.data()[i];
        differs = differs || a.eigenvectors.data()[i] != c.eigenvectors.data()[i];
    }
    EXPECT_TRUE(same);
    EXPECT_TRUE(differs || a.residuals != c.residuals);
}

int main() {
    const std::pair<const char*, void (*)()> tests[] = {{"two_dominant_pairs", two_dominant_pairs},
                                                        {"complex_matrix", complex_matrix},
                                                        {"throw_messages", throw_messages},
                                                        {"seed_governs_default_start", seed_governs_default_start}};
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
