// C++ façade test of EigSol::schur on a real matrix, a complex matrix and a float matrix (promoted to fp64):
// the structure of T, the figures r = ||A - Z T Z^H||_F / (n eps ||A||_F) and o = ||Z^H Z - I||_F / (n eps),
// the eigenvalues against NumPy's one to one, and the call without vectors against the full run bit for bit.
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

// argv: gen65 matrix, its expectations; the same two for cgen70 (tests/test_gpu_schur_facade.py writes them).
// A matrix file holds "n", then n * n lines "re im", column-major.  An expectation file holds one line
// "value_bound r_bound o_bound" (2 n eps ||A||_F, max(2, 3 r_LAPACK), max(2, 3 o_LAPACK)), then NumPy's
// eigenvalues "re im".
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
            else A(i, j) = static_cast<S>(re);
        }
    if (!in || n == 0) throw std::runtime_error(std::string("cannot read ") + path);
    return A;
}

struct Expect {
    double value_bound = 0, r_bound = 0, o_bound = 0;
    std::vector<C> w;
};
static Expect read_expect(const char* path) {
    std::ifstream in(path);
    Expect e;
    in >> e.value_bound >> e.r_bound >> e.o_bound;
    double re, im;
    while (in >> re >> im) e.w.emplace_back(re, im);
    if (e.w.empty()) throw std::runtime_error(std::string("cannot read ") + path);
    return e;
}

// ||A - Z T Z^H||_F / ||A||_F and ||Z^H Z - I||_F, accumulated in double
template <typename S>
static void figures(const EigSol::DenseMatrix<S>& A, const EigSol::DenseMatrix<S>& T, const EigSol::DenseMatrix<S>& Z,
                    double& res, double& orth) {
    const std::int64_t n = A.rows();
    std::vector<C> ZT(static_cast<std::size_t>(n * n));
    for (std::int64_t j = 0; j < n; ++j)
        for (std::int64_t i = 0; i < n; ++i) {
            C acc = 0;
            for (std::int64_t k = 0; k <= std::min(j + 1, n - 1); ++k) acc += C(Z(i, k)) * C(T(k, j));
            ZT[static_cast<std::size_t>(i + j * n)] = acc;
        }
    double fro = 0, s = 0, so = 0;
    for (std::int64_t j = 0; j < n; ++j)
        for (std::int64_t i = 0; i < n; ++i) {
            C acc = -C(A(i, j)), dot = (i == j) ? C(-1.0) : C(0.0);
            for (std::int64_t k = 0; k < n; ++k) {
                acc += ZT[static_cast<std::size_t>(i + k * n)] * std::conj(C(Z(j, k)));
                dot += std::conj(C(Z(k, i))) * C(Z(k, j));
            }
            s += std::norm(acc);
            so += std::norm(dot);
            fro += std::norm(C(A(i, j)));
        }
    res = std::sqrt(s) / std::sqrt(fro);
    orth = std::sqrt(so);
}

template <typename S>
static void structure(const EigSol::DenseMatrix<S>& T) {
    const std::int64_t n = T.rows();
    bool below = false, standard = true, consecutive = false;
    for (std::int64_t j = 0; j < n; ++j)
        for (std::int64_t i = j + 2; i < n; ++i) below = below || T(i, j) != S(0);
    for (std::int64_t k = 0; k + 1 < n; ++k) {
        if (T(k + 1, k) == S(0)) continue;
        if constexpr (std::is_floating_point_v<S>) {
            if (k + 2 < n && T(k + 2, k + 1) != S(0)) consecutive = true;
            const S a = T(k, k), d = T(k + 1, k + 1);
            standard = standard && std::memcmp(&a, &d, sizeof(S)) == 0 && std::signbit(T(k + 1, k)) != std::signbit(T(k, k + 1)) &&
                       T(k, k + 1) != S(0);
        } else {
            standard = false;   // a complex Schur form is upper triangular
        }
    }
    EXPECT_TRUE(!below);
    EXPECT_TRUE(!consecutive);
    EXPECT_TRUE(standard);
}

static double match_one_to_one(const std::vector<C>& w, std::vector<C> left) {
    double dw = 0;
    for (const C& x : w) {
        if (left.empty()) break;
        std::size_t best = 0;
        for (std::size_t k = 1; k < left.size(); ++k)
            if (std::abs(left[k] - x) < std::abs(left[best] - x)) best = k;
        dw = std::max(dw, std::abs(left[best] - x));
        left.erase(left.begin() + static_cast<std::ptrdiff_t>(best));
    }
    return dw;
}

template <typename S>
static void full_form(const char* mpath, const char* epath) {
    const auto A = read_dense<S>(mpath);
    const Expect e = read_expect(epath);
    const std::int64_t n = A.rows();
    const double eps = std::numeric_limits<double>::epsilon();
    const auto res = EigSol::schur<S>(A);
    EXPECT_TRUE(res.T.rows() == n && res.T.cols() == n && res.Z.rows() == n && res.Z.cols() == n);
    EXPECT_TRUE(static_cast<std::int64_t>(res.eigenvalues.size()) == n && e.w.size() == res.eigenvalues.size());
    EXPECT_TRUE(res.converged && res.iterations >= 1);
    structure(res.T);
    double rr = 0, oo = 0;
    figures(A, res.T, res.Z, rr, oo);
    const double r = rr / (static_cast<double>(n) * eps), o = oo / (static_cast<double>(n) * eps);
    const double dw = match_one_to_one(res.eigenvalues, e.w);
    std::printf("  n=%lld r=%.3f (<= %.3f) o=%.3f (<= %.3f) |w - w_numpy|=%.3e (<= %.3e)\n", static_cast<long long>(n), r,
                e.r_bound, o, e.o_bound, dw, e.value_bound);
    EXPECT_TRUE(r <= e.r_bound);
    EXPECT_TRUE(o <= e.o_bound);
    EXPECT_TRUE(dw <= e.value_bound);
    // a real matrix: the pairs are adjacent and bitwise conjugate, the positive imaginary part first
    if constexpr (std::is_floating_point_v<S>) {
        bool pairs = true;
        for (std::size_t k = 0; k < res.eigenvalues.size(); ++k) {
            if (res.eigenvalues[k].imag() == 0.0) continue;
            pairs = pairs && k + 1 < res.eigenvalues.size() && res.eigenvalues[k].imag() > 0.0 &&
                    res.eigenvalues[k + 1] == std::conj(res.eigenvalues[k]);
            ++k;
        }
        EXPECT_TRUE(pairs);
    }
    EigSol::SchurOptions novec;
    novec.vectors = false;
    const auto only = EigSol::schur<S>(A, novec);
    EXPECT_TRUE(only.Z.rows() == 0 && only.converged);
    EXPECT_TRUE(only.T.rows() == n && std::memcmp(only.T.data(), res.T.data(), static_cast<std::size_t>(n * n) * sizeof(S)) == 0);
    EXPECT_TRUE(only.eigenvalues == res.eigenvalues);
}

static void gen65() { full_form<double>(g_argv[1], g_argv[2]); }
static void cgen70() { full_form<C>(g_argv[3], g_argv[4]); }

// gen65 rounded to float: computed on the fp64 promotion, T and Z rounded back.  Each of the three factors of
// Z T Z^T carries a relative rounding of at most eps_f / 2 in the Frobenius norm, so the residual is at most
// 1.5 eps_f ||A||_F to first order (the fp64 error is 1e-8 of that): the bound is 2 eps_f ||A||_F.  Z = Q + E with
// ||E||_F <= (eps_f / 2) sqrt(n), so ||Z^T Z - I||_F <= eps_f sqrt(n) to first order: the bound is 1.5 eps_f sqrt(n).
static void gen65_float() {
    const auto A = read_dense<float>(g_argv[1]);
    const std::int64_t n = A.rows();
    const double epsf = std::numeric_limits<float>::epsilon();
    const auto res = EigSol::schur<float>(A);
    EXPECT_TRUE(res.T.rows() == n && res.Z.rows() == n && static_cast<std::int64_t>(res.eigenvalues.size()) == n);
    EXPECT_TRUE(res.converged);
    bool below = false;
    for (std::int64_t j = 0; j < n; ++j)
        for (std::int64_t i = j + 2; i < n; ++i) below = below || res.T(i, j) != 0.0f;
    EXPECT_TRUE(!below);
    double rr = 0, oo = 0;
    figures(A, res.T, res.Z, rr, oo);
    std::printf("  float n=%lld ||A - Z T Z^T||_F / ||A||_F=%.3e (<= %.3e) ||Z^T Z - I||_F=%.3e (<= %.3e)\n",
                static_cast<long long>(n), rr, 2 * epsf, oo, 1.5 * epsf * std::sqrt(static_cast<double>(n)));
    EXPECT_TRUE(rr <= 2 * epsf);
    EXPECT_TRUE(oo <= 1.5 * epsf * std::sqrt(static_cast<double>(n)));
    // the eigenvalues are those of the promoted matrix, in double
    const auto rd = EigSol::schur<double>(EigSol::detail::convert_dense<double>(A));
    EXPECT_TRUE(rd.eigenvalues == res.eigenvalues);
}

int main(int argc, char** argv) {
    if (argc != 5) {
        std::printf("usage: test_schur gen65.txt gen65_expect.txt cgen70.txt cgen70_expect.txt\n");
        return 2;
    }
    for (int i = 0; i < 5; ++i) g_argv[i] = argv[i];
    const std::pair<const char*, void (*)()> tests[] = {{"gen65", gen65}, {"cgen70", cgen70}, {"gen65_float", gen65_float}};
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
