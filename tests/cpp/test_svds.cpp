// C++ façade test of EigSol::svds (sparse, double) and EigSol::svds_dense (std::complex<double>): shapes, the
// order of s, the phase convention of V, the values-only call bit for bit and the argument checks.  s, the
// residuals, U and V are written out for the caller, which forms the figures.  Same minimal harness as
// test_krylov.cpp.  Needs a gfx950 device at run time.
#include <eigsol/eigsol.hpp>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
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

using SparseMat = EigSol::Matrix::Sparse<double>;
using C = std::complex<double>;

// argv (tests/test_gpu_svds_facade.py writes and reads them): sp_tall in the reader's "sparse" format, its
// start vector, where its result goes; planted (complex) as "M N" and M * N lines "re im" column-major, its
// start vector, where its result goes.  Vectors are "re im" lines.  A result file holds
// "M N k restarts applications converged", k lines of s, k lines of residuals, then U (M * k) and V (N * k)
// as "re im" lines, column-major.
static const char* g_argv[7];

template <typename S>
static EigSol::Vector<S> read_vector(const char* path) {
    std::ifstream in(path);
    std::vector<C> v;
    double re, im;
    while (in >> re >> im) v.emplace_back(re, im);
    EigSol::Vector<S> out(v.size());
    for (std::size_t i = 0; i < v.size(); ++i) {
        if constexpr (std::is_same_v<S, C>) out(i) = v[i];
        else out(i) = v[i].real();
    }
    return out;
}

static EigSol::DenseMatrix<C> read_dense(const char* path) {
    std::ifstream in(path);
    std::int64_t m = 0, n = 0;
    in >> m >> n;
    EigSol::DenseMatrix<C> A(m, n);
    for (std::int64_t j = 0; j < n; ++j)
        for (std::int64_t i = 0; i < m; ++i) {
            double re, im;
            in >> re >> im;
            A(i, j) = C(re, im);
        }
    if (!in || m == 0 || n == 0) throw std::runtime_error(std::string("cannot read ") + path);
    return A;
}

template <typename S>
static void check_and_write(const EigSol::SvdsResult<S>& r, std::int64_t M, std::int64_t N, int k, const char* opath) {
    EXPECT_TRUE(r.converged && r.restarts >= 1 && r.applications >= 2 * 20);
    EXPECT_TRUE(static_cast<int>(r.s.size()) == k && static_cast<int>(r.residuals.size()) == k);
    EXPECT_TRUE(r.U.rows() == M && r.U.cols() == k && r.V.rows() == N && r.V.cols() == k);
    for (int j = 0; j + 1 < k; ++j) EXPECT_TRUE(r.s[j] >= r.s[j + 1]);
    for (int j = 0; j < k; ++j) {
        double big = 0;
        std::int64_t at = 0;
        for (std::int64_t i = 0; i < N; ++i)
            if (std::abs(C(r.V(i, j))) > big) { big = std::abs(C(r.V(i, j))); at = i; }
        EXPECT_TRUE(C(r.V(at, j)).imag() == 0.0 && C(r.V(at, j)).real() > 0.0);
    }
    std::ofstream out(opath);
    out.precision(17);
    out << M << " " << N << " " << k << " " << r.restarts << " " << r.applications << " " << (r.converged ? 1 : 0) << "\n";
    for (double s : r.s) out << s << "\n";
    for (double s : r.residuals) out << s << "\n";
    for (int j = 0; j < k; ++j)
        for (std::int64_t i = 0; i < M; ++i) out << C(r.U(i, j)).real() << " " << C(r.U(i, j)).imag() << "\n";
    for (int j = 0; j < k; ++j)
        for (std::int64_t i = 0; i < N; ++i) out << C(r.V(i, j)).real() << " " << C(r.V(i, j)).imag() << "\n";
}

static void sp_tall_sparse_double() {
    const auto M = EigSol::readMatrixFromFile<double>(g_argv[1]);
    const auto v0 = read_vector<double>(g_argv[2]);
    EigSol::SvdsOptions o;
    o.nsv = 4;
    o.ncv = 20;
    const auto r = EigSol::svds<double>(M, o, v0);
    check_and_write(r, M.rows(), M.cols(), 4, g_argv[3]);
    // the values alone: the same bits
    o.vectors = false;
    const auto only = EigSol::svds<double>(M, o, v0);
    EXPECT_TRUE(only.U.rows() == 0 && only.V.rows() == 0);
    EXPECT_TRUE(only.s.size() == r.s.size() && std::memcmp(only.s.data(), r.s.data(), r.s.size() * sizeof(double)) == 0);
    // the default start vector and the default ncv (20)
    o.vectors = true;
    o.ncv = 0;
    EigSol::set_random_seed(5);
    const auto d = EigSol::svds<double>(M, o);
    EXPECT_TRUE(d.converged && d.s.size() == 4);
    for (int j = 0; j < 4; ++j) EXPECT_TRUE(std::abs(d.s[j] - r.s[j]) <= 1e-9 * r.s[0]);
    EXPECT_MESSAGE(EigSol::svds<double>(M, o, EigSol::Vector<double>(7)), "svds: start vector size mismatch");
}

static void planted_dense_complex() {
    const auto A = read_dense(g_argv[4]);
    const auto v0 = read_vector<C>(g_argv[5]);
    EigSol::SvdsOptions o;
    o.nsv = 6;
    o.ncv = 20;
    const auto r = EigSol::svds_dense<C>(A, o, v0);
    check_and_write(r, A.rows(), A.cols(), 6, g_argv[6]);
    o.maxRestarts = 1;
    o.tolerance = -1.0;
    const auto one = EigSol::svds_dense<C>(A, o, v0);
    EXPECT_TRUE(one.restarts == 1 && one.applications == 40 && !one.converged);
}

static void throw_messages() {
    EigSol::SvdsOptions o;
    SparseMat T(30, 12);
    for (int i = 0; i < 12; ++i) T.insert(i, i) = 1.0 + i;
    T.makeCompressed();
    EigSol::Matrix S(T);
    EXPECT_MESSAGE(EigSol::svds<C>(S, o), "svds: scalar type mismatch");
    EXPECT_MESSAGE(EigSol::svds<double>(EigSol::Matrix(SparseMat(0, 0)), o), "svds: matrix has zero size");
    EigSol::Matrix::Dense<double> D(2, 2);
    D << 2.0, 0.0, 0.0, 1.0;
    EXPECT_MESSAGE(EigSol::svds<double>(EigSol::Matrix(D), o), "svds: only sparse matrices are supported");
    EXPECT_MESSAGE(EigSol::svds_dense<double>(EigSol::DenseMatrix<double>(0, 3), o), "svds_dense: matrix has zero size");
    // library-side validation surfaces the library's message
    o.nsv = 3;
    o.ncv = 4;
    EXPECT_MESSAGE(EigSol::svds<double>(S, o), "svds: ncv must be at least nsv + 2");
    o.ncv = 13;
    EXPECT_MESSAGE(EigSol::svds<double>(S, o), "svds: ncv exceeds the smaller matrix dimension");
}

int main(int argc, char** argv) {
    if (argc != 7) {
        std::printf("usage: test_svds sp_tall.txt sp_tall_v0.txt sp_tall_out.txt planted.txt planted_v0.txt planted_out.txt\n");
        return 2;
    }
    for (int i = 0; i < 7; ++i) g_argv[i] = argv[i];
    const std::pair<const char*, void (*)()> tests[] = {{"sp_tall_sparse_double", sp_tall_sparse_double},
                                                        {"planted_dense_complex", planted_dense_complex},
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
    return g_fail ? 1 : 0;
}
