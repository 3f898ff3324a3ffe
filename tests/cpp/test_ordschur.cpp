// C++ façade test of SchurOptions::sort and EigSol::ordschur on a real and a complex matrix: the sorted call
// must have the bits of schur followed by ordschur with the Re < 0 mask, the selected eigenvalues must lead, and
// both results are written out so that tests/test_gpu_ordschur_facade.py can compare them with the Python call's
// bits.  Same minimal harness as test_schur.cpp.  Needs a gfx950 device.
#include <eigsol/eigsol.hpp>

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

using C = std::complex<double>;

// A matrix file holds "n", then n * n lines "re im", column-major.
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

template <typename S>
static bool same_bits(const EigSol::DenseMatrix<S>& a, const EigSol::DenseMatrix<S>& b) {
    return a.rows() == b.rows() && a.cols() == b.cols() &&
           std::memcmp(a.data(), b.data(), sizeof(S) * static_cast<std::size_t>(a.rows() * a.cols())) == 0;
}

// T, Z (column-major) and the eigenvalues as raw doubles, then sdim as text
template <typename S>
static void dump(const std::string& prefix, const EigSol::SchurResult<S>& r) {
    const std::size_t nn = static_cast<std::size_t>(r.T.rows() * r.T.cols());
    std::ofstream(prefix + "_T.bin", std::ios::binary).write(reinterpret_cast<const char*>(r.T.data()), sizeof(S) * nn);
    std::ofstream(prefix + "_Z.bin", std::ios::binary).write(reinterpret_cast<const char*>(r.Z.data()), sizeof(S) * nn);
    std::ofstream(prefix + "_w.bin", std::ios::binary)
        .write(reinterpret_cast<const char*>(r.eigenvalues.data()), sizeof(C) * r.eigenvalues.size());
    std::ofstream(prefix + "_sdim.txt") << r.sdim << " " << (r.ordered ? 1 : 0) << "\n";
}

template <typename S>
static void run_case(const char* matrix, const std::string& prefix) {
    const EigSol::DenseMatrix<S> A = read_dense<S>(matrix);
    const std::int64_t n = A.rows();
    const EigSol::SchurResult<S> plain = EigSol::schur<S>(A);
    EXPECT_TRUE(plain.converged);
    EXPECT_TRUE(plain.sdim == 0 && !plain.ordered);
    std::vector<bool> select(static_cast<std::size_t>(n));
    std::int64_t count = 0;
    for (std::size_t i = 0; i < select.size(); ++i) {
        select[i] = plain.eigenvalues[i].real() < 0.0;
        count += select[i] ? 1 : 0;
    }
    const EigSol::SchurResult<S> two = EigSol::ordschur<S>(plain, select);
    EigSol::SchurOptions opts;
    opts.sort = EigSol::SchurSort::LeftHalfPlane;
    const EigSol::SchurResult<S> one = EigSol::schur<S>(A, opts);
    EXPECT_TRUE(one.converged && one.ordered && two.ordered);
    EXPECT_TRUE(one.sdim == count && two.sdim == count);
    EXPECT_TRUE(one.iterations == plain.iterations && two.iterations == plain.iterations);
    EXPECT_TRUE(same_bits(one.T, two.T));
    EXPECT_TRUE(same_bits(one.Z, two.Z));
    EXPECT_TRUE(one.eigenvalues.size() == two.eigenvalues.size() &&
                std::memcmp(one.eigenvalues.data(), two.eigenvalues.data(), sizeof(C) * one.eigenvalues.size()) == 0);
    for (std::int64_t i = 0; i < n; ++i) EXPECT_TRUE((one.eigenvalues[static_cast<std::size_t>(i)].real() < 0.0) == (i < count));
    // without vectors: the same T and eigenvalues
    opts.vectors = false;
    const EigSol::SchurResult<S> nov = EigSol::schur<S>(A, opts);
    EXPECT_TRUE(same_bits(nov.T, one.T) && nov.Z.rows() == 0 && nov.sdim == count);
    // a mask of the wrong length throws
    bool threw = false;
    try {
        (void)EigSol::ordschur<S>(plain, std::vector<bool>(static_cast<std::size_t>(n + 1), true));
    } catch (const std::runtime_error&) {
        threw = true;
    }
    EXPECT_TRUE(threw);
    dump(prefix, one);
    std::printf("%s: n=%lld sdim=%lld\n", matrix, static_cast<long long>(n), static_cast<long long>(count));
}

// argv: real matrix, its output prefix, complex matrix, its output prefix
int main(int argc, char** argv) {
    if (argc != 5) {
        std::printf("usage: test_ordschur real.txt real_out complex.txt complex_out\n");
        return 2;
    }
    try {
        run_case<double>(argv[1], argv[2]);
        run_case<C>(argv[3], argv[4]);
        // float input runs on its fp64 promotion
        const EigSol::DenseMatrix<double> Ad = read_dense<double>(argv[1]);
        EigSol::DenseMatrix<float> Af(Ad.rows(), Ad.cols());
        for (std::int64_t j = 0; j < Ad.cols(); ++j)
            for (std::int64_t i = 0; i < Ad.rows(); ++i) Af(i, j) = static_cast<float>(Ad(i, j));
        EigSol::SchurOptions opts;
        opts.sort = EigSol::SchurSort::RightHalfPlane;
        const EigSol::SchurResult<float> rf = EigSol::schur<float>(Af, opts);
        EXPECT_TRUE(rf.converged && rf.ordered && rf.sdim > 0 && rf.sdim < Ad.rows());
        for (std::int64_t i = 0; i < Ad.rows(); ++i)
            EXPECT_TRUE((rf.eigenvalues[static_cast<std::size_t>(i)].real() >= 0.0) == (i < rf.sdim));
    } catch (const std::exception& e) {
        std::printf("  FAIL exception: %s\n", e.what());
        ++g_fail;
    }
    std::printf("%d checks, %d failed\n", g_checks, g_fail);
    if (g_fail == 0) std::printf("ALL PASSED\n");
    return g_fail == 0 ? 0 : 1;
}
