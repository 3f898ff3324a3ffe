// EigSol drop-in façade — solver entry points, same names, signatures, check order and exception
// messages as the reference, numeric core on the gfx950 device through the C ABI.
//
//   powerMethod<S>                 src/power_method/power_method.hpp:135-148
//   shiftedInversePowerMethod<S>   src/power_method/shifted_inverse_power_solver.hpp:112-125
//   solve_shifted<S>               src/matrix/solve_shifted.hpp:48-118
//   to_hessenberg<S> / _dense      src/qr_method/to_hessenberg.hpp:23-119
//   qr_decompose<S> / _dense       src/qr_method/qr_decompose.hpp:25-132
//   qr_eigenvalues<S> / _dense     src/qr_method/qr_eigenvalues.hpp:40-147
//   subspaceIteration<S> / _dense  new: nev dominant eigenpairs of a sparse matrix (eigsol_subspace_csr)
//                                  or of a DenseMatrix<S> (eigsol_subspace_dense)
//   svds<S> / svds_dense<S>        new: nsv largest singular triplets of a sparse or dense matrix (eigsol_svds_csr /
//                                  eigsol_svds_dense)
//   krylovSchur<S> / _dense        new: nev eigenpairs, dominant or nearest a shift (eigsol_krylov_csr /
//                                  eigsol_krylov_dense)
//   schur<S> / ordschur<S>         new: the Schur form of a DenseMatrix<S>, optionally sorted, and its reordering
//                                  (eigsol_schur_dense / eigsol_schur_sorted_dense / eigsol_ordschur_dense)
//   solve_sylvester<S> / solve_lyapunov<S>  new: A X + X B = C and A X + X A^H = Q on DenseMatrix<S>
//                                  (eigsol_sylvester_dense / eigsol_lyapunov_dense)
//
// Scalars: double and std::complex<double> natively; float and std::complex<float> natively for the
// power method and the triangular-CSR shifted inverse, promoted to fp64 for the other solvers
// (core.hpp, PromotedScalar); long double / std::complex<long double> in double-double on the
// device (core.hpp, WideScalar: every solver; qr_eigenvalues' Francis variant refines the fp64
// sweeps' eigenvalues in double-double).
//
// Start vector: the reference draws x0 with Eigen's Vector::Random (std::rand, not reproducible
// across Eigen versions).  Here x0 comes from a documented generator
// (std::mt19937_64 seeded with EigSol::random_seed(), U(-1, 1) per real/imaginary component);
// overloads taking an explicit x0 are provided.  Iteration semantics (counts, convergence test,
// zero-norm and maxIterations <= 0 cases) are the reference's, evaluated on the device.
#pragma once

#include <random>
#include <typeinfo>
#include <utility>

#include "matrix.hpp"

namespace EigSol {

inline std::uint64_t& random_seed() {
    static std::uint64_t seed = 0x5eed5eedULL;
    return seed;
}

namespace detail {
struct RandomState {
    std::mt19937_64 gen{random_seed()};
    std::uint64_t seeded = random_seed();
};
inline RandomState& random_state() {
    static RandomState st;
    return st;
}
// One generator for every scalar type; re-seeded whenever EigSol::random_seed() holds a new value
// since the last draw (so setting the seed between solves takes effect, like std::srand before the
// reference's Eigen Vector::Random).
inline std::mt19937_64& random_engine() {
    RandomState& st = random_state();
    if (st.seeded != random_seed()) {
        st.seeded = random_seed();
        st.gen.seed(st.seeded);
    }
    return st.gen;
}
}  // namespace detail

// std::srand counterpart: always restarts the start-vector sequence, also for an unchanged seed.
inline void set_random_seed(std::uint64_t seed) {
    random_seed() = seed;
    detail::random_state().seeded = seed;
    detail::random_state().gen.seed(seed);
}

template <ScalarConcept S>
Vector<S> random_vector(std::size_t n) {
    std::mt19937_64& gen = detail::random_engine();
    std::uniform_real_distribution<double> u(-1.0, 1.0);
    Vector<S> v(n);
    for (std::size_t i = 0; i < n; ++i) {
        if constexpr (is_complex_of_floating<S>::value) {
            const double re = u(gen);
            const double im = u(gen);
            v(i) = S(re, im);
        } else {
            v(i) = S(u(gen));
        }
    }
    return v;
}

template <typename S>
void DenseMatrix<S>::setRandom() {
    Vector<S> v = random_vector<S>(static_cast<std::size_t>(size()));
    std::copy(v.begin(), v.end(), d_.begin());
}

// QR iteration variant.  Francis (Hessenberg + implicit multishift sweeps with aggressive early
// deflation, the north_star path) is the default of every overload, as in the Python binding: it
// converges on general real and complex matrices (the reference's loop does not),
// deflates at LAPACK's threshold, reports `iterations` as the most sweeps any deflation needed
// (within [1, maxIterations] exactly when converged) and returns the real parts in `eigenvalues`
// with the complex eigenvalues in `eigenvalues_complex`.  The reference's own unshifted H <- RQ
// iteration (qr_eigenvalues.hpp:62-105: identical iteration counts, `converged` and positional
// diag(H)) is QRVariant::Unshifted.  The reference's tests check sorted eigenvalues, `converged`
// and 1 <= iterations <= maxIterations (qr_algorithms_test.cpp:253-332), which both satisfy.
enum class QRVariant { Francis = EIGSOL_QR_FRANCIS, Unshifted = EIGSOL_QR_UNSHIFTED };

namespace detail {

inline eigsol_solver_options copts(const SolverOptions& o) {
    eigsol_solver_options c;
    c.max_iterations = o.maxIterations;
    c.tolerance = o.tolerance;
    return c;
}

template <typename S>
void require_device_scalar(const char* who) {
    if constexpr (!DeviceCapable<S>)
        throw std::runtime_error(std::string(who) + ": scalar type not supported by the device path "
                                                    "(double, std::complex<double>, float, std::complex<float>)");
}

// element-wise conversions between a scalar type and its device (fp64) type
template <typename T, typename U>
Vector<T> convert_vec(const Vector<U>& v) {
    if constexpr (std::is_same_v<T, U>) return v;
    else {
        Vector<T> w(v.size());
        for (std::size_t i = 0; i < v.size(); ++i) w(i) = static_cast<T>(v(i));
        return w;
    }
}
template <typename T, typename U>
DenseMatrix<T> convert_dense(const DenseMatrix<U>& a) {
    DenseMatrix<T> b(a.rows(), a.cols());
    for (std::int64_t i = 0; i < a.size(); ++i) b.data()[i] = static_cast<T>(a.data()[i]);
    return b;
}

// long double: the same run with the vectors, the shift and the results as double-double pairs
template <typename S>
int power_run_wide(const DeviceMatrix& d, bool dense, const eigsol_solver_options& o, const Vector<S>& xs0,
                   const S* shift, EigenResult<S>& out) {
    using Wt = wire_t<S>;
    const std::vector<Wt> xw = to_wire_vec(xs0.data(), xs0.size());
    const Wt sh = shift ? to_wire(*shift) : to_wire(S(0));
    Wt lam{};
    std::vector<Wt> x(xs0.size());
    std::int32_t it = 0, conv = 0;
    int st;
    if (shift)
        st = dense ? eigsol_shifted_inverse_dense(d.dense(), &sh, &o, xw.data(), &lam, x.data(), &it, &conv)
                   : eigsol_shifted_inverse_csr(d.csr(), &sh, &o, xw.data(), &lam, x.data(), &it, &conv);
    else
        st = dense ? eigsol_power_dense(d.dense(), &o, xw.data(), &lam, x.data(), &it, &conv)
                   : eigsol_power_csr(d.csr(), &o, xw.data(), &lam, x.data(), &it, &conv);
    if (st == EIGSOL_OK) {
        Vector<S> xs(x.size());
        for (std::size_t i = 0; i < x.size(); ++i) xs(i) = from_wire(x[i]);
        out = EigenResult<S>(from_wire(lam), xs, it, conv != 0);
    }
    return st;
}

// One device run in scalar type D (S itself, or its fp64 promotion).
template <typename D, typename S>
int power_run(const DeviceMatrix& d, bool dense, const eigsol_solver_options& o, const Vector<S>& xs0,
              const S* shift, EigenResult<S>& out) {
    const Vector<D> xs = convert_vec<D>(xs0);
    const D sh = shift ? static_cast<D>(*shift) : D{};
    D lam{};
    Vector<D> x(xs0.size());
    std::int32_t it = 0, conv = 0;
    int st;
    if (shift)
        st = dense ? eigsol_shifted_inverse_dense(d.dense(), &sh, &o, xs.data(), &lam, x.data(), &it, &conv)
                   : eigsol_shifted_inverse_csr(d.csr(), &sh, &o, xs.data(), &lam, x.data(), &it, &conv);
    else
        st = dense ? eigsol_power_dense(d.dense(), &o, xs.data(), &lam, x.data(), &it, &conv)
                   : eigsol_power_csr(d.csr(), &o, xs.data(), &lam, x.data(), &it, &conv);
    if (st == EIGSOL_OK) out = EigenResult<S>(static_cast<S>(lam), convert_vec<S>(x), it, conv != 0);
    return st;
}

template <typename S>
EigenResult<S> power_like(const Matrix& M, const SolverOptions& opts, const Vector<S>* x0, const S* shift,
                          const char* who) {
    if (M.scalar_type() != typeid(S)) throw std::runtime_error(std::string(who) + ": scalar type mismatch");
    const std::int64_t r = M.rows(), c = M.cols();
    if (r != c) throw std::runtime_error(std::string(who) + ": matrix must be square");
    if (r == 0) throw std::runtime_error(std::string(who) + ": matrix has zero size");
    require_device_scalar<S>(who);
    EigenResult<S> res;
    if constexpr (DeviceCapable<S>) {
        Vector<S> xs0 = x0 ? *x0 : random_vector<S>(static_cast<std::size_t>(r));
        if (xs0.size() != static_cast<std::size_t>(r))
            throw std::runtime_error(std::string(who) + ": start vector size mismatch");
        const eigsol_solver_options o = copts(opts);
        // single precision runs natively (power method; shifted inverse on dense, banded and
        // triangular factors); only a general sparse pattern with neither a usable band nor a dense
        // factor that fits (ILU(0)-GMRES, double-only) is promoted to fp64
        int st = EIGSOL_E_UNSUPPORTED;
        if constexpr (WideScalar<S>) {   // long double: double-double kernels (see core.hpp)
            st = power_run_wide<S>(M.device<S>(), M.isDense(), o, xs0, shift, res);
        } else {
            st = power_run<S>(M.device<S>(), M.isDense(), o, xs0, shift, res);
        }
        if constexpr (PromotedScalar<S>) {
            if (st == EIGSOL_E_UNSUPPORTED && shift)
                st = power_run<device_scalar_t<S>>(M.device_fp64<S>(), M.isDense(), o, xs0, shift, res);
        }
        check(st, who);
    }
    return res;
}

template <typename S>
void dense_square_check(const DenseMatrix<S>& A, const char* who) {
    if (A.rows() != A.cols()) throw std::runtime_error(std::string(who) + ": A must be square");
}

}  // namespace detail

// ------------------------------------------------------------------------------ power methods
template <ScalarConcept S>
EigenResult<S> powerMethod(const Matrix& M, const SolverOptions& opts = SolverOptions{}) {
    return detail::power_like<S>(M, opts, nullptr, nullptr, "powerMethod");
}
template <ScalarConcept S>
EigenResult<S> powerMethod(const Matrix& M, const SolverOptions& opts, const Vector<S>& x0) {
    return detail::power_like<S>(M, opts, &x0, nullptr, "powerMethod");
}

template <ScalarConcept S>
EigenResult<S> shiftedInversePowerMethod(const Matrix& M,
                                         const ShiftedSolverOptions<S>& opts = ShiftedSolverOptions<S>{}) {
    return detail::power_like<S>(M, opts, nullptr, &opts.shift, "shiftedInversePowerMethod");
}
template <ScalarConcept S>
EigenResult<S> shiftedInversePowerMethod(const Matrix& M, const ShiftedSolverOptions<S>& opts, const Vector<S>& x0) {
    return detail::power_like<S>(M, opts, &x0, &opts.shift, "shiftedInversePowerMethod");
}

// ------------------------------------------------------------------------- block subspace iteration
// The opts.nev eigenpairs of largest modulus of a sparse matrix (eigsol_subspace_csr: orthogonal
// iteration with Rayleigh-Ritz on opts.block vectors).  S = double and std::complex<double>; the
// default start block is drawn with random_vector<S> (column by column), so set_random_seed governs it.
// subspaceIteration_dense takes a DenseMatrix<S> instead (eigsol_subspace_dense: the product runs on
// the fp64 matrix cores); the matrix is on the device for the duration of the call.
namespace detail {
// Defaults, start block and result of one run on an n x n matrix; entry(o, X0, eigenvalues,
// eigenvectors, residuals, iterations, converged) is the C entry bound to its matrix handle.
template <typename S, typename Entry>
SubspaceResult<S> subspace_device(std::int64_t n, const SubspaceOptions& opts, const DenseMatrix<S>* X0,
                                  const char* who, Entry&& entry) {
    SubspaceResult<S> res;
    if constexpr (!DeviceScalar<S>) {
        throw std::runtime_error(std::string(who) + ": scalar type not supported by the device path "
                                                    "(double, std::complex<double>)");
    } else {
        eigsol_subspace_options o;
        o.max_iterations = opts.maxIterations;
        o.tolerance = opts.tolerance;
        o.residual_tolerance = opts.residualTolerance;
        o.nev = opts.nev;
        if (opts.block > 0) o.block = opts.block;
        else if (X0) o.block = static_cast<int>(X0->cols());
        else o.block = static_cast<int>(std::min<std::int64_t>({n, 32, 2 * static_cast<std::int64_t>(opts.nev)}));
        DenseMatrix<S> start;
        if (X0) {
            if (X0->rows() != n || X0->cols() != o.block)
                throw std::runtime_error(std::string(who) + ": start block size mismatch");
        } else {
            start = DenseMatrix<S>(n, std::max(o.block, 0));
            start.setRandom();
            X0 = &start;
        }
        const std::size_t k = static_cast<std::size_t>(std::max(opts.nev, 0));
        res.eigenvalues.assign(std::max<std::size_t>(k, 1), {});
        res.residuals.assign(std::max<std::size_t>(k, 1), 0.0);
        res.eigenvectors = DenseMatrix<std::complex<double>>(n, static_cast<std::int64_t>(k));
        std::int32_t it = 0, conv = 0;
        const int st = entry(&o, X0->data(), reinterpret_cast<double*>(res.eigenvalues.data()),
                             k ? reinterpret_cast<double*>(res.eigenvectors.data()) : nullptr, res.residuals.data(),
                             &it, &conv);
        check(st, who);
        res.eigenvalues.resize(k);
        res.residuals.resize(k);
        res.iterations = it;
        res.converged = conv != 0;
    }
    return res;
}

template <typename S>
SubspaceResult<S> subspace_run(const Matrix& M, const SubspaceOptions& opts, const DenseMatrix<S>* X0) {
    const char* who = "subspaceIteration";
    if (M.scalar_type() != typeid(S)) throw std::runtime_error(std::string(who) + ": scalar type mismatch");
    const std::int64_t n = M.rows();
    if (n != M.cols()) throw std::runtime_error(std::string(who) + ": matrix must be square");
    if (n == 0) throw std::runtime_error(std::string(who) + ": matrix has zero size");
    if (M.isDense()) throw std::runtime_error(std::string(who) + ": only sparse matrices are supported");
    return subspace_device<S>(n, opts, X0, who, [&](auto... a) {
        if constexpr (DeviceScalar<S>) return eigsol_subspace_csr(M.device<S>().csr(), a...);
        else return static_cast<int>(EIGSOL_E_UNSUPPORTED);
    });
}

template <typename S>
SubspaceResult<S> subspace_run_dense(const DenseMatrix<S>& A, const SubspaceOptions& opts, const DenseMatrix<S>* X0) {
    const char* who = "subspaceIteration_dense";
    const std::int64_t n = A.rows();
    if (n != A.cols()) throw std::runtime_error(std::string(who) + ": matrix must be square");
    if (n == 0) throw std::runtime_error(std::string(who) + ": matrix has zero size");
    return subspace_device<S>(n, opts, X0, who, [&](auto... a) {
        if constexpr (DeviceScalar<S>) {
            // on the device for this call: the handle is freed on every return, a throw included
            const std::shared_ptr<DeviceMatrix> d = DeviceMatrix::dense(dtype_of<S>(), n, n, A.data());
            return eigsol_subspace_dense(d->dense(), a...);
        } else {
            return static_cast<int>(EIGSOL_E_UNSUPPORTED);
        }
    });
}
}  // namespace detail

template <ScalarConcept S>
SubspaceResult<S> subspaceIteration(const Matrix& M, const SubspaceOptions& opts = SubspaceOptions{}) {
    return detail::subspace_run<S>(M, opts, nullptr);
}
template <ScalarConcept S>
SubspaceResult<S> subspaceIteration(const Matrix& M, const SubspaceOptions& opts, const DenseMatrix<S>& X0) {
    return detail::subspace_run<S>(M, opts, &X0);
}
template <ScalarConcept S>
SubspaceResult<S> subspaceIteration_dense(const DenseMatrix<S>& A, const SubspaceOptions& opts = SubspaceOptions{}) {
    return detail::subspace_run_dense<S>(A, opts, nullptr);
}
template <ScalarConcept S>
SubspaceResult<S> subspaceIteration_dense(const DenseMatrix<S>& A, const SubspaceOptions& opts,
                                          const DenseMatrix<S>& X0) {
    return detail::subspace_run_dense<S>(A, opts, &X0);
}

// ----------------------------------------------------------------------------------- Krylov-Schur
// opts.nev eigenpairs of a sparse matrix by thick-restart Arnoldi (eigsol_krylov_csr): of largest
// modulus, or nearest opts.shift with opts.shiftInvert.  S = double and std::complex<double>; the
// default start vector is drawn with random_vector<S>, so set_random_seed governs it.
// krylovSchur_dense takes a DenseMatrix<S> instead (eigsol_krylov_dense); with shiftInvert and a shift
// next to an eigenvalue qr_eigenvalues_dense returned, it gives that eigenvalue's eigenvector.  The
// matrix is on the device for the duration of the call.
namespace detail {
// Defaults, start vector and result of one run on an n x n matrix; entry(o, sigma, v0, eigenvalues,
// eigenvectors, residuals, restarts, applications, converged) is the C entry bound to its handle.
template <typename S, typename Entry>
KrylovResult<S> krylov_device(std::int64_t n, const KrylovOptions<S>& opts, const Vector<S>* v0, const char* who,
                              Entry&& entry) {
    KrylovResult<S> res;
    if constexpr (!DeviceScalar<S>) {
        throw std::runtime_error(std::string(who) + ": scalar type not supported by the device path "
                                                    "(double, std::complex<double>)");
    } else {
        eigsol_krylov_options o;
        o.max_restarts = opts.maxRestarts;
        o.tolerance = opts.tolerance;
        o.nev = opts.nev;
        o.ncv = opts.ncv > 0 ? opts.ncv
                             : static_cast<int>(std::min<std::int64_t>(
                                   {n, 64, std::max<std::int64_t>(2 * static_cast<std::int64_t>(opts.nev) + 1, 20)}));
        o.mode = opts.shiftInvert ? EIGSOL_KRYLOV_SHIFT_INVERT : EIGSOL_KRYLOV_LM;
        Vector<S> start;
        if (v0) {
            if (static_cast<std::int64_t>(v0->size()) != n)
                throw std::runtime_error(std::string(who) + ": start vector size mismatch");
        } else {
            start = random_vector<S>(static_cast<std::size_t>(n));
            v0 = &start;
        }
        const std::size_t k = static_cast<std::size_t>(std::max(opts.nev, 0));
        res.eigenvalues.assign(std::max<std::size_t>(k, 1), {});
        res.residuals.assign(std::max<std::size_t>(k, 1), 0.0);
        res.eigenvectors = DenseMatrix<std::complex<double>>(n, static_cast<std::int64_t>(k));
        std::int32_t rs = 0, ap = 0, conv = 0;
        const S shift = opts.shift;
        const int st = entry(&o, &shift, v0->data(), reinterpret_cast<double*>(res.eigenvalues.data()),
                             k ? reinterpret_cast<double*>(res.eigenvectors.data()) : nullptr, res.residuals.data(),
                             &rs, &ap, &conv);
        check(st, who);
        res.eigenvalues.resize(k);
        res.residuals.resize(k);
        res.restarts = rs;
        res.applications = ap;
        res.converged = conv != 0;
    }
    return res;
}

template <typename S>
KrylovResult<S> krylov_run(const Matrix& M, const KrylovOptions<S>& opts, const Vector<S>* v0) {
    const char* who = "krylovSchur";
    if (M.scalar_type() != typeid(S)) throw std::runtime_error(std::string(who) + ": scalar type mismatch");
    const std::int64_t n = M.rows();
    if (n != M.cols()) throw std::runtime_error(std::string(who) + ": matrix must be square");
    if (n == 0) throw std::runtime_error(std::string(who) + ": matrix has zero size");
    if (M.isDense()) throw std::runtime_error(std::string(who) + ": only sparse matrices are supported");
    return krylov_device<S>(n, opts, v0, who, [&](auto... a) {
        if constexpr (DeviceScalar<S>) return eigsol_krylov_csr(M.device<S>().csr(), a...);
        else return static_cast<int>(EIGSOL_E_UNSUPPORTED);
    });
}

template <typename S>
KrylovResult<S> krylov_run_dense(const DenseMatrix<S>& A, const KrylovOptions<S>& opts, const Vector<S>* v0) {
    const char* who = "krylovSchur_dense";
    const std::int64_t n = A.rows();
    if (n != A.cols()) throw std::runtime_error(std::string(who) + ": matrix must be square");
    if (n == 0) throw std::runtime_error(std::string(who) + ": matrix has zero size");
    return krylov_device<S>(n, opts, v0, who, [&](auto... a) {
        if constexpr (DeviceScalar<S>) {
            // on the device for this call: the handle is freed on every return, a throw included
            const std::shared_ptr<DeviceMatrix> d = DeviceMatrix::dense(dtype_of<S>(), n, n, A.data());
            return eigsol_krylov_dense(d->dense(), a...);
        } else {
            return static_cast<int>(EIGSOL_E_UNSUPPORTED);
        }
    });
}
}  // namespace detail

template <ScalarConcept S>
KrylovResult<S> krylovSchur(const Matrix& M, const KrylovOptions<S>& opts = KrylovOptions<S>{}) {
    return detail::krylov_run<S>(M, opts, nullptr);
}
template <ScalarConcept S>
KrylovResult<S> krylovSchur(const Matrix& M, const KrylovOptions<S>& opts, const Vector<S>& v0) {
    return detail::krylov_run<S>(M, opts, &v0);
}
template <ScalarConcept S>
KrylovResult<S> krylovSchur_dense(const DenseMatrix<S>& A, const KrylovOptions<S>& opts = KrylovOptions<S>{}) {
    return detail::krylov_run_dense<S>(A, opts, nullptr);
}
template <ScalarConcept S>
KrylovResult<S> krylovSchur_dense(const DenseMatrix<S>& A, const KrylovOptions<S>& opts, const Vector<S>& v0) {
    return detail::krylov_run_dense<S>(A, opts, &v0);
}

// ------------------------------------------------------------------------------------------ svds
// opts.nsv largest singular triplets of a sparse matrix of any shape by thick-restart Golub-Kahan-Lanczos
// (eigsol_svds_csr; the adjoint handle is built and destroyed inside the call).  S = double and
// std::complex<double>; the default start vector (cols() entries) is drawn with random_vector<S>.
// svds_dense takes a DenseMatrix<S> instead (eigsol_svds_dense), on the device for the duration of the call.
namespace detail {
// entry(o, v0, s, U, V, residuals, restarts, applications, converged) is the C entry bound to its handle
template <typename S, typename Entry>
SvdsResult<S> svds_device(std::int64_t rows, std::int64_t cols, const SvdsOptions& opts, const Vector<S>* v0,
                          const char* who, Entry&& entry) {
    SvdsResult<S> res;
    if constexpr (!DeviceScalar<S>) {
        throw std::runtime_error(std::string(who) + ": scalar type not supported by the device path "
                                                    "(double, std::complex<double>)");
    } else {
        eigsol_svds_options o;
        o.max_restarts = opts.maxRestarts;
        o.tolerance = opts.tolerance;
        o.nsv = opts.nsv;
        o.ncv = opts.ncv > 0 ? opts.ncv
                             : static_cast<int>(std::min<std::int64_t>(
                                   {std::min(rows, cols), 64,
                                    std::max<std::int64_t>(2 * static_cast<std::int64_t>(opts.nsv) + 1, 20)}));
        Vector<S> start;
        if (v0) {
            if (static_cast<std::int64_t>(v0->size()) != cols)
                throw std::runtime_error(std::string(who) + ": start vector size mismatch");
        } else {
            start = random_vector<S>(static_cast<std::size_t>(cols));
            v0 = &start;
        }
        const std::size_t k = static_cast<std::size_t>(std::max(opts.nsv, 0));
        res.s.assign(std::max<std::size_t>(k, 1), 0.0);
        res.residuals.assign(std::max<std::size_t>(k, 1), 0.0);
        const bool vec = opts.vectors && k > 0;
        if (vec) {
            res.U = DenseMatrix<S>(rows, static_cast<std::int64_t>(k));
            res.V = DenseMatrix<S>(cols, static_cast<std::int64_t>(k));
        }
        std::int32_t rs = 0, ap = 0, conv = 0;
        const int st = entry(&o, v0->data(), res.s.data(), vec ? static_cast<void*>(res.U.data()) : nullptr,
                             vec ? static_cast<void*>(res.V.data()) : nullptr, res.residuals.data(), &rs, &ap, &conv);
        check(st, who);
        res.s.resize(k);
        res.residuals.resize(k);
        res.restarts = rs;
        res.applications = ap;
        res.converged = conv != 0;
    }
    return res;
}

template <typename S>
SvdsResult<S> svds_run(const Matrix& M, const SvdsOptions& opts, const Vector<S>* v0) {
    const char* who = "svds";
    if (M.scalar_type() != typeid(S)) throw std::runtime_error(std::string(who) + ": scalar type mismatch");
    if (M.rows() == 0 || M.cols() == 0) throw std::runtime_error(std::string(who) + ": matrix has zero size");
    if (M.isDense()) throw std::runtime_error(std::string(who) + ": only sparse matrices are supported");
    return svds_device<S>(M.rows(), M.cols(), opts, v0, who, [&](auto... a) {
        if constexpr (DeviceScalar<S>) return eigsol_svds_csr(M.device<S>().csr(), nullptr, a...);
        else return static_cast<int>(EIGSOL_E_UNSUPPORTED);
    });
}

template <typename S>
SvdsResult<S> svds_run_dense(const DenseMatrix<S>& A, const SvdsOptions& opts, const Vector<S>* v0) {
    const char* who = "svds_dense";
    if (A.rows() == 0 || A.cols() == 0) throw std::runtime_error(std::string(who) + ": matrix has zero size");
    return svds_device<S>(A.rows(), A.cols(), opts, v0, who, [&](auto... a) {
        if constexpr (DeviceScalar<S>) {
            // on the device for this call: the handle is freed on every return, a throw included
            const std::shared_ptr<DeviceMatrix> d = DeviceMatrix::dense(dtype_of<S>(), A.rows(), A.cols(), A.data());
            return eigsol_svds_dense(d->dense(), a...);
        } else {
            return static_cast<int>(EIGSOL_E_UNSUPPORTED);
        }
    });
}
}  // namespace detail

template <ScalarConcept S>
SvdsResult<S> svds(const Matrix& M, const SvdsOptions& opts = {}) {
    return detail::svds_run<S>(M, opts, nullptr);
}
template <ScalarConcept S>
SvdsResult<S> svds(const Matrix& M, const SvdsOptions& opts, const Vector<S>& v0) {
    return detail::svds_run<S>(M, opts, &v0);
}
template <ScalarConcept S>
SvdsResult<S> svds_dense(const DenseMatrix<S>& A, const SvdsOptions& opts = {}) {
    return detail::svds_run_dense<S>(A, opts, nullptr);
}
template <ScalarConcept S>
SvdsResult<S> svds_dense(const DenseMatrix<S>& A, const SvdsOptions& opts, const Vector<S>& v0) {
    return detail::svds_run_dense<S>(A, opts, &v0);
}

// ------------------------------------------------------------------------------------------ eigh
// Eigenvalues (ascending) and an orthonormal set of eigenvectors of the real symmetric / complex
// Hermitian matrix whose lower triangle is A's (eigsol_eigh_dense: blocked Hessenberg reduction,
// bisection, inverse iteration, back-transformation; the strict upper triangle is not read).
// EighOptions::method = Method::DC takes the tridiagonal eigenpairs by divide and conquer instead.
// S = double and std::complex<double>.  eigvalsh returns the eigenvalues alone (no vectors are formed).
// With a second matrix B (Hermitian positive definite, its lower triangle read): A x = lambda B x
// (eigsol_geigh_dense: Cholesky B = L L^H, C = L^-1 A L^-H, the solver above, X = L^-H Y); the
// eigenvectors are then B-orthonormal (X^H B X = I).  A B that is not positive definite throws the
// library's message, which names the first column whose pivot is not > 0.  cholesky(B) returns L alone.
namespace detail {
template <typename S>
EighResult<S> eigh_run(const DenseMatrix<S>& A, const EighOptions& opts, bool vectors, const char* who,
                       const DenseMatrix<S>* B = nullptr) {
    EighResult<S> res;
    const std::int64_t n = A.rows();
    if (n != A.cols()) throw std::runtime_error(std::string(who) + ": matrix must be square");
    if (B && (B->rows() != n || B->cols() != n)) throw std::runtime_error(std::string(who) + ": B must be square and of A's order");
    if (n == 0) throw std::runtime_error(std::string(who) + ": matrix has zero size");
    if constexpr (!DeviceScalar<S>) {
        throw std::runtime_error(std::string(who) + ": scalar type not supported by the device path "
                                                    "(double, std::complex<double>)");
    } else {
        eigsol_eigh_options o;
        o.select = opts.select == EighOptions::Select::Index   ? EIGSOL_EIGH_INDEX
                   : opts.select == EighOptions::Select::Value ? EIGSOL_EIGH_VALUE
                                                               : EIGSOL_EIGH_ALL;
        o.il = opts.il;
        o.iu = opts.iu;
        o.vl = opts.vl;
        o.vu = opts.vu;
        res.eigenvalues.assign(static_cast<std::size_t>(n), 0.0);
        DenseMatrix<S> Z;
        if (vectors) Z = DenseMatrix<S>(n, n);
        std::int64_t m = 0, nc = 0;
        void* zp = vectors ? static_cast<void*>(Z.data()) : nullptr;
        const std::int32_t method = opts.method == EighOptions::Method::DC ? EIGSOL_EIGH_METHOD_DC : EIGSOL_EIGH_METHOD_STEIN;
        if (B)
            check(eigsol_geigh_dense_m(ctx(), dtype_of<S>(), n, A.data(), B->data(), &o, method, res.eigenvalues.data(), zp,
                                       &m, &nc, nullptr),
                  who);
        else
            check(eigsol_eigh_dense_m(ctx(), dtype_of<S>(), n, A.data(), &o, method, res.eigenvalues.data(), zp, &m, &nc),
                  who);
        res.eigenvalues.resize(static_cast<std::size_t>(m));
        res.notConverged = nc;
        if (vectors) {
            res.eigenvectors = DenseMatrix<S>(n, m);
            for (std::int64_t j = 0; j < m; ++j)
                for (std::int64_t i = 0; i < n; ++i) res.eigenvectors(i, j) = Z(i, j);
        }
    }
    return res;
}
}  // namespace detail

template <ScalarConcept S>
EighResult<S> eigh(const DenseMatrix<S>& A, const EighOptions& opts = {}) {
    return detail::eigh_run<S>(A, opts, true, "eigh");
}
template <ScalarConcept S>
std::vector<double> eigvalsh(const DenseMatrix<S>& A, const EighOptions& opts = {}) {
    return detail::eigh_run<S>(A, opts, false, "eigvalsh").eigenvalues;
}
template <ScalarConcept S>
EighResult<S> eigh(const DenseMatrix<S>& A, const DenseMatrix<S>& B, const EighOptions& opts = {}) {
    return detail::eigh_run<S>(A, opts, true, "eigh", &B);
}
template <ScalarConcept S>
std::vector<double> eigvalsh(const DenseMatrix<S>& A, const DenseMatrix<S>& B, const EighOptions& opts = {}) {
    return detail::eigh_run<S>(A, opts, false, "eigvalsh", &B).eigenvalues;
}
// ------------------------------------------------------------------------------------------- eig
// Eigenvalues and right eigenvectors of a general dense matrix (eigsol_eig_dense: blocked Hessenberg reduction,
// the Francis sweeps of qr_eigenvalues on a copy of H, inverse iteration on H, back-transformation).
// S = double and std::complex<double>; the vectors are complex for both.  Column j of eigenvectors belongs
// to eigenvalues[select[j]] (eigenvalues[j] without a selection); a selection returns the full call's bits.
template <ScalarConcept S>
EigResult<S> eig(const DenseMatrix<S>& A, const EigOptions& opts = {}) {
    EigResult<S> res;
    const std::int64_t n = A.rows();
    if (n != A.cols()) throw std::runtime_error("eig: matrix must be square");
    if (n == 0) throw std::runtime_error("eig: matrix has zero size");
    if constexpr (!DeviceScalar<S>) {
        throw std::runtime_error("eig: scalar type not supported by the device path (double, std::complex<double>)");
    } else {
        eigsol_eig_options o;
        o.max_iterations = opts.maxIterations;
        o.batch = opts.batch;
        o.nsel = static_cast<std::int64_t>(opts.select.size());
        o.sel = opts.select.empty() ? nullptr : opts.select.data();
        const std::int64_t cap = opts.select.empty() ? n : o.nsel;
        res.eigenvalues.assign(static_cast<std::size_t>(n), std::complex<double>(0.0, 0.0));
        DenseMatrix<std::complex<double>> V;
        if (opts.vectors) V = DenseMatrix<std::complex<double>>(n, cap);
        std::int64_t m = 0, nc = 0;
        std::int32_t it = 0, conv = 0;
        detail::check(eigsol_eig_dense(detail::ctx(), detail::dtype_of<S>(), n, A.data(), &o,
                                       reinterpret_cast<double*>(res.eigenvalues.data()),
                                       opts.vectors ? static_cast<void*>(V.data()) : nullptr, &m, &it, &conv, &nc),
                      "eig");
        res.iterations = it;
        res.converged = conv != 0;
        res.notConverged = nc;
        if (opts.vectors) res.eigenvectors = std::move(V);
    }
    return res;
}

// ------------------------------------------------------------------------------------------- schur
// Schur form A = Z T Z^H of a general dense matrix (eigsol_schur_dense: blocked Hessenberg reduction, Q on the
// matrix cores, the sweeps of qr_eigenvalues applied to the whole of T and to Z, standard 2 x 2 blocks).  A real
// S gives the real Schur form, a complex S the complex one.  float and std::complex<float> run on their fp64
// promotion; T and Z are rounded back, the eigenvalues stay in double.
template <ScalarConcept S>
SchurResult<S> schur(const DenseMatrix<S>& A, const SchurOptions& opts = {}) {
    const std::int64_t n = A.rows();
    if (n != A.cols()) throw std::runtime_error("schur: matrix must be square");
    if (n == 0) throw std::runtime_error("schur: matrix has zero size");
    if constexpr (PromotedScalar<S>) {
        using D = device_scalar_t<S>;
        SchurResult<D> rd = schur<D>(detail::convert_dense<D>(A), opts);
        SchurResult<S> rs;
        rs.T = detail::convert_dense<S>(rd.T);
        if (opts.vectors) rs.Z = detail::convert_dense<S>(rd.Z);
        rs.eigenvalues = std::move(rd.eigenvalues);
        rs.iterations = rd.iterations;
        rs.converged = rd.converged;
        rs.sdim = rd.sdim;
        rs.ordered = rd.ordered;
        return rs;
    } else if constexpr (!DeviceScalar<S>) {
        throw std::runtime_error("schur: scalar type not supported by the device path (double, std::complex<double>)");
    } else {
        SchurResult<S> res;
        eigsol_solver_options o{};
        o.max_iterations = opts.maxIterations;
        res.T = DenseMatrix<S>(n, n);
        if (opts.vectors) res.Z = DenseMatrix<S>(n, n);
        res.eigenvalues.assign(static_cast<std::size_t>(n), std::complex<double>(0.0, 0.0));
        std::vector<double> wr(static_cast<std::size_t>(n), 0.0), wi(static_cast<std::size_t>(n), 0.0);
        constexpr bool real = std::is_floating_point_v<S>;
        std::int32_t it = 0, conv = 0, ord = 0;
        std::int64_t sdim = 0;
        void* const zp = opts.vectors ? static_cast<void*>(res.Z.data()) : nullptr;
        void* const wp = real ? static_cast<void*>(wr.data()) : static_cast<void*>(res.eigenvalues.data());
        if (opts.sort == SchurSort::None)
            detail::check(eigsol_schur_dense(detail::ctx(), detail::dtype_of<S>(), n, A.data(), &o, res.T.data(), zp, wp, wi.data(),
                                             &it, &conv),
                          "schur");
        else
            detail::check(eigsol_schur_sorted_dense(detail::ctx(), detail::dtype_of<S>(), n, A.data(), &o,
                                                    static_cast<int>(opts.sort), res.T.data(), zp, wp, wi.data(), &sdim, &it, &conv,
                                                    &ord),
                          "schur");
        res.sdim = sdim;
        res.ordered = ord != 0;
        if constexpr (real)
            for (std::size_t i = 0; i < wr.size(); ++i) res.eigenvalues[i] = std::complex<double>(wr[i], wi[i]);
        res.iterations = it;
        res.converged = conv != 0;
        return res;
    }
}

// ---------------------------------------------------------------------------------------- ordschur
// Reorders a Schur form so that the selected eigenvalues lead T (eigsol_ordschur_dense; LAPACK xTRSEN without its
// condition estimates): select holds one flag per row of T; for a real T a flag on either row of a 2 x 2 block
// selects the pair.  Z is updated where the input has one.  iterations / converged are carried over; sdim and
// ordered are the reordering's.  float and std::complex<float> run on their fp64 promotion, as in schur.
template <ScalarConcept S>
SchurResult<S> ordschur(const SchurResult<S>& in, const std::vector<bool>& select) {
    const std::int64_t n = in.T.rows();
    if (n != in.T.cols()) throw std::runtime_error("ordschur: T must be square");
    if (static_cast<std::int64_t>(select.size()) != n) throw std::runtime_error("ordschur: select needs one flag per row of T");
    const bool vectors = in.Z.rows() == n && in.Z.cols() == n && n > 0;
    if constexpr (PromotedScalar<S>) {
        using D = device_scalar_t<S>;
        SchurResult<D> id;
        id.T = detail::convert_dense<D>(in.T);
        if (vectors) id.Z = detail::convert_dense<D>(in.Z);
        id.iterations = in.iterations;
        id.converged = in.converged;
        SchurResult<D> rd = ordschur<D>(id, select);
        SchurResult<S> rs;
        rs.T = detail::convert_dense<S>(rd.T);
        if (vectors) rs.Z = detail::convert_dense<S>(rd.Z);
        rs.eigenvalues = std::move(rd.eigenvalues);
        rs.iterations = rd.iterations;
        rs.converged = rd.converged;
        rs.sdim = rd.sdim;
        rs.ordered = rd.ordered;
        return rs;
    } else if constexpr (!DeviceScalar<S>) {
        throw std::runtime_error("ordschur: scalar type not supported by the device path (double, std::complex<double>)");
    } else {
        SchurResult<S> res = in;
        std::vector<std::uint8_t> sel(static_cast<std::size_t>(n), 0);
        for (std::size_t i = 0; i < sel.size(); ++i) sel[i] = select[i] ? 1 : 0;
        res.eigenvalues.assign(static_cast<std::size_t>(n), std::complex<double>(0.0, 0.0));
        std::vector<double> wr(static_cast<std::size_t>(n), 0.0), wi(static_cast<std::size_t>(n), 0.0);
        constexpr bool real = std::is_floating_point_v<S>;
        std::int32_t ord = 0;
        std::int64_t sdim = 0;
        detail::check(eigsol_ordschur_dense(detail::ctx(), detail::dtype_of<S>(), n, res.T.data(),
                                            vectors ? static_cast<void*>(res.Z.data()) : nullptr, sel.data(),
                                            real ? static_cast<void*>(wr.data()) : static_cast<void*>(res.eigenvalues.data()),
                                            wi.data(), &sdim, &ord),
                      "ordschur");
        if constexpr (real)
            for (std::size_t i = 0; i < wr.size(); ++i) res.eigenvalues[i] = std::complex<double>(wr[i], wi[i]);
        res.sdim = sdim;
        res.ordered = ord != 0;
        return res;
    }
}

// ------------------------------------------------------------------------------- sylvester, lyapunov
// A X + X B = C (solve_sylvester, eigsol_sylvester_dense) and A X + X A^H = Q (solve_lyapunov,
// eigsol_lyapunov_dense) by Bartels-Stewart on the device: the Schur forms by schur's pipeline, the
// quasi-triangular equation by wavefronts of block solves and rank-K updates, the transforms on the matrix cores.
// opts.maxIterations bounds the sweeps of each Schur factorisation; opts.vectors is not read.  Throws if a
// factorisation does not converge.  float and std::complex<float> run on their fp64 promotion; X is rounded back.
namespace detail {
template <ScalarConcept S>
SylvesterResult<S> sylvester_run(const char* who, const DenseMatrix<S>& A, const DenseMatrix<S>* B, const DenseMatrix<S>& C,
                                 const SchurOptions& opts) {
    const std::int64_t m = A.rows(), n = B ? B->rows() : A.rows();
    if (m != A.cols() || (B && n != B->cols())) throw std::runtime_error(std::string(who) + ": matrix must be square");
    if (C.rows() != m || C.cols() != n) throw std::runtime_error(std::string(who) + ": the right-hand side does not fit");
    if (m == 0 || n == 0) throw std::runtime_error(std::string(who) + ": matrix has zero size");
    if constexpr (PromotedScalar<S>) {
        using D = device_scalar_t<S>;
        const DenseMatrix<D> Ad = convert_dense<D>(A), Cd = convert_dense<D>(C);
        SylvesterResult<D> rd;
        if (B) {
            const DenseMatrix<D> Bd = convert_dense<D>(*B);
            rd = sylvester_run<D>(who, Ad, &Bd, Cd, opts);
        } else {
            rd = sylvester_run<D>(who, Ad, nullptr, Cd, opts);
        }
        SylvesterResult<S> rs;
        rs.X = convert_dense<S>(rd.X);
        rs.perturbed = rd.perturbed;
        rs.converged = rd.converged;
        return rs;
    } else if constexpr (!DeviceScalar<S>) {
        throw std::runtime_error(std::string(who) + ": scalar type not supported by the device path (double, std::complex<double>)");
    } else {
        SylvesterResult<S> res;
        eigsol_solver_options o{};
        o.max_iterations = opts.maxIterations;
        res.X = DenseMatrix<S>(m, n);
        std::int32_t pert = 0, conv = 0;
        if (B)
            check(eigsol_sylvester_dense(ctx(), dtype_of<S>(), m, n, A.data(), B->data(), C.data(), &o, res.X.data(), &pert, &conv), who);
        else
            check(eigsol_lyapunov_dense(ctx(), dtype_of<S>(), m, A.data(), C.data(), &o, res.X.data(), &pert, &conv), who);
        if (!conv) throw std::runtime_error(std::string(who) + ": a Schur factorisation did not converge");
        res.perturbed = pert;
        res.converged = true;
        return res;
    }
}
}  // namespace detail

template <ScalarConcept S>
SylvesterResult<S> solve_sylvester(const DenseMatrix<S>& A, const DenseMatrix<S>& B, const DenseMatrix<S>& C,
                                   const SchurOptions& opts = {}) {
    return detail::sylvester_run<S>("solve_sylvester", A, &B, C, opts);
}

template <ScalarConcept S>
SylvesterResult<S> solve_lyapunov(const DenseMatrix<S>& A, const DenseMatrix<S>& Q, const SchurOptions& opts = {}) {
    return detail::sylvester_run<S>("solve_lyapunov", A, nullptr, Q, opts);
}

// ------------------------------------------------------------------------------------------- sqrtm
// Principal square root X of a square A (eigsol_sqrtm_dense; scipy.linalg.sqrtm): X X = A with every eigenvalue of
// X in the closed right half plane, through the Schur form on the device: schur's pipeline, the blocked
// triangular square root, the back-transformation on the matrix cores.  A real A keeps a real root wherever one
// exists.  Where the library reports a negative real eigenvalue (no real root), the call runs again on A cast to
// complex and the root comes in Xc with isComplex set; that costs a second Schur factorisation.
// opts.maxIterations bounds the sweeps; opts.vectors and opts.sort are not read.  Throws if the factorisation does
// not converge.  float and std::complex<float> run on their fp64 promotion; the root is rounded back.
template <ScalarConcept S>
SqrtmResult<S> sqrtm(const DenseMatrix<S>& A, const SchurOptions& opts = {}) {
    const std::int64_t n = A.rows();
    if (n != A.cols()) throw std::runtime_error("sqrtm: matrix must be square");
    if (n == 0) throw std::runtime_error("sqrtm: matrix has zero size");
    if constexpr (PromotedScalar<S>) {
        using D = device_scalar_t<S>;
        SqrtmResult<D> rd = sqrtm<D>(detail::convert_dense<D>(A), opts);
        SqrtmResult<S> rs;
        if (rd.isComplex) rs.Xc = detail::convert_dense<typename SqrtmResult<S>::Complex>(rd.Xc);
        else rs.X = detail::convert_dense<S>(rd.X);
        rs.isComplex = rd.isComplex;
        rs.perturbed = rd.perturbed;
        rs.converged = rd.converged;
        return rs;
    } else if constexpr (!DeviceScalar<S>) {
        throw std::runtime_error("sqrtm: scalar type not supported by the device path (double, std::complex<double>)");
    } else {
        SqrtmResult<S> res;
        eigsol_solver_options o{};
        o.max_iterations = opts.maxIterations;
        res.X = DenseMatrix<S>(n, n);
        std::int32_t pert = 0, conv = 0, cx = 0;
        detail::check(eigsol_sqrtm_dense(detail::ctx(), detail::dtype_of<S>(), n, A.data(), &o, res.X.data(), &pert, &conv, &cx), "sqrtm");
        if (!conv) throw std::runtime_error("sqrtm: the Schur factorisation did not converge");
        if constexpr (std::is_floating_point_v<S>) {
            if (cx) {
                using Z = typename SqrtmResult<S>::Complex;
                SqrtmResult<Z> rc = sqrtm<Z>(detail::convert_dense<Z>(A), opts);
                res.X = DenseMatrix<S>();
                res.Xc = std::move(rc.X);
                res.isComplex = true;
                res.perturbed = rc.perturbed;
                res.converged = rc.converged;
                return res;
            }
        }
        res.perturbed = pert;
        res.converged = true;
        return res;
    }
}

// ------------------------------------------------------------------------------------------- logm
// Principal logarithm X of a square A (eigsol_logm_dense; scipy.linalg.logm): exp(X) = A with the imaginary part of
// every eigenvalue of X in (-pi, pi], through the Schur form on the device: schur's pipeline, the inverse scaling
// and squaring logarithm of the triangular factor, the back-transformation on the matrix cores.  A real A keeps a
// real logarithm wherever one exists.  Where the library reports a negative real eigenvalue, the call runs again on A
// cast to complex and the logarithm comes in Xc with isComplex set; that costs a second Schur factorisation.
// opts.maxIterations bounds the sweeps; opts.vectors and opts.sort are not read.  Throws if the factorisation does
// not converge or A is singular.  float and std::complex<float> run on their fp64 promotion; X is rounded back.
template <ScalarConcept S>
LogmResult<S> logm(const DenseMatrix<S>& A, const SchurOptions& opts = {}) {
    const std::int64_t n = A.rows();
    if (n != A.cols()) throw std::runtime_error("logm: matrix must be square");
    if (n == 0) throw std::runtime_error("logm: matrix has zero size");
    if constexpr (PromotedScalar<S>) {
        using D = device_scalar_t<S>;
        LogmResult<D> rd = logm<D>(detail::convert_dense<D>(A), opts);
        LogmResult<S> rs;
        if (rd.isComplex) rs.Xc = detail::convert_dense<typename LogmResult<S>::Complex>(rd.Xc);
        else rs.X = detail::convert_dense<S>(rd.X);
        rs.isComplex = rd.isComplex;
        rs.roots = rd.roots;
        rs.degree = rd.degree;
        rs.perturbed = rd.perturbed;
        rs.converged = rd.converged;
        return rs;
    } else if constexpr (!DeviceScalar<S>) {
        throw std::runtime_error("logm: scalar type not supported by the device path (double, std::complex<double>)");
    } else {
        LogmResult<S> res;
        eigsol_solver_options o{};
        o.max_iterations = opts.maxIterations;
        res.X = DenseMatrix<S>(n, n);
        std::int32_t roots = 0, degree = 0, pert = 0, conv = 0, cx = 0;
        detail::check(eigsol_logm_dense(detail::ctx(), detail::dtype_of<S>(), n, A.data(), &o, res.X.data(), &roots, &degree, &pert,
                                        &conv, &cx),
                      "logm");
        if (!conv) throw std::runtime_error("logm: the Schur factorisation did not converge");
        if constexpr (std::is_floating_point_v<S>) {
            if (cx) {
                using Z = typename LogmResult<S>::Complex;
                LogmResult<Z> rc = logm<Z>(detail::convert_dense<Z>(A), opts);
                res.X = DenseMatrix<S>();
                res.Xc = std::move(rc.X);
                res.isComplex = true;
                res.roots = rc.roots;
                res.degree = rc.degree;
                res.perturbed = rc.perturbed;
                res.converged = rc.converged;
                return res;
            }
        }
        res.roots = roots;
        res.degree = degree;
        res.perturbed = pert;
        res.converged = true;
        return res;
    }
}

// ------------------------------------------------------------------------------------ solve, expm
// X with A X = B by LU with partial pivoting on the device (eigsol_solve_dense): the blocked factorisation of the
// shifted solves and a blocked substitution with all columns of B.  Throws where a pivot is exactly zero; the
// message names its column.  float and std::complex<float> run on their fp64 promotion; X is rounded back.
template <ScalarConcept S>
DenseMatrix<S> solve(const DenseMatrix<S>& A, const DenseMatrix<S>& B) {
    const std::int64_t n = A.rows();
    if (n != A.cols()) throw std::runtime_error("solve: matrix must be square");
    if (B.rows() != n) throw std::runtime_error("solve: size mismatch between A and B");
    if (n == 0 || B.cols() == 0) throw std::runtime_error("solve: matrix has zero size");
    if constexpr (PromotedScalar<S>) {
        using D = device_scalar_t<S>;
        return detail::convert_dense<S>(solve<D>(detail::convert_dense<D>(A), detail::convert_dense<D>(B)));
    } else if constexpr (!DeviceScalar<S>) {
        throw std::runtime_error("solve: scalar type not supported by the device path (double, std::complex<double>)");
    } else {
        DenseMatrix<S> X(n, B.cols());
        detail::check(eigsol_solve_dense(detail::ctx(), detail::dtype_of<S>(), n, B.cols(), A.data(), B.data(), X.data()), "solve");
        return X;
    }
}

// exp(A) of a square A (eigsol_expm_dense; scipy.linalg.expm): Higham's 2005 scaling and squaring on the device.
// The 1-norm decides the degree of the Pade approximant and the squarings; a real A gives a real X.  Throws on a
// non-finite entry and on a result that overflows.  float and std::complex<float> run on their fp64 promotion.
template <ScalarConcept S>
ExpmResult<S> expm(const DenseMatrix<S>& A) {
    const std::int64_t n = A.rows();
    if (n != A.cols()) throw std::runtime_error("expm: matrix must be square");
    if (n == 0) throw std::runtime_error("expm: matrix has zero size");
    if constexpr (PromotedScalar<S>) {
        using D = device_scalar_t<S>;
        ExpmResult<D> rd = expm<D>(detail::convert_dense<D>(A));
        ExpmResult<S> rs;
        rs.X = detail::convert_dense<S>(rd.X);
        rs.degree = rd.degree;
        rs.squarings = rd.squarings;
        return rs;
    } else if constexpr (!DeviceScalar<S>) {
        throw std::runtime_error("expm: scalar type not supported by the device path (double, std::complex<double>)");
    } else {
        ExpmResult<S> res;
        res.X = DenseMatrix<S>(n, n);
        std::int32_t m = 0, s = 0;
        detail::check(eigsol_expm_dense(detail::ctx(), detail::dtype_of<S>(), n, A.data(), res.X.data(), &m, &s), "expm");
        res.degree = m;
        res.squarings = s;
        return res;
    }
}

// ------------------------------------------------------------------------------------------- svd
// Thin singular value decomposition A = U diag(s) V^H of a dense m x n matrix (eigsol_svd_dense: block one-sided
// Jacobi on the fp64 matrix cores).  S = double and std::complex<double>.  svdvals returns the bits of svd's s.
namespace detail {
template <ScalarConcept S>
SvdResult<S> svd_run(const DenseMatrix<S>& A, const SvdOptions& opts, bool vectors, const char* who) {
    SvdResult<S> res;
    const std::int64_t m = A.rows(), n = A.cols();
    if (m == 0 || n == 0) throw std::runtime_error(std::string(who) + ": matrix has zero size");
    if constexpr (!DeviceScalar<S>) {
        throw std::runtime_error(std::string(who) +
                                 ": scalar type not supported by the device path (double, std::complex<double>)");
    } else {
        const std::int64_t k = std::min(m, n);
        eigsol_svd_options o;
        o.max_sweeps = opts.maxSweeps;
        res.s.assign(static_cast<std::size_t>(k), 0.0);
        DenseMatrix<S> U, V;
        if (vectors) {
            U = DenseMatrix<S>(m, k);
            V = DenseMatrix<S>(n, k);
        }
        std::int32_t sw = 0;
        std::int64_t nc = 0;
        detail::check(eigsol_svd_dense(detail::ctx(), detail::dtype_of<S>(), m, n, A.data(), &o, res.s.data(),
                                       vectors ? static_cast<void*>(U.data()) : nullptr,
                                       vectors ? static_cast<void*>(V.data()) : nullptr, &sw, &nc),
                      who);
        res.sweeps = sw;
        res.not_converged = nc;
        if (vectors) {
            res.U = std::move(U);
            res.V = std::move(V);
        }
    }
    return res;
}
}  // namespace detail
template <ScalarConcept S>
SvdResult<S> svd(const DenseMatrix<S>& A, const SvdOptions& opts = {}) {
    return detail::svd_run<S>(A, opts, true, "svd");
}
template <ScalarConcept S>
std::vector<double> svdvals(const DenseMatrix<S>& A, const SvdOptions& opts = {}) {
    return detail::svd_run<S>(A, opts, false, "svdvals").s;
}

// L of B = L L^H (eigsol_cholesky_dense): zero strict upper triangle, real positive diagonal.
template <ScalarConcept S>
DenseMatrix<S> cholesky(const DenseMatrix<S>& B) {
    const std::int64_t n = B.rows();
    if (n != B.cols()) throw std::runtime_error("cholesky: matrix must be square");
    if (n == 0) throw std::runtime_error("cholesky: matrix has zero size");
    if constexpr (!DeviceScalar<S>) {
        throw std::runtime_error("cholesky: scalar type not supported by the device path (double, std::complex<double>)");
    } else {
        DenseMatrix<S> L(n, n);
        detail::check(eigsol_cholesky_dense(detail::ctx(), detail::dtype_of<S>(), n, B.data(), L.data(), nullptr), "cholesky");
        return L;
    }
}

// --------------------------------------------------------------------------------- solve_shifted
template <ScalarConcept S>
Vector<S> solve_shifted(const Matrix& A, const S shift, const Vector<S>& b) {
    if (A.scalar_type() != typeid(S)) throw std::runtime_error("solve_shifted: scalar type mismatch");
    const char* kind = A.isDense() ? "dense" : "sparse";
    if (A.rows() != A.cols())
        throw std::runtime_error(std::string("solve_shifted: A must be square (") + kind + " case)");
    if (A.rows() != static_cast<std::int64_t>(b.size()))
        throw std::runtime_error(std::string("solve_shifted: size mismatch between A and b (") + kind + " case)");
    detail::require_device_scalar<S>("solve_shifted");
    Vector<S> x(b.size());
    if constexpr (DeviceCapable<S>) {
        if (b.size() == 0) return x;
        const std::int64_t n = static_cast<std::int64_t>(b.size());
        auto run = [&](auto tag, const detail::DeviceMatrix& d) {
            using D = decltype(tag);
            const D sh = static_cast<D>(shift);
            const Vector<D> bd = detail::convert_vec<D>(b);
            Vector<D> xd(b.size());
            const int st = A.isDense() ? eigsol_solve_shifted_dense(d.dense(), &sh, bd.data(), n, xd.data())
                                       : eigsol_solve_shifted_csr(d.csr(), &sh, bd.data(), n, xd.data());
            if (st == EIGSOL_OK) x = detail::convert_vec<S>(xd);
            return st;
        };
        // single precision natively (dense, banded and triangular factors in float); the fp64
        // factor only where the single-precision one is not built (general sparse via GMRES)
        int st = EIGSOL_E_UNSUPPORTED;
        if constexpr (WideScalar<S>) {   // double-double pairs in and out
            const detail::DeviceMatrix& d = A.device<S>();
            const wire_t<S> sh = to_wire(shift);
            const auto bw = to_wire_vec(b.data(), b.size());
            std::vector<wire_t<S>> xw(b.size());
            st = A.isDense() ? eigsol_solve_shifted_dense(d.dense(), &sh, bw.data(), n, xw.data())
                             : eigsol_solve_shifted_csr(d.csr(), &sh, bw.data(), n, xw.data());
            if (st == EIGSOL_OK)
                for (std::size_t i = 0; i < xw.size(); ++i) x(i) = from_wire(xw[i]);
        } else {
            st = run(S{}, A.device<S>());
        }
        if constexpr (PromotedScalar<S>)
            if (st == EIGSOL_E_UNSUPPORTED) st = run(device_scalar_t<S>{}, A.device_fp64<S>());
        detail::check(st, "solve_shifted");
    }
    return x;
}

// ------------------------------------------------------------------------------------ QR method
template <ScalarConcept S>
DenseMatrix<S> to_hessenberg_dense(const DenseMatrix<S>& A) {
    detail::dense_square_check(A, "to_hessenberg_dense");
    detail::require_device_scalar<S>("to_hessenberg_dense");
    DenseMatrix<S> H(A.rows(), A.cols());
    if constexpr (WideScalar<S>) {   // double-double reflectors
        if (A.rows() > 0) {
            const auto aw = to_wire_vec(A.data(), static_cast<std::size_t>(A.size()));
            std::vector<wire_t<S>> hw(aw.size());
            detail::check(eigsol_hessenberg_dense(detail::ctx(), detail::dtype_of<S>(), A.rows(), aw.data(), hw.data()),
                          "to_hessenberg_dense");
            for (std::size_t i = 0; i < hw.size(); ++i) H.data()[i] = from_wire(hw[i]);
        }
        return H;
    }
    if constexpr (DeviceScalar<S> || PromotedScalar<S>) {   // single precision: native float reduction
        if (A.rows() > 0)
            detail::check(eigsol_hessenberg_dense(detail::ctx(), detail::dtype_of<S>(), A.rows(), A.data(), H.data()),
                          "to_hessenberg_dense");
    }
    return H;
}

template <ScalarConcept S>
DenseMatrix<S> to_hessenberg(const Matrix& A) {
    if (!A.isDense()) throw std::runtime_error("to_hessenberg(Matrix): only dense matrices are supported");
    if (A.scalar_type() != typeid(S)) throw std::runtime_error("to_hessenberg(Matrix): scalar type mismatch");
    return to_hessenberg_dense<S>(A.cast<DenseMatrix<S>>());
}

template <ScalarConcept S>
void qr_decompose_dense(const DenseMatrix<S>& A, DenseMatrix<S>& Q, DenseMatrix<S>& R) {
    if (A.rows() == 0 || A.cols() == 0) throw std::runtime_error("qr_decompose_dense: empty matrix");
    detail::require_device_scalar<S>("qr_decompose_dense");
    if constexpr (WideScalar<S>) {   // double-double reflectors
        const auto aw = to_wire_vec(A.data(), static_cast<std::size_t>(A.size()));
        std::vector<wire_t<S>> qw(static_cast<std::size_t>(A.rows() * A.rows())), rw(aw.size());
        detail::check(eigsol_qr_decompose_dense(detail::ctx(), detail::dtype_of<S>(), A.rows(), A.cols(), aw.data(),
                                                qw.data(), rw.data()),
                      "qr_decompose_dense");
        Q = DenseMatrix<S>(A.rows(), A.rows());
        R = DenseMatrix<S>(A.rows(), A.cols());
        for (std::size_t i = 0; i < qw.size(); ++i) Q.data()[i] = from_wire(qw[i]);
        for (std::size_t i = 0; i < rw.size(); ++i) R.data()[i] = from_wire(rw[i]);
        return;
    }
    Q = DenseMatrix<S>(A.rows(), A.rows());
    R = DenseMatrix<S>(A.rows(), A.cols());
    if constexpr (DeviceScalar<S> || PromotedScalar<S>)   // single precision: native float QR
        detail::check(eigsol_qr_decompose_dense(detail::ctx(), detail::dtype_of<S>(), A.rows(), A.cols(), A.data(),
                                                Q.data(), R.data()),
                      "qr_decompose_dense");
}

template <ScalarConcept S>
std::pair<DenseMatrix<S>, DenseMatrix<S>> qr_decompose(const Matrix& A) {
    if (!A.isDense()) throw std::runtime_error("qr_decompose(Matrix): only dense matrices are supported");
    if (A.scalar_type() != typeid(S)) throw std::runtime_error("qr_decompose(Matrix): scalar type mismatch");
    DenseMatrix<S> Q, R;
    qr_decompose_dense<S>(A.cast<DenseMatrix<S>>(), Q, R);
    return {Q, R};
}

template <ScalarConcept S>
QRResult<S> qr_eigenvalues_dense(const DenseMatrix<S>& A, const SolverOptions& opts,
                                 QRVariant variant = QRVariant::Francis) {
    detail::dense_square_check(A, "qr_eigenvalues_dense");
    const std::int64_t n = A.rows();
    if (n == 0) return QRResult<S>(Vector<S>(), 0, true);   // qr_eigenvalues.hpp:55-57
    detail::require_device_scalar<S>("qr_eigenvalues_dense");
    if constexpr (WideScalar<S>) {
        // long double: Unshifted = the reference's own algorithm (H <- R Q, qr_eigenvalues.hpp:62-105)
        // in double-double; Francis = the fp64 multishift sweeps on the rounded double-double
        // Hessenberg matrix, every eigenvalue then refined in double-double by Newton's method on
        // det(H - mu I) (wide.hip), so no eigenvalue keeps fp64 accuracy only
        const auto aw = to_wire_vec(A.data(), static_cast<std::size_t>(A.size()));
        std::vector<wire_t<S>> ew(static_cast<std::size_t>(n));
        std::vector<double> eim(2 * static_cast<std::size_t>(n), 0.0);   // real long double: imaginary dd parts
        std::int32_t it = 0, conv = 0;
        const eigsol_solver_options o = detail::copts(opts);
        const bool francis = variant == QRVariant::Francis;
        detail::check(eigsol_qr_eigenvalues_dense(detail::ctx(), detail::dtype_of<S>(), n, aw.data(), &o,
                                                  static_cast<int>(variant), ew.data(),
                                                  francis ? eim.data() : nullptr, &it, &conv),
                      "qr_eigenvalues_dense");
        Vector<S> ev(static_cast<std::size_t>(n));
        for (std::int64_t i = 0; i < n; ++i) ev(i) = from_wire(ew[static_cast<std::size_t>(i)]);
        QRResult<S> r(ev, it, conv != 0);
        if (francis) {
            r.eigenvalues_complex_extended.resize(static_cast<std::size_t>(n));
            r.eigenvalues_complex.resize(static_cast<std::size_t>(n));
            for (std::int64_t i = 0; i < n; ++i) {
                std::complex<long double> z;
                if constexpr (std::is_same_v<S, long double>)
                    z = {ev(i), static_cast<long double>(eim[2 * i]) + static_cast<long double>(eim[2 * i + 1])};
                else z = ev(i);
                r.eigenvalues_complex_extended[i] = z;
                r.eigenvalues_complex[i] = {static_cast<double>(z.real()), static_cast<double>(z.imag())};
            }
        }
        return r;
    }
    // single precision: the reference's unshifted iteration natively in float; the Francis sweeps
    // (double kernels) on the fp64 promotion, eigenvalues rounded back
    if constexpr (PromotedScalar<S>) if (variant == QRVariant::Francis) {
        using D = device_scalar_t<S>;
        const QRResult<D> rd = qr_eigenvalues_dense<D>(detail::convert_dense<D>(A), opts, variant);
        QRResult<S> rs(detail::convert_vec<S>(rd.eigenvalues), rd.iterations, rd.converged);
        rs.eigenvalues_complex = rd.eigenvalues_complex;
        return rs;
    }
    QRResult<S> res;
    if constexpr (DeviceScalar<S> || PromotedScalar<S>) {
        Vector<S> ev(static_cast<std::size_t>(n));
        std::vector<double> wi(static_cast<std::size_t>(n), 0.0);
        std::int32_t it = 0, conv = 0;
        const eigsol_solver_options o = detail::copts(opts);
        detail::check(eigsol_qr_eigenvalues_dense(detail::ctx(), detail::dtype_of<S>(), n, A.data(), &o,
                                                  static_cast<int>(variant), ev.data(), wi.data(), &it, &conv),
                      "qr_eigenvalues_dense");
        res = QRResult<S>(ev, it, conv != 0);
        if (variant == QRVariant::Francis) {
            res.eigenvalues_complex.resize(static_cast<std::size_t>(n));
            for (std::int64_t i = 0; i < n; ++i) {
                if constexpr (std::is_same_v<S, double>) res.eigenvalues_complex[i] = {ev(i), wi[i]};
                else res.eigenvalues_complex[i] = ev(i);   // complex sweeps return the eigenvalues themselves
            }
        }
    }
    return res;
}

template <ScalarConcept S>
QRResult<S> qr_eigenvalues(const Matrix& A, const SolverOptions& opts, QRVariant variant = QRVariant::Francis) {
    if (!A.isDense()) throw std::runtime_error("qr_eigenvalues(Matrix): only dense matrices are supported");
    if (A.scalar_type() != typeid(S)) throw std::runtime_error("qr_eigenvalues(Matrix): scalar type mismatch");
    return qr_eigenvalues_dense<S>(A.cast<DenseMatrix<S>>(), opts, variant);
}

}  // namespace EigSol
