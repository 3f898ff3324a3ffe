/*
 * eigsol_hip.h — C ABI of the MI355X (gfx950) eigenvalue-solver hot path.
 *
 * This is the drop-in boundary for hugoheziyang/PCSC_Eigenvalue_Solver_Project.  The reference has
 * no FFI: its boundary is the header-only C++ template API, and the seam is the dense/sparse
 * dispatch inside each entry point.  Every function below replaces the numeric core behind one of
 * those seams (file:line in the reference):
 *
 *   powerMethod<S>                 src/power_method/power_method.hpp:135-148 (impl :47-99)
 *   shiftedInversePowerMethod<S>   src/power_method/shifted_inverse_power_solver.hpp:112-125 (impl :21-79)
 *   solve_shifted<S>               src/matrix/solve_shifted.hpp:48-118
 *   to_hessenberg<S>               src/qr_method/to_hessenberg.hpp:99-119 (impl :23-80)
 *   qr_eigenvalues<S>              src/qr_method/qr_eigenvalues.hpp:126-147 (impl :40-108)
 *   Matrix (dense / sparse store)  src/matrix/matrix.hpp:36-246
 *
 * The C++ drop-in façade (include/eigsol/...) keeps the reference's names, signatures and
 * exception messages and calls only this ABI.  Plain pointers and sizes; no torch / HIP types in
 * the signatures (streams are passed as void*).  Every call returns an eigsol_status; the
 * detail string of the last failure on the calling thread is eigsol_last_error().
 *
 * Scalars: EIGSOL_F64 = double, EIGSOL_C128 = std::complex<double> / double _Complex
 * (interleaved re, im), EIGSOL_F32 = float, EIGSOL_C64 = std::complex<float> (single-precision
 * paths listed at eigsol_dtype), EIGSOL_DD / EIGSOL_CDD = long double / std::complex<long double>
 * carried as double-double (see eigsol_dtype).  Dense storage is column-major (Matrix::Dense is an Eigen col-major
 * matrix, matrix.hpp:39-40).  Sparse storage is CSR with int32 indices on the device; the CSC
 * constructor accepts the reference's canonical Eigen::SparseMatrix<S> (ColMajor, int) layout
 * (matrix.hpp:43-44).
 */
#ifndef EIGSOL_HIP_H
#define EIGSOL_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define EIGSOL_ABI_VERSION 1

typedef enum eigsol_status {
    EIGSOL_OK = 0,
    EIGSOL_E_NOT_SQUARE = 1,      /* "...: matrix must be square"   power_method.hpp:54 */
    EIGSOL_E_ZERO_SIZE = 2,       /* "...: matrix has zero size"    power_method.hpp:57 */
    EIGSOL_E_SCALAR_MISMATCH = 3, /* "...: scalar type mismatch"    power_method.hpp:138 */
    EIGSOL_E_SIZE_MISMATCH = 4,   /* size mismatch between A and b  solve_shifted.hpp:71 */
    EIGSOL_E_NOT_DENSE = 5,       /* "only dense matrices"          qr_eigenvalues.hpp:132 */
    EIGSOL_E_SOLVER = 6,          /* factorisation failed           solve_shifted.hpp:109 */
    EIGSOL_E_HIP = 7,             /* HIP runtime error */
    EIGSOL_E_RCCL = 8,            /* RCCL error */
    EIGSOL_E_INVALID = 9,         /* invalid argument (null pointer, malformed CSR, ...) */
    EIGSOL_E_NO_DEVICE = 10,      /* no usable gfx950 device */
    EIGSOL_E_EMPTY = 11,          /* "empty matrix"                 qr_decompose.hpp:39 */
    EIGSOL_E_UNSUPPORTED = 12     /* structure not supported by the device path */
} eigsol_status;

/* EIGSOL_F32 / EIGSOL_C64: float and std::complex<float> (ScalarConcept, types.hpp:28-30), stored
 * and multiplied in single precision on the device (CSR / dense power iteration, plain SpMV/GEMV,
 * triangular-CSR shifted inverse).  Other solvers accept only F64 / C128 (the C++ façade promotes
 * float input for those).
 * EIGSOL_DD / EIGSOL_CDD: long double and std::complex<long double> (types.hpp:28-30; the x87
 * 80-bit format, 64-bit significand, under g++ on x86-64).  A value is a double-double: two doubles
 * {hi, lo} whose unevaluated sum is the value, |lo| <= ulp(hi)/2 (106-bit significand); complex
 * values are {re.hi, re.lo, im.hi, im.lo}.  Every finite long double inside the double exponent
 * range converts exactly (hi = (double)v, lo = (double)(v - hi)).  Computed in double-double on the
 * device: CSR / dense products, the power method, the shifted inverse and solve_shifted (the fp64
 * factor of A - sigma I refined to double-double accuracy by residuals computed in double-double),
 * to_hessenberg, qr_decompose and the reference's unshifted qr_eigenvalues; the Francis variant
 * runs the fp64 sweeps and refines every eigenvalue in double-double (eigsol_qr_eigenvalues_dense);
 * the row-sharded path returns EIGSOL_E_UNSUPPORTED. */
typedef enum eigsol_dtype {
    EIGSOL_F64 = 0,
    EIGSOL_C128 = 1,
    EIGSOL_F32 = 2,
    EIGSOL_C64 = 3,
    EIGSOL_DD = 4,
    EIGSOL_CDD = 5
} eigsol_dtype;

/* SolverOptions (src/option/solver_option.hpp:14-20). */
typedef struct eigsol_solver_options {
    int32_t max_iterations; /* default 1000 */
    double tolerance;       /* default 1e-10; |a-b| <= tol*(1+|a|), tolerance.hpp:28-33 */
} eigsol_solver_options;

typedef struct eigsol_ctx eigsol_ctx;     /* one device + one stream (+ optional RCCL communicator) */
typedef struct eigsol_csr eigsol_csr;     /* device-resident CSR matrix (rows of one rank)          */
typedef struct eigsol_dense eigsol_dense; /* device-resident column-major dense matrix             */
typedef struct eigsol_power eigsol_power; /* device-resident power-iteration session               */

/* ---------------------------------------------------------------- library / context */
int eigsol_abi_version(void);
const char* eigsol_status_string(int status);
const char* eigsol_last_error(void);
int eigsol_device_count(int* count);
int eigsol_ctx_create(int device, eigsol_ctx** out);
int eigsol_ctx_destroy(eigsol_ctx* ctx);
/* Use the caller's hipStream_t (NULL = the context's own stream).  All work is stream-ordered. */
int eigsol_ctx_set_stream(eigsol_ctx* ctx, void* hip_stream);
int eigsol_ctx_get_stream(eigsol_ctx* ctx, void** hip_stream);
int eigsol_ctx_synchronize(eigsol_ctx* ctx);

/* ---------------------------------------------------------------- device memory helpers */
int eigsol_malloc(eigsol_ctx* ctx, size_t bytes, void** dptr);
int eigsol_free(eigsol_ctx* ctx, void* dptr);
int eigsol_memcpy_h2d(eigsol_ctx* ctx, void* dst, const void* src, size_t bytes);
int eigsol_memcpy_d2h(eigsol_ctx* ctx, void* dst, const void* src, size_t bytes);

/* ---------------------------------------------------------------- matrices (host in, HBM resident) */
/* CSR: rowptr[nrows+1], colidx[nnz] (0-based, < ncols), values[nnz].  Columns inside a row are
 * sorted ascending on upload (the reference's CSC product sums each row in ascending column
 * order, power_method.hpp:69).  Requires nnz < 2^31 (Eigen StorageIndex = int). */
int eigsol_csr_create(eigsol_ctx* ctx, eigsol_dtype dtype, int64_t nrows, int64_t ncols,
                      int64_t nnz, const int32_t* rowptr, const int32_t* colidx,
                      const void* values, eigsol_csr** out);
/* CSC (Eigen::SparseMatrix<S> compressed storage: outer = column pointers). */
int eigsol_csr_create_from_csc(eigsol_ctx* ctx, eigsol_dtype dtype, int64_t nrows, int64_t ncols,
                               int64_t nnz, const int32_t* colptr, const int32_t* rowidx,
                               const void* values, eigsol_csr** out);
/* COO triplets (row[k], col[k], values[k]) in any order, the text reader's sparse entries
 * (file_matrix_reader.hpp:84-132, "row col value" lines): ordered by (row, column) into CSR
 * directly, with no CSC step; repeated positions are summed in input order (what Matrix::Sparse's
 * compression does with repeated insert()s). */
int eigsol_csr_create_from_coo(eigsol_ctx* ctx, eigsol_dtype dtype, int64_t nrows, int64_t ncols,
                               int64_t nnz, const int32_t* rowidx, const int32_t* colidx,
                               const void* values, eigsol_csr** out);
/* Copy the device CSR back (rowptr[nrows+1], colidx[nnz], values[nnz]; columns ascending within
 * each row, duplicates already summed).  Single-device matrices only. */
int eigsol_csr_download(eigsol_csr* A, int32_t* rowptr, int32_t* colidx, void* values);
int eigsol_csr_destroy(eigsol_csr* A);
int eigsol_csr_info(eigsol_csr* A, int64_t* nrows, int64_t* ncols, int64_t* nnz, int* dtype);
/* y = A*x on device buffers (x: ncols scalars, y: nrows scalars), stream-ordered.  Each row is an
 * ascending-column sequential sum of products: bitwise equal to the reference's CSC scatter. */
int eigsol_csr_spmv(eigsol_csr* A, const void* x_dev, void* y_dev);

/* Dense, column-major nrows x ncols (Matrix::Dense<S>). */
int eigsol_dense_create(eigsol_ctx* ctx, eigsol_dtype dtype, int64_t nrows, int64_t ncols,
                        const void* colmajor, eigsol_dense** out);
int eigsol_dense_destroy(eigsol_dense* A);
int eigsol_dense_gemv(eigsol_dense* A, const void* x_dev, void* y_dev);

/* ---------------------------------------------------------------- power method
 * powerMethod<S>(M, opts) (power_method.hpp:135-148) with an explicit start vector x0 in place
 * of Vector<S>::Random (power_method.hpp:62; x0 is normalised by the library exactly as
 * x.normalize()).  The device runs ONE fused product per iteration: the reference's second
 * product x.dot(A*x) (:81) is the next iteration's y (:69), so the eigenvalue sequence is the
 * reference's.  Outputs mirror EigenResult<S> (eigen_result.hpp:22-52).
 * One-shot form: host buffers; lambda_out = 1 scalar, x_out = n scalars (either may be NULL). */
int eigsol_power_csr(eigsol_csr* A, const eigsol_solver_options* opts, const void* x0,
                     void* lambda_out, void* x_out, int32_t* iterations, int32_t* converged);
int eigsol_power_dense(eigsol_dense* A, const eigsol_solver_options* opts, const void* x0,
                       void* lambda_out, void* x_out, int32_t* iterations, int32_t* converged);

/* Session form (device-resident; what a caller with data already in HBM uses, and what the
 * benchmark times).  begin() normalises x0 and resets the state; step(k) enqueues k fused
 * iterations (launches after convergence exit immediately); query() synchronises and reports
 * whether the reference loop has terminated; finish() writes EigenResult fields.
 * trace_capacity > 0 records the Rayleigh quotient of every completed iteration on the device. */
int eigsol_power_create_csr(eigsol_csr* A, int32_t trace_capacity, eigsol_power** out);
int eigsol_power_create_dense(eigsol_dense* A, int32_t trace_capacity, eigsol_power** out);
int eigsol_power_destroy(eigsol_power* s);
int eigsol_power_begin(eigsol_power* s, const eigsol_solver_options* opts, const void* x0,
                       int x0_on_device);
int eigsol_power_step(eigsol_power* s, int32_t nsteps);
int eigsol_power_query(eigsol_power* s, int32_t* done, int32_t* launches);
int eigsol_power_finish(eigsol_power* s, void* lambda_out, void* x_out, int x_out_on_device,
                        int32_t* iterations, int32_t* converged);
int eigsol_power_trace(eigsol_power* s, void* trace_host, int32_t capacity, int32_t* count);
/* Device-side description of the hot kernel for roofline accounting: algorithmic bytes moved by
 * one fused iteration and the grid used. */
int eigsol_power_kernel_info(eigsol_power* s, double* bytes_per_iteration, int32_t* grid_blocks,
                             int32_t* tiles, int32_t* variant);
/* Demangled name of the kernel a CSR power session launches per iteration (e.g.
 * "void eigsol::dev::csr_slice_kernel<double, true, 12, false, false>(...)"), the string rocprofv3
 * reports; empty for other sessions. */
int eigsol_power_kernel_name(eigsol_power* s, char* buf, size_t capacity);
/* Reference iterations one pass over the matrix runs: 2 for a CSR session on the pair path
 * (csr_pair_kernel; EIGSOL_POWER_PAIR=0 forces single launches), else 1.  eigsol_power_step keeps
 * counting reference iterations either way. */
int eigsol_power_iterations_per_pass(eigsol_power* s, int32_t* n);
/* variant: 0 = CSR, x gathered from HBM; 1 = CSR, x window staged in LDS; 2 = dense GEMV;
 *          3 = shifted inverse, sync-free triangular solve (tiles = dependency levels);
 *          4 = shifted inverse, dense LU substitution;
 *          5 = CSR in 64-row slices, one row per lane (tiles = slices);
 *          6 = CSR one row per lane (single-precision fallback layout);
 *          7 = shifted inverse, ILU(0)-preconditioned GMRES (general sparse; bytes and tiles of the
 *              last solve: algorithmic bytes of all its steps, Arnoldi steps);
 *          8 = shifted inverse, RCM-banded direct LU (general sparse; tiles = kl + ku);
 *          15 = double-double CSR product (EIGSOL_DD / EIGSOL_CDD power method, one row per lane);
 *          16 = double-double dense GEMV (row tiles x column chunks);
 *          17 = double-double shifted inverse: fp64 factor + residual refinement in double-double
 *               (tiles = refinement steps of the last solve, bytes = all of its passes);
 *          18 = shifted inverse, general sparse: GMRES preconditioned by the exact sparse LU of
 *               A - sigma I (symbolic fill without pivoting, used when the filled pattern holds at most
 *               EIGSOL_LU_FILL_CAP x nnz entries; tiles and bytes as for 7);
 *          20 = shifted inverse, dense LU substitution by triangles: chosen at set-up instead of 4's
 *               products with inverted 64 x 64 diagonal blocks when a block of L or U is ill
 *               conditioned (Skeel condition number above 1e6), or by EIGSOL_DENSE_TRSV=1 */

/* ---------------------------------------------------------------- block subspace iteration
 * The k = nev eigenpairs of largest modulus of a sparse or a dense matrix by orthogonal iteration
 * with Rayleigh-Ritz on a block of m = block >= k vectors (csrc/subspace.hip; the reference has no
 * counterpart).  The two entries differ in the product Z = A Q alone: eigsol_csr_spmm for a CSR
 * matrix, eigsol_dense_gemm for a dense one.  Block vectors on the device are row-major interleaved: n x m with the vector
 * index fastest, X[i * m + j].
 *   Q = cholqr2(X0); repeat: Z = A Q; B = Q^H Z; (theta, Y) = eig(B), sorted by |theta| descending
 *   (moduli equal to 1e-12 relative: the larger imaginary part first); stop when every wanted theta
 *   is within tolerance (1 + |theta|) of its nearest not-yet-matched wanted value of the previous
 *   iteration (|a-b| <= tol (1+|a|), a the new value) and, with residual_tolerance > 0, every wanted
 *   ||Z y - theta Q y|| / ||Q y|| <= residual_tolerance (1 + |theta|); else Q = cholqr2(Z).
 * iterations counts the products Z = A Q; max_iterations = 1 returns iterations = 1, converged = 0.
 * One host wait per iteration (B and the factorisations' error words; one more on an iteration
 * whose eigenvalue test passed and whose residuals are then formed); the Cholesky factorisations
 * and R^-1 stay on the device.  A factorisation that meets a pivot that is not positive or below
 * m 2^-52 max diag fails with EIGSOL_E_SOLVER ("subspace_iteration: block lost rank at column j"):
 * a rank-deficient X0, or A Q of rank below m (A of rank below m).  A cut between k and k + 1
 * through eigenvalues of equal modulus (a conjugate pair split by k = m, say) may never settle
 * and end with converged = 0.
 * Status: EIGSOL_E_INVALID (null pointers; nev < 1; block < nev; block > 32; block > n;
 * max_iterations < 1; m outside 1..32 for spmm / gemm), EIGSOL_E_NOT_SQUARE, EIGSOL_E_ZERO_SIZE,
 * EIGSOL_E_UNSUPPORTED (F32 / C64 / DD / CDD matrices and row-sharded matrices, spmm / gemm too);
 * all of these are decided before any device call.
 * Out of scope: single precision, double-double, row-sharded matrices and a
 * session / step form. */
typedef struct eigsol_subspace_options {
    int32_t max_iterations;      /* 1000 */
    double  tolerance;           /* 1e-10; < 0: never converges */
    double  residual_tolerance;  /* 0: off */
    int32_t nev;                 /* k >= 1 */
    int32_t block;               /* m: nev <= m <= 32, m <= n */
} eigsol_subspace_options;

/* Y = A X on device buffers, row-major interleaved blocks (X: ncols x m, Y: nrows x m),
 * stream-ordered.  Column j of Y is bitwise eigsol_csr_spmv of column j of X. */
int eigsol_csr_spmm(eigsol_csr* A, int32_t m, const void* X_dev, void* Y_dev);

/* X0: host, column-major n x m, matrix dtype.  eigenvalues: 2k doubles (re, im).  eigenvectors
 * (optional): n x k complex, column-major (2nk doubles), unit 2-norm.  residuals (optional): k
 * doubles, ||A x_j - theta_j x_j||_2 of the returned pairs (from Z = A Q of the last product). */
int eigsol_subspace_csr(eigsol_csr* A, const eigsol_subspace_options* opts, const void* X0,
                        double* eigenvalues, double* eigenvectors, double* residuals,
                        int32_t* iterations, int32_t* converged);

/* Y = A X for a dense matrix on device buffers, row-major interleaved blocks as for eigsol_csr_spmm
 * (X: ncols x m, X[i * m + j]; Y: nrows x m), 1 <= m <= 32, EIGSOL_F64 / EIGSOL_C128, any nrows,
 * ncols >= 0 (rectangular too), stream-ordered (csrc/dense_block.hip).  The products run on the
 * fp64 matrix cores (v_mfma_f64_16x16x4_f64; four real instructions per complex product) with m
 * padded to 16 or 32 block columns; the padding and the remainders of A are masked on load.  A is
 * read once per product.  Column chunks write partials to a workspace kept on the matrix (nchunk x
 * nrows x m scalars, allocated on first use); a second kernel adds them in ascending chunk order:
 * no floating-point atomics, two runs give identical bits.  The sums' order differs from
 * eigsol_dense_gemv's, so m = 1 agrees with it to rounding, not bitwise.
 * Status, decided before any device call: EIGSOL_E_INVALID (null pointer with a non-empty operand;
 * m outside 1..32), EIGSOL_E_UNSUPPORTED (F32 / C64 / DD / CDD).  nrows == 0 returns EIGSOL_OK;
 * ncols == 0 with nrows > 0 writes zeros to Y. */
int eigsol_dense_gemm(eigsol_dense* A, int32_t m, const void* X_dev, void* Y_dev);

/* eigsol_subspace_csr on a dense matrix: the same algorithm, arguments, output order, stopping test,
 * rank-loss rule, counters and status codes (no row-sharded case); Z = A Q through
 * eigsol_dense_gemm. */
int eigsol_subspace_dense(eigsol_dense* A, const eigsol_subspace_options* opts, const void* X0,
                          double* eigenvalues, double* eigenvectors, double* residuals,
                          int32_t* iterations, int32_t* converged);

/* ---------------------------------------------------------------- Krylov-Schur (thick-restart Arnoldi)
 * k = nev eigenpairs of a sparse or a dense matrix from a Krylov basis of m = ncv vectors (csrc/krylov.hip; the
 * reference has no counterpart), in two modes:
 *   EIGSOL_KRYLOV_LM            Op = A: the eigenvalues of largest modulus (the product runs on the
 *                               single-vector layout the eigsol_csr selected at upload, or
 *                               through eigsol_dense_gemv);
 *   EIGSOL_KRYLOV_SHIFT_INVERT  Op = (A - sigma I)^-1: the eigenvalues nearest sigma.  A - sigma I is
 *                               factored once (the factors of the shifted inverse iteration below) and
 *                               solved once per step; a factor failure (a singular A - sigma I, say)
 *                               returns with that path's own status and message.  For a dense
 *                               matrix the factor is the partial-pivot LU of the dense shifted
 *                               solves, which reports no zero pivot: a singular A - sigma I is not
 *                               detected there, and the loop is bounded by max_restarts.
 * V is n x (m + 1) on the device, column-major, in the matrix dtype; S is the (m + 1) x m Rayleigh
 * matrix, B = S[:m, :m], b^T = S[m, :m].
 *   v_0 = v0 / ||v0||, p = 0; cycle 1 .. max_restarts:
 *     steps j = p .. m-1, enqueued without a host wait: w = Op v_j; twice { c = V_j^H w; w -= V_j c;
 *       h += c } (V_j = V[:, :j+1], classical Gram-Schmidt with one reorthogonalisation); beta = ||w||;
 *       S[:j+1, j] = h, S[j+1, j] = beta, v_{j+1} = w / beta;
 *     one host wait (S, the breakdown word, the factor's error word);
 *     (theta, Y) = eig(B), ordered by |theta| descending (moduli equal to 1e-12 relative: the larger
 *       imaginary part first), est_i = |b^T y_i|; converged when est_i <= tolerance max(eps^(2/3),
 *       |theta_i|) for every i < k (ARPACK's test);
 *     else restart: p = k, or k + 1 for a real matrix when theta_{k-1} and theta_k are a conjugate
 *       pair; Q = an orthonormal basis (matrix dtype, m x p; for a real matrix of [Re Y_p, Im Y_p]) of
 *       the invariant subspace of B of theta_0 .. theta_{p-1}; V[:, :p] = V[:, :m] Q, v_p = v_m,
 *       S = 0, S[:p, :p] = Q^H B Q, S[p, :p] = b^T Q.
 *   lambda_i = theta_i (LM) or sigma + 1 / theta_i (shift-invert); x_i = V[:, :m] y_i scaled to unit
 *   2-norm; residual_i = ||A x_i - lambda_i x_i||_2 formed with A on the device.
 * Output order: that of theta, so largest |lambda| first (LM) or nearest sigma first (shift-invert).
 * Of a conjugate pair of a real matrix the member with the positive imaginary part comes first in
 * LM, the one with the negative imaginary part in shift-invert (Im 1/theta = -Im theta / |theta|^2).
 * Breakdown: a step with beta <= m 2^-52 ||Op v_j|| (the norm before orthogonalisation) found an
 * invariant subspace of dimension d = j + 1: it stores v_{j+1} = 0 and 1 + j in a device word.  At
 * the cycle's wait the host truncates to that subspace: d >= nev returns its Ritz pairs with
 * converged = 1 and applications counted up to the breakdown; d < nev fails with EIGSOL_E_SOLVER
 * ("krylov_schur: invariant subspace of dimension d < nev").  No restart with a fresh vector.
 * restarts counts the cycles run (max_restarts = 1: restarts = 1, applications = ncv); applications
 * counts w = Op v.
 * Status, all decided before any device call: EIGSOL_E_INVALID (null pointers; nev < 1;
 * ncv < nev + 2; ncv > 64; ncv > n; max_restarts < 1; unknown mode), EIGSOL_E_NOT_SQUARE,
 * EIGSOL_E_ZERO_SIZE, EIGSOL_E_UNSUPPORTED (F32 / C64 / DD / CDD matrices, row-sharded matrices).
 * Out of scope: single precision, double-double, row-sharded matrices, a session /
 * step form, generalised problems and selections other than these two. */
#define EIGSOL_KRYLOV_LM 0
#define EIGSOL_KRYLOV_SHIFT_INVERT 1
typedef struct eigsol_krylov_options {
    int32_t max_restarts; /* 300 */
    double  tolerance;    /* 1e-10; < 0: never converges */
    int32_t nev;          /* k >= 1 */
    int32_t ncv;          /* m: nev + 2 <= m <= 64, m <= n */
    int32_t mode;         /* EIGSOL_KRYLOV_LM / EIGSOL_KRYLOV_SHIFT_INVERT */
} eigsol_krylov_options;

/* sigma: one scalar of the matrix dtype, read only in shift-invert (may be NULL otherwise).  v0:
 * host, n scalars of the matrix dtype.  eigenvalues: 2k doubles (re, im).  eigenvectors (optional):
 * n x k complex, column-major (2nk doubles), unit 2-norm.  residuals (optional): k doubles.
 * restarts / applications / converged: optional. */
int eigsol_krylov_csr(eigsol_csr* A, const eigsol_krylov_options* opts, const void* sigma, const void* v0,
                      double* eigenvalues, double* eigenvectors, double* residuals, int32_t* restarts,
                      int32_t* applications, int32_t* converged);
/* eigsol_krylov_csr on a dense matrix: the same algorithm, arguments, output order, breakdown rule,
 * counters and status codes (no row-sharded case).  With shift-invert this returns the
 * eigenvectors that belong to an eigenvalue eigsol_qr_eigenvalues_dense found (sigma next to it). */
int eigsol_krylov_dense(eigsol_dense* A, const eigsol_krylov_options* opts, const void* sigma, const void* v0,
                        double* eigenvalues, double* eigenvectors, double* residuals, int32_t* restarts,
                        int32_t* applications, int32_t* converged);

/* The solver's two kernel groups on device buffers (dtype EIGSOL_F64 / EIGSOL_C128), enqueued on the
 * context's stream.
 * eigsol_krylov_orth: one orthogonalisation step of w (n scalars) against the j orthonormal columns
 * of V (n x j, column-major, leading dimension ldv >= n), 1 <= j <= 64: twice { c = V^H w;
 * w -= V c; h += c }, then w /= beta.  h_out (host, 2j doubles: re, im), beta_out (host: ||w|| after
 * the two passes) and wnorm_out (host: ||w|| before them) are optional; the call waits for the
 * stream when one of them is given.  A step with beta <= 64 2^-52 wnorm leaves w = 0 (breakdown).
 * eigsol_krylov_rotate: V[:, :p] <- V[:, :m] Q in place (V: n x m, column-major, ldv >= n; Q: host,
 * m x p column-major, of the dtype; 1 <= p <= m <= 64); columns p .. m-1 are left as they are.  Q
 * is copied before the call returns. */
int eigsol_krylov_orth(eigsol_ctx* ctx, int dtype, int64_t n, int32_t j, const void* V_dev, int64_t ldv,
                       void* w_dev, double* h_out, double* beta_out, double* wnorm_out);
int eigsol_krylov_rotate(eigsol_ctx* ctx, int dtype, int64_t n, int32_t m, int32_t p, void* V_dev,
                         int64_t ldv, const void* Q);

/* ---------------------------------------------------------------- svds (thick-restart Golub-Kahan-Lanczos)
 * The k = nsv largest singular triplets of a sparse or a dense M x N matrix from bases of m = ncv
 * vectors (csrc/svds.hip; the reference has no counterpart), without forming A^H A.
 *
 * Adjoint products.  eigsol_dense_gemv_h: y = A^H x on device buffers for a column-major dense matrix
 * of any shape (x: nrows scalars, y: ncols scalars), EIGSOL_F64 / EIGSOL_C128, stream-ordered
 * (csrc/dense_adjoint.hip).  A is read once; row chunks write partials to a workspace kept on the
 * matrix and a second kernel adds them in ascending chunk order: no floating-point atomics, the order
 * of every sum depends on the shape alone, two calls give identical bits.  For a complex matrix the
 * conjugate is taken on A.  Status: EIGSOL_E_INVALID (null pointer with a non-empty operand),
 * EIGSOL_E_UNSUPPORTED (F32 / C64 / DD / CDD); ncols == 0 returns EIGSOL_OK, nrows == 0 writes zeros.
 * eigsol_csr_adjoint: a new eigsol_csr holding A^H (ncols x nrows, values conjugated), built on the
 * host from A's downloaded arrays (A's CSR arrays are the CSC arrays of its transpose) through
 * eigsol_csr_create_from_csc, so it gets the layout selection of any uploaded matrix and its product
 * is eigsol_csr_spmv with its fixed ascending-column sum order.  The caller destroys it with
 * eigsol_csr_destroy.  Status: EIGSOL_E_INVALID (null pointer), EIGSOL_E_UNSUPPORTED (row-sharded
 * matrices; F32 / C64 / DD / CDD).
 *
 * The driver.  V is N x (m + 1) and U is M x m on the device, column-major, in the matrix dtype; B is
 * m x m upper triangular on the host.
 *   v_0 = v0 / ||v0||, p = 0; cycle 1 .. max_restarts:
 *     steps j = p .. m-1, enqueued without a host wait:
 *       u = A v_j; twice { c = U_j^H u; u -= U_j c; h += c } (U_j = U[:, :j]; classical Gram-Schmidt
 *         with one reorthogonalisation); alpha = ||u||; B[:j, j] = h, B[j, j] = alpha, u_j = u / alpha;
 *       w = A^H u_j; the same against V[:, :j+1], coefficients discarded; beta = ||w||; v_{j+1} = w / beta;
 *     one host wait (the columns h, alpha, beta, the breakdown word);
 *     B = X diag(s) Y^H (one-sided Jacobi on the host, s descending); est_i = beta_{m-1} |X[m-1, i]|;
 *     converged when est_i <= tolerance max(s_i, eps^(2/3) s_0) for every i < k;
 *     else restart: p = k; V[:, :p] = V[:, :m] Y[:, :p]; U[:, :p] = U[:, :m] X[:, :p]; v_p = v_m; B = 0,
 *       B[i, i] = s_i for i < p (the spike in column p of B is the h that step p computes).
 *   u_i = U[:, :m] x_i, v_i = V[:, :m] y_i; column i of V gets its largest-modulus component (the first
 *   on ties) real and positive, eigsol_svd_dense's convention, and u_i the same unit factor;
 *   residual_i = hypot(||A v_i - s_i u_i||_2, ||A^H u_i - s_i v_i||_2), formed with A and A^H on the device.
 * Breakdown: a norm at or below m 2^-52 times the norm before orthogonalisation stores a zero vector
 * and sets a device word, read at the cycle's wait.  beta_j: U[:, :j+1] and V[:, :j+1] span an
 * invariant pair of subspaces of dimension d = j + 1, with B[:d, :d].  alpha_j (a rank-deficient A
 * whose v0 has a null-space component): d = j on the left, j + 1 on the right, and the projected matrix
 * is the d x (d + 1) block [B[:d, :d] | h_j].  d >= nsv returns the triplets of that block with
 * converged = 1; d < nsv fails with EIGSOL_E_SOLVER ("svds: invariant subspace of dimension d <
 * nsv").  No restart with a fresh vector.  A small SVD that does not converge is EIGSOL_E_SOLVER.
 * restarts counts the cycles run; applications counts the products with A or A^H up to the breakdown
 * or the last step (max_restarts = 1: restarts = 1, applications = 2 ncv).
 * Status, all decided before any device call: EIGSOL_E_INVALID (null pointers; nsv < 1;
 * ncv < nsv + 2; ncv > 64; ncv > min(M, N); max_restarts < 1; an AH whose shape, dtype or context does
 * not match; a v0 with no finite nonzero norm), EIGSOL_E_ZERO_SIZE, EIGSOL_E_UNSUPPORTED (F32 / C64 /
 * DD / CDD matrices, row-sharded matrices).
 * Out of scope: the smallest or interior singular values, block Lanczos, single precision,
 * double-double, row-sharded matrices, a session / step form and matrix-free operators. */
typedef struct eigsol_svds_options {
    int32_t max_restarts; /* 300 */
    double  tolerance;    /* 1e-10; < 0: never converges */
    int32_t nsv;          /* k >= 1 */
    int32_t ncv;          /* m: nsv + 2 <= m <= 64, m <= min(M, N) */
} eigsol_svds_options;

int eigsol_csr_adjoint(eigsol_csr* A, eigsol_csr** out);
int eigsol_dense_gemv_h(eigsol_dense* A, const void* x_dev, void* y_dev);
/* AH: eigsol_csr_adjoint(A), or NULL (built and destroyed inside).  v0: host, ncols scalars of the
 * matrix dtype.  s: k doubles, descending.  U (optional): M x k, V (optional): N x k, column-major in
 * the matrix dtype (real for a real matrix).  residuals (optional): k doubles.  restarts /
 * applications / converged: optional. */
int eigsol_svds_csr(eigsol_csr* A, eigsol_csr* AH, const eigsol_svds_options* opts, const void* v0, double* s,
                    void* U, void* V, double* residuals, int32_t* restarts, int32_t* applications,
                    int32_t* converged);
/* eigsol_svds_csr on a dense matrix: the same algorithm, arguments, breakdown rules, counters and
 * status codes; the products are eigsol_dense_gemv and eigsol_dense_gemv_h. */
int eigsol_svds_dense(eigsol_dense* A, const eigsol_svds_options* opts, const void* v0, double* s, void* U,
                      void* V, double* residuals, int32_t* restarts, int32_t* applications, int32_t* converged);
/* The last eigsol_svds_* call's device time by stage, in ms from stream events: products with A,
 * products with A^H, orthogonalisation, restart + finish. */
int eigsol_svds_stage_times(eigsol_ctx* ctx, double* ms4);

/* ---------------------------------------------------------------- shifted inverse iteration
 * shiftedInversePowerMethod<S>(M, ShiftedSolverOptions<S>{sigma, maxIter, tol})
 * (shifted_inverse_power_solver.hpp:112-125, impl :21-79).  A - sigma I is factored ONCE at
 * session creation (the reference refactors every iteration, solve_shifted.hpp:75-79,96-106):
 *   - triangular CSR (upper or lower; a missing diagonal counts as 0, solve_shifted.hpp:100-102):
 *     the matrix is its own factor; one sync-free level-ordered triangular solve per iteration;
 *   - non-triangular CSR: reverse Cuthill-McKee + banded partial-pivot LU on the device (a direct
 *     factor, like SparseLU) when the band fits; otherwise the densified partial-pivot LU up to
 *     n = 16384, and ILU(0) + restarted GMRES (1e-12 relative residual) above it.  A GMRES solve
 *     that stalls above 1e-10 falls back to the densified LU where it fits the device, else fails
 *     with EIGSOL_E_SOLVER ("solve_shifted: SparseLU solve failed (...)", solve_shifted.hpp:112-114).
 *     EIGSOL_SPARSE_SOLVER=band|lu|gmres forces a path, EIGSOL_GMRES_FALLBACK=0 disables the fallback;
 *   - dense: partial-pivot LU on the device.
 * sigma points at ONE scalar of the matrix dtype.  A zero pivot of a sparse matrix fails with
 * EIGSOL_E_SOLVER ("solve_shifted: SparseLU factorization failed", solve_shifted.hpp:108-110).
 * The returned handle is a session: use eigsol_power_begin/step/query/finish/trace/kernel_info.
 * lambda_k = x_{k+1}^H A x_{k+1} is evaluated as sigma + conj(x_k^H y_k)/||y_k||^2 (A y_k = x_k +
 * sigma y_k), so an iteration reads only the factor. */
int eigsol_shifted_create_csr(eigsol_csr* A, const void* sigma, int32_t trace_capacity,
                              eigsol_power** out);
int eigsol_shifted_create_dense(eigsol_dense* A, const void* sigma, int32_t trace_capacity,
                                eigsol_power** out);
int eigsol_shifted_inverse_csr(eigsol_csr* A, const void* sigma, const eigsol_solver_options* opts,
                               const void* x0, void* lambda_out, void* x_out, int32_t* iterations,
                               int32_t* converged);
int eigsol_shifted_inverse_dense(eigsol_dense* A, const void* sigma,
                                 const eigsol_solver_options* opts, const void* x0,
                                 void* lambda_out, void* x_out, int32_t* iterations,
                                 int32_t* converged);
/* solve_shifted<S>(M, sigma, b) (solve_shifted.hpp:48-118): x = (A - sigma I)^{-1} b, host
 * buffers of nb scalars.  Status mirrors the reference's exceptions: NOT_SQUARE, SIZE_MISMATCH,
 * SOLVER. */
int eigsol_solve_shifted_csr(eigsol_csr* A, const void* sigma, const void* b, int64_t nb, void* x);
int eigsol_solve_shifted_dense(eigsol_dense* A, const void* sigma, const void* b, int64_t nb,
                               void* x);

/* ---------------------------------------------------------------- QR method (dense)
 * Host column-major buffers in and out; the work runs on the context's device.
 * to_hessenberg_dense<S>   (to_hessenberg.hpp:23-80): H = Householder reduction of A (n x n).
 * qr_decompose_dense<S>    (qr_decompose.hpp:25-86):  A (m x n) = Q (m x m) R (m x n); m or n
 *                          == 0 fails with EIGSOL_E_EMPTY ("qr_decompose_dense: empty matrix").
 * qr_eigenvalues_dense<S>  (qr_eigenvalues.hpp:40-108):
 *   variant EIGSOL_QR_UNSHIFTED — the reference algorithm exactly: Hessenberg, then H <- R Q until
 *     max|h(i,i-1)| <= tol (1 + ||H||_F); eigenvalues = diag(H) (eig_re_or_c: n scalars of the
 *     dtype; eig_im unused); iterations = iter + 1 (maxIter + 1 when not converged);
 *   variant EIGSOL_QR_FRANCIS (north_star; real matrices) — Hessenberg, then Francis multishift
 *     double-shift sweeps to quasi-triangular form with deflation at unit roundoff.  eig_re_or_c
 *     receives the real parts (= diag of the standardised real Schur form), eig_im (optional) the
 *     imaginary parts; iterations = the most sweeps any single deflation needed (>= 1), and
 *     converged = 0 when that exceeded maxIterations (so iterations <= maxIterations exactly when
 *     converged, as in the reference).  Complex matrices (EIGSOL_C128) run complex multishift
 *     sweeps and return the eigenvalues themselves in eig_re_or_c.
 *     EIGSOL_DD / EIGSOL_CDD (long double): the fp64 sweeps on the rounded double-double Hessenberg
 *     matrix, then every eigenvalue refined in double-double by Newton's method on det(H - mu I)
 *     (Hyman's recurrence, n <= 8192); eig_re_or_c receives n dd (real parts) / n cdd values, and
 *     for EIGSOL_DD eig_im (optional) the imaginary parts as n {hi, lo} pairs (2n doubles).
 *     fp64 eigenvalues within 1e-8 (1 + |lambda|) of each other are refined as a group, each
 *     Newton step deflated against the group's values already refined (so a cluster far tighter
 *     than the fp64 error still yields one value per eigenvalue), at most 16 steps each.  A value
 *     is refined when a step reached 2^-104 |mu| or the contraction of the steps shows the next
 *     one there.  It is NOT refined when it ran out of steps (the last iterate is returned), when
 *     the refinement moved it by more than 1e-8 (1 + |lambda|) or no step was usable (the fp64
 *     value is returned), or when it ended on another value's root (the later one gets its fp64
 *     value back): `converged` does not report these, eigsol_qr_refine_info does.
 * n == 0: iterations 0, converged 1 (qr_eigenvalues.hpp:55-57). */
#define EIGSOL_QR_FRANCIS 0
#define EIGSOL_QR_UNSHIFTED 1
int eigsol_hessenberg_dense(eigsol_ctx* ctx, int dtype, int64_t n, const void* A_colmajor,
                            void* H_out);
int eigsol_qr_decompose_dense(eigsol_ctx* ctx, int dtype, int64_t m, int64_t n,
                              const void* A_colmajor, void* Q_out, void* R_out);
int eigsol_qr_eigenvalues_dense(eigsol_ctx* ctx, int dtype, int64_t n, const void* A_colmajor,
                                const eigsol_solver_options* opts, int variant,
                                void* eig_re_or_c, double* eig_im, int32_t* iterations,
                                int32_t* converged);
/* The refinement of the context's last EIGSOL_DD / EIGSOL_CDD Francis call: how many of its
 * eigenvalues are not refined to the double-double floor (rules above; 0 before any such call) and
 * the most Newton steps one took.  Either pointer may be null. */
int eigsol_qr_refine_info(eigsol_ctx* ctx, int64_t* unrefined, int32_t* max_newton_steps);
/* Diagnostic: that refinement alone.  H_colmajor: a host upper-Hessenberg matrix of order n <= 8192
 * in the dtype's wire format (EIGSOL_DD / EIGSOL_CDD; entries below the subdiagonal are not
 * read); starts: `count` values as cdd (4 doubles each: re.hi, re.lo, im.hi, im.lo).  Runs what the
 * Francis variant runs on its fp64 eigenvalues: the same kernel instance for n, grouping,
 * deflation, discard and collision rules.  refined: `count` cdd values; steps: per value the
 * Newton steps taken, or -1 when it is not refined. */
int eigsol_hyman_refine(eigsol_ctx* ctx, int dtype, int64_t n, const void* H_colmajor, int64_t count,
                        const double* starts, double* refined, int32_t* steps);

/* ---------------------------------------------------------------- symmetric / Hermitian (dense)
 * All, or a selected range, of the eigenvalues of a real symmetric (EIGSOL_F64) or complex Hermitian
 * (EIGSOL_C128) matrix, and an orthonormal set of eigenvectors.  The reference has no such solver.
 * Algorithm: the lower triangle is mirrored on the device; the blocked Householder Hessenberg
 * reduction (the general one of eigsol_hessenberg_dense, not a symmetric tridiagonalisation) leaves
 * a tridiagonal H; T = D^H H D is real with non-negative off-diagonals for a unitary diagonal D of
 * accumulated sub-diagonal phases; T splits into blocks where |e_i| <= eps sqrt(|d_i d_{i+1}|) or
 * e_i^2 <= DBL_MIN (LAPACK dstebz's rule); every eigenvalue of every block is found, and the
 * selection taken from the sorted values, by bisection on the Sturm count (one lane each, to 2 eps max(|lo|, |hi|));
 * eigenvectors of T by inverse iteration with Gram-Schmidt inside clusters (LAPACK dstein's scheme:
 * eigenvalues of a block closer than 1e-3 ||T_block||_1 to their neighbour share a cluster, which
 * one workgroup works through in ascending order; at most 5 iterations each, deterministic start
 * vectors); Z = Q (D Z_T) with the reduction's stored
 * panels on the fp64 matrix cores.  No Francis sweeps run.  No floating-point atomics: two calls on
 * the same input return the same bits.
 * Read: A_colmajor (host, n x n, column-major): ONLY the lower triangle, diagonal included (for C128
 * the diagonal's imaginary parts are ignored); the strict upper triangle may hold anything.
 * opts (NULL: all): EIGSOL_EIGH_INDEX takes the il-th .. iu-th smallest (0-based, inclusive),
 * EIGSOL_EIGH_VALUE those with vl < lambda <= vu.  A selection returns bitwise the values the full
 * call returns at those places.
 * Out: *m_out eigenvalues in w, ascending (capacity n); Z (NULL: eigenvalues only), n x *m_out scalars
 * of the dtype, column-major with leading dimension n (capacity n x n): column j belongs to w[j], has
 * unit 2-norm, and its largest-modulus component (the first on ties) is real and positive.
 * not_converged (optional): how many eigenvectors failed dstein's growth test within 5 iterations
 * (their last iterate is returned; 0 on a values-only call).
 * Status, decided before any device call: EIGSOL_E_INVALID (n < 0; with n > 0 a null ctx, A, w or
 * m_out; unknown select; il > iu or an index outside 0 .. n-1; vl >= vu or a NaN bound; unknown
 * dtype), EIGSOL_E_UNSUPPORTED (F32 / C64 / DD / CDD; n above the order the blocked reduction
 * accepts: 16384 real, 8192 complex).  n == 0: EIGSOL_OK with *m_out = 0.  A non-finite entry in the
 * lower triangle fails with EIGSOL_E_SOLVER.
 * Out of scope: single precision and double-double, row-sharded matrices, a symmetric (sytrd) or
 * two-stage reduction, MRRR (divide and conquer: eigsol_eigh_dense_m below), and high relative accuracy
 * of tiny eigenvalues of graded matrices (the Householder reduction loses it; entries are not
 * rescaled, so e_i^2 must neither overflow nor underflow).  The generalised problem A x = lambda B x
 * is eigsol_geigh_dense (below); out of scope there: types 2 and 3 (A B x = lambda x,
 * B A x = lambda x), a semidefinite or indefinite B, single and double-double precision, a two-sided
 * reduction to standard form (LAPACK sygst), and sparse generalised problems in krylov_schur.
 * eigsol_eigh_stage_times: the context's last eigsol_eigh_dense call by stream events, 4 doubles in
 * ms: reduction (mirror, Hessenberg, extraction), bisection, inverse iteration, back-transformation
 * (with the copy of Z to the host); stages that did not run are 0. */
#define EIGSOL_EIGH_ALL 0
#define EIGSOL_EIGH_INDEX 1   /* il <= i <= iu, 0-based, ascending order */
#define EIGSOL_EIGH_VALUE 2   /* vl < lambda <= vu */
typedef struct eigsol_eigh_options {
    int32_t select;
    int64_t il, iu;
    double  vl, vu;
} eigsol_eigh_options;
int eigsol_eigh_dense(eigsol_ctx* ctx, int dtype, int64_t n, const void* A_colmajor,
                      const eigsol_eigh_options* opts, double* w, void* Z, int64_t* m_out,
                      int64_t* not_converged);
int eigsol_eigh_stage_times(eigsol_ctx* ctx, double* ms4);

/* ---------------------------------------------------------------- general dense eigenpairs
 * eigsol_eig_dense: the eigenvalues of a general real (EIGSOL_F64) or complex (EIGSOL_C128) dense matrix
 * and, for all or a selection of them, the right eigenvectors (csrc/eig.hip).  The reference has no such
 * solver.
 * Algorithm: the power-of-two range guard of eigsol_qr_eigenvalues_dense; the blocked Hessenberg
 * reduction with its panels kept (n >= 3; H = A for n <= 2); the Francis sweeps of
 * eigsol_qr_eigenvalues_dense(EIGSOL_QR_FRANCIS) on a copy of H; every eigenvector by inverse iteration on
 * H (LAPACK xHSEIN / xLAEIN's scheme), one workgroup per eigenvalue: H splits where h(i+1, i) == 0 exactly,
 * the vector of an eigenvalue of the block of rows [kl, kr) comes from the partial-pivot LU of
 * H(0:kr, 0:kr) - lambda I (pivots below eps3 = eps ||H_block||_1 replaced by eps3) and is zero below
 * row kr; eigenvalues of one block closer than eps3 are moved apart by eps3 for the vector's shift only;
 * xLAEIN's start vectors on the block's own rows (zero above them), accepted at ||x||_1 >= 0.1 / sqrt(kr),
 * at most kr - kl starts; x = Q y with the stored panels on the fp64 matrix cores.  A real matrix's real
 * eigenvalue runs in real arithmetic, a conjugate pair once in complex arithmetic.  No floating-point
 * atomics and fixed summation orders: two calls return the same bits, and a selection or another batch
 * size returns the bits of the full call.
 * Read: A_colmajor (host, n x n, column-major).  opts (NULL: 1000 sweeps, batch 0, all vectors):
 * max_iterations is the Francis sweeps' limit per deflation (as eigsol_solver_options'); batch > 0 is
 * the number of eigenvalues resident in one launch (each holds kr (kr + 1) / 2 scalars of U), 0 takes
 * as many as 32 GiB (or half of the free device memory) hold; sel (NULL: all) lists nsel indices into
 * w, in the order the columns of V are wanted; selecting one eigenvalue of a real matrix's conjugate
 * pair does not select the other.
 * Out: w, n complex eigenvalues as (re, im) pairs (2 n doubles), always all of them.  For
 * 64 <= n <= 16384 (real) / 8192 (complex) they are bitwise eigsol_qr_eigenvalues_dense's Francis
 * values in its order; below 64 that entry point reduces with per-reflector kernels and eig with the
 * blocked ones, so the bits may differ.  V (NULL: eigenvalues only): n x *m_out complex doubles (both
 * dtypes), column-major with leading dimension n; column j belongs to w[sel[j]] (w[j] without sel), has
 * unit 2-norm, and its largest-modulus component (the first on ties) is real and positive.  For a real
 * matrix the vector of a real eigenvalue has imaginary part exactly 0, and the vectors of a conjugate
 * pair are bitwise conjugates.  iterations / converged (optional): the Francis sweeps', as
 * eigsol_qr_eigenvalues_dense reports them.  not_converged (optional): eigenvalues whose every start
 * failed the growth test (their last iterate is returned; expected 0).
 * Status, decided before any device call: EIGSOL_E_INVALID (n < 0; with n > 0 a null ctx, A, w or m_out;
 * max_iterations < 1; batch < 0; nsel != 0 without sel; nsel < 0; a selected index outside 0 .. n-1;
 * unknown dtype), EIGSOL_E_UNSUPPORTED (F32 / C64 / DD / CDD; n above the order the blocked reduction
 * accepts: 16384 real, 8192 complex).  n == 0: EIGSOL_OK with *m_out = 0.  A non-finite eigenvalue or
 * entry of H fails with EIGSOL_E_SOLVER.
 * Out of scope: left eigenvectors and balancing (xGEBAL); the Schur form (no Schur vectors are
 * accumulated here; eigsol_schur_dense computes it); a basis for a multiple semisimple eigenvalue whose copies land in one unreduced block
 * of H (xHSEIN's known limit: the vectors returned for it satisfy the residual bound but may be
 * parallel); single precision and double-double.
 * eigsol_eig_stage_times: the context's last eigsol_eig_dense call by stream events, 4 doubles in ms:
 * reduction (guard, Hessenberg, copy), Francis, inverse iteration (with its plan), back-transformation
 * (with the normalisation and the copy of V to the host); stages that did not run are 0. */
typedef struct eigsol_eig_options {
    int32_t max_iterations;
    int32_t batch;
    int64_t nsel;
    const int64_t* sel;
} eigsol_eig_options;
int eigsol_eig_dense(eigsol_ctx* ctx, int dtype, int64_t n, const void* A_colmajor,
                     const eigsol_eig_options* opts, double* w, void* V, int64_t* m_out,
                     int32_t* iterations, int32_t* converged, int64_t* not_converged);
int eigsol_eig_stage_times(eigsol_ctx* ctx, double* ms4);

/* ---------------------------------------------------------------- Schur form (dense)
 * eigsol_schur_dense: the Schur form A = Z T Z^H of a general dense matrix (csrc/schur.hip; the sweeps in
 * csrc/francis.hip and csrc/zfrancis.hip).  EIGSOL_F64 gives the real Schur form (T quasi-triangular with
 * 1 x 1 and standard 2 x 2 diagonal blocks, Z orthogonal), EIGSOL_C128 the complex one (T upper
 * triangular, Z unitary).  The reference has no such solver.
 * Algorithm: (1) the power-of-two range guard of eigsol_qr_eigenvalues_dense; T and the eigenvalues are
 * scaled back exactly.  (2) The blocked Hessenberg reduction with its panels kept (n >= 3; H = A and
 * Q = I for n <= 2), the entries below the sub-diagonal stored as zeros; when Z is wanted, Z = Q by the
 * stored panels applied to the identity on the fp64 matrix cores, 4096 columns at a time, before the
 * sweeps.  (3) The multishift sweeps with aggressive early deflation of
 * eigsol_qr_eigenvalues_dense(EIGSOL_QR_FRANCIS), their chase kernels, shifts and launch geometry
 * unchanged, in Schur mode: each window's delayed updates reach the whole matrix,
 * H(s:e, e:n) <- U^H H(s:e, e:n) and H(0:s, s:e) <- H(0:s, s:e) U (every left region before every right
 * region), and Z(:, s:e) <- Z(:, s:e) U runs as one more launch that T never reads; the deflation
 * window's factor is applied to the same three ranges.  (4) A diagonal block of at most 96 rows (real:
 * T and V of the block fill the LDS) or 64 rows (complex) is finished by the one-wave Schur factorisation
 * with its factor V kept, and V is applied to the three ranges.  (5) Every sub-diagonal entry the
 * deflation test accepted is stored as 0.0.  (6) Real matrices: every 2 x 2 diagonal block is
 * standardised by a rotation (LAPACK dlanv2's contract): split into two 1 x 1 blocks with an exactly
 * zero sub-diagonal entry, or left with equal diagonal entries and off-diagonal entries of opposite
 * sign; the rotation is applied to the block's rows, its columns and Z's two columns, all row rotations
 * in one launch and all column rotations in the next.  (7) The eigenvalues are read from T's diagonal
 * blocks on the device.  No floating-point atomics and fixed summation orders: two calls return the same
 * bits, and T and the eigenvalues are the same bits with and without Z.
 * Read: A_colmajor (host, n x n, column-major).  opts (NULL: 1000): max_iterations is the sweeps' limit
 * per deflation; tolerance is not read.
 * Out: T_out, n x n in A's scalar type, column-major; nothing below the first sub-diagonal is non-zero.
 * Z_out (NULL: no Schur vectors), n x n likewise.  The eigenvalues in the order of T's diagonal:
 * EIGSOL_F64 writes the real parts to eig_re_or_c and the imaginary parts to eig_im (n doubles each); the
 * two eigenvalues of a 2 x 2 block [a b; c a] are adjacent and bitwise conjugate,
 * a + i sqrt|b| sqrt|c| first and a - i sqrt|b| sqrt|c| second.  EIGSOL_C128 writes n complex doubles to
 * eig_re_or_c (T's diagonal) and does not read eig_im.  iterations / converged (optional): as
 * eigsol_qr_eigenvalues_dense reports them.
 * Not converged (a deflation took more than max_iterations sweeps): EIGSOL_OK with *converged = 0; T_out
 * is upper Hessenberg only (its 2 x 2 blocks are not standardised, the eigenvalues are read from what its
 * diagonal blocks hold), and A = Z T Z^H holds all the same.
 * Status, decided before any device call: EIGSOL_E_INVALID (n < 0; a null ctx; with n > 0 a null A, T_out
 * or eig_re_or_c, or a null eig_im with EIGSOL_F64; max_iterations < 1; unknown dtype),
 * EIGSOL_E_UNSUPPORTED (F32 / C64 / DD / CDD; n above the order the blocked reduction accepts, which is
 * eigsol_eigh_dense's: 16384 real, 8192 complex).  n == 0: EIGSOL_OK with *converged = 1.  A non-finite
 * entry of A fails with EIGSOL_E_SOLVER (found on the host, before the upload).
 * Out of scope: the complex Schur form of a real matrix (rsf2csf; reordering the diagonal blocks is
 * eigsol_ordschur_dense below); eigenvectors from T (xTREVC) and any change to eigsol_eig_dense; balancing;
 * single precision and double-double; any tuning of the deflation window or the chase.
 * eigsol_schur_stage_times: the context's last eigsol_schur_dense call by stream events, 4 doubles in ms:
 * reduction (guard, Hessenberg), forming Q, the sweeps with their updates, finish (standardisation,
 * scaling back, eigenvalues, the copies to the host). */
int eigsol_schur_dense(eigsol_ctx* ctx, int dtype, int64_t n, const void* A_colmajor,
                       const eigsol_solver_options* opts, void* T_out, void* Z_out, void* eig_re_or_c,
                       double* eig_im, int32_t* iterations, int32_t* converged);
int eigsol_schur_stage_times(eigsol_ctx* ctx, double* ms4);

/* ---------------------------------------------------------------- reordering a Schur form (dense)
 * eigsol_ordschur_dense (LAPACK xTRSEN without its condition estimates; scipy.linalg.schur's sort=): reorders
 * a Schur form A = Z T Z^H in place so that the selected eigenvalues lead T (csrc/ordschur.hip).  T_inout
 * (host, n x n, column-major) is upper triangular (C128) or real quasi-triangular in eigsol_schur_dense's
 * standard form (F64); Z_inout (NULL: none) is n x n likewise and receives Z U.  select holds one byte per
 * row of T, non-zero: selected; for a real T a flag on either row of a 2 x 2 block selects the pair (LAPACK's
 * rule).  The final order is the stable partition of T's diagonal blocks: the selected ones in their order,
 * then the others in theirs, which is xTRSEN's.
 * Algorithm: the power-of-two range guard of eigsol_schur_dense, undone exactly at the end; one flag byte
 * per row on the device, which moves with its row; rounds of disjoint windows of two half-windows (47 rows
 * real, 32 complex), even rounds on [2 k h, (2 k + 2) h), odd rounds on [(2 k + 1) h, (2 k + 3) h), a real
 * window taking the 2 x 2 block that straddles its lower end and leaving the one that straddles its upper
 * end to the window above.  One wave per window moves the window's selected blocks to its top in LDS by
 * swaps of adjacent blocks (LAPACK dlaexc with its stability test, the small Sylvester equation solved by
 * complete pivoting, every new 2 x 2 block standardised and possibly split; ztrexc's rotation for C128) and
 * keeps the window's factor U; three launches on the fp64 matrix cores then apply U to T's columns right of
 * the window, T's rows above it and Z's columns.  The host reads three words per round and stops after an
 * even and an odd round without work.  No atomics: two calls give the same bits, and T and the eigenvalues
 * have the same bits with and without Z; a selection that is already leading returns its input bit for bit.
 * Out: the eigenvalues of the reordered T as eigsol_schur_dense writes them (eig_im is required for F64);
 * *sdim (optional) the number of selected rows after the pair rule; *ordered (optional) 1, or 0 where a swap
 * was rejected by dlaexc's test (the blocks are too close to exchange): the reordering stops after that
 * round, T is a valid Schur form, A = Z T Z^H holds and the flags' count is still reported.
 * Status: EIGSOL_E_INVALID (n < 0; null ctx; with n > 0 a null T_inout, select or eig_re_or_c, or a null
 * eig_im with F64; unknown dtype; T with a non-zero below the sub-diagonal, a non-zero complex sub-diagonal
 * entry, two consecutive non-zero real sub-diagonal entries or a real 2 x 2 block that is not in standard
 * form), EIGSOL_E_UNSUPPORTED (F32 / C64 / DD / CDD; n above eigsol_schur_dense's order), EIGSOL_E_SOLVER (a
 * non-finite entry of T or Z, found on the host).  n == 0: EIGSOL_OK with *sdim = 0, *ordered = 1.
 *
 * eigsol_schur_sorted_dense: eigsol_schur_dense followed by the reordering for sort = EIGSOL_SORT_LHP
 * (Re < 0), _RHP (Re >= 0), _IUC (|lambda| <= 1) or _OUC (|lambda| > 1), scipy.linalg.schur's definitions, the
 * modulus tested as re re + im im against 1;
 * T and Z stay on the device in between and the flags are built there from the eigenvalues.  The result has
 * the bits of eigsol_schur_dense followed by eigsol_ordschur_dense with the same selection.  Arguments and
 * status as eigsol_schur_dense, and EIGSOL_E_INVALID for an unknown sort code.  A factorisation that did not
 * converge is not reordered: *converged = 0, *ordered = 0, *sdim = 0.  eigsol_schur_stage_times then
 * counts the reordering in its last stage.
 * eigsol_ordschur_stats: the context's last reordering (either entry): its time in ms by stream events, the
 * rounds that did work, the windows that did work and the swaps; null outputs are skipped.
 * Out of scope: xTRSEN's condition estimates s and sep, use of U's block-triangular structure, pipelined
 * swap chains, rsf2csf, generalised (QZ) reordering, single precision and double-double. */
enum { EIGSOL_SORT_LHP = 1, EIGSOL_SORT_RHP = 2, EIGSOL_SORT_IUC = 3, EIGSOL_SORT_OUC = 4 };
int eigsol_ordschur_dense(eigsol_ctx* ctx, int dtype, int64_t n, void* T_inout, void* Z_inout, const uint8_t* select,
                          void* eig_re_or_c, double* eig_im, int64_t* sdim, int32_t* ordered);
int eigsol_schur_sorted_dense(eigsol_ctx* ctx, int dtype, int64_t n, const void* A_colmajor,
                              const eigsol_solver_options* opts, int sort, void* T_out, void* Z_out,
                              void* eig_re_or_c, double* eig_im, int64_t* sdim, int32_t* iterations,
                              int32_t* converged, int32_t* ordered);
int eigsol_ordschur_stats(eigsol_ctx* ctx, double* ms, int32_t* rounds, int32_t* windows, int32_t* swaps);

/* ---------------------------------------------------------------- Sylvester and Lyapunov equations (dense)
 * Bartels-Stewart on the device (csrc/sylvester.hip).  The reference has no such solver; the routines below
 * correspond to LAPACK xTRSYL and to scipy.linalg.solve_sylvester / solve_continuous_lyapunov.  All matrices
 * are column-major host arrays of EIGSOL_F64 or EIGSOL_C128 scalars.
 *
 * eigsol_trsyl_dense (LAPACK dtrsyl / ztrsyl with isgn = +1, without its scale factor): solves
 * R Y + Y op(S) = F in place in F_inout (m x n), op(S) = S, or S^H when trans_b != 0.  R (m x m) and S (n x n)
 * are upper triangular (C128) or real quasi-triangular in eigsol_schur_dense's standard form (F64: 2 x 2
 * diagonal blocks with equal diagonal entries and off-diagonal entries of opposite sign).  The structure is
 * checked on the host before the upload: a non-zero below the sub-diagonal, a non-zero complex sub-diagonal
 * entry, or two consecutive non-zero real sub-diagonal entries fail with EIGSOL_E_INVALID.  The matrices are
 * cut into blocks of 63 or 64 (F64) / 32 (C128) rows that split no 2 x 2 block; the blocks of one
 * anti-diagonal wavefront are solved by one launch (one workgroup per block, in LDS) and applied by two
 * batched rank-K launches on the fp64 matrix cores.  No atomics: two calls give the same bits.
 * A pivot of a 1 x 1 .. 4 x 4 diagonal system below smin = max(eps max(max|R_ii|, max|S_jj|), 2^-1022 / eps)
 * in modulus is replaced by smin (dlasy2's rule); *perturbed counts the blocks in which that happened (0: the
 * equation was solved as posed).  There is no overflow scale factor: an ill-posed equation can give a
 * non-finite Y.
 *
 * eigsol_sylvester_dense (scipy.linalg.solve_sylvester; LAPACK xGEES + xTRSYL): solves A X + X B = C, A m x m,
 * B n x n, C and X_out m x n: A = U R U^H and B = V S V^H by the pipeline of eigsol_schur_dense, F = U^H C V,
 * the triangular stage, X = U Y V^H; between the three uploads and the one download everything stays on the
 * device.  eigsol_lyapunov_dense (scipy.linalg.solve_continuous_lyapunov): solves A X + X A^H = Q with one
 * Schur form, F = U^H Q U, the triangular stage with op(S) = R^H, X = U Y U^H.  opts->max_iterations bounds the
 * sweeps of each Schur factorisation (null opts: 1000).  If one does not converge, *converged = 0, X_out is
 * not written and the call returns EIGSOL_OK; else *converged = 1.
 * Status: EIGSOL_E_INVALID (null pointers, negative orders, unknown dtype, max_iterations < 1),
 * EIGSOL_E_UNSUPPORTED (F32 / C64 / DD / CDD; an order above eigsol_schur_dense's: 16384 real, 8192 complex),
 * EIGSOL_E_SOLVER (a non-finite entry in any input, found on the host before the upload).  m == 0 or n == 0:
 * EIGSOL_OK with nothing written but *perturbed = 0 and *converged = 1.
 * Out of scope: discrete-time (Stein) and generalised equations, the sign variant A X - X B, xTRSYL's scale
 * factor, inputs outside eigsol_schur_dense's range guard, single precision and double-double.
 * eigsol_sylvester_stage_times: the context's last eigsol_sylvester_dense / eigsol_lyapunov_dense call by
 * stream events, 5 doubles in ms: Schur of A, Schur of B (0 for Lyapunov), the transforms in, the triangular
 * stage, the transforms out with the copy to the host. */
int eigsol_trsyl_dense(eigsol_ctx* ctx, int dtype, int64_t m, int64_t n, const void* R_colmajor,
                       const void* S_colmajor, int trans_b, void* F_inout, int32_t* perturbed);
int eigsol_sylvester_dense(eigsol_ctx* ctx, int dtype, int64_t m, int64_t n, const void* A_colmajor,
                           const void* B_colmajor, const void* C_colmajor, const eigsol_solver_options* opts,
                           void* X_out, int32_t* perturbed, int32_t* converged);
int eigsol_lyapunov_dense(eigsol_ctx* ctx, int dtype, int64_t n, const void* A_colmajor, const void* Q_colmajor,
                          const eigsol_solver_options* opts, void* X_out, int32_t* perturbed, int32_t* converged);
int eigsol_sylvester_stage_times(eigsol_ctx* ctx, double* ms5);

/* ---------------------------------------------------------------- principal matrix square root (dense)
 * Through the Schur form on the device (csrc/sqrtm.hip).  The reference has no such solver; the routines
 * correspond to scipy.linalg.sqrtm.  All matrices are column-major host arrays of EIGSOL_F64 or EIGSOL_C128.
 *
 * eigsol_trsqrt_dense: the triangular stage alone, U_out = T^(1/2), U^2 = T with every eigenvalue of U in the
 * closed right half plane.  T (n x n) is upper triangular (C128) or real quasi-triangular (F64) whose 2 x 2
 * diagonal blocks have complex eigenvalues (any such block, not only eigsol_schur_dense's standard form).  The
 * host checks before the upload and fails with EIGSOL_E_INVALID on: a non-zero below the sub-diagonal, a
 * non-zero complex sub-diagonal entry, two consecutive non-zero real sub-diagonal entries, a real 2 x 2 block
 * with real eigenvalues, and a negative real 1 x 1 block (no real root: pass T as C128).  T is cut into the
 * blocks of eigsol_trsyl_dense; one launch takes the root of every diagonal block (in LDS: the scalar and
 * 2 x 2 roots, then the small Sylvester systems U_gg Y + Y U_hh = rhs along the super-diagonals), and each block
 * super-diagonal is two launches: the sums over earlier blocks on the fp64 matrix cores and the block solves
 * U_ii Y + Y U_jj = F_ij of eigsol_trsyl_dense.  No atomics: two calls give the same bits.  U is real for real
 * T, the entrywise principal root for diagonal T (a complex entry on the negative real axis, with an imaginary
 * part of either zero, goes to the positive imaginary axis), and T scaled by 4^e gives U scaled by 2^e exactly.
 * A pivot below smin = max(eps max|U_gg|, 2^-1022 / eps) is replaced by smin; *perturbed counts the blocks in
 * which that happened: 0 means the root was computed as posed, a positive value that T has a (nearly) repeated
 * eigenvalue at 0 and U solves a nearby problem or does not exist.  There is no overflow scaling.
 *
 * eigsol_sqrtm_dense: X_out = A^(1/2) (n x n): A = Z T Z^H by the pipeline of eigsol_schur_dense, the triangular
 * stage, X = Z U Z^H on the matrix cores; between the upload and the download everything stays on the device.
 * A real A whose real Schur form has a negative 1 x 1 block has no real square root: the call then returns
 * EIGSOL_OK with *needs_complex = 1 (*converged = 1, *perturbed = 0) and leaves X_out untouched; the caller
 * passes A as EIGSOL_C128, which costs a second Schur factorisation.  A zero 1 x 1 block is not negative.
 * *needs_complex = 0 otherwise.  EIGSOL_C128 storage of a matrix whose entries are all real (what such a caller
 * sends): a diagonal entry of the complex T left of the imaginary axis whose imaginary part is at most
 * n eps ||A||_F in modulus is a real eigenvalue up to the factorisation's backward error, and its imaginary part
 * is set to +0, so that its root lies on the positive imaginary axis whatever sign the rounding left (what
 * scipy.linalg.sqrtm returns through rsf2csf).  opts->max_iterations bounds the sweeps of the Schur factorisation (null opts:
 * 1000); if it does not converge, *converged = 0, X_out is not written and the call returns EIGSOL_OK.
 * Status: EIGSOL_E_INVALID (null pointers, negative order, unknown dtype, max_iterations < 1),
 * EIGSOL_E_UNSUPPORTED (F32 / C64 / DD / CDD; an order above eigsol_schur_dense's), EIGSOL_E_SOLVER (a
 * non-finite entry, found on the host before the upload).  n == 0: EIGSOL_OK, nothing written but the flags.
 * Out of scope: funm, signm, non-principal roots, rsf2csf, a condition or error estimate.
 * eigsol_sqrtm_stage_times: the context's last eigsol_sqrtm_dense call by stream events, 4 doubles in ms: the
 * Schur factorisation, the triangular stage, the transform with the copy to the host, and their sum. */
int eigsol_trsqrt_dense(eigsol_ctx* ctx, int dtype, int64_t n, const void* T_colmajor, void* U_out, int32_t* perturbed);
int eigsol_sqrtm_dense(eigsol_ctx* ctx, int dtype, int64_t n, const void* A_colmajor, const eigsol_solver_options* opts,
                       void* X_out, int32_t* perturbed, int32_t* converged, int32_t* needs_complex);
int eigsol_sqrtm_stage_times(eigsol_ctx* ctx, double* ms4);

/* ---------------------------------------------------------------- product, solve and exponential (dense)
 * Column-major host arrays of EIGSOL_F64 or EIGSOL_C128 in and out; the reference has no such routines.
 *
 * eigsol_gemm_dense: C_out (m x n) = A (m x k) B (k x n) on the fp64 matrix cores (csrc/gemm.hip): a workgroup
 * owns a 128 x 128 (complex: 128 x 64) tile of C, stages slices of 16 of K through LDS and keeps the tile in
 * registers; C is written once.  One lane sums an entry in ascending k: no split-K, no atomics, two calls
 * give the same bits.  Any m, n, k >= 0 (k == 0: C = 0).
 *
 * eigsol_solve_dense: X_out (n x nrhs) = A^-1 B by LU with partial pivoting, the blocked factorisation of the
 * shifted solves (csrc/dense_lu.hip), and a blocked substitution with all right-hand sides: the diagonal blocks by
 * substitution, the rest on the matrix cores.  X_out may be B.  An exactly zero pivot fails with EIGSOL_E_SOLVER and
 * the message names its column (0-based); nothing is written then.  No condition estimate, no refinement.
 *
 * eigsol_expm_dense: X_out = exp(A) (n x n) by Higham's 2005 scaling and squaring (csrc/expm.hip;
 * scipy.linalg.expm without the 2009 norm estimates): alpha = ||A||_1 on the device, eigsol_expm_plan's degree and
 * squarings (returned in *degree and *squarings, either may be null), the [m/m] Pade approximant of 2^-s A by
 * three to six products and one LU solve with n right-hand sides, s squarings.  Real A gives real X; A = 0
 * gives exactly I.  A strongly non-normal A is scaled by its norm alone and may be squared more often than SciPy
 * squares it.  EIGSOL_E_SOLVER: a non-finite entry (found on the host before the upload), a 1-norm that
 * overflows, or a non-finite result ("result overflows"; X_out then holds it).
 * eigsol_expm_stage_times: the context's last eigsol_expm_dense call by stream events, 6 doubles in ms: the
 * upload with the norm, the Pade products, the LU factorisation, the substitution, the squarings, and the whole
 * call: these five, the pass that looks for a non-finite entry and the copy to the host.
 * eigsol_expm_plan (host only): the first degree m of 3, 5, 7, 9, 13 with alpha <= theta_m (Higham's Table 2.3)
 * and s = 0; beyond theta_13 m = 13 and s is the smallest integer with alpha 2^-s <= theta_13.  EIGSOL_E_INVALID
 * for a negative or non-finite alpha.
 * Status of the three device entries: EIGSOL_E_INVALID (null pointers, a negative size, unknown dtype),
 * EIGSOL_E_UNSUPPORTED (F32 / C64 / DD / CDD; an order whose matrix does not fit).  An empty result: EIGSOL_OK.
 * Out of scope: funm, signm, the action of exp(A) on a vector, Frechet derivatives, condition estimates,
 * batches. */
int eigsol_gemm_dense(eigsol_ctx* ctx, int dtype, int64_t m, int64_t n, int64_t k, const void* A_colmajor,
                      const void* B_colmajor, void* C_out);
int eigsol_solve_dense(eigsol_ctx* ctx, int dtype, int64_t n, int64_t nrhs, const void* A_colmajor, const void* B_colmajor,
                       void* X_out);
int eigsol_expm_plan(double alpha, int32_t* degree, int32_t* squarings);
int eigsol_expm_dense(eigsol_ctx* ctx, int dtype, int64_t n, const void* A_colmajor, void* X_out, int32_t* degree,
                      int32_t* squarings);
int eigsol_expm_stage_times(eigsol_ctx* ctx, double* ms6);

/* ---------------------------------------------------------------- principal matrix logarithm (dense)
 * Through the Schur form on the device (csrc/logm.hip): the Schur-Pade inverse scaling and squaring method (Higham,
 * Functions of Matrices, Alg. 11.9, with the bounds theta_1 .. theta_7 of Al-Mohy and Higham (2012) applied to the
 * 1-norm).  The reference has no such solver; the routines correspond to scipy.linalg.logm.  All matrices are
 * column-major host arrays of EIGSOL_F64 or EIGSOL_C128.
 *
 * eigsol_trlogm_dense: the triangular stage alone, L_out = log T, the principal logarithm: exp(L) = T and every
 * eigenvalue of L has its imaginary part in (-pi, pi].  T as for eigsol_trsqrt_dense, with the same host checks
 * (EIGSOL_E_INVALID: a non-zero below the sub-diagonal, a non-zero complex sub-diagonal entry, two consecutive
 * non-zero real sub-diagonal entries, a real 2 x 2 block with real eigenvalues, a negative real 1 x 1 block: pass T
 * as C128); a zero 1 x 1 diagonal block (T is singular) fails with EIGSOL_E_SOLVER and the message names its row
 * (0-based).  The stage keeps T's three inner diagonals, takes square roots of T in place with the kernels of
 * eigsol_trsqrt_dense, and after each forms R = T^(1/2^s) - I and ||R||_1 (one host wait of 8 bytes per root);
 * eigsol_logm_plan decides from the norm whether to stop; more than 64 roots fail with EIGSOL_E_SOLVER.  Then the
 * [m / m] Pade approximant of log(I + R) through its partial fractions sum_j alpha_j (I + beta_j R)^-1 R (alpha, beta:
 * the m-point Gauss-Legendre rule on [0, 1]): the m block triangular systems are solved together, one launch that
 * inverts the diagonal blocks I + beta_j R_ii (condition at most 1.81, as ||R||_1 <= 0.288) and one launch per block
 * super-diagonal on the fp64 matrix cores, with no host wait between them (their scratch, m n^2 scalars, is allocated
 * first); L = 2^s sum_j alpha_j X_j.  L's diagonal blocks are
 * recomputed from T itself: log t for a 1 x 1 block (C128: ln|t| + i atan2(im, re), an imaginary part of -0.0
 * counting as +0.0, so both zeros on the negative real axis give +i pi), ln|lambda| I + (atan2(mu, a) / mu)(B - a I)
 * for a real 2 x 2 block with eigenvalues a +- i mu; and the super-diagonal entry between two 1 x 1 blocks by Al-Mohy
 * and Higham's formula (2012, eq. 5.6).  L has exact zeros below the quasi-triangle, is real for real T, the
 * entrywise principal logarithm for diagonal T, and exactly 0 with *roots = 0 and *degree = 0 for T = I.  No
 * atomics: two calls give the same bits.  *roots, *degree (1 .. 7) and *perturbed (the sum of the root stages'
 * counts, see eigsol_trsqrt_dense) may be null.
 *
 * eigsol_logm_dense: X_out = log A (n x n): A = Z T Z^H by the pipeline of eigsol_schur_dense, the triangular
 * stage, X = Z L Z^H on the matrix cores.  A real A whose real Schur form has a negative 1 x 1 block has no real
 * logarithm: the call then returns EIGSOL_OK with *needs_complex = 1 (*converged = 1) and leaves X_out untouched;
 * the caller passes A as EIGSOL_C128, which costs a second Schur factorisation.  For EIGSOL_C128 storage of a matrix
 * whose entries are all real, the real negative eigenvalues are put on the axis with imaginary part +0 as in
 * eigsol_sqrtm_dense, so that their logarithms have imaginary part +pi (scipy.linalg.logm's branch).  A singular A
 * (an exactly zero 1 x 1 block of T) fails with EIGSOL_E_SOLVER.  opts->max_iterations bounds the sweeps of the
 * Schur factorisation (null opts: 1000); if it does not converge, *converged = 0, X_out is not written and the call
 * returns EIGSOL_OK.  Status otherwise as eigsol_sqrtm_dense.  n == 0: EIGSOL_OK, nothing written but the flags.
 * eigsol_logm_plan (host only): *degree for ||R||_1 = norm: 0 (another root) while norm > theta_7 = 0.288; else
 * with j1 = min{m : norm <= theta_m} and j2 = min{m : norm / 2 <= theta_m}, j1 if j1 - j2 <= 1 or tried != 0 (the
 * test was reached before), else 0.  EIGSOL_E_INVALID for a negative or non-finite norm.
 * eigsol_logm_stage_times: the context's last eigsol_logm_dense call by stream events, 5 doubles in ms: the Schur
 * factorisation, the root loop, the Pade stage, the transform with the copy to the host, and their sum.
 * Out of scope: the alpha_p norm estimates of the 2012 algorithm, the cancellation-free recomputation of R's
 * diagonal, degrees above 7, funm, signm and fractional powers, Frechet derivatives and condition estimates. */
int eigsol_trlogm_dense(eigsol_ctx* ctx, int dtype, int64_t n, const void* T_colmajor, void* L_out, int32_t* roots,
                        int32_t* degree, int32_t* perturbed);
int eigsol_logm_dense(eigsol_ctx* ctx, int dtype, int64_t n, const void* A_colmajor, const eigsol_solver_options* opts,
                      void* X_out, int32_t* roots, int32_t* degree, int32_t* perturbed, int32_t* converged,
                      int32_t* needs_complex);
int eigsol_logm_plan(double norm, int32_t tried, int32_t* degree);
int eigsol_logm_stage_times(eigsol_ctx* ctx, double* ms5);

/* ---------------------------------------------------------------- singular value decomposition (dense)
 * eigsol_svd_dense: the thin singular value decomposition A = U diag(s) V^H of a real (EIGSOL_F64) or
 * complex (EIGSOL_C128) dense m x n matrix, k = min(m, n) (csrc/svd.hip).  The reference has no such solver.
 * Algorithm: block one-sided Jacobi (Hestenes).  m < n works on A^H with the roles of U and V swapped.  The
 * matrix is scaled by a power of two so that its largest component lies in [1, 2), and s is scaled back.
 * The columns are cut into blocks of 32 (real) / 16 (complex); a sweep visits every pair of blocks once in
 * a round-robin schedule whose steps hold disjoint pairs, and each step is three launches: the pairs' Gram
 * matrices on the fp64 matrix cores (row chunks, partials added in a fixed order); per pair one workgroup
 * that skips the pair where max |g_ij| / sqrt(g_ii g_jj) <= tol = sqrt(max(m, n)) eps, else diagonalises G
 * by cyclic two-sided Jacobi to the same tolerance (Rutishauser's rotation, parallel disjoint rotations)
 * and polishes the accumulated rotation J by one Newton-Schulz step; X <- X J on the matrix cores for the
 * pair's columns of W and, where accumulated, of V.  The host reads the pairs' maxima once per sweep and
 * stops where none exceeds tol.  Then s_j = ||w_j||_2 sorted descending (stable), u_j = w_j / s_j.  No
 * floating-point atomics and fixed summation orders: two calls return the same bits, and s does not
 * depend on which of U and V are asked for.
 * Read: A_colmajor (host, m x n, column-major, leading dimension m).  opts (NULL: 60): max_sweeps.
 * Out: s, k singular values, descending.  U (NULL: not wanted): m x k; V (NULL: not wanted): n x k, V
 * itself and not V^H; both column-major with orthonormal columns.  Column j of V has its
 * largest-modulus component (the first on ties) real and positive, and U's phase follows from
 * A V = U diag(s).  A column of U (for m < n: of V) whose singular value is exactly 0 completes the
 * orthonormal set: unit vectors e_k in ascending k, each orthogonalised twice against all columns,
 * accepted at norm >= 0.5; that loop is serial over such columns, which is acceptable because exact
 * zeros are rare.  sweeps (optional): the sweeps run, the last of which rotated nothing where the call
 * converged.  not_converged (optional): the pairs of blocks still above tol when max_sweeps ran out (the
 * result so far is returned; expected 0).
 * Status, decided before any device call: EIGSOL_E_INVALID (m < 0 or n < 0; with m, n > 0 a null ctx, A
 * or s; max_sweeps < 1; unknown dtype), EIGSOL_E_UNSUPPORTED (F32 / C64 / DD / CDD; more than 2^31
 * entries).  m == 0 or n == 0: EIGSOL_OK, nothing written but *sweeps = 0 and *not_converged = 0.  A
 * non-finite entry fails with EIGSOL_E_SOLVER.
 * Out of scope: full_matrices (the square U of a tall matrix); single precision and double-double; QR
 * preconditioning of tall or ill-conditioned matrices (Drmac-Veselic), which would cut the sweeps of
 * ill-conditioned matrices; a bidiagonal (gesdd) path; truncated or selected triplets; columns whose
 * norm lies more than about 2^500 below the largest (their squares underflow in G).
 * eigsol_svd_stage_times: the context's last eigsol_svd_dense call by stream events, 4 doubles in ms:
 * Gram, pair Jacobi, apply (each summed over all steps), finish (norms, sort, normalisation, completion,
 * phases and the copies to the host). */
typedef struct eigsol_svd_options {
    int32_t max_sweeps;
} eigsol_svd_options;
int eigsol_svd_dense(eigsol_ctx* ctx, int dtype, int64_t m, int64_t n, const void* A_colmajor,
                     const eigsol_svd_options* opts, double* s, void* U, void* V, int32_t* sweeps,
                     int64_t* not_converged);
int eigsol_svd_stage_times(eigsol_ctx* ctx, double* ms4);

/* ---------------------------------------------------------------- Cholesky and A x = lambda B x (dense)
 * eigsol_cholesky_dense: B = L L^H of a real symmetric / complex Hermitian positive definite B
 * (EIGSOL_F64 / EIGSOL_C128; host, n x n, column-major; ONLY the lower triangle is read, and for
 * C128 the diagonal's imaginary parts are ignored).  Blocked and right-looking with block width 64
 * (real) or 32 (complex); the trailing update runs on the fp64 matrix cores.  L_colmajor (host, n x n)
 * receives L with an exactly zero strict upper triangle and a real positive diagonal.
 * eigsol_geigh_dense: type 1 only, A x = lambda B x with A Hermitian and B Hermitian positive
 * definite (the lower triangles of both are read, as above).  B = L L^H; C = L^-1 A L^-H by two blocked
 * triangular solves with n right-hand sides and a conjugate transpose between (2 n^3 flops against
 * sygst's n^3); eigsol_eigh_dense's solver on C without leaving the device; X = L^-H Y by a blocked
 * upper-triangular solve.  opts, w, Z, m_out and not_converged are eigsol_eigh_dense's, but the columns
 * of Z are B-orthonormal (Z^H B Z = I, LAPACK's convention) instead of unit 2-norm; the phase
 * convention is the same.  A selection returns bitwise the values of the full call; two calls on the
 * same input return the same bits; a values-only call (Z NULL) skips the eigenvector stages.
 * info (optional, both entries): -1 on success; else the 0-based index of the first column whose
 * pivot is not > 0 (NaN included), the call returns EIGSOL_E_SOLVER and the message names the index
 * and says "not positive definite".  A non-finite entry in either lower triangle fails with
 * EIGSOL_E_SOLVER.
 * Status, decided before any device call: as eigsol_eigh_dense (EIGSOL_E_INVALID: n < 0; with n > 0
 * a null ctx, A, B, w or m_out - for the Cholesky entry B or L; a bad selection; an unknown dtype;
 * EIGSOL_E_UNSUPPORTED: F32 / C64 / DD / CDD; n above eigsol_eigh_dense's limit).  n == 0: EIGSOL_OK
 * with *m_out = 0 and *info = -1.
 * eigsol_geigh_stage_times: the context's last eigsol_geigh_dense call by stream events, 7 doubles in
 * ms: cholesky (with the mirroring), standardise, reduction, bisection, inverse_iteration,
 * back_transform (the stored-panel step and the copy of Z), triangular_back_solve; stages that did
 * not run are 0. */
int eigsol_cholesky_dense(eigsol_ctx* ctx, int dtype, int64_t n, const void* B_colmajor,
                          void* L_colmajor, int64_t* info);
int eigsol_geigh_dense(eigsol_ctx* ctx, int dtype, int64_t n, const void* A_colmajor, const void* B_colmajor,
                       const eigsol_eigh_options* opts, double* w, void* Z, int64_t* m_out,
                       int64_t* not_converged, int64_t* info);
int eigsol_geigh_stage_times(eigsol_ctx* ctx, double* ms7);
/* Host only (no device): the plan eigsol_eigh_dense makes for the tridiagonal T = (d: n, e: n - 1)
 * and m of its eigenvalues w (ascending).  block_of[i] (n): the split block of row i, blocks numbered
 * from 0 upwards; cluster_of[j] (m): the cluster of w[j], clusters numbered in the order their first
 * eigenvalue appears in w.  An eigenvalue is given to the block whose Sturm count claims it (equal
 * eigenvalues of several blocks: the lowest block that has one left); within a block it starts a new
 * cluster when it lies more than 1e-3 ||T_block||_1 above the block's previous one.  Fails with
 * EIGSOL_E_INVALID on null pointers, n < 0, m < 0, m > n, a descending w, or a w[j] that no block
 * claims. */
int eigsol_tridiag_plan(int64_t n, const double* d, const double* e, int64_t m, const double* w,
                        int64_t* block_of, int64_t* cluster_of, int64_t* nblocks, int64_t* nclusters);

/* ---------------------------------------------------------------- eigh by divide and conquer
 * eigsol_eigh_dense_m / eigsol_geigh_dense_m: eigsol_eigh_dense / eigsol_geigh_dense with the method
 * of the tridiagonal stage as an argument after opts.  EIGSOL_EIGH_METHOD_STEIN is the existing entry,
 * bit for bit (the existing entries are method 0).  EIGSOL_EIGH_METHOD_DC replaces bisection and
 * inverse iteration by Cuppen's divide and conquer with Gu and Eisenstat's stabilisation (LAPACK
 * dstedc / dlaed1-4's scheme; csrc/eigh_dc.hip): every split block of T is scaled by the power of two
 * that brings its largest entry into [1, 2) (exact; undone on the eigenvalues), then halved down to leaves of
 * order <= 64 (EIGSOL_DC_LEAF = 2 .. 64, read per call, overrides the leaf order); at a cut c
 * rho = e_c is taken off d_c and d_{c+1}; the leaves are solved by implicit QL, one wave each; then,
 * level by level and all merges of a level in the same launches: dlaed2's deflation on the host
 * (eigsol_dc_deflate below, one host wait per level), the secular equation's roots one lane each,
 * relative to the nearer pole, by bisection on the offset; Loewner's recomputed z; the vector matrix U
 * with unit columns; Q(:, kept) <- Q(:, kept) U on the fp64 matrix cores.  The orthogonality of the
 * vectors does not depend on how the spectrum clusters.
 * Under DC: dtypes, order limit, scaling, mirroring, the non-finite check, the phase convention and
 * (generalised) B-orthonormality are the existing ones.  w holds the divide-and-conquer values: within
 * 2 n eps ||A||_F of LAPACK's but not bitwise eigsol_eigh_dense's.  A selection computes every pair of
 * T and takes the selected columns of the sorted list before the back-transformation: it returns
 * bitwise the full DC call's values, and its vectors too as long as the back-transformation sums in
 * the same order for both column counts (it does for n <= 4096).  EIGSOL_EIGH_VALUE compares with the
 * computed values.  A values-only call (Z NULL) is the bisection path whatever the method.
 * not_converged: leaf eigenvalues (60 QL sweeps) or secular roots (400 bisection steps) that hit
 * their iteration cap; expected 0.  No floating-point atomics: two calls return the same bits.
 * Workspace: three n x n real matrices on the device (Q, the permuted Q, U), freed before the
 * back-transformation.  An unknown method returns EIGSOL_E_INVALID before any device call.
 * Under DC eigsol_eigh_stage_times reports the whole tridiagonal stage in its third slot and 0 in
 * the second.  eigsol_eigh_dc_stage_times: the context's last DC call, 6 doubles in ms: reduction,
 * leaves, host deflation (wall time of the scan alone; the uploads and the wait are in no slot), secular +
 * Loewner + vector kernels
 * (with the rotations and the column permutation), merge GEMMs (with the copy of the deflated
 * columns), back-transformation; by stream events except the host stage. */
#define EIGSOL_EIGH_METHOD_STEIN 0
#define EIGSOL_EIGH_METHOD_DC 1
int eigsol_eigh_dense_m(eigsol_ctx* ctx, int dtype, int64_t n, const void* A_colmajor,
                        const eigsol_eigh_options* opts, int32_t method, double* w, void* Z,
                        int64_t* m_out, int64_t* not_converged);
int eigsol_geigh_dense_m(eigsol_ctx* ctx, int dtype, int64_t n, const void* A_colmajor, const void* B_colmajor,
                         const eigsol_eigh_options* opts, int32_t method, double* w, void* Z,
                         int64_t* m_out, int64_t* not_converged, int64_t* info);
int eigsol_eigh_dc_stage_times(eigsol_ctx* ctx, double* ms6);
/* Host only (no device): the deflation step of one divide-and-conquer merge, dlaed2's rules, on
 * D + rho z z^T with D = diag(d) (n poles in any order: the eigenvalues of the two halves, the first
 * n1 from the left one; n1 is only checked, 1 <= n1 < n: the poles are sorted whole, not merged from two
 * sorted halves) and z (n) the halves' boundary rows.  The caller scales the problem so that max |d| is
 * of order 1, as the driver does: tol below takes |z| <= 1 as the scale of the poles.  z is divided by its 2-norm
 * and rho multiplied by its square; the poles are sorted (stable); tol = 8 u max(max |d|, max |z|),
 * u = 2^-53.  In ascending order of the poles: j is dropped when rho |z_j| <= tol; a pole j is rotated
 * together with the last kept candidate p when |t c s| <= tol (t = d_j - d_p, (c, s) = (z_j, -z_p) /
 * hypot(z_j, z_p)): columns (p, j) <- (c p + s j, c j - s p), z_j = hypot, z_p = 0, d_p and d_j
 * replaced by the rotated diagonal, p deflated and j the new candidate.
 * Out: *k_out kept poles; perm (n): perm[q] = the old index of new place q, the kept poles first and
 * ascending, then the deflated ones in the order they were dropped; dk (n): the values at the new
 * places (kept poles, then deflated eigenvalues); zk (n): the kept z, then zeros; *rho_out;
 * *nrot_out rotations in the order to apply them, rot_cols (2 per rotation, capacity 2 (n - 1)): old
 * indices (p, j); rot_cs (2 per rotation): (c, s); *tol_out (optional).
 * EIGSOL_E_INVALID: a null pointer, n < 2, n1 outside 1 .. n - 1, rho <= 0 or a non-finite input. */
int eigsol_dc_deflate(int64_t n, int64_t n1, const double* d, const double* z, double rho,
                      int64_t* k_out, int64_t* perm, double* dk, double* zk, double* rho_out,
                      int64_t* nrot_out, int64_t* rot_cols, double* rot_cs, double* tol_out);

/* ---------------------------------------------------------------- row-sharded power iteration
 * One process per GPU; RCCL over xGMI (the reference has no distribution: SURVEY.md §2.1).
 * Rank r owns global rows [row_begins[r], row_begins[r+1]).  Bootstrap: rank 0 calls
 * eigsol_dist_get_unique_id, broadcasts the bytes with any transport, every rank calls
 * eigsol_ctx_create_dist.  eigsol_csr_create_dist is collective; the resulting matrix is used with
 * the eigsol_power_* session functions unchanged (x0 / x_out hold the rank's own rows).  Each
 * iteration exchanges x plus one 32-byte all-gather of rank partials; every rank reaches the same
 * termination decision.  The x exchange (chosen collectively, eigsol_exchange_mode):
 *   EIGSOL_EXCHANGE_HALO      only the entries other ranks read, point to point (banded matrices);
 *   EIGSOL_EXCHANGE_ALLGATHER every rank keeps all of x and the row blocks are all-gathered
 *                             (unstructured columns, where a rank reads most of x anyway). */
#define EIGSOL_EXCHANGE_HALO 0
#define EIGSOL_EXCHANGE_ALLGATHER 1
int eigsol_dist_unique_id_bytes(void);
int eigsol_dist_get_unique_id(void* id_out);
/* Test transport: an id that makes eigsol_ctx_create_dist join an in-process loopback world of
 * nranks ranks instead of an RCCL communicator (one host thread per rank, any devices of this
 * process, e.g. all on one GPU).  Every exchange of the row-sharded path runs as device copies
 * between the ranks' buffers, so the whole device-side path (ghost layout, pack, halo and
 * all-gather slots, rank-order partials) can be tested where RCCL cannot run several ranks. */
int eigsol_dist_loopback_id(int nranks, void* id_out);
int eigsol_ctx_create_dist(int device, int rank, int nranks, const void* unique_id,
                           eigsol_ctx** out);
int eigsol_csr_create_dist(eigsol_ctx* ctx, eigsol_dtype dtype, const int64_t* row_begins,
                           int64_t nnz_local, const int32_t* rowptr_local,
                           const int32_t* colidx_global, const void* values, eigsol_csr** out);
/* Host-only planning used by eigsol_csr_create_dist (no device, no communication): remaps global
 * columns to the local x-space [ghosts of lower ranks | own rows | ghosts of higher ranks] and
 * lists the ghosts (ascending global index) with their per-owner counts. */
int eigsol_ghost_plan(int nranks, const int64_t* row_begins, int rank, int64_t nnz_local,
                      const int32_t* colidx_global, int32_t* colidx_local, int64_t* nghost,
                      int64_t* ghost_global, int64_t* recv_counts);
/* Host-only: the exchange every rank of eigsol_csr_create_dist selects from the P x P ghost counts
 * (ghost_counts[r * P + q] = entries rank r reads from rank q): all-gather when some rank reads at
 * least a quarter of the rows it does not own, else halo.  EIGSOL_DIST_EXCHANGE=halo|allgather
 * overrides. */
int eigsol_exchange_mode(int nranks, const int64_t* row_begins, const int64_t* ghost_counts, int* mode);
/* The exchange a row-sharded matrix uses (EIGSOL_EXCHANGE_*) and its number of ghost entries. */
int eigsol_csr_dist_info(const eigsol_csr* A, int* mode, int64_t* nghost);

/* Host-collective bootstrap, no RCCL communicator: `allgather` gathers bytes_per_rank host bytes
 * from every rank into recv (rank order) and returns 0 on success; the library calls it for its
 * setup steps only (ghost plan counts and request lists, inbox addresses / IPC handles, barriers)
 * and never from a kernel-issuing hot loop.  Any host transport works (MPI, torch.distributed
 * gloo, sockets).  Row-sharded sessions on such a context use the device-side peer exchange. */
typedef int (*eigsol_allgather_fn)(const void* send, void* recv, size_t bytes_per_rank, void* user);
int eigsol_ctx_create_dist_host(int device, int rank, int nranks, eigsol_allgather_fn allgather,
                                void* user, eigsol_ctx** out);

/* Per-iteration transport of a power session (eigsol_power_transport):
 *   EIGSOL_TRANSPORT_LOCAL     one GPU, nothing to exchange;
 *   EIGSOL_TRANSPORT_COLLECTIVE host-enqueued pack kernel + RCCL group (or loopback copies) after
 *                              every launch (all-gather exchange, non-sliced layouts);
 *   EIGSOL_TRANSPORT_PEER      device-side: the fused SpMV's epilogue stores the halo rows and the
 *                              rank partial straight into every peer's inbox (IPC-mapped over xGMI,
 *                              or same-device pointers in a loopback world) and raises an epoch
 *                              flag there; the next launch's prologue waits for the peers' flags.
 *                              No host round trip, no extra launch.  EIGSOL_DIST_TRANSPORT=
 *                              collective|peer overrides the collective choice (halo matrices in
 *                              the sliced layout use peer by default). */
#define EIGSOL_TRANSPORT_LOCAL 0
#define EIGSOL_TRANSPORT_COLLECTIVE 1
#define EIGSOL_TRANSPORT_PEER 2
int eigsol_power_transport(const eigsol_power* s, int* transport);

/* Host-only planning of the peer exchange (no device): this rank's push list.  requests holds
 * the global rows other ranks read from this rank, grouped by requesting rank in rank order with
 * counts ghost_counts[q * P + rank] (each group ascending, as eigsol_ghost_plan lists them);
 * ghost_counts is the all-gathered P x P matrix of eigsol_ghost_plan's recv_counts.  Output: per
 * request an entry {local row, peer, slot, 0}, where slot indexes the peer's ghost list (its
 * [lower | upper] ghost order), sorted by local row. */
int eigsol_peer_plan(int nranks, int rank, const int64_t* row_begins, const int64_t* ghost_counts,
                     const int64_t* requests, int64_t nreq, int32_t* push_out);
/* This context's place in the world: device, rank, ranks, and how it exchanges (0 none, 1 RCCL
 * communicator, 2 in-process loopback world, 3 caller's host all-gather + device peer inboxes). */
int eigsol_ctx_info(eigsol_ctx* ctx, int* device, int* rank, int* nranks, int* comm_kind);

/* ---------------------------------------------------------------- measurement
 * The device's practical HBM bandwidth ("verify the spec with a STREAM-like kernel
 * on the box"): hand-written gfx950 streams over `bytes` (use >= 2 GiB: beyond the 256 MB
 * Infinity Cache) with non-temporal loads / stores, four in flight per lane, timed with HIP events
 * over `reps` launches on the context's stream, best over 1/2/4/8 workgroups per CU.
 * read = load only (16- and 8-byte loads, the better), copy = load + store (both directions
 * counted), write = store only (GB/s). */
int eigsol_hbm_probe(eigsol_ctx* ctx, size_t bytes, int reps, double* read_gbps, double* copy_gbps,
                     double* write_gbps, int* best_blocks_per_cu);
/* The headline SpMV's read / write mix (12 reads : 1 write of 16-byte non-temporal words) over
 * `bytes` of reads: GB/s of both directions, best over 1/2/4/8 workgroups per CU. */
int eigsol_hbm_probe_mix(eigsol_ctx* ctx, size_t bytes, int reps, double* mix_gbps, int* best_blocks_per_cu);

/* ---------------------------------------------------------------- sparse LU analysis (host only)
 * The symbolic factorization the general-sparse shifted solve runs before choosing the exact LU
 * over ILU(0) (variant 18 vs 7): the pattern of A with its diagonal inserted, closed under fill
 * for LU without pivoting (row i = its own columns plus, for every k < i in it in ascending order,
 * fill included, row k's columns past k).  Stops once the pattern would pass `cap` entries.
 * *nnz_out = the filled pattern's entries, or -1 when it exceeds cap; *lower_levels_out (optional)
 * = dependency levels of its strict lower part (the numeric factorization's launches).  Rows must
 * be sorted; needs no device. */
int eigsol_sparse_lu_fill(int64_t n, const int32_t* rowptr, const int32_t* colidx, int64_t cap, int64_t* nnz_out,
                          int32_t* lower_levels_out);

/* The nested-dissection multifrontal plan of the general-sparse shifted solve (variant 19; host
 * only): the ordering of the pattern of A + A^T and the supernodal structure.  perm_out (n
 * entries, new -> old) and fronts_out (4 int32 per front: first column, pivots, struct size,
 * parent front or -1; fronts in postorder) may be null; fronts_cap = room in fronts_out (fronts).
 * stats_out[8] = fronts, tree heights, largest front order, most pivots of a front, stored factor
 * entries, sum of squared front orders, factorization flops (complex arithmetic if is_complex),
 * 1.0 when the plan is consistent.  Call once with fronts_out = null to size it. */
int eigsol_mf_analyze(int64_t n, const int32_t* rowptr, const int32_t* colidx, int32_t leaf, int32_t is_complex,
                      int32_t* perm_out, int32_t* fronts_out, int64_t fronts_cap, double* stats_out);

#ifdef __cplusplus
}
#endif
#endif /* EIGSOL_HIP_H */
