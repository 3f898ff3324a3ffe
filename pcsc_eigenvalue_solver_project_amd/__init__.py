"""MI355X-native eigenvalue-solver hot path (Python view of the C ABI).

The product is ``libeigsol_hip.so`` (hand-written HIP kernels for gfx950, ``csrc/``) behind the
C ABI in ``include/eigsol_hip.h`` and the C++ drop-in façade in ``include/eigsol/``.  This package
is the thin Python view used by the tests and the benchmark; its names follow the reference's
C++ API (``SolverOptions``, ``EigenResult``, ``power_method`` ≙ ``EigSol::powerMethod``).
No CPU fallback exists: without the library or a gfx950 device every call raises ``EigSolError``.
"""
from __future__ import annotations

import ctypes   # by its own name where a parameter is called C (solve_sylvester)
import ctypes as C
from dataclasses import dataclass
from typing import Optional

import numpy as np

from ._capi import (EIGSOL_C64, EIGSOL_C128, EIGSOL_CDD, EIGSOL_DD, EIGSOL_E_INVALID, EIGSOL_E_SIZE_MISMATCH, EIGSOL_E_SOLVER,
                    EIGSOL_E_UNSUPPORTED, EIGSOL_F32,
                    EIGSOL_F64, EIGSOL_KRYLOV_LM, EIGSOL_KRYLOV_SHIFT_INVERT, EigSolError, KrylovOptionsC, SolverOptionsC,
                    SubspaceOptionsC, call, check, last_error, lib)
from ._capi import EIGSOL_EIGH_INDEX, EIGSOL_EIGH_VALUE, EighOptionsC
from ._capi import EigOptionsC, SvdOptionsC, SvdsOptionsC

__all__ = [
    "EigSolError", "SolverOptions", "EigenResult", "Context", "CsrMatrix", "DenseMatrix",
    "PowerSession", "power_method", "device_count", "lib", "last_error",
    "SubspaceOptions", "SubspaceResult", "subspace_iteration", "spmm", "dense_mm",
    "KrylovOptions", "KrylovResult", "krylov_schur", "krylov_orth", "krylov_rotate",
    "EighResult", "eigh", "eigvalsh", "eigh_stage_times", "tridiag_plan", "eigh_dc_stage_times", "dc_deflate",
    "cholesky", "geigh_stage_times", "EigResult", "eig", "eig_stage_times", "SchurResult", "schur", "schur_stage_times",
    "OrdSchurResult", "ordschur", "ordschur_stats",
    "SylvesterResult", "solve_sylvester", "solve_continuous_lyapunov", "trsyl", "sylvester_stage_times",
    "SqrtmResult", "sqrtm", "trsqrt", "sqrtm_stage_times",
    "LogmResult", "logm", "trlogm", "logm_stage_times", "logm_plan",
    "matmul", "solve", "ExpmResult", "expm", "expm_stage_times", "expm_plan",
    "SvdResult", "svd", "svdvals", "svd_stage_times",
    "SvdsOptions", "SvdsResult", "svds", "svds_stage_times", "dense_mv_h",
]


@dataclass
class SolverOptions:
    """``EigSol::SolverOptions`` (src/option/solver_option.hpp:14-20)."""

    maxIterations: int = 1000
    tolerance: float = 1e-10

    def to_c(self) -> SolverOptionsC:
        return SolverOptionsC(int(self.maxIterations), float(self.tolerance))


@dataclass
class EigenResult:
    """``EigSol::EigenResult<S>`` (src/result/eigen_result.hpp:22-52)."""

    eigenvalue: complex | float
    eigenvector: np.ndarray
    iterations: int
    converged: bool


def _dtype_code(dt) -> int:
    dt = np.dtype(dt)
    if dt == np.float64:
        return EIGSOL_F64
    if dt == np.complex128:
        return EIGSOL_C128
    if dt == np.float32:
        return EIGSOL_F32
    if dt == np.complex64:
        return EIGSOL_C64
    if dt == np.longdouble:
        return EIGSOL_DD
    if dt == np.clongdouble:
        return EIGSOL_CDD
    raise EigSolError(3, f"scalar type mismatch: {dt} (supported: float64, complex128, float32, complex64, "
                         "longdouble, clongdouble)")


def _np_dtype(code: int):
    return {EIGSOL_C128: np.complex128, EIGSOL_F32: np.float32, EIGSOL_C64: np.complex64,
            EIGSOL_DD: np.longdouble, EIGSOL_CDD: np.clongdouble}.get(code, np.float64)


def _ptr(a: np.ndarray) -> C.c_void_p:
    return a.ctypes.data_as(C.c_void_p)


def is_wide(dtype) -> bool:
    """long double / std::complex<long double>: crosses the C ABI as double-double pairs."""
    return np.dtype(dtype) in (np.dtype(np.longdouble), np.dtype(np.clongdouble))


def to_wire(a, dtype) -> np.ndarray:
    """Host scalars of ``dtype`` in the C ABI's layout (a contiguous buffer, flattened in C order).
    long double values become double-double pairs {hi = (double) v, lo = (double)(v - hi)}.  Exact
    for the x87 format (64-bit significand: 53 bits in hi, 11 in lo) while lo is a normal double,
    i.e. |v| >= ~2^-1010 (1e-304); below that lo falls under the subnormal grid, the pair is the nearest double-double and a
    RuntimeWarning says so.  A long double with another significand (IEEE binary128 on aarch64)
    is refused: its values do not fit {hi, lo}."""
    a = np.ascontiguousarray(a, dtype=dtype)
    if not is_wide(dtype):
        return a
    if np.finfo(np.longdouble).nmant != 63:
        raise EigSolError(EIGSOL_E_UNSUPPORTED, "long double is not the x87 80-bit format on this platform; "
                                                "the double-double wire format cannot carry it exactly")
    flat = a.reshape(-1)
    parts = [flat.real, flat.imag] if np.iscomplexobj(flat) else [flat]
    cols = []
    for p in parts:
        with np.errstate(over="ignore"):
            hi = p.astype(np.float64)
        if np.any(np.isinf(hi) & np.isfinite(p)):
            raise EigSolError(EIGSOL_E_INVALID, "long double value outside the double exponent range "
                                                "(double-double carries |v| < 1.8e308)")
        fin = np.isfinite(p)
        with np.errstate(invalid="ignore"):
            lo = np.where(fin, (p - hi.astype(np.longdouble)), 0).astype(np.float64)   # inf / NaN: lo = 0
        if np.any(fin & (hi.astype(np.longdouble) + lo.astype(np.longdouble) != p)):
            import warnings
            warnings.warn("long double values below ~2^-1010 (1e-304) lose low bits in the double-double wire format "
                          "(the low part falls under the subnormal grid)", RuntimeWarning, stacklevel=2)
        cols += [hi, lo]
    return np.ascontiguousarray(np.stack(cols, axis=-1))


def wire_buffer(dtype, n: int) -> np.ndarray:
    """Output buffer for n scalars of ``dtype`` in the C ABI's layout."""
    if not is_wide(dtype):
        return np.empty(max(n, 0), dtype=dtype)
    return np.zeros((max(n, 0), 4 if np.dtype(dtype) == np.clongdouble else 2), dtype=np.float64)


def from_wire(w: np.ndarray, dtype) -> np.ndarray:
    """Inverse of to_wire (double-double hi + lo rounded to the nearest long double)."""
    if not is_wide(dtype):
        return w
    w = np.asarray(w, dtype=np.float64).reshape(-1, 4 if np.dtype(dtype) == np.clongdouble else 2)
    re = w[:, 0].astype(np.longdouble) + w[:, 1].astype(np.longdouble)
    if np.dtype(dtype) == np.longdouble:
        return re
    z = np.empty(len(w), dtype=np.clongdouble)
    z.real = re
    z.imag = w[:, 2].astype(np.longdouble) + w[:, 3].astype(np.longdouble)
    return z


def _scalar(v, dtype):
    """eigenvalue as a Python / numpy scalar (long double kept at its precision)."""
    if is_wide(dtype):
        return v
    return complex(v) if np.iscomplexobj(v) else float(v)


def _vector(v, dtype, n: int, what: str) -> np.ndarray:
    """Host vector of exactly n entries (the C ABI copies n scalars from the pointer)."""
    v = np.ascontiguousarray(v, dtype=dtype).reshape(-1)
    if len(v) != n:
        raise EigSolError(EIGSOL_E_SIZE_MISMATCH, f"{what} has {len(v)} entries, the matrix has {n} rows")
    return to_wire(v, dtype)


def device_count() -> int:
    n = C.c_int(0)
    st = lib().eigsol_device_count(C.byref(n))
    return int(n.value) if st == 0 else 0


class Context:
    """One gfx950 device + one stream (``eigsol_ctx``)."""

    def __init__(self, device: int = 0, stream: Optional[int] = None):
        h = C.c_void_p()
        call("eigsol_ctx_create", int(device), C.byref(h))
        self.handle = h
        self.device = device
        if stream is not None:
            self.set_stream(stream)

    def set_stream(self, stream_ptr: Optional[int]) -> None:
        call("eigsol_ctx_set_stream", self.handle, C.c_void_p(stream_ptr or 0))

    def synchronize(self) -> None:
        call("eigsol_ctx_synchronize", self.handle)

    def malloc(self, nbytes: int) -> int:
        p = C.c_void_p()
        call("eigsol_malloc", self.handle, C.c_size_t(nbytes), C.byref(p))
        return int(p.value or 0)

    def free(self, ptr: int) -> None:
        call("eigsol_free", self.handle, C.c_void_p(ptr))

    def h2d(self, dptr: int, host: np.ndarray) -> None:
        host = np.ascontiguousarray(host)
        call("eigsol_memcpy_h2d", self.handle, C.c_void_p(dptr), _ptr(host), C.c_size_t(host.nbytes))

    def d2h(self, host: np.ndarray, dptr: int) -> np.ndarray:
        call("eigsol_memcpy_d2h", self.handle, _ptr(host), C.c_void_p(dptr), C.c_size_t(host.nbytes))
        return host

    def close(self) -> None:
        if getattr(self, "handle", None):
            lib().eigsol_ctx_destroy(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class CsrMatrix:
    """Device-resident CSR matrix (``eigsol_csr``)."""

    def __init__(self, ctx: Context, rowptr, colidx, values, shape, layout: str = "csr"):
        values = np.ascontiguousarray(values)
        code = _dtype_code(values.dtype)
        ptr = np.ascontiguousarray(rowptr, dtype=np.int32)
        idx = np.ascontiguousarray(colidx, dtype=np.int32)
        nrows, ncols = int(shape[0]), int(shape[1])
        nouter = nrows if layout == "csr" else ncols
        if len(ptr) != nouter + 1:
            raise EigSolError(EIGSOL_E_SIZE_MISMATCH,
                              f"{layout} pointer array has {len(ptr)} entries, expected {nouter + 1}")
        if len(values) != len(idx):
            raise EigSolError(EIGSOL_E_SIZE_MISMATCH,
                              f"values ({len(values)}) and index array ({len(idx)}) lengths differ")
        h = C.c_void_p()
        fn = "eigsol_csr_create" if layout == "csr" else "eigsol_csr_create_from_csc"
        vw = to_wire(values, values.dtype)
        call(fn, ctx.handle, code, nrows, ncols, len(idx), _ptr(ptr), _ptr(idx), _ptr(vw), C.byref(h))
        self.ctx, self.handle = ctx, h
        self.shape = (nrows, ncols)
        self.nnz = len(idx)
        self.dtype = _np_dtype(code)

    @classmethod
    def from_scipy(cls, ctx: Context, M):
        import scipy.sparse as sp
        if sp.isspmatrix_csc(M) or isinstance(M, sp.csc_array):
            M = M.copy()
            M.sort_indices()
            return cls(ctx, M.indptr, M.indices, M.data, M.shape, layout="csc")
        M = sp.csr_matrix(M)
        M.sort_indices()
        return cls(ctx, M.indptr, M.indices, M.data, M.shape)

    @classmethod
    def from_coo(cls, ctx: Context, rows, cols, values, shape):
        """Triplets in any order straight to the device CSR (``eigsol_csr_create_from_coo``):
        repeated positions are summed in input order, as the reader's Matrix::Sparse does."""
        values = np.ascontiguousarray(values)
        code = _dtype_code(values.dtype)
        r = np.ascontiguousarray(rows, dtype=np.int32)
        c = np.ascontiguousarray(cols, dtype=np.int32)
        if not (len(r) == len(c) == len(values)):
            raise EigSolError(EIGSOL_E_SIZE_MISMATCH,
                              f"triplet arrays differ in length ({len(r)}, {len(c)}, {len(values)})")
        h = C.c_void_p()
        vw = to_wire(values, values.dtype)
        call("eigsol_csr_create_from_coo", ctx.handle, code, int(shape[0]), int(shape[1]), len(r), _ptr(r),
             _ptr(c), _ptr(vw), C.byref(h))
        self = cls.__new__(cls)
        self.ctx, self.handle = ctx, h
        self.shape = (int(shape[0]), int(shape[1]))
        nnz = C.c_int64()
        call("eigsol_csr_info", h, None, None, C.byref(nnz), None)
        self.nnz = nnz.value
        self.dtype = _np_dtype(code)
        return self

    def download(self):
        """(rowptr, colidx, values) of the device CSR (``eigsol_csr_download``)."""
        rp = np.empty(self.shape[0] + 1, np.int32)
        ci = np.empty(self.nnz, np.int32)
        v = wire_buffer(self.dtype, self.nnz)
        call("eigsol_csr_download", self.handle, _ptr(rp), _ptr(ci), _ptr(v))
        return rp, ci, from_wire(v, self.dtype)

    def adjoint(self) -> "CsrMatrix":
        """A new device matrix holding A^H (``eigsol_csr_adjoint``): ncols x nrows, values conjugated, uploaded
        like any matrix, so its ``spmv`` is the product with A^H.  The caller closes it."""
        h = C.c_void_p()
        call("eigsol_csr_adjoint", self.handle, C.byref(h))
        out = CsrMatrix.__new__(CsrMatrix)
        out.ctx, out.handle = self.ctx, h
        out.shape = (self.shape[1], self.shape[0])
        out.nnz = self.nnz
        out.dtype = self.dtype
        return out

    def spmv(self, x_dev: int, y_dev: int) -> None:
        call("eigsol_csr_spmv", self.handle, C.c_void_p(x_dev), C.c_void_p(y_dev))

    def spmm(self, x_dev: int, y_dev: int, m: int) -> None:
        """Y = A X on row-major interleaved device blocks (X: ncols x m, Y: nrows x m)."""
        call("eigsol_csr_spmm", self.handle, int(m), C.c_void_p(x_dev), C.c_void_p(y_dev))

    def close(self) -> None:
        if getattr(self, "handle", None):
            lib().eigsol_csr_destroy(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class DenseMatrix:
    """Device-resident column-major dense matrix (``eigsol_dense``; ``Matrix::Dense<S>``)."""

    def __init__(self, ctx: Context, A: np.ndarray):
        A = np.asarray(A)
        code = _dtype_code(A.dtype)
        Af = to_wire(np.asfortranarray(A).ravel(order="F"), A.dtype)   # column-major
        h = C.c_void_p()
        call("eigsol_dense_create", ctx.handle, code, A.shape[0], A.shape[1], _ptr(Af), C.byref(h))
        self.ctx, self.handle = ctx, h
        self.shape = A.shape
        self.dtype = _np_dtype(code)

    def gemv(self, x_dev: int, y_dev: int) -> None:
        call("eigsol_dense_gemv", self.handle, C.c_void_p(x_dev), C.c_void_p(y_dev))

    def gemv_h(self, x_dev: int, y_dev: int) -> None:
        """y = A^H x on device vectors (x: nrows scalars, y: ncols scalars)."""
        call("eigsol_dense_gemv_h", self.handle, C.c_void_p(x_dev), C.c_void_p(y_dev))

    def gemm(self, x_dev: int, y_dev: int, m: int) -> None:
        """Y = A X on row-major interleaved device blocks (X: ncols x m, Y: nrows x m)."""
        call("eigsol_dense_gemm", self.handle, int(m), C.c_void_p(x_dev), C.c_void_p(y_dev))

    def close(self) -> None:
        if getattr(self, "handle", None):
            lib().eigsol_dense_destroy(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class PowerSession:
    """Device-resident power iteration (``eigsol_power``): begin / step / query / finish."""

    def __init__(self, matrix, trace_capacity: int = 0):
        h = C.c_void_p()
        if isinstance(matrix, CsrMatrix):
            call("eigsol_power_create_csr", matrix.handle, int(trace_capacity), C.byref(h))
        else:
            call("eigsol_power_create_dense", matrix.handle, int(trace_capacity), C.byref(h))
        self.matrix, self.handle = matrix, h
        self.n = matrix.shape[0]
        self.dtype = matrix.dtype

    def begin(self, opts: SolverOptions, x0=None, x0_dev: Optional[int] = None) -> None:
        o = opts.to_c()
        if x0_dev is not None:
            call("eigsol_power_begin", self.handle, C.byref(o), C.c_void_p(x0_dev), 1)
        else:
            x = _vector(x0, self.dtype, self.n, "x0")
            self._x0 = x
            call("eigsol_power_begin", self.handle, C.byref(o), _ptr(x), 0)

    def step(self, n: int) -> None:
        call("eigsol_power_step", self.handle, int(n))

    def query(self):
        done, launches = C.c_int32(0), C.c_int32(0)
        call("eigsol_power_query", self.handle, C.byref(done), C.byref(launches))
        return bool(done.value), int(launches.value)

    def finish(self, want_vector: bool = True) -> EigenResult:
        lam = wire_buffer(self.dtype, 1)
        x = wire_buffer(self.dtype, self.n) if want_vector else None
        it, conv = C.c_int32(0), C.c_int32(0)
        call("eigsol_power_finish", self.handle, _ptr(lam), None if x is None else _ptr(x), 0,
             C.byref(it), C.byref(conv))
        ev = _scalar(from_wire(lam, self.dtype)[0], self.dtype)
        return EigenResult(ev, None if x is None else from_wire(x, self.dtype), int(it.value), bool(conv.value))

    def trace(self, capacity: int) -> np.ndarray:
        buf = wire_buffer(self.dtype, max(capacity, 1))
        cnt = C.c_int32(0)
        call("eigsol_power_trace", self.handle, _ptr(buf), int(capacity), C.byref(cnt))
        return from_wire(buf, self.dtype)[: cnt.value]

    def transport(self) -> int:
        """EIGSOL_TRANSPORT_LOCAL / _COLLECTIVE / _PEER (per-iteration exchange of this session)."""
        t = C.c_int(0)
        call("eigsol_power_transport", self.handle, C.byref(t))
        return t.value

    def kernel_info(self):
        b, g, t, v = C.c_double(0), C.c_int32(0), C.c_int32(0), C.c_int32(0)
        call("eigsol_power_kernel_info", self.handle, C.byref(b), C.byref(g), C.byref(t), C.byref(v))
        names = {0: "csr_kernel (x gathered from HBM)", 1: "csr_win_kernel (x window staged in LDS)",
                 2: "dense_kernel (GEMV)", 3: "sptrsv_kernel (sync-free triangular solve)",
                 4: "dense LU substitution (dense_lu_solve_kernel on one CU up to n = 64, else "
                    "dense_trsv2_kernel: 64-row block rows, inverted diagonal blocks, value flags)",
                 5: "csr_slice_kernel (64-row slices, one row per lane)",
                 6: "csr_row_kernel (one row per lane, single-precision fallback layout)",
                 7: "ILU(0)-preconditioned GMRES (tiles = Arnoldi steps of the last solve)",
                 8: "band_solve_kernel (RCM-banded LU; tiles = kl + ku)",
                 9: "csr_kernel column-block passes (x blocks L2-resident; tiles = blocks)",
                 10: "csr_bin_kernel (column-binned row chunks, row sums in LDS; tiles = chunks)",
                 11: "csr_bin_kernel in two row halves per iteration, the first half's all-gather "
                     "overlapped with the second half (row-sharded; tiles = chunks)",
                 12: "sptrsv multi-solve kernel (sync-free triangular solves, 2 iterations per launch, "
                     "solve j one dependency round behind solve j-1)",
                 13: "sptrsv multi-solve kernel (sync-free triangular solves, 3 iterations per launch, "
                     "solve j one dependency round behind solve j-1)",
                 14: "sptrsv multi-solve kernel (sync-free triangular solves, 4 iterations per launch, "
                     "solve j one dependency round behind solve j-1)",
                 15: "wide power_fused2_kernel (double-double: x = y / normY, A x and the norm / Rayleigh partials in one pass; a tile's row sums by 2-32 lanes per row into LDS, then one row's epilogue per thread)",
                 16: "wide gemv kernels (double-double dense product)",
                 17: "wide shifted inverse (fp64 factor + double-double residual refinement; "
                     "tiles = refinement steps of the last solve)",
                 18: "GMRES over the exact sparse LU (complete fill, no pivoting; tiles = Arnoldi "
                     "steps of the last solve)",
                 19: "GMRES over the nested-dissection multifrontal LU (dense fronts, pivoting inside each "
                     "front; tiles = Arnoldi steps of the last solve)",
                 20: "dense LU substitution by triangles (dense_trsv_kernel: 64-row block rows, 64-step "
                     "triangles, epoch flags; chosen for a factor whose diagonal blocks are too ill "
                     "conditioned for products with their inverses, or by EIGSOL_DENSE_TRSV=1)"}
        ipp = C.c_int32(1)
        call("eigsol_power_iterations_per_pass", self.handle, C.byref(ipp))
        return {"bytes_per_iteration": b.value, "grid": g.value, "tiles": t.value,
                "variant": v.value, "kernel": names.get(v.value, "?"),
                "iterations_per_launch": v.value - 10 if 12 <= v.value <= 14 else 1,
                "iterations_per_pass": ipp.value}

    def kernel_name(self) -> str:
        """Demangled name of the per-iteration kernel (CSR power sessions), as rocprofv3 reports it."""
        buf = C.create_string_buffer(512)
        call("eigsol_power_kernel_name", self.handle, buf, 512)
        return buf.value.decode()

    def close(self) -> None:
        if getattr(self, "handle", None):
            lib().eigsol_power_destroy(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def power_method(matrix, opts: SolverOptions = SolverOptions(), x0=None) -> EigenResult:
    """``EigSol::powerMethod<S>`` on a device-resident matrix, with an explicit start vector."""
    if x0 is None:
        rng = np.random.default_rng(0)
        x0 = rng.uniform(-1, 1, matrix.shape[0])
        if np.issubdtype(matrix.dtype, np.complexfloating):
            x0 = x0 + 1j * rng.uniform(-1, 1, matrix.shape[0])
    x0 = _vector(x0, matrix.dtype, matrix.shape[0], "x0")
    lam = wire_buffer(matrix.dtype, 1)
    x = wire_buffer(matrix.dtype, matrix.shape[0])
    it, conv = C.c_int32(0), C.c_int32(0)
    o = opts.to_c()
    fn = "eigsol_power_csr" if isinstance(matrix, CsrMatrix) else "eigsol_power_dense"
    call(fn, matrix.handle, C.byref(o), _ptr(x0), _ptr(lam), _ptr(x), C.byref(it), C.byref(conv))
    ev = _scalar(from_wire(lam, matrix.dtype)[0], matrix.dtype)
    return EigenResult(ev, from_wire(x, matrix.dtype), int(it.value), bool(conv.value))


# ------------------------------------------------------------------------ block subspace iteration
def spmm(matrix: CsrMatrix, X) -> np.ndarray:
    """``A @ X`` for a host block X (ncols x m, 1 <= m <= 32) through ``eigsol_csr_spmm``: column j of
    the result is bitwise ``CsrMatrix.spmv`` of column j."""
    X = np.asarray(X)
    nrows, ncols = matrix.shape
    if X.ndim != 2 or X.shape[0] != ncols:
        raise EigSolError(EIGSOL_E_SIZE_MISMATCH, f"X has shape {X.shape}, the matrix has {ncols} columns")
    m = X.shape[1]
    return _block_product(matrix, X, matrix.spmm)


def dense_mm(matrix: DenseMatrix, X) -> np.ndarray:
    """``A @ X`` for a host block X (ncols x m, 1 <= m <= 32) through ``eigsol_dense_gemm`` (the fp64
    matrix cores; double and complex double matrices)."""
    X = np.asarray(X)
    if X.ndim != 2 or X.shape[0] != matrix.shape[1]:
        raise EigSolError(EIGSOL_E_SIZE_MISMATCH, f"X has shape {X.shape}, the matrix has {matrix.shape[1]} columns")
    if is_wide(matrix.dtype):
        raise EigSolError(EIGSOL_E_UNSUPPORTED, "dense_mm: long double matrices are not supported")
    return _block_product(matrix, X, matrix.gemm)


def _block_product(matrix, X, product) -> np.ndarray:
    nrows, m = matrix.shape[0], X.shape[1]
    Xr = np.ascontiguousarray(X, dtype=matrix.dtype)      # row-major = interleaved
    Y = np.empty((nrows, m), dtype=matrix.dtype)
    ctx = matrix.ctx
    dx, dy = ctx.malloc(max(Xr.nbytes, 16)), ctx.malloc(max(Y.nbytes, 16))
    try:
        if Xr.nbytes:
            ctx.h2d(dx, Xr)
        product(dx, dy, m)
        if Y.nbytes:
            ctx.d2h(Y, dy)
    finally:
        ctx.free(dx)
        ctx.free(dy)
    return Y


@dataclass
class SubspaceOptions:
    """Options of :func:`subspace_iteration` (``eigsol_subspace_options`` without nev / block)."""

    max_iterations: int = 1000
    tolerance: float = 1e-10          # < 0: never converges
    residual_tolerance: float = 0.0   # 0: the eigenvalue test alone decides


@dataclass
class SubspaceResult:
    eigenvalues: np.ndarray    # k complex, |.| descending, a conjugate pair +imag first
    eigenvectors: np.ndarray   # n x k complex, unit columns
    residuals: np.ndarray      # k: ||A x - theta x||_2
    iterations: int            # products Z = A Q
    converged: bool


def subspace_iteration(matrix, nev: int, opts: SubspaceOptions = SubspaceOptions(), block: Optional[int] = None,
                       X0=None, seed: int = 0) -> SubspaceResult:
    """The ``nev`` eigenpairs of largest modulus of a device-resident CSR or dense matrix by block
    subspace iteration with Rayleigh-Ritz (``eigsol_subspace_csr`` / ``eigsol_subspace_dense``).  ``block`` (default min(n, 32, 2 nev))
    vectors are iterated; ``X0`` (n x block) defaults to uniform(-1, 1) entries from
    ``numpy.random.default_rng(seed)``.  A cut between nev and nev + 1 through eigenvalues of equal
    modulus (a conjugate pair split by nev = block) may end with ``converged`` false."""
    n = matrix.shape[0]
    nev = int(nev)
    m = min(n, 32, 2 * nev) if block is None else int(block)
    if X0 is None:
        rng = np.random.default_rng(seed)
        X0 = rng.uniform(-1, 1, (n, max(m, 0)))
        if np.issubdtype(matrix.dtype, np.complexfloating):
            X0 = X0 + 1j * rng.uniform(-1, 1, (n, max(m, 0)))
    X0 = np.asarray(X0)
    if X0.ndim != 2 or X0.shape != (n, m):
        raise EigSolError(EIGSOL_E_SIZE_MISMATCH, f"X0 has shape {X0.shape}, expected ({n}, {m})")
    if is_wide(matrix.dtype):
        raise EigSolError(EIGSOL_E_UNSUPPORTED, "subspace_iteration: long double matrices are not supported")
    Xf = np.asfortranarray(X0, dtype=matrix.dtype)         # column-major n x m
    k = max(nev, 0)
    ev = np.zeros(max(k, 1), dtype=np.complex128)
    vec = np.zeros((n, k), dtype=np.complex128, order="F")
    res = np.zeros(max(k, 1))
    it, conv = C.c_int32(0), C.c_int32(0)
    o = SubspaceOptionsC(int(opts.max_iterations), float(opts.tolerance), float(opts.residual_tolerance), nev, m)
    pd = C.POINTER(C.c_double)
    fn = "eigsol_subspace_dense" if isinstance(matrix, DenseMatrix) else "eigsol_subspace_csr"
    call(fn, matrix.handle, C.byref(o), _ptr(Xf), ev.ctypes.data_as(pd),
         vec.ctypes.data_as(pd) if vec.size else None, res.ctypes.data_as(pd), C.byref(it), C.byref(conv))
    return SubspaceResult(ev[:k], vec, res[:k], int(it.value), bool(conv.value))


# ------------------------------------------------------------------------------------ Krylov-Schur
@dataclass
class KrylovOptions:
    """Options of :func:`krylov_schur` (``eigsol_krylov_options`` without nev / ncv / mode)."""

    max_restarts: int = 300
    tolerance: float = 1e-10          # < 0: never converges


@dataclass
class KrylovResult:
    eigenvalues: np.ndarray    # k complex: largest modulus first, or nearest sigma first
    eigenvectors: np.ndarray   # n x k complex, unit columns
    residuals: np.ndarray      # k: ||A x - lambda x||_2
    restarts: int              # restart cycles run
    applications: int          # products A v, or solves with A - sigma I
    converged: bool


def default_ncv(n: int, nev: int) -> int:
    return min(n, 64, max(2 * nev + 1, 20))


def krylov_schur(matrix, nev: int, opts: KrylovOptions = KrylovOptions(), sigma=None, ncv: Optional[int] = None,
                 v0=None, seed: int = 0) -> KrylovResult:
    """``nev`` eigenpairs of a device-resident CSR or dense matrix by the Krylov-Schur method
    (``eigsol_krylov_csr`` / ``eigsol_krylov_dense``): those of largest modulus (``sigma is None``), or those nearest ``sigma``
    through one factorisation of A - sigma I.  ``ncv`` basis vectors (default
    min(n, 64, max(2 nev + 1, 20))); ``v0`` defaults to uniform(-1, 1) entries from
    ``numpy.random.default_rng(seed)`` (complex for complex matrices)."""
    n = matrix.shape[0]
    nev = int(nev)
    m = default_ncv(n, nev) if ncv is None else int(ncv)
    if v0 is None:
        rng = np.random.default_rng(seed)
        v0 = rng.uniform(-1, 1, n)
        if np.issubdtype(matrix.dtype, np.complexfloating):
            v0 = v0 + 1j * rng.uniform(-1, 1, n)
    if is_wide(matrix.dtype):
        raise EigSolError(EIGSOL_E_UNSUPPORTED, "krylov_schur: long double matrices are not supported")
    v0 = _vector(v0, matrix.dtype, n, "v0")
    k = max(nev, 0)
    ev = np.zeros(max(k, 1), dtype=np.complex128)
    vec = np.zeros((n, k), dtype=np.complex128, order="F")
    res = np.zeros(max(k, 1))
    rs, ap, conv = C.c_int32(0), C.c_int32(0), C.c_int32(0)
    o = KrylovOptionsC(int(opts.max_restarts), float(opts.tolerance), nev, m,
                       EIGSOL_KRYLOV_LM if sigma is None else EIGSOL_KRYLOV_SHIFT_INVERT)
    sg = None if sigma is None else _sigma(sigma, matrix.dtype)
    pd = C.POINTER(C.c_double)
    fn = "eigsol_krylov_dense" if isinstance(matrix, DenseMatrix) else "eigsol_krylov_csr"
    call(fn, matrix.handle, C.byref(o), None if sg is None else _ptr(sg), _ptr(v0),
         ev.ctypes.data_as(pd), vec.ctypes.data_as(pd) if vec.size else None, res.ctypes.data_as(pd), C.byref(rs),
         C.byref(ap), C.byref(conv))
    return KrylovResult(ev[:k], vec, res[:k], int(rs.value), int(ap.value), bool(conv.value))


def krylov_orth(ctx: Context, V, w):
    """One orthogonalisation step of the Krylov-Schur solver (``eigsol_krylov_orth``) on host arrays:
    w (n) against the orthonormal columns of V (n x j), two Gram-Schmidt passes, then normalised.
    Returns (w_out, h, beta, wnorm)."""
    V = np.asfortranarray(V)
    if V.ndim != 2 or np.shape(w) != (V.shape[0],):
        raise EigSolError(EIGSOL_E_SIZE_MISMATCH, f"V has shape {V.shape}, w has shape {np.shape(w)}")
    n, j = V.shape
    w = np.ascontiguousarray(w, dtype=V.dtype)
    code = _dtype_code(V.dtype)
    h = np.zeros(max(j, 1), dtype=np.complex128)
    beta, wn = C.c_double(0), C.c_double(0)
    dv, dw = ctx.malloc(max(V.nbytes, 16)), ctx.malloc(max(w.nbytes, 16))
    try:
        ctx.h2d(dv, V.ravel(order="F"))                     # column-major, ld = n
        ctx.h2d(dw, w)
        call("eigsol_krylov_orth", ctx.handle, code, n, j, C.c_void_p(dv), n, C.c_void_p(dw),
             h.ctypes.data_as(C.POINTER(C.c_double)), C.byref(beta), C.byref(wn))
        out = ctx.d2h(np.empty(n, dtype=V.dtype), dw)
    finally:
        ctx.free(dv)
        ctx.free(dw)
    return out, (h[:j] if np.iscomplexobj(V) else h[:j].real.copy()), beta.value, wn.value


def krylov_rotate(ctx: Context, V, Q) -> np.ndarray:
    """``V[:, :p] <- V[:, :m] Q`` in place on the device (``eigsol_krylov_rotate``) for host arrays
    V (n x m) and Q (m x p); returns the n x m result (columns p .. m-1 unchanged)."""
    V = np.asfortranarray(V)
    Q = np.asfortranarray(Q, dtype=V.dtype)
    if V.ndim != 2 or Q.ndim != 2 or Q.shape[0] != V.shape[1]:
        raise EigSolError(EIGSOL_E_SIZE_MISMATCH, f"V has shape {V.shape}, Q has shape {Q.shape}")
    n, m = V.shape
    dv = ctx.malloc(max(V.nbytes, 16))
    try:
        ctx.h2d(dv, V.ravel(order="F"))                     # column-major, ld = n
        call("eigsol_krylov_rotate", ctx.handle, _dtype_code(V.dtype), n, m, Q.shape[1], C.c_void_p(dv), n, _ptr(Q))
        out = ctx.d2h(np.empty(n * m, dtype=V.dtype), dv).reshape((n, m), order="F")
    finally:
        ctx.free(dv)
    return out


@dataclass
class ShiftedSolverOptions(SolverOptions):
    """``EigSol::ShiftedSolverOptions<S>`` (src/option/shifted_solver_option.hpp:24-68)."""

    shift: complex | float = 0.0


def _sigma(shift, dtype) -> np.ndarray:
    if not np.issubdtype(dtype, np.complexfloating) and np.iscomplexobj(shift) and complex(shift).imag != 0:
        raise EigSolError(3, "scalar type mismatch: complex shift for a real matrix")
    return to_wire(np.array([shift], dtype=dtype), dtype)


class ShiftedSession(PowerSession):
    """Shifted inverse iteration session: A - sigma I factored once on the device
    (``eigsol_shifted_create_*``); driven with the PowerSession methods."""

    def __init__(self, matrix, shift, trace_capacity: int = 0):
        h = C.c_void_p()
        sig = _sigma(shift, matrix.dtype)
        fn = "eigsol_shifted_create_csr" if isinstance(matrix, CsrMatrix) else "eigsol_shifted_create_dense"
        call(fn, matrix.handle, _ptr(sig), int(trace_capacity), C.byref(h))
        self.matrix, self.handle = matrix, h
        self.n = matrix.shape[0]
        self.dtype = matrix.dtype
        self.shift = from_wire(sig, matrix.dtype)[0]


def shifted_inverse_power_method(matrix, opts: ShiftedSolverOptions = ShiftedSolverOptions(),
                                  x0=None) -> EigenResult:
    """``EigSol::shiftedInversePowerMethod<S>`` with an explicit start vector."""
    if x0 is None:
        rng = np.random.default_rng(0)
        x0 = rng.uniform(-1, 1, matrix.shape[0])
        if np.issubdtype(matrix.dtype, np.complexfloating):
            x0 = x0 + 1j * rng.uniform(-1, 1, matrix.shape[0])
    x0 = _vector(x0, matrix.dtype, matrix.shape[0], "x0")
    sig = _sigma(opts.shift, matrix.dtype)
    lam = wire_buffer(matrix.dtype, 1)
    x = wire_buffer(matrix.dtype, matrix.shape[0])
    it, conv = C.c_int32(0), C.c_int32(0)
    o = opts.to_c()
    fn = "eigsol_shifted_inverse_csr" if isinstance(matrix, CsrMatrix) else "eigsol_shifted_inverse_dense"
    call(fn, matrix.handle, _ptr(sig), C.byref(o), _ptr(x0), _ptr(lam), _ptr(x), C.byref(it), C.byref(conv))
    ev = _scalar(from_wire(lam, matrix.dtype)[0], matrix.dtype)
    return EigenResult(ev, from_wire(x, matrix.dtype), int(it.value), bool(conv.value))


def solve_shifted(matrix, shift, b) -> np.ndarray:
    """``EigSol::solve_shifted<S>``: x = (A - shift I)^{-1} b on the device."""
    b = np.ascontiguousarray(b, dtype=matrix.dtype).reshape(-1)
    nb = len(b)
    sig = _sigma(shift, matrix.dtype)
    x = wire_buffer(matrix.dtype, nb)
    bw = to_wire(b, matrix.dtype)
    fn = "eigsol_solve_shifted_csr" if isinstance(matrix, CsrMatrix) else "eigsol_solve_shifted_dense"
    call(fn, matrix.handle, _ptr(sig), _ptr(bw), nb, _ptr(x))
    return from_wire(x, matrix.dtype)


# ------------------------------------------------------------------------------------ QR method
@dataclass
class QRResult:
    """``EigSol::QRResult<S>`` (src/result/qr_result.hpp:25-43).  For the Francis variant on a
    real matrix, ``eigenvalues`` holds the real parts (the diagonal of the standardised real Schur
    form) and ``eigenvalues_complex`` the full complex eigenvalues.  ``unrefined`` (long double
    Francis only, else 0) counts the eigenvalues the double-double refinement did not bring to its
    floor (``eigsol_qr_refine_info``): those are fp64-grade, whatever ``converged`` says."""

    eigenvalues: np.ndarray
    iterations: int
    converged: bool
    eigenvalues_complex: Optional[np.ndarray] = None
    unrefined: int = 0


def _square_dense(A, who: str) -> np.ndarray:
    A = np.asarray(A)
    if A.ndim != 2 or A.shape[0] != A.shape[1]:
        raise EigSolError(1, f"{who}: A must be square")
    return A


def to_hessenberg(ctx: Context, A) -> np.ndarray:
    """``EigSol::to_hessenberg_dense<S>`` (to_hessenberg.hpp:23-80) on the device."""
    A = _square_dense(A, "to_hessenberg_dense")
    code = _dtype_code(A.dtype)
    n = A.shape[0]
    if is_wide(A.dtype):
        Hw = wire_buffer(A.dtype, n * n)
        call("eigsol_hessenberg_dense", ctx.handle, code, n, _ptr(to_wire(A.ravel(order="F"), A.dtype)), _ptr(Hw))
        return from_wire(Hw, A.dtype).reshape((n, n), order="F")
    Af = np.asfortranarray(A)
    H = np.empty_like(Af, order="F")
    call("eigsol_hessenberg_dense", ctx.handle, code, n, _ptr(Af), _ptr(H))
    return H


def qr_decompose(ctx: Context, A):
    """``EigSol::qr_decompose_dense<S>`` (qr_decompose.hpp:25-86): returns (Q, R)."""
    A = np.asarray(A)
    code = _dtype_code(A.dtype)
    m, n = A.shape
    if is_wide(A.dtype):
        Qw, Rw = wire_buffer(A.dtype, m * m), wire_buffer(A.dtype, m * n)
        call("eigsol_qr_decompose_dense", ctx.handle, code, m, n, _ptr(to_wire(A.ravel(order="F"), A.dtype)),
             _ptr(Qw), _ptr(Rw))
        return (from_wire(Qw, A.dtype).reshape((m, m), order="F"), from_wire(Rw, A.dtype).reshape((m, n), order="F"))
    Af = np.asfortranarray(A)
    Q = np.empty((m, m), dtype=A.dtype, order="F")
    R = np.empty((m, n), dtype=A.dtype, order="F")
    call("eigsol_qr_decompose_dense", ctx.handle, code, m, n, _ptr(Af), _ptr(Q), _ptr(R))
    return Q, R


def qr_eigenvalues(ctx: Context, A, opts: SolverOptions = SolverOptions(), variant: str = "francis") -> QRResult:
    """``EigSol::qr_eigenvalues<S>``.  variant "unshifted" = the reference algorithm
    (qr_eigenvalues.hpp:40-108); "francis" = implicit multishift sweeps (real: double-shift
    bulges, francis.hip; complex: complex two-shift bulges, zfrancis.hip)."""
    A = _square_dense(A, "qr_eigenvalues_dense")
    code = _dtype_code(A.dtype)
    n = A.shape[0]
    v = 1 if variant == "unshifted" else 0
    if is_wide(A.dtype):
        # long double: "unshifted" = the reference's iteration in double-double; "francis" = the fp64
        # multishift sweeps on the rounded double-double Hessenberg matrix, every eigenvalue then
        # refined in double-double by Newton's method on det(H - mu I) (wide.hip)
        eig = wire_buffer(A.dtype, max(n, 1))
        eim = np.zeros((max(n, 1), 2)) if (v == 0 and A.dtype == np.longdouble) else None
        it, conv = C.c_int32(0), C.c_int32(0)
        o = opts.to_c()
        call("eigsol_qr_eigenvalues_dense", ctx.handle, code, n, _ptr(to_wire(A.ravel(order="F"), A.dtype)),
             C.byref(o), v, _ptr(eig), None if eim is None else _ptr(eim), C.byref(it), C.byref(conv))
        ev = from_wire(eig, A.dtype)[:n]
        full = None
        if v == 0:
            full = ev.astype(np.clongdouble)
            if eim is not None:
                full = full + np.clongdouble(1j) * from_wire(eim, np.longdouble)[:n]
        unref = C.c_int64(0)
        if v == 0 and n:
            call("eigsol_qr_refine_info", ctx.handle, C.byref(unref), None)
        return QRResult(ev, int(it.value), bool(conv.value), full, int(unref.value))
    if v == 0 and A.dtype in (np.float32, np.complex64):
        # single precision: the multishift sweeps are double kernels (as in the C++ facade, the
        # matrix is promoted and the eigenvalues rounded back); "unshifted" runs natively in float
        wide = np.float64 if A.dtype == np.float32 else np.complex128
        r = qr_eigenvalues(ctx, A.astype(wide), opts, variant)
        return QRResult(r.eigenvalues.astype(A.dtype), r.iterations, r.converged,
                        None if r.eigenvalues_complex is None else r.eigenvalues_complex.astype(np.complex64))
    Af = np.asfortranarray(A)
    eig = np.zeros(max(n, 1), dtype=A.dtype)
    wi = np.zeros(max(n, 1))
    it, conv = C.c_int32(0), C.c_int32(0)
    o = opts.to_c()
    call("eigsol_qr_eigenvalues_dense", ctx.handle, code, n, _ptr(Af), C.byref(o), v, _ptr(eig),
         _ptr(wi), C.byref(it), C.byref(conv))
    eig = eig[:n]
    full = None
    if v == 0 and A.dtype == np.float64:
        full = eig + 1j * wi[:n]
    elif v == 0 and A.dtype == np.complex128:
        full = eig.copy()
    return QRResult(eig, int(it.value), bool(conv.value), full)


@dataclass
class EighResult:
    """Result of :func:`eigh`: ``eigenvalues`` ascending (m), ``eigenvectors`` n x m with unit columns
    (column j belongs to eigenvalue j; its largest-modulus component is real and positive),
    ``not_converged`` the number of vectors that failed the inverse iteration's growth test (with
    ``method="dc"``: the leaf eigenvalues and secular roots that hit their iteration cap; expected 0).
    With ``B`` (A x = lambda B x) the columns are B-orthonormal (X^H B X = I) instead of unit 2-norm."""

    eigenvalues: np.ndarray
    eigenvectors: np.ndarray
    not_converged: int


_EIGH_METHODS = {"stein": 0, "dc": 1}


def _eigh_call(ctx: Context, A, select, vectors: bool, who: str, B=None, method="stein"):
    if method not in _EIGH_METHODS:
        raise EigSolError(EIGSOL_E_INVALID, f'{who}: method is "stein" or "dc"')
    A = _square_dense(A, who)
    code = _dtype_code(A.dtype)
    n = A.shape[0]
    if B is not None:
        B = np.asarray(B)
        if B.shape != A.shape:
            raise EigSolError(EIGSOL_E_SIZE_MISMATCH, f"{who}: B must be square and of A's order")
        if B.dtype != A.dtype:
            raise EigSolError(3, f"{who}: scalar type mismatch: A is {A.dtype}, B is {B.dtype}")
    o = None
    if select is not None:
        if len(select) != 3 or select[0] not in ("i", "v"):
            raise EigSolError(EIGSOL_E_INVALID, f'{who}: select is None, ("i", il, iu) or ("v", vl, vu)')
        o = (EighOptionsC(EIGSOL_EIGH_INDEX, int(select[1]), int(select[2]), 0.0, 0.0) if select[0] == "i"
             else EighOptionsC(EIGSOL_EIGH_VALUE, 0, 0, float(select[1]), float(select[2])))
    Af = np.asfortranarray(A)
    w = np.zeros(max(n, 1))
    Z = np.zeros((n, max(n, 1)), dtype=A.dtype, order="F") if vectors else None
    m, nc = C.c_int64(0), C.c_int64(0)
    mcode = _EIGH_METHODS[method]
    if B is None:
        call("eigsol_eigh_dense_m", ctx.handle, code, n, _ptr(Af), None if o is None else C.byref(o), mcode, _ptr(w),
             None if Z is None else _ptr(Z), C.byref(m), C.byref(nc))
    else:
        Bf = np.asfortranarray(B)
        call("eigsol_geigh_dense_m", ctx.handle, code, n, _ptr(Af), _ptr(Bf), None if o is None else C.byref(o), mcode,
             _ptr(w), None if Z is None else _ptr(Z), C.byref(m), C.byref(nc), None)
    k = int(m.value)
    return w[:k].copy(), (None if Z is None else np.asfortranarray(Z[:, :k])), int(nc.value)


def eigvalsh(ctx: Context, A, select=None, B=None, method="stein") -> np.ndarray:
    """Eigenvalues (ascending) of the real symmetric / complex Hermitian matrix whose lower triangle
    is that of ``A`` (float64 / complex128; the strict upper triangle is not read), on the device
    (``eigsol_eigh_dense``): Hessenberg reduction, then bisection.  ``select``: ``None`` (all),
    ``("i", il, iu)`` (0-based, inclusive) or ``("v", vl, vu)`` (vl < lambda <= vu).
    With ``B`` (Hermitian positive definite, same shape and dtype; its lower triangle is read): the
    eigenvalues of A x = lambda B x (``eigsol_geigh_dense``: Cholesky, reduction to standard form).
    ``method`` is accepted and ignored: no vectors are formed, so the values are the bisection path's."""
    return _eigh_call(ctx, A, select, False, "eigvalsh", B, method)[0]


def eigh(ctx: Context, A, select=None, B=None, method="stein") -> EighResult:
    """:func:`eigvalsh` with an orthonormal set of eigenvectors (inverse iteration on the tridiagonal
    matrix, back-transformed through the reduction's stored reflectors).  With ``B`` the eigenvectors
    of A x = lambda B x, B-orthonormal; a ``B`` that is not positive definite raises with the first
    failing column's index in the message.
    ``method="dc"`` (``eigsol_eigh_dense_m``) takes the eigenpairs of the tridiagonal matrix by divide and
    conquer instead: its cost does not depend on how the spectrum clusters, the eigenvalues are its own
    (within 2 n eps ||A||_F of LAPACK's, not bitwise :func:`eigvalsh`'s), and a selection returns the bits of
    the full ``"dc"`` call's columns.  ``EIGSOL_DC_LEAF`` (2 .. 64, default 64) sets the leaf order."""
    w, Z, nc = _eigh_call(ctx, A, select, True, "eigh", B, method)
    return EighResult(w, Z, nc)


@dataclass
class EigResult:
    """Result of :func:`eig`: ``values`` all n eigenvalues (complex128, :func:`qr_eigenvalues`' Francis order),
    ``vectors`` n x m complex128 with unit columns (column j belongs to ``values[select[j]]``, or to
    ``values[j]`` without a selection; its largest-modulus component is real and positive), ``iterations`` /
    ``converged`` the Francis sweeps' as :class:`QRResult` reports them, ``not_converged`` the eigenvalues
    whose inverse iteration failed the growth test from every start vector (expected 0)."""

    values: np.ndarray
    vectors: np.ndarray
    iterations: int
    converged: bool
    not_converged: int


def eig(ctx: Context, A, select=None, opts: SolverOptions = SolverOptions(), batch: int = 0) -> EigResult:
    """Eigenvalues and right eigenvectors of a general dense matrix (float64 / complex128) on the device
    (``eigsol_eig_dense``): blocked Hessenberg reduction, the Francis sweeps of :func:`qr_eigenvalues` on a
    copy of H, every eigenvector by inverse iteration on H (LAPACK xHSEIN's scheme, one workgroup per
    eigenvalue), back-transformed through the reduction's stored reflectors.  ``select``: ``None`` (all) or a
    sequence of indices into ``values``; a selection returns the bits of the full call's columns.
    ``opts.maxIterations`` limits the sweeps; ``batch`` > 0 fixes how many eigenvalues are resident at once
    (0: as many as the workspace cap holds)."""
    A = _square_dense(A, "eig")
    code = _dtype_code(A.dtype)
    n = A.shape[0]
    Af = np.asfortranarray(A)
    sel = None
    if select is not None:
        sel = np.ascontiguousarray(np.asarray(select, dtype=np.int64).ravel())
    o = EigOptionsC(int(opts.maxIterations), int(batch), 0 if sel is None else int(sel.size),
                    None if sel is None else sel.ctypes.data_as(C.POINTER(C.c_int64)))
    if sel is not None and sel.size == 0:   # an empty selection: the eigenvalues alone
        o.sel = None
    m_cap = n if sel is None else int(sel.size)
    w = np.zeros(max(n, 1), dtype=np.complex128)
    want = m_cap > 0
    V = np.zeros((n, max(m_cap, 1)), dtype=np.complex128, order="F")
    m, nc = C.c_int64(0), C.c_int64(0)
    it, conv = C.c_int32(0), C.c_int32(0)
    call("eigsol_eig_dense", ctx.handle, code, n, _ptr(Af), C.byref(o), _ptr(w), _ptr(V) if want else None, C.byref(m),
         C.byref(it), C.byref(conv), C.byref(nc))
    k = int(m.value)
    return EigResult(w[:n].copy(), np.asfortranarray(V[:, :k]), int(it.value), bool(conv.value), int(nc.value))


def eig_stage_times(ctx: Context) -> dict:
    """The context's last :func:`eig` call by stream events, in seconds."""
    ms = (C.c_double * 4)()
    call("eigsol_eig_stage_times", ctx.handle, ms)
    return {k: ms[i] * 1e-3 for i, k in enumerate(("reduction", "francis", "inverse_iteration", "back_transform"))}


@dataclass
class SchurResult:
    """Result of :func:`schur`: ``A = Z @ T @ Z.conj().T``.  ``T`` n x n in A's dtype, Fortran order (real input:
    quasi-triangular, every 2 x 2 diagonal block with equal diagonal entries and off-diagonal entries of
    opposite sign; complex input: upper triangular), ``Z`` n x n orthogonal / unitary or ``None``,
    ``eigenvalues`` complex128 in the order of T's diagonal (a conjugate pair is adjacent, bitwise conjugate,
    the member with the positive imaginary part first), ``iterations`` / ``converged`` the sweeps' as
    :class:`QRResult` reports them.  Not converged: T is upper Hessenberg only; the product still holds.
    With ``sort``: ``sdim`` the number of leading eigenvalues that satisfy it and ``ordered`` whether every swap
    was accepted (see :class:`OrdSchurResult`); ``None`` without."""

    T: np.ndarray
    Z: Optional[np.ndarray]
    eigenvalues: np.ndarray
    iterations: int
    converged: bool
    sdim: Optional[int] = None
    ordered: Optional[bool] = None


_SORT_CODES = {"lhp": 1, "rhp": 2, "iuc": 3, "ouc": 4}   # EIGSOL_SORT_*


def schur(ctx: Context, A, vectors: bool = True, opts: SolverOptions = SolverOptions(), sort=None) -> SchurResult:
    """Schur form of a general dense matrix on the device (``eigsol_schur_dense``): float64 input gives the real
    Schur form, complex128 input the complex one.  Blocked Hessenberg reduction, Q formed on the matrix cores,
    the multishift sweeps of :func:`qr_eigenvalues` with every update applied to the whole of T and to Z, the
    2 x 2 blocks of a real T standardised on the device.  ``vectors=False`` skips Z; T and the eigenvalues
    are the same bits either way.  ``opts.maxIterations`` limits the sweeps per deflation.

    ``sort`` (SciPy's ``schur(sort=)``): ``"lhp"``, ``"rhp"``, ``"iuc"`` or ``"ouc"`` reorders the form on the
    device before anything is copied back (``eigsol_schur_sorted_dense``); a boolean mask or a callable runs
    :func:`ordschur` on the result.  Either way the bits are those of ``schur`` followed by :func:`ordschur`."""
    if sort is not None and not isinstance(sort, str):
        r = schur(ctx, A, vectors, opts)
        if not r.converged:
            return SchurResult(r.T, r.Z, r.eigenvalues, r.iterations, False, 0, False)
        o = ordschur(ctx, r.T, r.Z, sort)
        return SchurResult(o.T, o.Z, o.eigenvalues, r.iterations, r.converged, o.sdim, o.ordered)
    if sort is not None and sort not in _SORT_CODES:
        raise EigSolError(EIGSOL_E_INVALID, f"schur: sort is one of {sorted(_SORT_CODES)}, a mask or a callable, got {sort!r}")
    A = _square_dense(A, "schur")
    code = _dtype_code(A.dtype)
    n = A.shape[0]
    Af = np.asfortranarray(A)
    o = SolverOptionsC(int(opts.maxIterations), float(opts.tolerance))
    T = np.zeros((n, n), dtype=A.dtype, order="F")
    Z = np.zeros((n, n), dtype=A.dtype, order="F") if vectors else None
    real = not np.iscomplexobj(A)
    wr = np.zeros(max(n, 1), dtype=np.float64 if real else np.complex128)
    wi = np.zeros(max(n, 1), dtype=np.float64)
    it, conv = C.c_int32(0), C.c_int32(0)
    sdim, ordered = None, None
    if sort is None:
        call("eigsol_schur_dense", ctx.handle, code, n, _ptr(Af), C.byref(o), _ptr(T), _ptr(Z) if vectors and n else None,
             _ptr(wr), wi.ctypes.data_as(C.POINTER(C.c_double)), C.byref(it), C.byref(conv))
    else:
        sd, od = C.c_int64(0), C.c_int32(0)
        call("eigsol_schur_sorted_dense", ctx.handle, code, n, _ptr(Af), C.byref(o), _SORT_CODES[sort], _ptr(T),
             _ptr(Z) if vectors and n else None, _ptr(wr), wi.ctypes.data_as(C.POINTER(C.c_double)), C.byref(sd), C.byref(it),
             C.byref(conv), C.byref(od))
        sdim, ordered = int(sd.value), bool(od.value)
    w = (wr[:n] + 1j * wi[:n]) if real else wr[:n].copy()
    return SchurResult(T, Z, np.asarray(w, dtype=np.complex128), int(it.value), bool(conv.value), sdim, ordered)


@dataclass
class OrdSchurResult:
    """Result of :func:`ordschur`: the reordered ``T`` and ``Z`` (``None`` if none was given), Fortran order, in
    T's dtype; ``eigenvalues`` under :class:`SchurResult`'s contract; ``sdim`` the number of selected rows (a
    selected conjugate pair counts two), which now lead; ``ordered`` false where a swap was rejected because two
    blocks were too close to exchange: T is then a valid Schur form of the same matrix, partly reordered."""

    T: np.ndarray
    Z: Optional[np.ndarray]
    eigenvalues: np.ndarray
    sdim: int
    ordered: bool


def _block_eigenvalues(T: np.ndarray) -> np.ndarray:
    """Eigenvalues of a (quasi-)triangular T in standard form, by :class:`SchurResult`'s contract."""
    n = T.shape[0]
    w = np.array(np.diagonal(T), dtype=np.complex128)
    if not np.iscomplexobj(T) and n > 1:
        lo, up = np.diagonal(T, -1), np.diagonal(T, 1)
        for k in np.nonzero(lo)[0]:
            im = np.sqrt(abs(up[k])) * np.sqrt(abs(lo[k]))
            w[k] = complex(T[k, k], im)
            w[k + 1] = complex(T[k + 1, k + 1], -im)
    return w


def ordschur(ctx: Context, T, Z, select) -> OrdSchurResult:
    """Reorders a Schur form ``A = Z T Z^H`` on the device so that the selected eigenvalues lead T
    (``eigsol_ordschur_dense``; LAPACK ``xTRSEN`` without its condition estimates).  ``T`` float64
    (quasi-triangular, :func:`schur`'s standard 2 x 2 blocks) or complex128 (triangular); ``Z`` of the same
    order, or ``None``.  ``select``: a boolean array with one flag per row of T (real T: a flag on either row of
    a 2 x 2 block selects the pair); ``"lhp"`` (Re < 0), ``"rhp"`` (Re >= 0), ``"iuc"`` (|lambda| <= 1) or
    ``"ouc"`` (|lambda| > 1); or a callable that maps the complex eigenvalue array to a boolean array, evaluated
    on the host.  The selected blocks keep their order, and so do the others."""
    T = np.asarray(T)
    if T.ndim != 2 or T.shape[0] != T.shape[1]:
        raise EigSolError(EIGSOL_E_NOT_SQUARE, f"ordschur: T must be square, got shape {T.shape}")
    n = T.shape[0]
    dt = np.complex128 if np.iscomplexobj(T) or (Z is not None and np.iscomplexobj(Z)) else np.float64
    To = np.array(T, dtype=dt, order="F", copy=True)
    Zo = None
    if Z is not None:
        Zo = np.array(Z, dtype=dt, order="F", copy=True)
        if Zo.shape != (n, n):
            raise EigSolError(EIGSOL_E_SIZE_MISMATCH, f"ordschur: Z {Zo.shape} does not fit T {T.shape}")
    if isinstance(select, str) or callable(select):
        w = _block_eigenvalues(To)
        if callable(select):
            mask = select(w)
        elif select == "lhp":
            mask = w.real < 0
        elif select == "rhp":
            mask = w.real >= 0
        elif select == "iuc":
            mask = w.real * w.real + w.imag * w.imag <= 1.0   # the device's expression, rounding for rounding
        elif select == "ouc":
            mask = w.real * w.real + w.imag * w.imag > 1.0
        else:
            raise EigSolError(EIGSOL_E_INVALID, f"ordschur: select is one of {sorted(_SORT_CODES)}, a mask or a callable")
    else:
        mask = select
    mask = np.ascontiguousarray(np.asarray(mask).astype(bool).astype(np.uint8))
    if mask.shape != (n,):
        raise EigSolError(EIGSOL_E_SIZE_MISMATCH, f"ordschur: select needs one flag per row of T ({n}), got shape {mask.shape}")
    real = dt == np.float64
    wr = np.zeros(max(n, 1), dtype=np.float64 if real else np.complex128)
    wi = np.zeros(max(n, 1), dtype=np.float64)
    sd, od = C.c_int64(0), C.c_int32(0)
    call("eigsol_ordschur_dense", ctx.handle, _dtype_code(dt), n, _ptr(To), _ptr(Zo) if Zo is not None and n else None,
         _ptr(mask) if n else None, _ptr(wr), wi.ctypes.data_as(C.POINTER(C.c_double)), C.byref(sd), C.byref(od))
    w = (wr[:n] + 1j * wi[:n]) if real else wr[:n].copy()
    return OrdSchurResult(To, Zo, np.asarray(w, dtype=np.complex128), int(sd.value), bool(od.value))


def ordschur_stats(ctx: Context) -> dict:
    """The context's last reordering (:func:`ordschur` or ``schur(sort=...)``): ``seconds`` by stream events,
    ``rounds`` and ``windows`` that did work, and ``swaps`` of adjacent blocks."""
    ms = C.c_double(0.0)
    r, wn, sw = C.c_int32(0), C.c_int32(0), C.c_int32(0)
    call("eigsol_ordschur_stats", ctx.handle, C.byref(ms), C.byref(r), C.byref(wn), C.byref(sw))
    return {"seconds": ms.value * 1e-3, "rounds": int(r.value), "windows": int(wn.value), "swaps": int(sw.value)}


def schur_stage_times(ctx: Context) -> dict:
    """The context's last :func:`schur` call by stream events, in seconds."""
    ms = (C.c_double * 4)()
    call("eigsol_schur_stage_times", ctx.handle, ms)
    return {k: ms[i] * 1e-3 for i, k in enumerate(("reduction", "form_q", "sweeps", "finish"))}


@dataclass
class SylvesterResult:
    """Result of :func:`solve_sylvester` / :func:`solve_continuous_lyapunov`: ``X`` m x n, Fortran order, float64
    (all inputs real) or complex128; ``perturbed`` the number of diagonal block pairs of the triangular stage in
    which a pivot below LAPACK's ``smin`` was replaced by it (0: the equation was solved as posed; positive: A
    and -B share an eigenvalue to working precision and X solves a nearby equation); ``converged`` both Schur
    factorisations converged (a result is only returned when they did)."""

    X: np.ndarray
    perturbed: int
    converged: bool


def _syl_operands(who: str, *mats):
    mats = [np.asarray(M) for M in mats]
    dt = np.complex128 if any(np.iscomplexobj(M) for M in mats) else np.float64
    for M in mats:
        if M.ndim != 2:
            raise EigSolError(EIGSOL_E_SIZE_MISMATCH, f"{who}: every operand is a matrix, got shape {M.shape}")
    return [np.asfortranarray(M, dtype=dt) for M in mats], dt


def _syl_finish(who: str, X, pert, conv) -> SylvesterResult:
    if not conv.value:
        raise EigSolError(EIGSOL_E_SOLVER, f"{who}: a Schur factorisation did not converge")
    return SylvesterResult(X, int(pert.value), True)


def solve_sylvester(ctx: Context, A, B, C, opts: SolverOptions = SolverOptions()) -> SylvesterResult:
    """Solves ``A X + X B = C`` on the device by Bartels-Stewart (``eigsol_sylvester_dense``; SciPy's
    ``solve_sylvester``): the Schur forms of A (m x m) and B (n x n) by :func:`schur`'s pipeline, the
    quasi-triangular equation by anti-diagonal wavefronts of block solves in LDS and rank-K updates on the
    matrix cores, the four transforms on the matrix cores.  Complex input anywhere promotes every operand to
    complex128, else float64.  Raises :class:`EigSolError` if a Schur factorisation does not converge."""
    (A, B, Cm), dt = _syl_operands("solve_sylvester", A, B, C)
    m, n = A.shape[0], B.shape[0]
    if A.shape != (m, m) or B.shape != (n, n) or Cm.shape != (m, n):
        raise EigSolError(EIGSOL_E_SIZE_MISMATCH,
                          f"solve_sylvester: A {A.shape}, B {B.shape} and C {Cm.shape} do not form A X + X B = C")
    o = SolverOptionsC(int(opts.maxIterations), float(opts.tolerance))
    X = np.zeros((m, n), dtype=dt, order="F")
    pert, conv = ctypes.c_int32(0), ctypes.c_int32(0)
    call("eigsol_sylvester_dense", ctx.handle, _dtype_code(dt), m, n, _ptr(A), _ptr(B), _ptr(Cm), ctypes.byref(o), _ptr(X),
         ctypes.byref(pert), ctypes.byref(conv))
    return _syl_finish("solve_sylvester", X, pert, conv)


def solve_continuous_lyapunov(ctx: Context, A, Q, opts: SolverOptions = SolverOptions()) -> SylvesterResult:
    """Solves ``A X + X A^H = Q`` on the device (``eigsol_lyapunov_dense``; SciPy's
    ``solve_continuous_lyapunov``): one Schur form serves both sides.  Otherwise as :func:`solve_sylvester`."""
    (A, Qm), dt = _syl_operands("solve_continuous_lyapunov", A, Q)
    n = A.shape[0]
    if A.shape != (n, n) or Qm.shape != (n, n):
        raise EigSolError(EIGSOL_E_SIZE_MISMATCH,
                          f"solve_continuous_lyapunov: A {A.shape} and Q {Qm.shape} must be square and of one order")
    o = SolverOptionsC(int(opts.maxIterations), float(opts.tolerance))
    X = np.zeros((n, n), dtype=dt, order="F")
    pert, conv = C.c_int32(0), C.c_int32(0)
    call("eigsol_lyapunov_dense", ctx.handle, _dtype_code(dt), n, _ptr(A), _ptr(Qm), C.byref(o), _ptr(X), C.byref(pert),
         C.byref(conv))
    return _syl_finish("solve_continuous_lyapunov", X, pert, conv)


def trsyl(ctx: Context, R, S, F, trans_b: bool = False):
    """The triangular stage alone (``eigsol_trsyl_dense``; LAPACK ``xTRSYL`` without its scale factor): solves
    ``R Y + Y op(S) = F`` with op(S) = S, or S^H when ``trans_b``.  R and S are upper triangular (complex) or
    quasi-triangular in :func:`schur`'s standard form (real); anything else raises ``EIGSOL_E_INVALID``.
    Returns ``(Y, perturbed)``, Y m x n in Fortran order."""
    (R, S, Fm), dt = _syl_operands("trsyl", R, S, F)
    m, n = R.shape[0], S.shape[0]
    if R.shape != (m, m) or S.shape != (n, n) or Fm.shape != (m, n):
        raise EigSolError(EIGSOL_E_SIZE_MISMATCH, f"trsyl: R {R.shape}, S {S.shape} and F {Fm.shape} do not fit")
    Y = np.array(Fm, dtype=dt, order="F", copy=True)
    pert = C.c_int32(0)
    call("eigsol_trsyl_dense", ctx.handle, _dtype_code(dt), m, n, _ptr(R), _ptr(S), 1 if trans_b else 0, _ptr(Y),
         C.byref(pert))
    return Y, int(pert.value)


def sylvester_stage_times(ctx: Context) -> dict:
    """The context's last :func:`solve_sylvester` / :func:`solve_continuous_lyapunov` call by stream events, in
    seconds."""
    ms = (C.c_double * 5)()
    call("eigsol_sylvester_stage_times", ctx.handle, ms)
    return {k: ms[i] * 1e-3 for i, k in enumerate(("schur_a", "schur_b", "transform_in", "triangular", "transform_out"))}


@dataclass
class SqrtmResult:
    """Result of :func:`sqrtm`: ``X`` n x n, Fortran order, float64 for a real A without negative real
    eigenvalues, else complex128; ``perturbed`` the number of blocks of the triangular stage in which a pivot
    below ``smin`` was replaced by it (0: the root was computed as posed; positive: A has a (nearly) repeated
    eigenvalue at 0 and X solves a nearby problem, or no root exists); ``converged`` the Schur factorisation
    converged (a result is only returned when it did)."""

    X: np.ndarray
    perturbed: int
    converged: bool


def _sqrtm_operand(A, who: str) -> np.ndarray:
    A = _square_dense(A, who)
    if not np.issubdtype(A.dtype, np.inexact):
        A = A.astype(np.float64)
    return np.asfortranarray(A)


def sqrtm(ctx: Context, A, opts: SolverOptions = SolverOptions()) -> SqrtmResult:
    """Principal square root of a square matrix on the device (``eigsol_sqrtm_dense``; SciPy's ``sqrtm``):
    ``X @ X = A`` with every eigenvalue of X in the closed right half plane.  A = Z T Z^H by :func:`schur`'s
    pipeline, U = T^(1/2) by the blocked recurrence of :func:`trsqrt`, X = Z U Z^H on the matrix cores.  A real
    A keeps a real X whenever one exists (no negative real eigenvalue); otherwise the library reports that the
    real Schur form has a negative 1 x 1 block, and the call runs again on A cast to complex128 and returns a
    complex X, which costs a second Schur factorisation; a negative real eigenvalue's root is then on the positive
    imaginary axis, as SciPy's.  float32 and long double input is refused with
    ``EIGSOL_E_UNSUPPORTED``, a matrix that is not square with status 1, a non-finite entry with
    ``EIGSOL_E_SOLVER``.  Raises :class:`EigSolError` if the Schur factorisation does not converge."""
    A = _sqrtm_operand(A, "sqrtm")
    n = A.shape[0]
    o = SolverOptionsC(int(opts.maxIterations), float(opts.tolerance))
    while True:
        X = np.zeros((n, n), dtype=A.dtype, order="F")
        pert, conv, cx = C.c_int32(0), C.c_int32(0), C.c_int32(0)
        call("eigsol_sqrtm_dense", ctx.handle, _dtype_code(A.dtype), n, _ptr(A), C.byref(o), _ptr(X), C.byref(pert),
             C.byref(conv), C.byref(cx))
        if not conv.value:
            raise EigSolError(EIGSOL_E_SOLVER, "sqrtm: the Schur factorisation did not converge")
        if not cx.value:
            return SqrtmResult(X, int(pert.value), True)
        A = np.asfortranarray(A, dtype=np.complex128)


def trsqrt(ctx: Context, T):
    """The triangular stage alone (``eigsol_trsqrt_dense``): ``U @ U = T`` for an upper triangular (complex) or
    real quasi-triangular T whose 2 x 2 diagonal blocks have complex eigenvalues.  Anything else, and a real T
    with a negative 1 x 1 block (pass it as complex), raises ``EIGSOL_E_INVALID``.  Returns ``(U, perturbed)``, U
    in Fortran order and T's dtype."""
    T = _sqrtm_operand(T, "trsqrt")
    n = T.shape[0]
    U = np.zeros((n, n), dtype=T.dtype, order="F")
    pert = C.c_int32(0)
    call("eigsol_trsqrt_dense", ctx.handle, _dtype_code(T.dtype), n, _ptr(T), _ptr(U), C.byref(pert))
    return U, int(pert.value)


def sqrtm_stage_times(ctx: Context) -> dict:
    """The context's last ``eigsol_sqrtm_dense`` call by stream events, in seconds (a :func:`sqrtm` that went
    to complex: its second call)."""
    ms = (C.c_double * 4)()
    call("eigsol_sqrtm_stage_times", ctx.handle, ms)
    return {k: ms[i] * 1e-3 for i, k in enumerate(("schur", "triangular", "transform", "total"))}


# ------------------------------------------------------------------------------- logm
@dataclass
class LogmResult:
    """Result of :func:`logm`: ``X`` n x n, Fortran order, float64 for a real A without negative real eigenvalues,
    else complex128; ``roots`` the number of square roots taken of the triangular factor and ``degree`` of the Pade
    approximant (1 to 7; 0 where A is the identity); ``perturbed`` the sum of the root stages' counts (see
    :class:`SqrtmResult`; 0: every root was computed as posed); ``converged`` the Schur factorisation converged (a
    result is only returned when it did)."""

    X: np.ndarray
    roots: int
    degree: int
    perturbed: int
    converged: bool


def logm(ctx: Context, A, opts: SolverOptions = SolverOptions()) -> LogmResult:
    """Principal logarithm of a square matrix on the device (``eigsol_logm_dense``; SciPy's ``logm``):
    ``exp(X) = A`` with the imaginary part of every eigenvalue of X in (-pi, pi].  A = Z T Z^H by :func:`schur`'s
    pipeline, L = log T by the inverse scaling and squaring of :func:`trlogm`, X = Z L Z^H on the matrix cores.  A
    real A keeps a real X whenever one exists (no negative real eigenvalue); otherwise the call runs again on A cast
    to complex128, which costs a second Schur factorisation, and a negative real eigenvalue's logarithm has
    imaginary part +pi, as SciPy's.  A singular A (a zero on the diagonal of T) and a non-finite entry raise
    :class:`EigSolError` with ``EIGSOL_E_SOLVER``; float32 and long double input is refused with
    ``EIGSOL_E_UNSUPPORTED``, a matrix that is not square with status 1."""
    A = _sqrtm_operand(A, "logm")
    n = A.shape[0]
    o = SolverOptionsC(int(opts.maxIterations), float(opts.tolerance))
    while True:
        X = np.zeros((n, n), dtype=A.dtype, order="F")
        s, m, pert, conv, cx = (C.c_int32(0) for _ in range(5))
        call("eigsol_logm_dense", ctx.handle, _dtype_code(A.dtype), n, _ptr(A), C.byref(o), _ptr(X), C.byref(s), C.byref(m),
             C.byref(pert), C.byref(conv), C.byref(cx))
        if not conv.value:
            raise EigSolError(EIGSOL_E_SOLVER, "logm: the Schur factorisation did not converge")
        if not cx.value:
            return LogmResult(X, int(s.value), int(m.value), int(pert.value), True)
        A = np.asfortranarray(A, dtype=np.complex128)


def trlogm(ctx: Context, T):
    """The triangular stage alone (``eigsol_trlogm_dense``): ``L = log T`` for an upper triangular (complex) or
    real quasi-triangular T whose 2 x 2 diagonal blocks have complex eigenvalues.  Anything else, and a real T
    with a negative 1 x 1 block (pass it as complex), raises ``EIGSOL_E_INVALID``; a zero diagonal entry raises
    ``EIGSOL_E_SOLVER`` and names the row.  Returns ``(L, roots, degree, perturbed)``, L in Fortran order and T's
    dtype."""
    T = _sqrtm_operand(T, "trlogm")
    n = T.shape[0]
    L = np.zeros((n, n), dtype=T.dtype, order="F")
    s, m, pert = C.c_int32(0), C.c_int32(0), C.c_int32(0)
    call("eigsol_trlogm_dense", ctx.handle, _dtype_code(T.dtype), n, _ptr(T), _ptr(L), C.byref(s), C.byref(m), C.byref(pert))
    return L, int(s.value), int(m.value), int(pert.value)


def logm_stage_times(ctx: Context) -> dict:
    """The context's last ``eigsol_logm_dense`` call by stream events, in seconds (a :func:`logm` that went to
    complex: its second call)."""
    ms = (C.c_double * 5)()
    call("eigsol_logm_stage_times", ctx.handle, ms)
    return {k: ms[i] * 1e-3 for i, k in enumerate(("schur", "roots", "pade", "transform", "total"))}


def logm_plan(norm: float, tried: bool = False) -> int:
    """Host only (``eigsol_logm_plan``): the Pade degree with which the root loop of :func:`logm` stops at
    ||T^(1/2^s) - I||_1 = ``norm``, or 0: another root.  ``tried``: the loop has been below theta_7 before."""
    m = C.c_int32(0)
    call("eigsol_logm_plan", float(norm), 1 if tried else 0, C.byref(m))
    return int(m.value)


# ------------------------------------------------------------------------------- matmul, solve, expm
def _dense_operand(A) -> np.ndarray:
    A = np.asarray(A)
    if not np.issubdtype(A.dtype, np.inexact):
        A = A.astype(np.float64)
    return A


def matmul(ctx: Context, A, B) -> np.ndarray:
    """``A @ B`` for host matrices on the fp64 matrix cores (``eigsol_gemm_dense``; float64 / complex128, a real
    and a complex operand give a complex product): an LDS-tiled MFMA kernel that sums every entry in ascending k,
    so two calls return the same bits.  The result is in Fortran order."""
    A, B = _dense_operand(A), _dense_operand(B)
    if A.ndim != 2 or B.ndim != 2 or A.shape[1] != B.shape[0]:
        raise EigSolError(EIGSOL_E_SIZE_MISMATCH, f"matmul: shapes {A.shape} and {B.shape} do not match")
    dt = np.result_type(A.dtype, B.dtype)
    code = _dtype_code(dt)
    Af, Bf = np.asfortranarray(A, dtype=dt), np.asfortranarray(B, dtype=dt)
    m, k = A.shape
    n = B.shape[1]
    Cm = np.zeros((m, n), dtype=dt, order="F")
    call("eigsol_gemm_dense", ctx.handle, code, m, n, k, _ptr(Af), _ptr(Bf), _ptr(Cm))
    return Cm


def solve(ctx: Context, A, B) -> np.ndarray:
    """``X`` with ``A @ X = B`` by LU with partial pivoting on the device (``eigsol_solve_dense``; float64 /
    complex128).  ``B`` is a vector (n) or a matrix (n x nrhs); X has its shape, a matrix in Fortran order.  Raises
    ``EigSolError`` (``EIGSOL_E_SOLVER``) naming the column of the first exactly zero pivot when A is singular."""
    A = _dense_operand(_square_dense(A, "solve"))
    B = _dense_operand(B)
    n = A.shape[0]
    if B.ndim not in (1, 2) or B.shape[0] != n:
        raise EigSolError(EIGSOL_E_SIZE_MISMATCH, f"solve: B has shape {B.shape}, A has order {n}")
    dt = np.result_type(A.dtype, B.dtype)
    code = _dtype_code(dt)
    Af = np.asfortranarray(A, dtype=dt)
    X = np.array(B.reshape(n, -1), dtype=dt, order="F")
    call("eigsol_solve_dense", ctx.handle, code, n, X.shape[1], _ptr(Af), _ptr(X), _ptr(X))
    return X[:, 0].copy() if B.ndim == 1 else X


@dataclass
class ExpmResult:
    """Result of :func:`expm`: ``X`` n x n, Fortran order, float64 for real input and else complex128; ``degree``
    of the Pade approximant (3, 5, 7, 9 or 13) and the number of ``squarings``."""

    X: np.ndarray
    degree: int
    squarings: int


def expm(ctx: Context, A) -> ExpmResult:
    """Matrix exponential on the device (``eigsol_expm_dense``; SciPy's ``expm``) by Higham's 2005 scaling and
    squaring: the 1-norm decides the degree and the squarings (:func:`expm_plan`), the Pade approximant of the
    scaled matrix takes three to six products on the matrix cores and one LU solve, then the squarings.  Integer
    input is cast to float64; float32 and long double input is refused with ``EIGSOL_E_UNSUPPORTED``, a matrix that
    is not square with status 1, a non-finite entry and a result that overflows with ``EIGSOL_E_SOLVER``."""
    A = np.asfortranarray(_dense_operand(_square_dense(A, "expm")))
    n = A.shape[0]
    X = np.zeros((n, n), dtype=A.dtype, order="F")
    m, s = C.c_int32(0), C.c_int32(0)
    call("eigsol_expm_dense", ctx.handle, _dtype_code(A.dtype), n, _ptr(A), _ptr(X), C.byref(m), C.byref(s))
    return ExpmResult(X, int(m.value), int(s.value))


def expm_stage_times(ctx: Context) -> dict:
    """The context's last ``eigsol_expm_dense`` call by stream events, in seconds."""
    ms = (C.c_double * 6)()
    call("eigsol_expm_stage_times", ctx.handle, ms)
    return {k: ms[i] * 1e-3 for i, k in enumerate(("norm", "pade", "factor", "substitution", "squarings", "total"))}


def expm_plan(alpha: float):
    """Host only (``eigsol_expm_plan``): ``(degree, squarings)`` that :func:`expm` uses for a matrix of 1-norm
    ``alpha``."""
    m, s = C.c_int32(0), C.c_int32(0)
    call("eigsol_expm_plan", float(alpha), C.byref(m), C.byref(s))
    return int(m.value), int(s.value)


@dataclass
class SvdResult:
    """Result of :func:`svd`: ``U`` m x k, ``s`` the k = min(m, n) singular values (descending), ``Vh`` k x n, so
    that ``A = (U * s) @ Vh`` as with NumPy's thin SVD; column j of ``Vh.conj().T`` has its largest-modulus
    component real and positive.  ``sweeps`` the Jacobi sweeps run, ``not_converged`` the pairs of column
    blocks still above the tolerance when ``max_sweeps`` ran out (expected 0).  Without vectors ``U`` and
    ``Vh`` are ``None``."""

    U: Optional[np.ndarray]
    s: np.ndarray
    Vh: Optional[np.ndarray]
    sweeps: int
    not_converged: int


def _svd_call(ctx: Context, A, want_u: bool, want_v: bool, max_sweeps: int):
    A = np.asarray(A)
    if A.ndim != 2:
        raise ValueError("svd: a two-dimensional matrix is expected")
    if A.dtype.kind not in "fc":   # integers and booleans; other float widths are the C entry's to refuse
        A = A.astype(np.float64)
    code = _dtype_code(A.dtype)
    m, n = A.shape
    k = min(m, n)
    Af = np.asfortranarray(A)
    s = np.zeros(max(k, 1), dtype=np.float64)
    U = np.zeros((m, k), dtype=A.dtype, order="F") if want_u else None
    V = np.zeros((n, k), dtype=A.dtype, order="F") if want_v else None
    o = SvdOptionsC(int(max_sweeps))
    sw, nc = C.c_int32(0), C.c_int64(0)
    call("eigsol_svd_dense", ctx.handle, code, m, n, _ptr(Af), C.byref(o), s.ctypes.data_as(C.POINTER(C.c_double)),
         _ptr(U) if want_u and U.size else None, _ptr(V) if want_v and V.size else None, C.byref(sw), C.byref(nc))
    return s[:k].copy(), U, V, int(sw.value), int(nc.value)


def svd(ctx: Context, A, vectors: bool = True, max_sweeps: int = 60) -> SvdResult:
    """Thin singular value decomposition of a dense m x n matrix (float64 / complex128) on the device
    (``eigsol_svd_dense``): block one-sided Jacobi on the fp64 matrix cores; see :class:`SvdResult`.
    ``vectors=False`` computes the singular values alone (the same bits)."""
    s, U, V, sw, nc = _svd_call(ctx, A, vectors, vectors, max_sweeps)
    if not vectors:
        return SvdResult(None, s, None, sw, nc)
    return SvdResult(U, s, np.ascontiguousarray(V.conj().T), sw, nc)


def svdvals(ctx: Context, A) -> np.ndarray:
    """The singular values of a dense m x n matrix, descending (:func:`svd` without vectors)."""
    return _svd_call(ctx, A, False, False, 60)[0]


def svd_stage_times(ctx: Context) -> dict:
    """The context's last :func:`svd` / :func:`svdvals` call by stream events, in seconds."""
    ms = (C.c_double * 4)()
    call("eigsol_svd_stage_times", ctx.handle, ms)
    return {k: ms[i] * 1e-3 for i, k in enumerate(("gram", "pair_jacobi", "apply", "finish"))}


# ------------------------------------------------------------------------------------------- svds
def dense_mv_h(matrix: DenseMatrix, x) -> np.ndarray:
    """``A^H @ x`` for a host vector x (nrows) through ``eigsol_dense_gemv_h`` (double and complex double
    matrices of any shape); two calls return the same bits."""
    nrows, ncols = matrix.shape
    if np.shape(x) != (nrows,):
        raise EigSolError(EIGSOL_E_SIZE_MISMATCH, f"x has shape {np.shape(x)}, the matrix has {nrows} rows")
    if is_wide(matrix.dtype):
        raise EigSolError(EIGSOL_E_UNSUPPORTED, "dense_mv_h: long double matrices are not supported")
    xh = np.ascontiguousarray(x, dtype=matrix.dtype)
    y = np.empty(ncols, dtype=matrix.dtype)
    ctx = matrix.ctx
    dx, dy = ctx.malloc(max(xh.nbytes, 16)), ctx.malloc(max(y.nbytes, 16))
    try:
        if xh.nbytes:
            ctx.h2d(dx, xh)
        matrix.gemv_h(dx, dy)
        if y.nbytes:
            ctx.d2h(y, dy)
    finally:
        ctx.free(dx)
        ctx.free(dy)
    return y


@dataclass
class SvdsOptions:
    """Options of :func:`svds` (``eigsol_svds_options`` without nsv / ncv)."""

    max_restarts: int = 300
    tolerance: float = 1e-10          # < 0: never converges


@dataclass
class SvdsResult:
    s: np.ndarray                     # k singular values, descending
    U: Optional[np.ndarray]           # M x k in the matrix dtype (None without vectors)
    V: Optional[np.ndarray]           # N x k; the largest-modulus component of every column real and positive
    residuals: np.ndarray             # k: hypot(||A v - s u||_2, ||A^H u - s v||_2)
    restarts: int                     # restart cycles run
    applications: int                 # products with A or A^H
    converged: bool


def default_svds_ncv(shape, nsv: int) -> int:
    return min(min(shape), 64, max(2 * nsv + 1, 20))


def svds(matrix, nsv: int, opts: SvdsOptions = SvdsOptions(), ncv: Optional[int] = None, v0=None, seed: int = 0,
         vectors: bool = True, adjoint: Optional[CsrMatrix] = None) -> SvdsResult:
    """The ``nsv`` largest singular triplets of a device-resident CSR or dense matrix by thick-restart
    Golub-Kahan-Lanczos (``eigsol_svds_csr`` / ``eigsol_svds_dense``), without forming A^H A.  ``ncv``
    basis vectors (default min(min(M, N), 64, max(2 nsv + 1, 20))); ``v0`` (N entries) defaults to
    uniform(-1, 1) entries from ``numpy.random.default_rng(seed)`` (complex for complex matrices).  For a
    CSR matrix ``adjoint`` may be its :meth:`CsrMatrix.adjoint`, kept by a caller who solves more than
    once; without it the handle is built and destroyed inside.  ``vectors=False`` returns the values and
    residuals alone (the same bits)."""
    M, N = matrix.shape
    nsv = int(nsv)
    m = default_svds_ncv((M, N), nsv) if ncv is None else int(ncv)
    if v0 is None:
        rng = np.random.default_rng(seed)
        v0 = rng.uniform(-1, 1, N)
        if np.issubdtype(matrix.dtype, np.complexfloating):
            v0 = v0 + 1j * rng.uniform(-1, 1, N)
    if is_wide(matrix.dtype):
        raise EigSolError(EIGSOL_E_UNSUPPORTED, "svds: long double matrices are not supported")
    v0 = _vector(v0, matrix.dtype, N, "v0")
    k = max(nsv, 0)
    s = np.zeros(max(k, 1))
    res = np.zeros(max(k, 1))
    U = np.zeros((M, k), dtype=matrix.dtype, order="F") if vectors else None
    V = np.zeros((N, k), dtype=matrix.dtype, order="F") if vectors else None
    rs, ap, conv = C.c_int32(0), C.c_int32(0), C.c_int32(0)
    o = SvdsOptionsC(int(opts.max_restarts), float(opts.tolerance), nsv, m)
    pd = C.POINTER(C.c_double)
    tail = (C.byref(o), _ptr(v0), s.ctypes.data_as(pd), _ptr(U) if vectors and U.size else None,
            _ptr(V) if vectors and V.size else None, res.ctypes.data_as(pd), C.byref(rs), C.byref(ap), C.byref(conv))
    if isinstance(matrix, DenseMatrix):
        if adjoint is not None:
            raise EigSolError(EIGSOL_E_INVALID, "svds: adjoint= applies to CSR matrices")
        call("eigsol_svds_dense", matrix.handle, *tail)
    else:
        call("eigsol_svds_csr", matrix.handle, None if adjoint is None else adjoint.handle, *tail)
    return SvdsResult(s[:k].copy(), U, V, res[:k].copy(), int(rs.value), int(ap.value), bool(conv.value))


def svds_stage_times(ctx: Context) -> dict:
    """The context's last :func:`svds` call by stream events, in seconds."""
    ms = (C.c_double * 4)()
    call("eigsol_svds_stage_times", ctx.handle, ms)
    return {k: ms[i] * 1e-3 for i, k in enumerate(("product", "adjoint_product", "orthogonalisation", "restart_finish"))}


def cholesky(ctx: Context, B) -> np.ndarray:
    """L of B = L L^H (``eigsol_cholesky_dense``; float64 / complex128; only the lower triangle of ``B``
    is read): zero strict upper triangle, real positive diagonal.  Raises ``EigSolError`` naming the
    first column whose pivot is not > 0 when ``B`` is not positive definite."""
    B = _square_dense(B, "cholesky")
    code = _dtype_code(B.dtype)
    n = B.shape[0]
    Bf = np.asfortranarray(B)
    L = np.zeros((n, n), dtype=B.dtype, order="F")
    call("eigsol_cholesky_dense", ctx.handle, code, n, _ptr(Bf), _ptr(L), None)
    return L


def geigh_stage_times(ctx: Context) -> dict:
    """The context's last :func:`eigh` / :func:`eigvalsh` call with ``B`` by stream events, in seconds."""
    ms = (C.c_double * 7)()
    call("eigsol_geigh_stage_times", ctx.handle, ms)
    return {k: ms[i] * 1e-3 for i, k in enumerate(("cholesky", "standardise", "reduction", "bisection",
                                                   "inverse_iteration", "back_transform", "triangular_back_solve"))}


def eigh_stage_times(ctx: Context) -> dict:
    """The context's last :func:`eigh` / :func:`eigvalsh` call by stream events, in seconds."""
    ms = (C.c_double * 4)()
    call("eigsol_eigh_stage_times", ctx.handle, ms)
    return {k: ms[i] * 1e-3 for i, k in enumerate(("reduction", "bisection", "inverse_iteration", "back_transform"))}


def eigh_dc_stage_times(ctx: Context) -> dict:
    """The context's last :func:`eigh` call with ``method="dc"``, in seconds (``host_deflation`` is the wall time
    of the host scans alone)."""
    ms = (C.c_double * 6)()
    call("eigsol_eigh_dc_stage_times", ctx.handle, ms)
    return {k: ms[i] * 1e-3 for i, k in enumerate(("reduction", "leaves", "host_deflation", "secular_vectors",
                                                   "merge_gemm", "back_transform"))}


def dc_deflate(d, z, rho, n1=None):
    """Host only (``eigsol_dc_deflate``): the deflation of one divide-and-conquer merge D + rho z z^T.
    Returns a dict: k, perm, dk, zk, rho, rot (list of (a, b, c, s)), tol."""
    d = np.ascontiguousarray(d, dtype=np.float64)
    z = np.ascontiguousarray(z, dtype=np.float64)
    n = d.size
    if z.size != n:
        raise EigSolError(EIGSOL_E_SIZE_MISMATCH, "dc_deflate: d and z must have the same length")
    n1 = n // 2 if n1 is None else int(n1)
    cap = max(n, 2)
    perm, cols = np.zeros(cap, dtype=np.int64), np.zeros(2 * cap, dtype=np.int64)
    dk, zk, cs = np.zeros(cap), np.zeros(cap), np.zeros(2 * cap)
    k, nrot = C.c_int64(0), C.c_int64(0)
    rho_out, tol = C.c_double(0.0), C.c_double(0.0)
    call("eigsol_dc_deflate", n, n1, _ptr(d) if n else _ptr(dk), _ptr(z) if n else _ptr(zk), float(rho), C.byref(k),
         _ptr(perm), _ptr(dk), _ptr(zk), C.byref(rho_out), C.byref(nrot), _ptr(cols), _ptr(cs), C.byref(tol))
    r = int(nrot.value)
    rot = [(int(cols[2 * q]), int(cols[2 * q + 1]), float(cs[2 * q]), float(cs[2 * q + 1])) for q in range(r)]
    return dict(k=int(k.value), perm=perm[:n].copy(), dk=dk[:n].copy(), zk=zk[:n].copy(), rho=rho_out.value, rot=rot,
                tol=tol.value)


def tridiag_plan(d, e, w):
    """Host only (``eigsol_tridiag_plan``): the split blocks of the tridiagonal (d, e) and the clusters
    of its ascending eigenvalues ``w`` that :func:`eigh` uses.  Returns (block_of, cluster_of, nblocks,
    nclusters)."""
    d = np.ascontiguousarray(d, dtype=np.float64)
    e = np.ascontiguousarray(e, dtype=np.float64)
    w = np.ascontiguousarray(w, dtype=np.float64)
    n, m = d.size, w.size
    if e.size != max(n - 1, 0):
        raise EigSolError(EIGSOL_E_SIZE_MISMATCH, "tridiag_plan: e must hold n - 1 entries")
    eb = np.zeros(max(n, 1))
    eb[:e.size] = e
    bo, co = np.zeros(max(n, 1), dtype=np.int64), np.zeros(max(m, 1), dtype=np.int64)
    nb, ncl = C.c_int64(0), C.c_int64(0)
    call("eigsol_tridiag_plan", n, _ptr(d) if n else _ptr(eb), _ptr(eb), m, _ptr(w) if m else _ptr(co), _ptr(bo),
         _ptr(co), C.byref(nb), C.byref(ncl))
    return bo[:n], co[:m], int(nb.value), int(ncl.value)


def hyman_refine(ctx: Context, H, starts):
    """Diagnostic (``eigsol_hyman_refine``): the long double Francis variant's refinement alone, on
    the upper-Hessenberg long double / complex long double matrix ``H`` from the values ``starts``.
    A float64 / complex128 ``H`` is taken as the long double matrix of the same values (low parts
    zero).  Returns (refined values as clongdouble, Newton steps per value with -1 = not refined)."""
    H = _square_dense(H, "hyman_refine")
    n = H.shape[0]
    if is_wide(H.dtype):
        code, Hw = _dtype_code(H.dtype), to_wire(H.ravel(order="F"), H.dtype)
    elif H.dtype in (np.float64, np.complex128):
        cx = H.dtype == np.complex128
        code = EIGSOL_CDD if cx else EIGSOL_DD
        Hw = np.zeros((n * n, 4 if cx else 2))
        Hw[:, 0] = H.real.ravel(order="F")
        if cx:
            Hw[:, 2] = H.imag.ravel(order="F")
    else:
        raise EigSolError(3, "hyman_refine: H must be (complex) long double or double")
    st = np.ascontiguousarray(starts, dtype=np.clongdouble).reshape(-1)
    cnt = len(st)
    out = wire_buffer(np.clongdouble, max(cnt, 1))
    steps = np.zeros(max(cnt, 1), dtype=np.int32)
    call("eigsol_hyman_refine", ctx.handle, code, n, _ptr(Hw), cnt, _ptr(to_wire(st, np.clongdouble)), _ptr(out),
         _ptr(steps))
    return from_wire(out, np.clongdouble)[:cnt], steps[:cnt]
