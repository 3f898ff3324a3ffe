"""Host-side helpers for the Householder tests (to_hessenberg / qr_decompose): test matrices, the embedding
that makes to_hessenberg hand back its own Q, backward-error figures in long double, and reference runs in the
scalar's own precision.  numpy and the CPU oracle only.

The embedding.  With p = n + pad and C = [I_n ; 0] (p x n), reduce

    M = [ 0_p  C ]        order N = n + p
        [ 0    A ]

The first p columns are zero, so their reflectors are skipped (to_hessenberg.hpp:46-48); from column p on the
column below the diagonal is A's, so the reflectors are exactly A's; their right updates act on all N rows.
The result is [[0, C Q], [0, H]] with A = Q H Q^H: Q arrives in the top-right n x n block, made by the same
panel, GEMV and rank-k kernels that make H.  pad moves A's first column to any offset inside a panel.

Figures (eps that of A's dtype, every product in long double):

    r = ||Q H Q^H - A||_F / (n eps ||A||_F)        o = ||Q^H Q - I||_F / (n eps)                (Hessenberg)
    r = ||Q R - A||_F / (max(m, n) eps ||A||_F)    o = ||Q^H Q - I||_F / (m eps)                (QR)

The condition on a device result is r <= max(2, 3 r_ref) and o <= max(2, 3 o_ref), with "ref" the figure of
the reference algorithm run in the same precision on the same matrix (the rule of tests/test_gpu_eigh.py).
"""
import numpy as np

from oracle import oracle as O

DTYPES = (np.float64, np.complex128, np.float32, np.complex64)
KINDS = ("random", "zerotails", "blocks", "herm", "hess")
PROBE_ABOVE = 260           # hess_figures uses the 8-column probe form from n > 260


def is_complex(dtype):
    return np.issubdtype(np.dtype(dtype), np.complexfloating)


def panel_width(dtype):
    """Columns per blocked Hessenberg panel (HessCfg<S>::NB)."""
    return 16 if is_complex(dtype) else 32


def wide_type(dtype):
    return np.clongdouble if is_complex(dtype) else np.longdouble


def double_type(dtype):
    return np.complex128 if is_complex(dtype) else np.float64


def normal(rng, shape, dtype):
    A = rng.standard_normal(shape)
    if is_complex(dtype):
        A = A + 1j * rng.standard_normal(shape)
    return A


def skip_columns(n, dtype):
    """Columns of the zerotails / blocks families: a panel's first and last column, the last reflector."""
    nb = panel_width(dtype)
    return sorted({k for k in (0, 5, nb - 1, nb, n - 3) if 0 <= k <= n - 3})


def matrix(kind, n, dtype, seed):
    """Square test matrix; values are made in fp64 and then rounded to dtype.

    random     standard normal (plus 1j * normal for complex)
    zerotails  random with A[k+2:, k] = 0 for k in skip_columns and A[8, 7] = 0.  Only column 0's tail is still
               zero when its reflector is formed (the earlier reflectors' updates fill the others), so this
               family plants one true skip and otherwise exact zeros that the reduction must overwrite
    blocks     random with A[k+2:, :k+2] = 0 for k in skip_columns (block upper triangular) and A[8, 7] = 0: the
               reflectors of the leading block never touch the rows below it, so columns k and k + 1 ARE
               skipped, beside live ones; A[8, 7] is the first subdiagonal entry of the block that starts at
               column 7, so its reflector has x(0) == 0 over a live tail (sign = 1, to_hessenberg.hpp:51-55)
    herm       B + B^H
    hess       triu(random, -1): every reflector is skipped
    """
    A = normal(np.random.default_rng(seed), (n, n), dtype)
    if kind == "random":
        pass
    elif kind == "zerotails":
        for k in skip_columns(n, dtype):
            A[k + 2:, k] = 0
        if n > 9:
            A[8, 7] = 0
    elif kind == "blocks":
        for k in skip_columns(n, dtype):
            A[k + 2:, :k + 2] = 0
        if n > 9:
            A[8, 7] = 0
    elif kind == "herm":
        A = A + A.conj().T
    elif kind == "hess":
        A = np.triu(A, -1)
    else:
        raise ValueError(kind)
    return np.asfortranarray(A.astype(dtype))


def rectangle(m, n, dtype, seed):
    return np.asfortranarray(normal(np.random.default_rng(seed), (m, n), dtype).astype(dtype))


def embed(A, pad):
    """(M, p): the embedding of the module docstring."""
    n = A.shape[0]
    p = n + pad
    M = np.zeros((n + p, n + p), dtype=A.dtype, order="F")
    M[:n, p:] = np.eye(n, dtype=A.dtype)
    M[p:, p:] = A
    return M, p


def split(HM, n, p):
    """(Q, H, rest_max) of a reduced embedding; rest_max is the largest modulus outside Q's and H's blocks."""
    Q = HM[:n, p:]
    H = HM[p:, p:]
    rest = max(float(np.abs(HM[:, :p]).max()), float(np.abs(HM[n:p, p:]).max()) if p > n else 0.0)
    return Q, H, rest


def _fro(X):
    return float(np.sqrt((np.abs(X) ** 2).sum()))


def hess_figures(A, Q, H):
    """(r, o) of A = Q H Q^H; from n > PROBE_ABOVE through an 8-column probe X:
    r = ||Q (H (Q^H X)) - A X||_F / (n eps ||A||_F ||X||_F), o = ||Q^H (Q X) - X||_F / (n eps ||X||_F)."""
    n = A.shape[0]
    eps = float(np.finfo(A.dtype).eps)
    W = wide_type(A.dtype)
    Aw, Qw, Hw = A.astype(W), Q.astype(W), H.astype(W)
    QH = Qw.conj().T
    na = _fro(Aw)
    if n > PROBE_ABOVE:
        X = np.random.default_rng(1).standard_normal((n, 8)).astype(W)
        nx = _fro(X)
        r = _fro(Qw @ (Hw @ (QH @ X)) - Aw @ X) / (n * eps * na * nx)
        o = _fro(QH @ (Qw @ X) - X) / (n * eps * nx)
    else:
        r = _fro(Qw @ Hw @ QH - Aw) / (n * eps * na)
        o = _fro(QH @ Qw - np.eye(n, dtype=W)) / (n * eps)
    return r, o


def qr_figures(A, Q, R):
    """(r, o) of A = Q R, with R as returned: anything left below its diagonal counts."""
    m, n = A.shape
    eps = float(np.finfo(A.dtype).eps)
    W = wide_type(A.dtype)
    Aw, Qw, Rw = A.astype(W), Q.astype(W), R.astype(W)
    r = _fro(Qw @ Rw - Aw) / (max(m, n) * eps * _fro(Aw))
    o = _fro(Qw.conj().T @ Qw - np.eye(m, dtype=W)) / (m * eps)
    return r, o


def within_cap(fig, ref):
    return fig <= max(2.0, 3.0 * ref)


# ------------------------------------------------------------------ the reference's loops, in the array's dtype
def _norm(x):
    """||x||_2 summed in x's own precision.  Sums and products are spelled out with numpy reductions rather
    than BLAS calls, whose summation order depends on the operands' alignment: the loop then gives the same
    bits for the same columns wherever they sit in a larger matrix."""
    return np.sqrt((x.real * x.real + x.imag * x.imag).sum())


def _vh_times(v, B):
    return (v.conj()[:, None] * B).sum(axis=0)


def _times_v(B, v):
    return (B * v[None, :]).sum(axis=1)


def reflector(x):
    """to_hessenberg.hpp:42-66 / qr_decompose.hpp:51-74: the unit v of I - 2 v v^H, or None on the two
    'continue' guards.  Every value stays in x's dtype."""
    t = x.dtype.type
    if x.size < 2 or _norm(x[1:]) == 0:
        return None
    norm_x = _norm(x)
    sign = t(1)
    if x[0] != 0:
        sign = x[0] / t(abs(x[0]))
    alpha = -sign * t(norm_x)
    v = x.copy()
    v[0] -= alpha
    vnorm = _norm(v)
    if vnorm == 0:
        return None
    v /= t(vnorm)
    assert v.dtype == x.dtype
    return v


def hess_loop(A, reflectors=None):
    """to_hessenberg.hpp:38-77 as a numpy loop in A's dtype: skip on a zero tail, sign = x0 / |x0| or 1,
    normalised v, left update then right update.  reflectors (a list) receives (k, v) of every live step."""
    H = np.array(A, order="F", copy=True)
    n = H.shape[0]
    two = H.dtype.type(2)
    for k in range(n - 2):
        v = reflector(H[k + 1:, k])
        if v is None:
            continue
        if reflectors is not None:
            reflectors.append((k, v))
        left = H[k + 1:, k:]
        left -= two * np.outer(v, _vh_times(v, left))
        right = H[:, k + 1:]
        right -= two * np.outer(_times_v(right, v), v.conj())
    assert H.dtype == A.dtype
    return H


def qr_loop(A, reflectors=None):
    """qr_decompose.hpp:46-85 as a numpy loop in A's dtype; returns (Q, R)."""
    R = np.array(A, order="F", copy=True)
    m, n = R.shape
    Q = np.eye(m, dtype=R.dtype, order="F")
    two = R.dtype.type(2)
    for k in range(min(m, n)):
        v = reflector(R[k:, k])
        if v is None:
            continue
        if reflectors is not None:
            reflectors.append((k, v))
        sub = R[k:, k:]
        sub -= two * np.outer(v, _vh_times(v, sub))
        right = Q[:, k:]
        right -= two * np.outer(_times_v(right, v), v.conj())
    assert Q.dtype == A.dtype and R.dtype == A.dtype
    return Q, R


def is_single(dtype):
    return np.dtype(dtype) in (np.dtype(np.float32), np.dtype(np.complex64))


def reference_hess(M):
    """The reference reduction in M's own precision: the oracle for f64 / c128; for f32 / c64, which the oracle
    library does not instantiate, the numpy loop above."""
    return hess_loop(M) if is_single(M.dtype) else O.hessenberg(M)


def reference_qr(A):
    return qr_loop(A) if is_single(A.dtype) else O.qr_decompose(A)


def align_phases(H, Href):
    """Href under the diagonal unitary similarity D Href D^H that gives it H's subdiagonal phases, and D's
    diagonal d (d_0 = 1; +-1 for real matrices).  The reference's reflector takes its sign / phase from x0, and
    where |x0| / ||x|| is below the working precision two precisions legitimately choose opposite reflectors;
    the Hessenberg forms then differ by such a D.  A zero subdiagonal entry on either side keeps d."""
    n = H.shape[0]
    Hd, Hr = H.astype(np.complex128), Href.astype(np.complex128)
    d = np.ones(n, np.complex128)
    for i in range(n - 1):   # h(i+1, i) = d(i+1) h_ref(i+1, i) conj(d(i))
        a, b = Hd[i + 1, i], Hr[i + 1, i]
        d[i + 1] = d[i] if a == 0 or b == 0 else d[i] * (a / abs(a)) / (b / abs(b))
    if not is_complex(H.dtype):
        d = np.where(d.real < 0, -1.0, 1.0).astype(np.complex128)
    out = d[:, None] * Hr * np.conj(d)[None, :]
    return (out if is_complex(H.dtype) else out.real), d


# ------------------------------------------------------------------ the cases of the GPU and CPU tests
# (n, pad): N = 2 n + pad is the order the device reduces
HESS_EMBEDDED = [(20, 0), (31, 1), (32, 0), (32, 1), (33, 0), (33, 1), (65, 3), (130, 0), (260, 7)]
HESS_EMBEDDED_LARGE = [(600, 0), (1050, 0)]          # f64 / c128, random, probe form
HESS_EMBEDDED_KINDS = ("random", "zerotails", "blocks", "herm")
HESS_FALLBACK = [(32, 0), (33, 1), (65, 3), (130, 0)]
HESS_DIRECT = [3, 20, 63, 64, 65, 66, 67, 130]
HESS_DIRECT_KINDS = ("random", "zerotails", "blocks")
HESS_ALREADY = [20, 64, 97]
REFERENCE_LIMIT = 600                                 # above it only r <= 2 and o <= 2 apply

QR_UNBLOCKED = [(1, 5), (5, 1), (40, 40), (300, 40), (40, 300), (63, 63)]
QR_BLOCKED = [(64, 64), (65, 65), (96, 64), (255, 97)]
QR_COOP = [(256, 64), (256, 256), (257, 65), (300, 96), (520, 130)]
QR_NO_COOP = [(257, 65), (300, 96)]


def seed_of(*parts):
    """A fixed seed per case (Python's hash of a str changes from run to run)."""
    s = 0
    for c in "/".join(str(p) for p in parts):
        s = (s * 131 + ord(c)) % (2 ** 31 - 1)
    return s


def dtype_name(dtype):
    return {"float64": "f64", "complex128": "c128", "float32": "f32", "complex64": "c64"}[np.dtype(dtype).name]
