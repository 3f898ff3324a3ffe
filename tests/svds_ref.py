"""NumPy restatement of svds (csrc/svds.hip; algorithm in include/eigsol_hip.h): thick-restart Golub-Kahan-Lanczos
with the same steps (classical Gram-Schmidt with one reorthogonalisation against all of U and all of V, breakdown
floor m 2^-52 ||w before||), stopping test, restart rule and breakdown rules, with numpy.linalg.svd for the small
SVD.  Only the order of the floating-point sums differs (BLAS here, ordered workgroup partials there).

It also holds the named cases of the svds tests and their four figures.  With n = max(M, N), eps = 2^-52 and
den_i = tol max(s_i, eps^(2/3) s_0) + n eps s_0:
    r   = max residual_i / den_i          e   = max |s_i - s_i^reference| / den_i
    o_u = ||U^H U - I||_F / (n eps)        o_v = ||V^H V - I||_F / (n eps)
The reference values are LAPACK's (numpy.linalg.svd); for `big` (20000 x 3000: a dense SVD takes minutes) they
are the roots of the leading eigenvalues of the Gram matrix A^H A from numpy.linalg.eigvalsh, whose error for the
values asked for, all within a factor 2 of s_0, is a few eps s_0: far below the n eps s_0 in den.

`python tests/svds_ref.py` rewrites tests/golden/svds_ref_figures.json.
"""
import functools
import json
import os

import numpy as np

EPS = 2.0 ** -52
TOL = 1e-10
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "svds_ref_figures.json")

# name -> (shape, nsv, ncv)
CASES = {
    "sp_tall": ((600, 257), 4, 20),
    "sp_wide": ((257, 600), 4, 20),
    "planted": ((300, 129), 6, 20),
    "cluster": ((300, 129), 4, 20),
    "rank3": ((200, 90), 2, 8),
    "rank3k3": ((200, 90), 3, 8),
    "graded": ((300, 64), 5, 16),
    "slow": ((300, 129), 3, 12),
}
BIG = ((20000, 3000), 4, 20)
DTYPES = (np.float64, np.complex128)


def _randn(rng, shape, dtype):
    a = rng.standard_normal(shape)
    if dtype == np.complex128:
        a = a + 1j * rng.standard_normal(shape)
    return a.astype(dtype)


def _with_sigma(rng, shape, sigma, dtype):
    M, N = shape
    P, _ = np.linalg.qr(_randn(rng, (M, N), dtype))
    Q, _ = np.linalg.qr(_randn(rng, (N, N), dtype))
    return (P * np.asarray(sigma)) @ Q.conj().T


@functools.lru_cache(maxsize=None)
def matrix(name, dtype):
    """The named case as a dense read-only array (the sparse cases hold their zeros)."""
    dtype = np.dtype(dtype).type
    shape = CASES[name][0]
    if name == "sp_wide":
        A = np.ascontiguousarray(matrix("sp_tall", dtype).conj().T)
    elif name == "sp_tall":
        rng = np.random.default_rng(11)
        A = np.where(rng.random(shape) < 0.03, _randn(rng, shape, dtype), 0).astype(dtype)
    elif name == "planted":
        A = _with_sigma(np.random.default_rng(12), shape, np.r_[10.0, 9, 8, 7, 6, 5, np.linspace(1, 0.01, 123)], dtype)
    elif name == "cluster":
        A = _with_sigma(np.random.default_rng(13), shape, np.r_[5.0, 5, 5 * (1 - 1e-9), 3, np.linspace(1, 0.5, 125)], dtype)
    elif name in ("rank3", "rank3k3"):
        rng = np.random.default_rng(14)
        A = _randn(rng, (shape[0], 3), dtype) @ _randn(rng, (3, shape[1]), dtype)
    elif name == "graded":
        A = _with_sigma(np.random.default_rng(15), shape, 2.0 ** -np.arange(64), dtype)
    elif name == "slow":
        A = _with_sigma(np.random.default_rng(16), shape, np.linspace(1, 0.9, 129), dtype)
    else:
        raise KeyError(name)
    A.setflags(write=False)
    return A


def csr_arrays(A):
    """(rowptr, colidx, values) of the nonzero entries of a dense array, columns ascending in every row"""
    rows, cols = np.nonzero(A)
    rowptr = np.zeros(A.shape[0] + 1, np.int32)
    np.cumsum(np.bincount(rows, minlength=A.shape[0]), out=rowptr[1:])
    return rowptr, cols.astype(np.int32), np.ascontiguousarray(A[rows, cols])


@functools.lru_cache(maxsize=None)
def big_csr(dtype):
    """`big`: 20000 x 3000, 8 entries per row in distinct uniformly drawn columns; (rowptr, colidx, values)"""
    dtype = np.dtype(dtype).type
    (M, N), per = BIG[0], 8
    rng = np.random.default_rng(17)
    cols = np.sort(rng.integers(0, N, (M, per)), axis=1)
    while True:
        dup = np.nonzero((cols[:, 1:] == cols[:, :-1]).any(axis=1))[0]
        if dup.size == 0:
            break
        cols[dup] = np.sort(rng.integers(0, N, (dup.size, per)), axis=1)
    vals = _randn(rng, M * per, dtype)
    rowptr = (np.arange(M + 1) * per).astype(np.int32)
    return rowptr, cols.reshape(-1).astype(np.int32), vals


class CsrOp:
    """A CSR matrix with the two products the restatement needs (NumPy only)"""

    def __init__(self, rowptr, colidx, values, shape):
        self.rp, self.ci, self.v, self.shape = rowptr, colidx, values, shape
        self.rows = np.repeat(np.arange(shape[0]), np.diff(rowptr))
        self.dtype = values.dtype

    def mv(self, x):
        y = np.zeros(self.shape[0], dtype=np.result_type(self.dtype, x.dtype))
        np.add.at(y, self.rows, self.v * x[self.ci])
        return y

    def mv_h(self, x):
        y = np.zeros(self.shape[1], dtype=np.result_type(self.dtype, x.dtype))
        np.add.at(y, self.ci, self.v.conj() * x[self.rows])
        return y

    def gram(self):
        D = np.zeros(self.shape, dtype=self.dtype)
        D[self.rows, self.ci] = self.v
        return D.conj().T @ D


class DenseOp:
    def __init__(self, A):
        self.A, self.AH, self.shape, self.dtype = A, np.ascontiguousarray(A.conj().T), A.shape, A.dtype

    def mv(self, x):
        return self.A @ x

    def mv_h(self, x):
        return self.AH @ x


def start_vector(N, dtype, seed=5):
    rng = np.random.default_rng(seed)
    v0 = rng.uniform(-1, 1, N)
    if np.dtype(dtype).kind == "c":
        v0 = v0 + 1j * rng.uniform(-1, 1, N)
    return v0.astype(dtype)


def _cgs2(Q, w, floor_mult):
    """twice { c = Q^H w; w -= Q c; h += c }, then the norm: (w / beta or 0, h, beta or 0, broke)"""
    wn = np.linalg.norm(w)
    h = np.zeros(Q.shape[1], dtype=w.dtype)
    for _ in range(2):
        c = Q.conj().T @ w
        w = w - Q @ c
        h = h + c
    beta = np.linalg.norm(w)
    if not beta > floor_mult * EPS * wn:
        return np.zeros_like(w), h, 0.0, True
    return w / beta, h, beta, False


def _phase(V, U):
    for j in range(V.shape[1]):
        k = int(np.argmax(np.abs(V[:, j])))
        pm = abs(V[k, j])
        if pm > 0:
            f = np.conj(V[k, j]) / pm
            V[:, j] *= f
            V[k, j] = pm
            U[:, j] *= f


def svds(op, nsv, ncv, v0, tol=TOL, max_restarts=300):
    """dict(s, U, V, residuals, restarts, applications, converged); raises ArithmeticError on an invariant
    subspace of dimension below nsv"""
    M, N = op.shape
    m, k = ncv, nsv
    dt = op.dtype
    V = np.zeros((N, m + 1), dtype=dt)
    U = np.zeros((M, m), dtype=dt)
    B = np.zeros((m, m), dtype=dt)
    V[:, 0] = v0 / np.linalg.norm(v0)
    p, apps, conv = 0, 0, False
    dl = dr = m
    for cycle in range(1, max_restarts + 1):
        kind, jb, beta, hlast = None, m, 0.0, None
        for j in range(p, m):
            u, h, alpha, broke = _cgs2(U[:, :j], op.mv(V[:, j]), m)
            apps += 1
            if broke:
                kind, jb, hlast = "alpha", j, h
                break
            B[:j, j], B[j, j], U[:, j] = h, alpha, u
            w, _, beta, broke = _cgs2(V[:, :j + 1], op.mv_h(u), m)
            apps += 1
            V[:, j + 1] = w
            if broke:
                kind, jb = "beta", j
                break
        if kind:
            d = jb if kind == "alpha" else jb + 1
            if d < k:
                raise ArithmeticError(f"svds: invariant subspace of dimension {d} < nsv")
            C = np.c_[B[:d, :d], hlast] if kind == "alpha" else B[:d, :d]
            X, s, Yh = np.linalg.svd(C, full_matrices=False)
            Y = Yh.conj().T
            dl, dr, conv = d, C.shape[1], True
            break
        X, s, Yh = np.linalg.svd(B)
        Y = Yh.conj().T
        est = beta * np.abs(X[m - 1, :k])
        if tol >= 0 and np.all(est <= tol * np.maximum(s[:k], EPS ** (2 / 3) * s[0])):
            conv = True
            break
        if cycle == max_restarts:
            break
        p = k
        V[:, :p] = V[:, :m] @ Y[:, :p]
        U[:, :p] = U[:, :m] @ X[:, :p]
        V[:, p] = V[:, m]
        B[:] = 0
        B[np.arange(p), np.arange(p)] = s[:p]
    Uk = U[:, :dl] @ X[:, :k]
    Vk = V[:, :dr] @ Y[:, :k]
    _phase(Vk, Uk)
    res = np.array([np.hypot(np.linalg.norm(op.mv(Vk[:, i]) - s[i] * Uk[:, i]),
                             np.linalg.norm(op.mv_h(Uk[:, i]) - s[i] * Vk[:, i])) for i in range(k)])
    return dict(s=s[:k].copy(), U=Uk, V=Vk, residuals=res, restarts=cycle, applications=apps, converged=conv)


def figures(shape, s, U, V, residuals, s_ref, tol=TOL):
    """(r, e, o_u, o_v)"""
    n = max(shape)
    k = len(s)
    den = tol * np.maximum(s, EPS ** (2 / 3) * s[0]) + n * EPS * s[0]
    r = float(np.max(residuals / den))
    e = float(np.max(np.abs(s - s_ref[:k]) / den))
    o_u = float(np.linalg.norm(U.conj().T @ U - np.eye(k)) / (n * EPS))
    o_v = float(np.linalg.norm(V.conj().T @ V - np.eye(k)) / (n * EPS))
    return r, e, o_u, o_v


FIGS = ("r", "e", "o_u", "o_v")


def reference_s(name, dtype):
    """the leading singular values of the case from LAPACK (`big`: from the Gram matrix, see the module text)"""
    if name == "big":
        rp, ci, v = big_csr(dtype)
        w = np.linalg.eigvalsh(CsrOp(rp, ci, v, BIG[0]).gram())
        return np.sqrt(w[::-1][:BIG[1]])
    return np.linalg.svd(matrix(name, dtype), compute_uv=False)[:CASES[name][1]]


def operator(name, dtype):
    if name == "big":
        return CsrOp(*big_csr(dtype), BIG[0])
    return DenseOp(matrix(name, dtype))


def key(name, dtype):
    return f"{name}-{np.dtype(dtype).name}"


def run_case(name, dtype):
    """The restatement on a named case: its result, the reference values and the record the golden file pins"""
    shape, nsv, ncv = BIG if name == "big" else CASES[name]
    op = operator(name, dtype)
    res = svds(op, nsv, ncv, start_vector(shape[1], dtype))
    s_ref = reference_s(name, dtype)
    fig = figures(shape, res["s"], res["U"], res["V"], res["residuals"], s_ref)
    rec = dict(zip(FIGS, fig), restarts=res["restarts"], applications=res["applications"],
               converged=bool(res["converged"]), s_ref=[float(x) for x in s_ref])
    return res, rec


def load_golden():
    with open(GOLDEN) as f:
        return json.load(f)


# the two exact breakdown cases: (matrix, v0, ncv, applications).  fail=True: the variant on which nsv = 3
# reaches the driver (ncv >= nsv + 2 = 5 needs min(M, N) >= 5, so the alpha case grows to 7 x 5) and must fail
# there on an invariant subspace of dimension 2
def breakdown_case(kind, dtype, fail=False):
    if fail:
        A = np.zeros((7, 5), dtype=dtype)
        d = [3, 2, 1, 0.5, 0.25] if kind == "beta" else [3, 2, 0, 0, 0]
        A[np.arange(5), np.arange(5)] = d
        v0 = np.zeros(5, dtype=dtype)
        v0[:2 if kind == "beta" else 3] = 1
        return A, v0, 5, None
    if kind == "beta":
        A = np.zeros((7, 5), dtype=dtype)
        A[np.arange(5), np.arange(5)] = [3, 2, 1, 0.5, 0.25]
        v0 = np.zeros(5, dtype=dtype)
        v0[:2] = 1
        return A, v0, 4, 4
    A = np.zeros((6, 4), dtype=dtype)
    A[0, 0], A[1, 1] = 3, 2
    v0 = np.zeros(4, dtype=dtype)
    v0[:3] = 1
    return A, v0, 4, 5


if __name__ == "__main__":
    out = {}
    for nm in list(CASES) + ["big"]:
        for dt in DTYPES:
            _, rec = run_case(nm, dt)
            out[key(nm, dt)] = rec
            print(key(nm, dt), {q: (f"{rec[q]:.3g}" if q in FIGS else rec[q]) for q in rec if q != "s_ref"})
    with open(GOLDEN, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")
