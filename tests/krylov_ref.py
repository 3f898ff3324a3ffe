"""numpy restatement of the Krylov-Schur solver (csrc/krylov.hip) and the test matrices it is pinned
on.  Same steps, the same stopping test and the same restart rule as the device driver; the rounding
of the reductions, eig(B) (numpy.linalg.eig here, the library's own small QR there) and the way the
orthonormal restart basis Q is computed (an SVD here, a pivoted Gram-Schmidt there) differ.  The
shift-invert operator is scipy's sparse LU."""
import functools

import numpy as np
import scipy.sparse as sp
import scipy.sparse.linalg as spla

from subspace_ref import CASES as SUBSPACE_CASES, N, match_error, ritz_order  # noqa: F401

TOL = 1e-10
MAX_RESTARTS = 300
EPS23 = (2.0 ** -52) ** (2.0 / 3.0)


class InvariantSubspace(Exception):
    """Breakdown with an invariant subspace smaller than nev."""


def operator(A, sigma):
    """w = Op v: A v, or (A - sigma I)^-1 v through one sparse LU."""
    if sigma is None:
        return lambda v: A @ v
    lu = spla.splu(sp.csc_matrix(A - sigma * sp.identity(A.shape[0], dtype=A.dtype)))
    return lu.solve


def restart_size(theta, k, real):
    """p = k, or k + 1 when a real matrix's theta_{k-1}, theta_k are a conjugate pair."""
    if real and theta[k - 1].imag > 0 and abs(theta[k] - np.conj(theta[k - 1])) <= 1e-8 * abs(theta[k - 1]):
        return k + 1
    return k


def restart_basis(Yp, real):
    """Orthonormal basis (matrix dtype) of span(Yp); for a real matrix of [Re Yp, Im Yp], rank p."""
    p = Yp.shape[1]
    if real:
        U, _, _ = np.linalg.svd(np.hstack([Yp.real, Yp.imag]), full_matrices=False)
        return U[:, :p]
    Q, _ = np.linalg.qr(Yp)
    return Q


def krylov_schur(A, k, m, v0, sigma=None, tol=TOL, max_restarts=MAX_RESTARTS):
    """Returns dict(eigenvalues, eigenvectors, residuals, restarts, applications, converged)."""
    n = A.shape[0]
    real = not np.iscomplexobj(A)
    dt = np.float64 if real else np.complex128
    op = operator(A, sigma)
    V = np.zeros((n, m + 1), dtype=dt)
    S = np.zeros((m + 1, m), dtype=dt)
    V[:, 0] = np.asarray(v0, dtype=dt) / np.linalg.norm(v0)
    p = 0
    apps = 0
    conv = False
    d = m
    cycle = 0
    for cycle in range(1, max_restarts + 1):
        broke = None
        for j in range(p, m):
            w = op(V[:, j])
            apps += 1
            wn = np.linalg.norm(w)
            h = np.zeros(j + 1, dtype=dt)
            for _ in range(2):
                c = V[:, :j + 1].conj().T @ w
                w = w - V[:, :j + 1] @ c
                h += c
            beta = np.linalg.norm(w)
            S[:j + 1, j] = h
            if beta <= m * 2.0 ** -52 * wn:
                broke = j
                break
            S[j + 1, j] = beta
            V[:, j + 1] = w / beta
        d = m if broke is None else broke + 1
        B, b = S[:d, :d], (S[d, :d] if broke is None else np.zeros(d, dtype=dt))
        theta, Y = np.linalg.eig(B)
        order = ritz_order(theta)
        theta, Y = theta[order].astype(complex), Y[:, order].astype(complex)
        if broke is not None:
            if d < k:
                raise InvariantSubspace(d)
            conv = True
            break
        est = np.abs(b @ Y)
        if tol >= 0 and np.all(est[:k] <= tol * np.maximum(EPS23, np.abs(theta[:k]))):
            conv = True
            break
        if cycle == max_restarts:
            break
        p = restart_size(theta, k, real)
        Q = restart_basis(Y[:, :p], real).astype(dt)
        V[:, :p] = V[:, :m] @ Q
        V[:, p] = V[:, m]
        Snew = np.zeros_like(S)
        Snew[:p, :p] = Q.conj().T @ B @ Q
        Snew[p, :p] = b @ Q
        S = Snew
    lam = theta[:k] if sigma is None else sigma + 1.0 / theta[:k]
    X = V[:, :d] @ Y[:, :k]
    X = X / np.linalg.norm(X, axis=0)
    res = np.linalg.norm(A @ X - X * lam, axis=0)
    return dict(eigenvalues=lam, eigenvectors=X, residuals=res, restarts=cycle, applications=apps, converged=conv)


# ------------------------------------------------------------------ the pinned inputs
def lap():
    """tridiag(-1, 2, -1) + diag(linspace(0, 1, N)): a spectrum without a gap."""
    return (sp.diags([-np.ones(N - 1), 2 * np.ones(N), -np.ones(N - 1)], [-1, 0, 1])
            + sp.diags(np.linspace(0, 1, N))).tocsr()


def pair():
    """Real nonsymmetric; the eigenvalues nearest 2.2 are the pair 2 +- 0.5i of the leading block."""
    rng = np.random.default_rng(401)
    h = N // 2
    d = np.concatenate([rng.uniform(-3, 1.5, h), rng.uniform(2.9, 6, N - h)])
    D = sp.lil_matrix((N, N))
    D.setdiag(d)
    D[0, 0], D[0, 1], D[1, 0], D[1, 1] = 2, .5, -.5, 2
    S = sp.random(N, N, density=4 / N, random_state=np.random.default_rng(402), format="csr")
    return (D.tocsr() + 0.05 * S).tocsr()


def _start(seed, cplx=False):
    r = np.random.default_rng(seed)
    v = r.uniform(-1, 1, N)
    return v + 1j * r.uniform(-1, 1, N) if cplx else v


MATRICES = {
    "a": lambda: SUBSPACE_CASES["a"]()[0],
    "b": lambda: SUBSPACE_CASES["b"]()[0],
    "c": lambda: SUBSPACE_CASES["c"]()[0].astype(np.complex128),
    "lap": lap,
    "pair": pair,
}

# name -> (matrix, k, m, sigma, seed of the start vector)
CASES = {
    "a_lm": ("a", 4, 20, None, 501),
    "b_lm": ("b", 4, 20, None, 502),
    "c_lm": ("c", 4, 20, None, 503),
    "lap_lm": ("lap", 4, 24, None, 504),
    "lap_si": ("lap", 4, 20, 0.0, 505),
    "pair_si_k1": ("pair", 1, 20, 2.2, 506),
    "pair_si_k2": ("pair", 2, 20, 2.2, 506),
    "pair_si_k3": ("pair", 3, 20, 2.2, 506),
    "pair_si_k5": ("pair", 5, 20, 2.2, 506),
    "b_si": ("b", 3, 20, 7.5, 507),
}


@functools.lru_cache(maxsize=None)
def matrix(key):
    return MATRICES[key]()


@functools.lru_cache(maxsize=None)
def spectrum(key):
    """Every eigenvalue by numpy.linalg.eigvals: computed once per matrix."""
    return np.linalg.eigvals(matrix(key).toarray())


def case(name):
    """(A, k, m, sigma, v0)."""
    key, k, m, sigma, seed = CASES[name]
    A = matrix(key)
    return A, k, m, sigma, _start(seed, np.iscomplexobj(A))


def wanted(name):
    """The k eigenvalues of largest modulus, or nearest sigma, of the case's matrix."""
    key, k, _, sigma, _ = CASES[name]
    w = spectrum(key)
    return w[np.argsort(-abs(w) if sigma is None else abs(w - sigma))][:k]


@functools.lru_cache(maxsize=None)
def reference(name):
    """The restatement's run of the case: computed once."""
    A, k, m, sigma, v0 = case(name)
    return krylov_schur(A, k, m, v0, sigma)


def fold(z):
    """Eigenvalues mapped to the closed upper half plane.  The spectrum of a real matrix is closed
    under conjugation, so where nev cuts a conjugate pair either member is a right answer: values of
    a real matrix are compared after this map."""
    z = np.asarray(z, dtype=complex)
    return z.real + 1j * np.abs(z.imag)


def eigenvalue_error(name, got):
    """match_error of got against numpy's wanted eigenvalues (folded for a real matrix)."""
    want = wanted(name)
    if not np.iscomplexobj(matrix(CASES[name][0])):
        got, want = fold(got), fold(want)
    return match_error(got, want)


def breakdown_case(n=300):
    """(A, v0, eigenvalues of the block): block-diagonal, v0 supported on the leading 5 x 5 block, so
    the Krylov space of v0 is that block's invariant subspace and step 4 breaks down."""
    rng = np.random.default_rng(601)
    T = np.diag([9.0, -7.0, 5.0, 3.0, 1.0]) + np.triu(rng.uniform(-1, 1, (5, 5)), 1)
    P, _ = np.linalg.qr(rng.uniform(-1, 1, (5, 5)))
    rest = sp.diags(rng.uniform(-2, 2, n - 5)) + 0.05 * sp.random(n - 5, n - 5, density=4 / n,
                                                                  random_state=np.random.default_rng(602))
    A = sp.block_diag([sp.csr_matrix(P @ T @ P.T), rest]).tocsr()
    v0 = np.zeros(n)
    v0[:5] = rng.uniform(-1, 1, 5)
    return A, v0, np.array([9.0, -7.0, 5.0, 3.0, 1.0])
