"""Test matrices and a NumPy restatement of the generalised symmetric-definite eigensolver
(eigsol_geigh_dense: A x = lambda B x) and of the Cholesky factorisation (eigsol_cholesky_dense), shared by
tests/test_geigh_cpu.py, tests/test_gpu_cholesky.py, tests/test_gpu_geigh.py and tests/test_gpu_geigh_facade.py.

The restatement: L = numpy.linalg.cholesky(B); W = solve(L, A); C = solve(L, W^H)^H with its lower triangle
mirrored; (w, Y) = eigh_ref.restatement(C, select); X = solve(L^H, Y).  Reference eigenvalues:
numpy.linalg.eigvalsh(C).  Every matrix is seeded; references are computed once and must not be modified.

Figures:
    r = ||A X - B X diag(w)||_F / (n eps (||A||_F + max|w| ||B||_F) ||X||_F)
    o = ||X^H B X - I||_F / (n eps cond_2(B))
    value bound = 2 n eps ||B^-1||_2 (||A||_F + max|w| ||B||_F)
    c = ||L L^H - B||_F / (n eps ||B||_F)"""
import functools

import numpy as np

import eigh_ref

EPS = np.finfo(np.float64).eps


def _rng(seed):
    return np.random.default_rng(seed)


def _spd(n, kappa, seed, cplx=False):
    """Q diag(logspace(0, -log10 kappa)) Q^H with a seeded orthogonal / unitary Q."""
    g = _rng(seed)
    M = g.standard_normal((n, n))
    if cplx:
        M = M + 1j * g.standard_normal((n, n))
    Q, _ = np.linalg.qr(M)
    B = (Q * np.logspace(0, -np.log10(kappa), n)) @ Q.conj().T
    return (B + B.conj().T) / 2


def _lap_pair(n):
    A = 2 * np.eye(n) - np.diag(np.ones(n - 1), 1) - np.diag(np.ones(n - 1), -1)
    B = (4 * np.eye(n) + np.diag(np.ones(n - 1), 1) + np.diag(np.ones(n - 1), -1)) / 6
    return A, B


def gdiag50_ab():
    return np.arange(1, 51) % 7 - 3.0, 4.0 ** (np.arange(50) % 5 - 2)


def glap300_closed_form():
    th = np.arange(1, 301) * np.pi / 301
    return (2 - 2 * np.cos(th)) / ((4 + 2 * np.cos(th)) / 6)


_BUILDERS = {
    "gsym97": lambda: (eigh_ref._sym(97, 101), _spd(97, 10.0, 102)),
    "gherm70": lambda: (eigh_ref._herm(70, 103), _spd(70, 10.0, 104, cplx=True)),
    "gcond130": lambda: (eigh_ref._sym(130, 105), _spd(130, 1e6, 106)),
    "gsym200": lambda: (eigh_ref._sym(200, 107), _spd(200, 100.0, 108)),
    "glap300": lambda: _lap_pair(300),
    "gdiag50": lambda: tuple(np.diag(v) for v in gdiag50_ab()),
}
NAMES = list(_BUILDERS)


@functools.lru_cache(maxsize=None)
def _pair(name):
    A, B = _BUILDERS[name]()
    A.setflags(write=False)
    B.setflags(write=False)
    return A, B


def pair(name):
    """(A, B) of the named problem (read-only)."""
    return _pair(name)


def spd(n, kappa, seed, cplx=False):
    B = _spd(n, kappa, seed, cplx)
    B.setflags(write=False)
    return B


def standard_form(A, B):
    """(L, C): B = L L^H and C = L^-1 A L^-H with its lower triangle mirrored."""
    A, B = eigh_ref.mirror_lower(np.asarray(A)), eigh_ref.mirror_lower(np.asarray(B))
    L = np.linalg.cholesky(B)
    W = np.linalg.solve(L, A)
    C = np.linalg.solve(L, W.conj().T).conj().T
    return L, eigh_ref.mirror_lower(C)


def restatement(A, B, select=None):
    """(w, X) by the NumPy restatement, for the same selection the device call takes."""
    L, C = standard_form(A, B)
    w, Y = eigh_ref.restatement(C, select)
    return w, np.linalg.solve(L.conj().T, Y)


@functools.lru_cache(maxsize=None)
def _reference(name):
    A, B = pair(name)
    w, X = restatement(A, B)
    wl = np.linalg.eigvalsh(standard_form(A, B)[1])
    for a in (w, X, wl):
        a.setflags(write=False)
    return w, X, wl


def reference(name):
    """(restatement eigenvalues, restatement eigenvectors, numpy.linalg.eigvalsh(C) eigenvalues), all of them."""
    return _reference(name)


def fro(M):
    return float(np.linalg.norm(M))


def _scale(A, B, w):
    wmax = float(np.abs(w).max()) if np.size(w) else 0.0
    return fro(A) + wmax * fro(B)


def r_figure(A, B, w, X):
    A, B = eigh_ref.mirror_lower(np.asarray(A)), eigh_ref.mirror_lower(np.asarray(B))
    if X.shape[1] == 0:
        return 0.0
    return fro(A @ X - (B @ X) * w) / (A.shape[0] * EPS * _scale(A, B, w) * fro(X))


def o_figure(B, X):
    B = eigh_ref.mirror_lower(np.asarray(B))
    m = X.shape[1]
    if m == 0:
        return 0.0
    return fro(X.conj().T @ B @ X - np.eye(m)) / (B.shape[0] * EPS * float(np.linalg.cond(B, 2)))


def value_bound(A, B, w_all):
    """2 n eps ||B^-1||_2 (||A||_F + max|lambda| ||B||_F), max over all the eigenvalues."""
    A, B = eigh_ref.mirror_lower(np.asarray(A)), eigh_ref.mirror_lower(np.asarray(B))
    binv = 1.0 / float(np.linalg.eigvalsh(B)[0])
    return 2 * A.shape[0] * EPS * binv * _scale(A, B, w_all)


def c_figure(B, L):
    """||L L^H - B||_F / (n eps ||B||_F) against the mirrored lower triangle of B."""
    B = eigh_ref.mirror_lower(np.asarray(B))
    return fro(L @ L.conj().T - B) / (B.shape[0] * EPS * fro(B))


def check_phase(X):
    """Every column's largest-modulus component (the first on ties) is real and positive."""
    for j in range(X.shape[1]):
        z = X[:, j]
        a = np.abs(z)
        if np.isrealobj(z):
            assert z[int(np.argmax(a))] > 0
        else:   # moduli are rounded: any component within rounding of the largest
            near = np.nonzero(a >= a.max() * (1 - 8 * EPS))[0]
            assert any(z[k].imag == 0 and z[k].real > 0 for k in near)
