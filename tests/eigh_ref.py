"""Test matrices and a CPU restatement of the symmetric / Hermitian eigensolver (eigsol_eigh_dense),
shared by tests/test_eigh_cpu.py, tests/test_gpu_eigh.py and tests/test_gpu_eigh_facade.py.

The restatement: scipy.linalg.hessenberg(calc_q=True) of the mirrored lower triangle; d_i = Re h_ii,
e_i = |h_{i+1,i}| and the unitary diagonal D of accumulated sub-diagonal phases (D_0 = 1,
D_{i+1} = D_i h_{i+1,i} / |h_{i+1,i}|, 1 where that entry is zero), so D^H H D is real with
non-negative off-diagonals; scipy.linalg.eigh_tridiagonal(lapack_driver="stebz") (bisection + dstein);
Z = Q D z.  Every matrix is seeded; references are computed once and must not be modified."""
import functools

import numpy as np
import scipy.linalg as sl

EPS = np.finfo(np.float64).eps


def _rng(seed):
    return np.random.default_rng(seed)


def _sym(n, seed):
    B = _rng(seed).standard_normal((n, n))
    return (B + B.T) / 2


def _herm(n, seed):
    g = _rng(seed)
    B = g.standard_normal((n, n)) + 1j * g.standard_normal((n, n))
    return (B + B.conj().T) / 2


def _planted(lam, seed):
    n = lam.size
    Q, _ = np.linalg.qr(_rng(seed).standard_normal((n, n)))
    A = (Q * lam) @ Q.T
    return (A + A.T) / 2


def _wilkinson(m):
    n = 2 * m + 1
    return np.diag(np.abs(np.arange(-m, m + 1)).astype(float)) + np.diag(np.ones(n - 1), 1) + np.diag(np.ones(n - 1), -1)


def _laplacian(n):
    return 2 * np.eye(n) - np.diag(np.ones(n - 1), 1) - np.diag(np.ones(n - 1), -1)


def _blockdiag():
    A = np.zeros((64, 64))
    A[:33, :33] = _sym(33, 21)
    A[33:, 33:] = _sym(31, 22)
    return A


def cluster99_spectrum():
    return np.concatenate([np.linspace(-3, 3, 88), 1.5 + 1e-12 * np.arange(8), [0.25] * 3])


def loose72_spectrum():
    return np.concatenate([np.linspace(1, 2, 60), 5 + 1e-6 * np.arange(12)])


_BUILDERS = {
    "sym97": lambda: _sym(97, 1),
    "sym200": lambda: _sym(200, 2),
    "herm70": lambda: _herm(70, 3),
    "cluster99": lambda: _planted(cluster99_spectrum(), 4),
    "loose72": lambda: _planted(loose72_spectrum(), 5),
    "wilk21": lambda: _wilkinson(10),
    "lap300": lambda: _laplacian(300),
    "diag50": lambda: np.diag(np.round(_rng(6).standard_normal(50) * 8) / 4),
    "eye40": lambda: np.eye(40),
    "zero9": lambda: np.zeros((9, 9)),
    "blockdiag": _blockdiag,
    "rank1": lambda: np.ones((65, 65)),
    "n1": lambda: np.array([[-2.5]]),
    "n2": lambda: np.array([[1.0, -3.0], [-3.0, 0.5]]),
    "n3": lambda: _sym(3, 7),
    "sym1030": lambda: _sym(1030, 8),
}
# every matrix of the accuracy conditions (sym1030 is GPU only, with a selection)
NAMES = [k for k in _BUILDERS if k != "sym1030"]


@functools.lru_cache(maxsize=None)
def _matrix(name):
    A = _BUILDERS[name]()
    A.setflags(write=False)
    return A


def matrix(name):
    return _matrix(name)


def mirror_lower(A):
    """The Hermitian matrix whose lower triangle (diagonal's imaginary part dropped) is A's."""
    L = np.tril(A, -1)
    return L + L.conj().T + np.diag(np.real(np.diag(A))).astype(A.dtype)


def tridiagonal(A):
    """(d, e, D, Q) of the restatement: A = Q H Q^H, D^H H D = tridiag(d, e) real, e >= 0."""
    A = mirror_lower(np.asarray(A))
    n = A.shape[0]
    if n >= 3:
        H, Q = sl.hessenberg(A, calc_q=True)
    else:
        H, Q = A.copy(), np.eye(n, dtype=A.dtype)
    d = np.real(np.diag(H)).copy()
    sub = np.diag(H, -1)
    e = np.abs(sub)
    D = np.ones(n, dtype=A.dtype)
    for i in range(n - 1):
        D[i + 1] = D[i] * (sub[i] / e[i] if e[i] != 0 else 1.0)
    return d, e, D, Q


def select_args(select):
    if select is None:
        return dict(select="a")
    if select[0] == "i":
        return dict(select="i", select_range=(int(select[1]), int(select[2])))
    return dict(select="v", select_range=(float(select[1]), float(select[2])))


def restatement(A, select=None):
    """(w, Z) by the CPU restatement, for the same selection the device call takes."""
    d, e, D, Q = tridiagonal(A)
    if d.size == 1:
        w, z = d.copy(), np.ones((1, 1))
        if select is not None and select[0] == "v" and not (select[1] < w[0] <= select[2]):
            w, z = w[:0], z[:, :0]
    else:
        w, z = sl.eigh_tridiagonal(d, e, lapack_driver="stebz", **select_args(select))
    return w, Q @ (D[:, None] * z)


@functools.lru_cache(maxsize=None)
def _reference(name):
    A = matrix(name)
    w, Z = restatement(A)
    wl = np.linalg.eigvalsh(mirror_lower(A))
    for a in (w, Z, wl):
        a.setflags(write=False)
    return w, Z, wl


def reference(name):
    """(restatement eigenvalues, restatement eigenvectors, numpy.linalg.eigvalsh eigenvalues), all of them."""
    return _reference(name)


def fro(A):
    return float(np.linalg.norm(A))


def r_figure(A, w, Z):
    """||A Z - Z diag(w)||_F / (n eps ||A||_F), ||A||_F replaced by 1 for the zero matrix."""
    A = mirror_lower(np.asarray(A))
    n = A.shape[0]
    nA = fro(A)
    if Z.shape[1] == 0:
        return 0.0
    return fro(A @ Z - Z * w) / (n * EPS * (nA if nA > 0 else 1.0))


def o_figure(Z):
    """||Z^H Z - I||_F / (n eps)."""
    n, m = Z.shape
    if m == 0:
        return 0.0
    return fro(Z.conj().T @ Z - np.eye(m)) / (n * EPS)


def value_bound(A):
    """2 n eps ||A||_F: the allowed distance of an eigenvalue from LAPACK's."""
    A = mirror_lower(np.asarray(A))
    return 2 * A.shape[0] * EPS * fro(A)
