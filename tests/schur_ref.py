"""Figures, the structure check and the named matrices of the ``schur`` tests (csrc/schur.hip).

The matrices are tests/eig_ref.py's, by name, plus the cases that sit on the Schur-mode paths' edges.

Figures of a Schur form (T, Z) of A, both formed under ``eig_ref._in_range``'s exact power-of-two scaling:
    r = ||A - Z T Z^H||_F / (n eps ||A||_F)   (||A||_F replaced by 1 for a zero matrix)
    o = ||Z^H Z - I||_F / (n eps)
"""
import numpy as np

import eig_ref as R

EPS = R.EPS

_NEW = {
    "n2real": lambda: np.array([[1.0, 2.0], [3.0, 4.0]]),
    "gen96": lambda: R._gen(96, 96),
    "gen130": lambda: R._gen(130, 130),
    "gen450": lambda: R._gen(450, 450),
    "cgen64": lambda: R._gen(64, 64) + 1j * R._gen(64, 65),
    "cgen310": lambda: R._gen(310, 310) + 1j * R._gen(310, 311),
}
NAMES = ["n1", "n2rot", "n2real", "n3", "gen63", "gen64", "gen65", "gen96", "gen97", "gen130", "gen450", "gen1030",
         "cgen70", "cgen64", "cgen310", "grcar100", "jordan40", "graded60", "blk40", "kron30", "sym65", "tri30",
         "eye7", "zero5", "diag50", "gen97_big", "gen97_small"]
# every eigenvalue is compared with numpy.linalg.eigvals one to one
WELL_CONDITIONED = [k for k in NAMES if k in R.WELL_CONDITIONED or k.startswith("gen") or k.startswith("cgen")]
_cache = {}


def matrix(name):
    if name in R._BUILDERS:
        return R.matrix(name)
    if name not in _cache:
        A = np.asfortranarray(_NEW[name]())
        A.setflags(write=False)
        _cache[name] = A
    return _cache[name]


def _scaled(X, e):
    X = np.asarray(X)
    return np.ldexp(X.real, e) + 1j * np.ldexp(X.imag, e) if np.iscomplexobj(X) else np.ldexp(X, e)


def figures(A, T, Z):
    """(r, o) of the Schur form (T, Z) of A."""
    n = A.shape[0]
    e = R._in_range(A)
    As, Ts = _scaled(A, e), _scaled(T, e)
    fro = float(np.linalg.norm(As))
    if fro == 0.0:
        fro = 1.0
    r = float(np.linalg.norm(As - Z @ Ts @ Z.conj().T)) / (n * EPS * fro)
    o = float(np.linalg.norm(Z.conj().T @ Z - np.eye(n))) / (n * EPS)
    return r, o


def check_structure(T, real):
    """Raises AssertionError unless T is a Schur form's T: exact zeros below the first sub-diagonal; complex:
    upper triangular; real: no two consecutive non-zero sub-diagonal entries, and every 2 x 2 block has
    bitwise equal diagonal entries and off-diagonal entries of opposite sign."""
    T = np.asarray(T)
    n = T.shape[0]
    assert T.shape == (n, n)
    assert not np.any(np.tril(T, -2)), "a non-zero entry below the first sub-diagonal"
    sub = np.diagonal(T, -1)
    if not real:
        assert not np.any(sub), "a complex Schur form must be upper triangular"
        return
    assert not np.iscomplexobj(T)
    nz = sub != 0
    assert not np.any(nz[:-1] & nz[1:]), "two consecutive non-zero sub-diagonal entries"
    for k in np.nonzero(nz)[0]:
        assert T[k, k].tobytes() == T[k + 1, k + 1].tobytes(), f"block at {k}: unequal diagonal entries"
        # T[k + 1, k] T[k, k + 1] < 0, by the signs: the product of two entries near 2^-600 underflows to -0
        assert np.sign(T[k + 1, k]) * np.sign(T[k, k + 1]) < 0, f"block at {k}: off-diagonal entries not of opposite sign"


def block_eigenvalues(T):
    """The eigenvalues of a (quasi-)triangular T in the order of its diagonal; a standardised 2 x 2 block
    [a b; c a] gives a + i sqrt|b| sqrt|c| first, then its conjugate."""
    T = np.asarray(T)
    n = T.shape[0]
    w = np.array(np.diagonal(T), dtype=np.complex128)
    if np.iscomplexobj(T):
        return w
    k = 0
    while k + 1 < n:
        if T[k + 1, k] != 0:
            im = np.sqrt(abs(T[k, k + 1])) * np.sqrt(abs(T[k + 1, k]))
            w[k] = complex(T[k, k], im)
            w[k + 1] = complex(T[k + 1, k + 1], -im)
            k += 2
        else:
            k += 1
    return w


def value_bound(A):
    """2 n eps ||A||_F, formed without overflow"""
    e = R._in_range(A)
    return float(np.ldexp(2 * A.shape[0] * EPS * np.linalg.norm(_scaled(A, e)), -e))


def pairs_conjugate(w):
    """True where every eigenvalue with a non-zero imaginary part has its bitwise conjugate next to it (the
    eigenvalues of a real matrix)."""
    w = np.asarray(w)
    k = 0
    while k < w.size:
        if w[k].imag == 0:
            k += 1
            continue
        if k + 1 >= w.size or w[k + 1].real.tobytes() != w[k].real.tobytes() or w[k + 1].imag != -w[k].imag:
            return False
        k += 2
    return True
