"""Figures, cases and the NumPy restatements for the matrix logarithm tests (csrc/logm.hip).

The method is the Schur-Pade inverse scaling and squaring logarithm (Higham, Functions of Matrices, Alg. 11.9, with
the bounds theta_1 .. theta_7 of Al-Mohy and Higham (2012) applied to the 1-norm): square roots of the
(quasi-)triangular T until ||T^(1/2^s) - I||_1 allows a Pade degree m <= 7 (``plan``), the approximant of
log(I + R) through its partial fractions sum_j alpha_j (I + beta_j R)^-1 R with the m-point Gauss-Legendre rule on
[0, 1] (``NODES``), L = 2^s r_m(R), and the diagonal blocks and the super-diagonal entries between two 1 x 1 blocks
recomputed from T itself (``log_scalar``, ``log_block2``, ``superdiag_entry``).

``trlogm_ref(T)`` restates the device's schedule: the partition of sylvester_ref.starts, the roots by
sqrtm_ref.trsqrt_ref, explicitly inverted diagonal blocks W_ji = (I + beta_j R_ii)^-1, the block super-diagonals in
order with k ascending, the sum over j ascending.  ``logm_unblocked(T)`` is the same algorithm with the roots of
sqrtm_ref.sqrt_recurrence and plain triangular solves.  Both return (L, roots, degree).

Figure of a logarithm X of A (``figure_e``):
    e = ||exp(X) - A||_F / (n eps ||A||_F),   exp by expm_ref.expm_2005,
so nothing in it comes from the code under test or from SciPy.  e is not a backward error: exp amplifies the error
of X by up to ||X|| cond(exp, X), which is why the bound is taken relative to a reference's e on the same case:
    e <= max(2, 3 x the reference's e)   (``bound``),
the reference being ``logm_unblocked`` on the triangular cases and ``scipy.linalg.logm`` on the full ones.
tests/test_logm_cpu.py records them in tests/golden/logm_ref_figures.json, with ``mp_gap``: the distance of both
references to the logarithm recomputed in mpmath at 50 digits (``mp_log``), on the cases of order <= 65.

The cases are those of tests/sqrtm_ref.py: ``TRI_ALL`` for the triangular stage, the named full cases of order
<= 200 (``NAMES``; none of them is singular), ``NEEDS_COMPLEX`` for the real matrices whose logarithm is complex.
"""
import json
import math
import os

import numpy as np

import expm_ref as X5
import sqrtm_ref as Q
import sylvester_ref as Y

EPS = Q.EPS
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ACCURACY_JSON = os.path.join(ROOT, "profiles", "logm_accuracy.json")
GOLDEN = os.path.join(ROOT, "tests", "golden", "logm_ref_figures.json")
_figures = {}

THETA = (1.59e-5, 2.31e-3, 1.94e-2, 6.21e-2, 1.28e-1, 2.06e-1, 2.88e-1)
MAX_ROOTS = 64
# m: (beta_1 .. beta_m, alpha_1 .. alpha_m): nodes and weights of the m-point Gauss-Legendre rule on [0, 1]
NODES = {
    1: ((0.5,), (1.0,)),
    2: ((0.21132486540518712, 0.78867513459481288), (0.5, 0.5)),
    3: ((0.11270166537925831, 0.5, 0.88729833462074169),
        (0.27777777777777778, 0.44444444444444444, 0.27777777777777778)),
    4: ((0.069431844202973712, 0.33000947820757187, 0.66999052179242813, 0.93056815579702629),
        (0.17392742256872693, 0.32607257743127307, 0.32607257743127307, 0.17392742256872693)),
    5: ((0.046910077030668004, 0.23076534494715845, 0.5, 0.76923465505284155, 0.953089922969332),
        (0.11846344252809454, 0.23931433524968323, 0.28444444444444444, 0.23931433524968323, 0.11846344252809454)),
    6: ((0.033765242898423986, 0.16939530676686774, 0.38069040695840155, 0.61930959304159845, 0.83060469323313226,
         0.96623475710157601),
        (0.085662246189585173, 0.1803807865240693, 0.23395696728634552, 0.23395696728634552, 0.1803807865240693,
         0.085662246189585173)),
    7: ((0.025446043828620738, 0.12923440720030278, 0.29707742431130142, 0.5, 0.70292257568869858,
         0.87076559279969722, 0.97455395617137926),
        (0.064742483084434847, 0.13985269574463833, 0.19091502525255947, 0.20897959183673469, 0.19091502525255947,
         0.13985269574463833, 0.064742483084434847)),
}


def record(key, **kw):
    """One case's measured figures into profiles/logm_accuracy.json (the GPU tests of both files)."""
    if not _figures and os.path.exists(ACCURACY_JSON):   # a partial run keeps the other cases' figures
        with open(ACCURACY_JSON) as f:
            _figures.update(json.load(f))
    _figures[key] = {k: float(v) for k, v in kw.items()}
    os.makedirs(os.path.dirname(ACCURACY_JSON), exist_ok=True)
    with open(ACCURACY_JSON, "w") as f:
        json.dump(_figures, f, indent=1, sort_keys=True)
        f.write("\n")


def golden():
    with open(GOLDEN) as f:
        return json.load(f)


def figure_e(A, X):
    A = np.asarray(A)
    n = A.shape[0]
    with np.errstate(all="ignore"):
        E = X5.expm_2005(np.asarray(X))[0]
        num = float(np.linalg.norm(E - A))
    den = float(np.linalg.norm(A))
    return num / (n * EPS * (den if den else 1.0)) if np.isfinite(num) else float("inf")


def bound(ref_e):
    return max(2.0, 3.0 * ref_e)


def gap(Xa, Xb):
    den = np.linalg.norm(Xb)
    return float(np.linalg.norm(Xa - Xb) / (den if den else 1.0))


# ------------------------------------------------------------------ the plan
def plan(norm, tried):
    """The degree for ||R||_1 = norm, or 0: take another root.  ``tried``: the test j1 - j2 <= 1 was reached
    before (after which the next visit stops whatever it finds)."""
    if not norm <= THETA[6]:
        return 0
    j1 = next(m for m in range(1, 8) if norm <= THETA[m - 1])
    j2 = next(m for m in range(1, 8) if norm / 2.0 <= THETA[m - 1])
    return j1 if (j1 - j2 <= 1 or tried) else 0


def norm1(A):
    return float(np.abs(A).sum(axis=0).max()) if A.size else 0.0


# ------------------------------------------------------------------ the scalar formulas (small_log.hpp)
def log_modulus(x, y):
    """ln sqrt(x^2 + y^2), through log1p near the unit circle as small_log.hpp: log(hypot) alone loses the relative
    accuracy of a logarithm near 0 to the rounding of the modulus"""
    big, small = max(abs(x), abs(y)), min(abs(x), abs(y))
    if 0.5 < big < 2.0 and small < 2.0:
        d = (big - 1.0) * (big + 1.0) + small * small
        if -0.5 < d < 1.0:
            return 0.5 * math.log1p(d)
    return math.log(math.hypot(x, y))


def log_scalar(t):
    """principal logarithm; complex: an imaginary part of -0.0 counts as +0.0"""
    if isinstance(t, complex) or np.iscomplexobj(t):
        t = complex(t)
        return complex(log_modulus(t.real, t.imag), math.atan2(t.imag + 0.0, t.real))
    return math.log(t)


def log_block2(B):
    """the logarithm of a real 2 x 2 block with eigenvalues a +- i mu, mu > 0"""
    a = (B[0, 0] + B[1, 1]) / 2.0
    d = (B[0, 0] - B[1, 1]) / 2.0
    mu2 = -(d * d + B[0, 1] * B[1, 0])
    assert mu2 > 0
    mu = math.sqrt(mu2)
    M = np.array([[d, B[0, 1]], [B[1, 0], -d]])
    return log_modulus(a, mu) * np.eye(2) + (math.atan2(mu, a) / mu) * M


def superdiag_entry(l1, l2, t12):
    """the (1, 2) entry of log [l1 t12; 0 l2] (Al-Mohy and Higham 2012, eq. 5.6)"""
    cx = any(isinstance(v, complex) or np.iscomplexobj(v) for v in (l1, l2, t12))
    if l1 == l2:
        return t12 / l1
    if abs(l2 - l1) > abs(l1 + l2) / 2.0:
        return t12 * (log_scalar(l2) - log_scalar(l1)) / (l2 - l1)
    z = (l2 - l1) / (l2 + l1)
    if not cx:
        return t12 * 2.0 * math.atanh(z) / (l2 - l1)
    w = log_scalar(l2) - log_scalar(l1)
    u = math.ceil((w.imag - math.pi) / (2.0 * math.pi))
    return t12 * 2.0 * (np.arctanh(complex(z)) + 1j * math.pi * u) / (l2 - l1)


def _recompute(L, T0):
    """the diagonal blocks of L and the super-diagonal entries between two 1 x 1 blocks, from T0"""
    n = T0.shape[0]
    g = Q.groups(T0)
    one = np.zeros(n + 1, dtype=bool)
    for k in range(len(g) - 1):
        a, b = g[k], g[k + 1]
        if b - a == 1:
            one[a] = True
            L[a, a] = log_scalar(T0[a, a])
        else:
            L[a:b, a:b] = log_block2(T0[a:b, a:b])
    for k in range(n - 1):
        if one[k] and one[k + 1]:
            L[k, k + 1] = superdiag_entry(T0[k, k], T0[k + 1, k + 1], T0[k, k + 1])
    L[~Q.quasi_mask(T0)] = 0
    return L


def check_input(T):
    T = np.asarray(T)
    g = Q.groups(T)
    for k in range(len(g) - 1):
        if g[k + 1] - g[k] == 1 and T[g[k], g[k]] == 0:
            raise ZeroDivisionError(f"row {g[k]}: a zero eigenvalue")


def _ising(T, root, pade):
    """(L, roots, degree): roots by ``root`` until the plan stops, then ``pade(R, m)``, scaling and the
    recomputed diagonal"""
    T0 = np.array(T, order="F")
    check_input(T0)
    n = T0.shape[0]
    I = np.eye(n, dtype=T0.dtype)
    U, s, tried = T0, 0, False
    while True:
        R = U - I
        nr = norm1(R)
        if nr == 0.0:
            return np.zeros_like(T0), s, 0
        m = plan(nr, tried)
        if m:
            break
        tried = tried or nr <= THETA[6]
        if s == MAX_ROOTS:
            raise ArithmeticError("more than 64 square roots")
        U = root(U)
        s += 1
    L = pade(R, m) * math.ldexp(1.0, s)
    return _recompute(np.asfortranarray(L), T0), s, m


def _pade_blocked(R, m):
    st = Y.starts(R)
    p = len(st) - 1
    sl = [slice(st[b], st[b + 1]) for b in range(p)]
    beta, alpha = NODES[m]
    L = np.zeros_like(R)
    for j in range(m):
        W = [np.linalg.inv(np.eye(st[b + 1] - st[b], dtype=R.dtype) + beta[j] * R[sl[b], sl[b]]) for b in range(p)]
        Xj = np.zeros_like(R)
        for d in range(p):
            for i in range(p - d):
                c = i + d
                S = np.zeros_like(R[sl[i], sl[c]])
                for k in range(i + 1, c + 1):
                    S = S + R[sl[i], sl[k]] @ Xj[sl[k], sl[c]]
                Xj[sl[i], sl[c]] = W[i] @ (R[sl[i], sl[c]] - beta[j] * S)
        L = L + alpha[j] * Xj
    return L


def _pade_plain(R, m):
    beta, alpha = NODES[m]
    I = np.eye(R.shape[0], dtype=R.dtype)
    L = np.zeros_like(R)
    for j in range(m):
        L = L + alpha[j] * np.linalg.solve(I + beta[j] * R, R)
    return L


def trlogm_ref(T):
    return _ising(T, Q.trsqrt_ref, _pade_blocked)


def logm_unblocked(T):
    return _ising(T, Q.sqrt_recurrence, _pade_plain)


# ------------------------------------------------------------------ cases
TRI_ALL = Q.TRI_ALL
tri_case = Q.tri_case
case = Q.case
NAMES = [k for k in Q.NAMES if Q.order_of(k) <= 200]
NEEDS_COMPLEX = Q.NEEDS_COMPLEX
REAL_LOG = [k for k in NAMES if k in Q.REAL_ROOT]
MP_NAMES = [k for k in NAMES if Q.order_of(k) <= 65]
MP_TRI = [k for k in TRI_ALL if Q.tri_case(k).shape[0] <= 65]


def scipy_log(A, want_real, imag_tol=None):
    """scipy.linalg.logm's logarithm; cast to float64 where ``want_real`` after checking that its imaginary
    part is at rounding level: ||Im X||_F <= imag_tol max(||Re X||_F, 1), by default 100 n eps (near_neg130, whose
    pairs lie within 1e-9 of the negative real axis, comes back from SciPy with an imaginary part of 1e-7 relative
    size and takes 1e-6)."""
    import scipy.linalg as sla
    X = sla.logm(np.array(A))
    if isinstance(X, tuple):
        X = X[0]
    X = np.asarray(X)
    if want_real and np.iscomplexobj(X):
        tol = 100 * A.shape[0] * EPS if imag_tol is None else imag_tol
        assert np.linalg.norm(X.imag) <= tol * max(np.linalg.norm(X.real), 1.0)
        X = X.real
    if not want_real:
        X = X.astype(np.complex128)
    return np.asfortranarray(X)


def mp_log(A, dps=50):
    """The principal logarithm recomputed in mpmath at ``dps`` digits, rounded to complex128: the complex Schur
    form A = Q T Q^H (mpmath.schur), square roots of the triangular T by the Bjorck-Hammarling recurrence until
    ||T - I||_1 < 1e-3, the Mercator series, L Q-transformed back.  A diagonal entry with a negative real part and
    an imaginary part of rounding size (a real negative eigenvalue of a real A) is put on the axis with
    imaginary part +0, SciPy's branch."""
    import mpmath as mp
    A = np.asarray(A)
    n = A.shape[0]
    with mp.workdps(dps + 15):
        M = mp.matrix([[mp.mpc(complex(v)) for v in row] for row in A])
        if np.all(np.tril(A, -1) == 0):
            Qm, T = mp.eye(n), M
        else:
            Qm, T = mp.schur(M)
        tiny = mp.mpf(10) ** (-dps + 5)
        t = [[T[i, j] for j in range(n)] for i in range(n)]
        for i in range(n):
            for j in range(i):
                t[i][j] = mp.mpc(0)
            if mp.re(t[i][i]) < 0 and abs(mp.im(t[i][i])) <= tiny * abs(t[i][i]):
                t[i][i] = mp.mpc(mp.re(t[i][i]), 0)
        s = 0
        while True:
            nr = max(sum(abs(t[i][j] - (1 if i == j else 0)) for i in range(j + 1)) for j in range(n))
            if nr < mp.mpf("1e-3"):
                break
            u = [[mp.mpc(0)] * n for _ in range(n)]
            for i in range(n):
                u[i][i] = mp.sqrt(t[i][i])
            for d in range(1, n):
                for i in range(n - d):
                    j = i + d
                    acc = t[i][j]
                    for k in range(i + 1, j):
                        acc -= u[i][k] * u[k][j]
                    u[i][j] = acc / (u[i][i] + u[j][j])
            t, s = u, s + 1
        Rm = mp.matrix(n, n)
        for i in range(n):
            for j in range(i, n):
                Rm[i, j] = t[i][j] - (1 if i == j else 0)
        P, L, k = Rm.copy(), mp.matrix(n, n), 1
        tol = mp.mpf(10) ** (-dps - 8)
        while True:
            L += P * (mp.mpf((-1) ** (k + 1)) / k)
            if mp.mnorm(P, 1) < tol:
                break
            P = P * Rm
            k += 1
        L = Qm * (L * 2 ** s) * Qm.H
        return np.array([[complex(L[i, j]) for j in range(n)] for i in range(n)], dtype=np.complex128)


def schur_of(A):
    """(T, Z) of scipy.linalg.schur: the real form for a real A without negative real eigenvalues, else the complex
    form with the real negative eigenvalues put on the axis (imaginary part +0), as the device does."""
    import scipy.linalg as sla
    A = np.asarray(A)
    if not np.iscomplexobj(A):
        T, Z = sla.schur(A, output="real")
        g = Q.groups(T)
        if not any(g[k + 1] - g[k] == 1 and T[g[k], g[k]] < 0 for k in range(len(g) - 1)):
            return T, Z
    T, Z = sla.schur(A.astype(np.complex128), output="complex")
    if not np.iscomplexobj(A) or not np.any(A.imag):
        d = np.diagonal(T).copy()
        snap = (d.real < 0) & (np.abs(d.imag) <= A.shape[0] * EPS * np.linalg.norm(A))
        d[snap] = d[snap].real + 0j
        T = np.triu(T, 1) + np.diag(d)
    return np.triu(T) if np.iscomplexobj(T) else T, Z


def logm_via_schur(A):
    """(X, roots, degree): ``logm_unblocked`` on SciPy's Schur form, transformed back"""
    T, Z = schur_of(A)
    L, s, m = logm_unblocked(T)
    return np.asfortranarray(Z @ L @ Z.conj().T), s, m


ROUND_TRIP = ("r130_2", "c130_2")   # expm_ref cases: order 130, ||A||_1 = 2, so every |Im lambda| < pi


def round_trip_ref(name):
    """||logm(expm(A)) - A||_F / ||A||_F with expm_2005 and logm_via_schur"""
    A = X5.case(name)
    return gap(logm_via_schur(X5.expm_2005(A)[0])[0], A)
