"""Cases, figures and the NumPy restatement for the matrix exponential tests (csrc/expm.hip).

``expm_2005(A)`` restates the device algorithm: the plan from ||A||_1 (``plan``), the Pade polynomials in the
grouping of csrc/expm.hip, ``numpy.linalg.solve`` for (V - U) X = V + U, s squarings.  It returns (X, m, s).
``plan`` finds the squarings in exact rational arithmetic, on purpose not the way csrc/expm_plan.hpp does.

Cases.  ``case("r<n>_<target>")`` is eig_ref._gen(n, n) scaled to ||A||_1 = target, ``"c<n>_<target>"`` the same
plus i _gen(n, n + 1).  The targets give m = 3, 5, 7, 9, 13 with s = 0, then s = 3 and s = 8; each lies far from a
threshold, so the last bit of the norm cannot change the plan.  Orders 3, 33 and 65 take every target, the orders
above 65 take 5 and 40, the others a few.  A case with target 1000 whose restatement is not finite is dropped when
the list is built (``OVERFLOWING``), finite meaning that its Frobenius norm is, which g divides by.  That drops
order 3: its entries reach 1e205 (real) and 1e232 (complex), whose squares overflow.  tests/test_gpu_expm.py checks
on these two that the device returns finite entries, and the overflow itself on scalars.

Figure: g(X) = ||X - X_scipy||_F / ||X_scipy||_F with X_scipy = scipy.linalg.expm(A).
Bound: g(device) <= 3 max(g(expm_2005) on the case, floor), the floor being the largest g(expm_2005) over the
cases of the same scalar type and s (the convention of sqrtm_ref.bound_cw; 3 is the project's allowance for another
summation order).  tests/test_expm_cpu.py records every case's g(expm_2005) and the floors in
tests/golden/expm_ref_figures.json, with the distances of SciPy and of the restatement to mpmath at 60 digits for
the cases of order <= 33: SciPy is far more accurate than the 2005 algorithm at small norms (so "3 x SciPy's own
error" cannot be met) and less accurate on order 3 at targets 5 and 40.
"""
import json
import math
import os
from fractions import Fraction

import numpy as np
import scipy.linalg as sla

import eig_ref as R

EPS = R.EPS
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ACCURACY_JSON = os.path.join(ROOT, "profiles", "expm_accuracy.json")
GOLDEN = os.path.join(ROOT, "tests", "golden", "expm_ref_figures.json")
_figures = {}

DEGREES = (3, 5, 7, 9, 13)
THETA = (1.495585217958292e-2, 2.539398330063230e-1, 9.504178996162932e-1, 2.097847961257068, 5.371920351148152)
PADE = {
    3: (120., 60., 12., 1.),
    5: (30240., 15120., 3360., 420., 30., 1.),
    7: (17297280., 8648640., 1995840., 277200., 25200., 1512., 56., 1.),
    9: (17643225600., 8821612800., 2075673600., 302702400., 30270240., 2162160., 110880., 3960., 90., 1.),
    13: (64764752532480000., 32382376266240000., 7771770303897600., 1187353796428800., 129060195264000.,
         10559470521600., 670442572800., 33522128640., 1323241920., 40840800., 960960., 16380., 182., 1.),
}
TARGETS = (0.01, 0.2, 0.8, 2, 5, 40, 1000)
PLAN_OF_TARGET = {0.01: (3, 0), 0.2: (5, 0), 0.8: (7, 0), 2: (9, 0), 5: (13, 0), 40: (13, 3), 1000: (13, 8)}
ORDERS = (1, 2, 3, 17, 33, 63, 64, 65, 129, 200)
_TARGETS_OF = {1: (0.2, 5, 40), 2: (0.01, 2, 40), 3: TARGETS, 17: (0.8, 5, 1000), 33: TARGETS, 63: (2, 40), 64: (5, 40),
               65: TARGETS, 129: (5, 40), 200: (5, 40)}
MP_MAX_ORDER = 33


def record(key, **kw):
    """One case's measured figures into profiles/expm_accuracy.json."""
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


def plan(alpha):
    """(m, s) for ||A||_1 = alpha: the first degree with alpha <= theta_m, else 13 and the smallest s with
    alpha 2^-s <= theta_13, decided in exact rational arithmetic."""
    for m, th in zip(DEGREES, THETA):
        if alpha <= th:
            return m, 0
    a, th = Fraction(alpha), Fraction(THETA[-1])
    s = max(math.frexp(alpha)[1] - 6, 0)
    while a / 2 ** s > th:
        s += 1
    return 13, s


def norm1(A):
    return float(np.abs(A).sum(axis=0).max())


def pade_uv(A, m):
    """U (odd) and V (even) of the degree-m approximant, products and sums grouped as in csrc/expm.hip."""
    b = PADE[m]
    I = np.eye(A.shape[0], dtype=A.dtype)
    A2 = A @ A
    if m == 3:
        return A @ (b[3] * A2 + b[1] * I), b[2] * A2 + b[0] * I
    A4 = A2 @ A2
    if m == 5:
        return A @ (b[5] * A4 + b[3] * A2 + b[1] * I), b[4] * A4 + b[2] * A2 + b[0] * I
    A6 = A4 @ A2
    if m == 7:
        return A @ (b[7] * A6 + b[5] * A4 + b[3] * A2 + b[1] * I), b[6] * A6 + b[4] * A4 + b[2] * A2 + b[0] * I
    if m == 9:
        A8 = A6 @ A2
        return (A @ (b[9] * A8 + b[7] * A6 + b[5] * A4 + b[3] * A2 + b[1] * I),
                b[8] * A8 + b[6] * A6 + b[4] * A4 + b[2] * A2 + b[0] * I)
    Z = A6 @ (b[13] * A6 + b[11] * A4 + b[9] * A2) + b[7] * A6 + b[5] * A4 + b[3] * A2 + b[1] * I
    V = A6 @ (b[12] * A6 + b[10] * A4 + b[8] * A2) + b[6] * A6 + b[4] * A4 + b[2] * A2 + b[0] * I
    return A @ Z, V


def expm_2005(A):
    """Higham's 2005 scaling and squaring as csrc/expm.hip runs it; returns (X, m, s)."""
    A = np.array(A, dtype=np.complex128 if np.iscomplexobj(A) else np.float64)
    n = A.shape[0]
    alpha = norm1(A)
    m, s = plan(alpha)
    if alpha == 0.0:
        return np.eye(n, dtype=A.dtype), m, s
    with np.errstate(all="ignore"):
        U, V = pade_uv(A * math.ldexp(1.0, -s), m)   # a power of two: exact
        X = np.linalg.solve(V - U, V + U)
        for _ in range(s):
            X = X @ X
    return X, m, s


def gap(X, Xref):
    """g: ||X - Xref||_F / ||Xref||_F"""
    return float(np.linalg.norm(np.asarray(X) - Xref) / np.linalg.norm(Xref))


def mp_expm(A, dps=60):
    """exp(A) in mpmath at ``dps`` digits, rounded to A's type"""
    import mpmath as mp

    with mp.workdps(dps):
        n = A.shape[0]
        M = mp.matrix(n, n)
        for i in range(n):
            for j in range(n):
                M[i, j] = mp.mpc(complex(A[i, j]))
        X = mp.expm(M)
        out = np.array([[complex(X[i, j]) for j in range(n)] for i in range(n)])
    return out if np.iscomplexobj(A) else out.real


def _name(cx, n, target):
    return f"{'c' if cx else 'r'}{n}_{target}"


_cases, _restated, _scipy = {}, {}, {}


def case(name):
    if name not in _cases:
        cx = name[0] == "c"
        n, target = name[1:].split("_")
        n, target = int(n), float(target)
        A = R._gen(n, n)
        if cx:
            A = A + 1j * R._gen(n, n + 1)
        A = np.asfortranarray(A * (target / norm1(A)))
        A.setflags(write=False)
        _cases[name] = A
    return _cases[name]


def restated(name):
    """expm_2005 on the case, computed once"""
    if name not in _restated:
        _restated[name] = expm_2005(case(name))
    return _restated[name]


def scipy_expm(name):
    if name not in _scipy:
        X = sla.expm(np.array(case(name)))
        X.setflags(write=False)
        _scipy[name] = X
    return _scipy[name]


def target_of(name):
    t = float(name.split("_")[1])
    return int(t) if t == int(t) else t


def _build_names():
    names, dropped = [], []
    for cx in (False, True):
        for n in ORDERS:
            for t in _TARGETS_OF[n]:
                nm = _name(cx, n, t)
                if t == 1000 and not np.isfinite(np.linalg.norm(restated(nm)[0])):   # g divides by this norm
                    dropped.append(nm)
                    continue
                names.append(nm)
    return names, dropped


NAMES, OVERFLOWING = _build_names()


def floors(g_ref):
    """{type letter + s: the largest g(expm_2005) over that type's cases with that s}"""
    out = {}
    for nm, g in g_ref.items():
        key = f"{nm[0]}{PLAN_OF_TARGET[target_of(nm)][1]}"
        out[key] = max(out.get(key, 0.0), g)
    return out


def bound(name, rec=None):
    rec = golden() if rec is None else rec
    key = f"{name[0]}{PLAN_OF_TARGET[target_of(name)][1]}"
    return 3.0 * max(rec["g_ref"][name], rec["floors"][key])
