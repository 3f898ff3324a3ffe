"""Figures, cases and the NumPy restatements for the matrix square root tests (csrc/sqrtm.hip).

Figure of a root X of A (``figure``):
    r = ||X^2 - A||_F / (n eps ||X||_F^2)
It divides by ||X||^2 and not by ||A||: that is what a backward-stable root can deliver (Higham, Functions of
Matrices, section 6.1).  Componentwise figure of the triangular stage U^2 = T (``figure_cw``), formed in long
double and not divided by the order, as sylvester_ref.figure_cw:
    w = max over the upper (quasi-)triangle of |U^2 - T|_ij / (eps (|U| |U|)_ij)
r is nearly blind on triangular input (1e-3 down to 1e-10 for a correct root on the cases below), so w is the
figure that bites there.

Bounds.  r <= max(2, 3 x SciPy's r on the case) (``bound``).  w <= max(3 x the unblocked recurrence's w on the
case, the scalar type's floor) (``bound_cw``), the floor being 3 x the recurrence's largest w over all constructed
cases of that type.  tests/test_sqrtm_cpu.py records all of them in tests/golden/sqrtm_ref_figures.json.

References.  Full matrices: ``scipy.linalg.sqrtm`` (``scipy_root``), cast to the real type where its imaginary
part is at rounding level.  The triangular stage has no LAPACK or SciPy routine for a quasi-triangular T, so its
reference is ``sqrt_recurrence``: the unblocked recurrence in float64 (Bjorck and Hammarling; Higham's real Schur
method), entry groups by T's 1 x 1 / 2 x 2 diagonal blocks, pair systems with a 2 x 2 member by
``scipy.linalg.solve_sylvester``.  ``trsqrt_ref`` restates the device's partition and two-launch schedule with
that recurrence for the diagonal blocks and ``block_solve``, substitution over the diagonal groups, for the block solves.

Constructed triangular cases (``TRI``; ``tri_case(name)``), built as sylvester_ref.tri: strict triangle
N(0, 1) / sqrt(n), diagonal uniform in [1, 2] (complex: plus i uniform in [-1, 1]), 2 x 2 blocks [a b; -c a] with
b, c in [0.5, 1.5].  The orders and pair positions are the smallest at which each path of the partition (NB = 64
real, 32 complex) and of the schedule can go wrong; see ``_TRI_SPECS``.  Hard cases (``TRI_HARD``): nn65p / nn65c,
undamped N(0, 1) triangles; near_neg130, order 130 with pairs theta = -1, mu = 1e-3, 1e-6, 1e-9 at rows 10, 63, 100
(alpha is about mu / 2 and ||U||_F reaches 1e8); cneg65, complex with diagonal entries -1 +- 1e-9 i and -2 + 1e-12 i.

Named full cases (``NAMES``; ``case(name)``): "r<n>" / "c<n>" are eig_ref._gen(n, n) (+ i _gen(n, n + 1)) plus
(||.||_2 + 1) I, n in ``ORDERS``; "ur<n>" / "uc<n>" the same unshifted (the real ones have negative real
eigenvalues, so their root is complex); sym65, diag50, tri30 and graded60 of eig_ref shifted likewise; "eye7";
"rot90", whose root is the rotation by 45 degrees.
"""
import json
import os

import numpy as np
import scipy.linalg as sla

import eig_ref as R
import sylvester_ref as Y

EPS = R.EPS
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ACCURACY_JSON = os.path.join(ROOT, "profiles", "sqrtm_accuracy.json")
GOLDEN = os.path.join(ROOT, "tests", "golden", "sqrtm_ref_figures.json")
_figures = {}


def record(key, **kw):
    """One case's measured figures into profiles/sqrtm_accuracy.json (the GPU tests of both files)."""
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


def figure(A, X):
    n = A.shape[0]
    den = np.linalg.norm(X) ** 2
    if den == 0.0:
        den = 1.0
    return float(np.linalg.norm(X @ X - A)) / (n * EPS * den)


def quasi_mask(T):
    """True on the upper triangle and on T's non-zero sub-diagonal entries"""
    n = T.shape[0]
    M = np.triu(np.ones((n, n), dtype=bool))
    k = np.flatnonzero(np.diagonal(T, -1) != 0)
    M[k + 1, k] = True
    return M


def figure_cw(T, U):
    """The componentwise figure w of U in U^2 = T, in long double; inf where an entry's denominator is 0 and its
    residual is not, or where anything is not finite."""
    lt = np.clongdouble if (np.iscomplexobj(T) or np.iscomplexobj(U)) else np.longdouble
    Tl, Ul = np.asarray(T).astype(lt), np.asarray(U).astype(lt)
    M = quasi_mask(T)
    res = np.abs(Ul @ Ul - Tl)[M]
    den = (np.abs(Ul) @ np.abs(Ul))[M]
    if not (np.all(np.isfinite(res)) and np.all(np.isfinite(den))):
        return float("inf")
    zero = den == 0
    if np.any(res[zero] != 0):
        return float("inf")
    if np.all(zero):
        return 0.0
    return float(np.max(res[~zero] / den[~zero]) / np.longdouble(EPS))


def bound(scipy_r):
    return max(2.0, 3.0 * scipy_r)


def bound_cw(rec_w, dtype_floor):
    return max(3.0 * rec_w, dtype_floor)


def _frozen(*arrays):
    out = tuple(np.asfortranarray(a) for a in arrays)
    for a in out:
        a.setflags(write=False)
    return out


# ------------------------------------------------------------------ constructed triangular cases
_TRI_SPECS = {   # name: (order, rows that start a 2 x 2 block, complex)
    "n1": (1, [], False),
    "n2pair": (2, [0], False),                        # one 2 x 2 block and nothing else
    "n3": (3, [1], False),
    "r63": (63, [10, 30], False),                     # one block, one row short of NB
    "r64": (64, [62], False),                         # a pair at the block's end
    "r65": (65, [63], False),                         # a pair across rows 63 | 64: the boundary moves up to 63
    "r65b": (65, [0, 30, 62], False),
    "r129": (129, [63, 126], False),                  # both boundaries move: blocks of 63, 63, 3
    "r130": (130, [10, 63, 100, 127], False),         # three blocks: the first non-empty sum over k
    "r200": (200, list(range(0, 199, 7)), False),     # four blocks: two chunks in order
    "pairs130": (130, list(range(0, 130, 2)), False),
    "c1": (1, [], True),
    "c33": (33, [], True),                            # 2 blocks
    "c65": (65, [], True),                            # 3 blocks
    "c130": (130, [], True),                          # 5 blocks
}
TRI = list(_TRI_SPECS)


def _undamped(n, pairs, seed, cplx):
    rng = np.random.default_rng(seed)
    T = np.triu(rng.standard_normal((n, n)), 1)
    if cplx:
        T = T + 1j * np.triu(rng.standard_normal((n, n)), 1)
        return T + np.diag(rng.uniform(1.0, 2.0, n) + 1j * rng.uniform(-1.0, 1.0, n))
    T = T + np.diag(rng.uniform(1.0, 2.0, n))
    for k in pairs:
        T[k + 1, k + 1] = T[k, k]
        T[k, k + 1] = rng.uniform(0.5, 1.5)
        T[k + 1, k] = -rng.uniform(0.5, 1.5)
    return T


def _near_neg(seed):
    T = np.array(Y.tri(130, [10, 63, 100], seed))
    for k, mu in ((10, 1e-3), (63, 1e-6), (100, 1e-9)):
        T[k, k] = T[k + 1, k + 1] = -1.0
        T[k, k + 1], T[k + 1, k] = mu, -mu
    return T


def _cneg(seed):
    T = np.array(Y.tri(65, [], seed, True))
    T[5, 5], T[31, 31], T[40, 40] = -1.0 + 1e-9j, -1.0 - 1e-9j, -2.0 + 1e-12j
    return T


_HARD = {
    "nn65p": lambda seed: _undamped(65, [10, 30, 63], seed, False),
    "nn65c": lambda seed: _undamped(65, [], seed, True),
    "near_neg130": _near_neg,
    "cneg65": _cneg,
}
TRI_HARD = list(_HARD)
TRI_ALL = TRI + TRI_HARD
_tri_cache = {}


def tri_case(name):
    """T of a constructed case, built once and read-only."""
    if name not in _tri_cache:
        if name in _HARD:
            T = _HARD[name](17000 + 5 * TRI_HARD.index(name))
        else:
            n, pairs, cplx = _TRI_SPECS[name]
            T = Y.tri(n, pairs, 15000 + 3 * TRI.index(name), cplx)
        _tri_cache[name], = _frozen(T)
    return _tri_cache[name]


def is_complex_case(name):
    return np.iscomplexobj(tri_case(name))


# ------------------------------------------------------------------ the recurrence and the device's schedule
def groups(T):
    """starts of T's diagonal groups (1 x 1, or 2 x 2 where the sub-diagonal entry is non-zero), with n appended"""
    n = T.shape[0]
    g, k = [], 0
    while k < n:
        g.append(k)
        k += 2 if (k + 1 < n and T[k + 1, k] != 0) else 1
    return g + [n]


def _sqrt_scalar(t):
    if np.iscomplexobj(t):
        return np.sqrt(complex(t.real, t.imag + 0.0))   # -0.0 counts as +0.0
    return np.sqrt(t)


def sqrt_block2(B):
    """the root of a real 2 x 2 block with eigenvalues theta +- i mu, by the formulas of small_sqrt.hpp"""
    theta, d = (B[0, 0] + B[1, 1]) / 2.0, (B[0, 0] - B[1, 1]) / 2.0
    mu2 = -(d * d + B[0, 1] * B[1, 0])
    assert mu2 > 0
    mu, lam = np.sqrt(mu2), np.sqrt(theta * theta + mu2)
    alpha = np.sqrt((lam + theta) / 2.0) if theta >= 0 else mu / (2.0 * np.sqrt((lam - theta) / 2.0))
    t = 2.0 * alpha   # B - theta I has the diagonal (d, -d)
    return np.array([[alpha + d / t, B[0, 1] / t], [B[1, 0] / t, alpha - d / t]])


def sqrt_recurrence(T):
    """U^2 = T by the unblocked recurrence in T's precision: the groups' own roots, then the group super-diagonals."""
    T = np.asarray(T)
    U = np.zeros_like(T)
    g = groups(T)
    ng = len(g) - 1
    for k in range(ng):
        a, b = g[k], g[k + 1]
        if b - a == 1:
            U[a, a] = _sqrt_scalar(T[a, a])
        else:
            U[a:b, a:b] = sqrt_block2(T[a:b, a:b])
    for e in range(1, ng):
        for k in range(ng - e):
            a0, a1, b0, b1 = g[k], g[k + 1], g[k + e], g[k + e + 1]
            rhs = T[a0:a1, b0:b1] - U[a0:a1, a1:b0] @ U[a1:b0, b0:b1]
            if a1 - a0 == 1 and b1 - b0 == 1:
                U[a0, b0] = rhs[0, 0] / (U[a0, a0] + U[b0, b0])
            else:
                U[a0:a1, b0:b1] = sla.solve_sylvester(U[a0:a1, a0:a1], U[b0:b1, b0:b1], rhs)
    return U


def block_solve(Ri, Sj, F):
    """R_ii Y + Y S_jj = F for quasi-triangular R_ii, S_jj by substitution over their diagonal groups (rows from
    the bottom, columns from the left), as the one-workgroup kernel: scipy.linalg.solve_sylvester on a whole
    block would go through a Schur form of U_ii, which is backward stable in norm only."""
    Yv = np.array(F)
    ga, gb = groups(Ri), groups(Sj)
    for bi in range(len(gb) - 1):
        b0, b1 = gb[bi], gb[bi + 1]
        for ai in range(len(ga) - 2, -1, -1):
            a0, a1 = ga[ai], ga[ai + 1]
            rhs = F[a0:a1, b0:b1] - (Ri[a0:a1, a1:] @ Yv[a1:, b0:b1] + Yv[a0:a1, :b0] @ Sj[:b0, b0:b1])
            if a1 - a0 == 1 and b1 - b0 == 1:
                Yv[a0, b0] = rhs[0, 0] / (Ri[a0, a0] + Sj[b0, b0])
            else:
                Yv[a0:a1, b0:b1] = sla.solve_sylvester(Ri[a0:a1, a0:a1], Sj[b0:b1, b0:b1], rhs)
    return Yv


def trsqrt_ref(T):
    """The device's partition and schedule: all diagonal blocks, then per block super-diagonal s all sums
    T_ij - sum_k U_ik U_kj (k ascending), then all block solves U_ii Y + Y U_jj = F_ij."""
    T = np.asarray(T)
    U = np.array(T, order="F")
    st = Y.starts(T)
    p = len(st) - 1
    sl = [slice(st[b], st[b + 1]) for b in range(p)]
    for b in range(p):
        U[sl[b], sl[b]] = sqrt_recurrence(T[sl[b], sl[b]])
    for s in range(1, p):
        for i in range(p - s):
            for k in range(i + 1, i + s):
                U[sl[i], sl[i + s]] -= U[sl[i], sl[k]] @ U[sl[k], sl[i + s]]
        for i in range(p - s):
            j = i + s
            U[sl[i], sl[j]] = block_solve(U[sl[i], sl[i]], U[sl[j], sl[j]], U[sl[i], sl[j]])
    return U


def group_eigenvalues(U):
    """the eigenvalues of U's diagonal groups"""
    g = groups(U)
    out = []
    for k in range(len(g) - 1):
        out.extend(np.linalg.eigvals(np.atleast_2d(U[g[k]:g[k + 1], g[k]:g[k + 1]])))
    return np.array(out)


# ------------------------------------------------------------------ named full cases
ORDERS = [1, 2, 3, 63, 64, 65, 129, 130, 200, 450]
UNSHIFTED_REAL, UNSHIFTED_CPLX = [63, 65, 130], [65, 130]
EIG_NAMED = ["sym65", "diag50", "tri30", "graded60"]


def _gen(n, cplx):
    A = R._gen(n, n)
    return A + 1j * R._gen(n, n + 1) if cplx else A


_BUILDERS = {}
for _n in ORDERS:
    _BUILDERS[f"r{_n}"] = (lambda n=_n: Y._shift(_gen(n, False)))
    _BUILDERS[f"c{_n}"] = (lambda n=_n: Y._shift(_gen(n, True)))
for _n in UNSHIFTED_REAL:
    _BUILDERS[f"ur{_n}"] = (lambda n=_n: _gen(n, False))
for _n in UNSHIFTED_CPLX:
    _BUILDERS[f"uc{_n}"] = (lambda n=_n: _gen(n, True))
for _k in EIG_NAMED:
    _BUILDERS[_k] = (lambda k=_k: Y._shift(np.array(R.matrix(k))))
_BUILDERS["eye7"] = lambda: np.eye(7)
_BUILDERS["rot90"] = lambda: np.array([[0.0, -1.0], [1.0, 0.0]])
NAMES = list(_BUILDERS)
REAL_ROOT = [k for k in NAMES if not (k.startswith("c") or k.startswith("u"))]   # real input, real root
NEEDS_COMPLEX = [f"ur{n}" for n in UNSHIFTED_REAL]
_cache = {}


def case(name):
    """A of a named case, built once and read-only."""
    if name not in _cache:
        _cache[name], = _frozen(_BUILDERS[name]())
    return _cache[name]


def order_of(name):
    return int(name.lstrip("urc")) if name.lstrip("urc").isdigit() else case(name).shape[0]


MP_NAMES = [k for k in NAMES if order_of(k) <= 65]   # the cases whose root is recomputed in mpmath


def scipy_root(A, want_real):
    """scipy.linalg.sqrtm's root; cast to float64 where ``want_real`` after checking that its imaginary part is
    at rounding level."""
    X = sla.sqrtm(np.array(A))
    if want_real and np.iscomplexobj(X):
        assert np.linalg.norm(X.imag) <= 100 * A.shape[0] * EPS * np.linalg.norm(X.real)
        X = X.real
    if not want_real:
        X = X.astype(np.complex128)
    return np.asfortranarray(X)


def mp_root(A, dps=50):
    """The principal root recomputed in mpmath at ``dps`` digits, rounded to complex128: mpmath.sqrtm (the
    Denman-Beavers iteration) where A's spectrum lies in the open right half plane; else, as that iteration
    breaks down on and near the negative real axis, through mpmath.eig, V diag(sqrt(lambda)) V^-1, with the
    root of a negative real eigenvalue on the positive imaginary axis (the named cases are diagonalisable)."""
    import mpmath as mp
    n = A.shape[0]
    with mp.workdps(dps):
        M = mp.matrix([[mp.mpc(complex(v)) for v in row] for row in np.asarray(A)])
        ev = np.linalg.eigvals(A)
        on_axis = np.any(ev.real <= 0)
        if not on_axis:
            X = mp.sqrtm(M)
        else:
            E, V = mp.eig(M)
            roots = []
            for lam in E:
                if abs(mp.im(lam)) <= mp.mpf(10) ** (-dps + 10) * abs(lam) and mp.re(lam) < 0:
                    roots.append(mp.mpc(0, mp.sqrt(-mp.re(lam))))
                else:
                    roots.append(mp.sqrt(lam))
            X = V * mp.diag(roots) * mp.inverse(V)
        return np.array([[complex(X[i, j]) for j in range(n)] for i in range(n)], dtype=np.complex128)


def gap(Xa, Xb):
    den = np.linalg.norm(Xb)
    return float(np.linalg.norm(Xa - Xb) / (den if den else 1.0))
