"""Figure, cases and the NumPy restatement of the triangular stage for the Sylvester / Lyapunov tests
(csrc/sylvester.hip).

Figure of a solution X of A X + X op(B) = C (A m x m, B n x n; ``Bop`` below is op(B) itself):
    r = ||A X + X op(B) - C||_F / (max(m, n) eps ((||A||_F + ||B||_F) ||X||_F + ||C||_F))
No case here lies outside the range in which these norms can be formed, so nothing is rescaled.

Named cases (``NAMES``; ``case(name)`` gives A, B, C): A = _gen(m, m), B = _gen(n, n + 1000),
C = _gen(max(m, n), 7)[:m, :n] from tests/eig_ref.py, real ("r63x65") and complex ("c63x65": the imaginary
parts are _gen with the next seed, as schur_ref's cgen matrices); "shifted65" / "shifted130" add
(||.||_2 + 1) I to A and to B, so the spectra of A and -B are well separated; "lyap65" / "lyap130"
(``LYAPUNOV``; B = A^T) take that A with Q = C + C^T; eig_ref's jordan40, graded60, blk40, kron30, sym65, tri30
and diag50 stand against B = _gen(33, 33).

Constructed triangular cases (``TRI``; ``tri_case(name)`` gives R, S, F) for the triangular stage alone: the
strict upper triangle is standard normal / sqrt(order), which keeps the triangular solves' growth moderate so
that the figure stays sensitive to every block; the diagonal is uniform in [1, 2]; a 2 x 2 block at row k is
[a b; -c a] with b, c in [0.5, 1.5].  Every eigenvalue has its real part in [1, 2], so lambda_i + mu_j is at
least 2 in modulus and no pivot is perturbed.  The block positions are chosen by name to reach every path of
the partition rule with NB = 64 (real) / 32 (complex).
"""
import numpy as np
import scipy.linalg as sla
from scipy.linalg import lapack

import eig_ref as R

EPS = R.EPS
NB_REAL, NB_CPLX = 64, 32


def nb_of(T):
    return NB_CPLX if np.iscomplexobj(T) else NB_REAL


def figure(A, Bop, C, X):
    m, n = C.shape
    den = (np.linalg.norm(A) + np.linalg.norm(Bop)) * np.linalg.norm(X) + np.linalg.norm(C)
    if den == 0.0:
        den = 1.0
    return float(np.linalg.norm(A @ X + X @ Bop - C)) / (max(m, n) * EPS * den)


# ------------------------------------------------------------------ named cases
def _rect(m, n, seed):
    return R._gen(max(m, n), seed)[:m, :n]


def _general(m, n, cplx):
    A, B, C = R._gen(m, m), R._gen(n, n + 1000), _rect(m, n, 7)
    if cplx:
        A = A + 1j * R._gen(m, m + 1)
        B = B + 1j * R._gen(n, n + 1001)
        C = C + 1j * _rect(m, n, 8)
    return A, B, C


def _shift(M):
    return M + (np.linalg.norm(M, 2) + 1.0) * np.eye(M.shape[0])


def _shifted(m):
    A, B, C = _general(m, m, False)
    return _shift(A), _shift(B), C


def _lyap(m):
    A, _, C = _shifted(m)
    return A, A.T, C + C.T


def _named(name):
    A = np.array(R.matrix(name))
    return A, R._gen(33, 33), _rect(A.shape[0], 33, 7)


SHAPES = [(1, 1), (2, 2), (1, 5), (3, 2), (63, 65), (64, 64), (65, 63), (66, 130), (130, 66), (97, 33), (200, 7), (450, 450)]
EIG_NAMED = ["jordan40", "graded60", "blk40", "kron30", "sym65", "tri30", "diag50"]
_BUILDERS = {}
for _m, _n in SHAPES:
    _BUILDERS[f"r{_m}x{_n}"] = (lambda m=_m, n=_n: _general(m, n, False))
    _BUILDERS[f"c{_m}x{_n}"] = (lambda m=_m, n=_n: _general(m, n, True))
for _m in (65, 130):
    _BUILDERS[f"shifted{_m}"] = (lambda m=_m: _shifted(m))
    _BUILDERS[f"lyap{_m}"] = (lambda m=_m: _lyap(m))
for _k in EIG_NAMED:
    _BUILDERS[_k] = (lambda k=_k: _named(k))
LYAPUNOV = ["lyap65", "lyap130"]
NAMES = [k for k in _BUILDERS if k not in LYAPUNOV]
_cache = {}


def _frozen(*arrays):
    out = tuple(np.asfortranarray(a) for a in arrays)
    for a in out:
        a.setflags(write=False)
    return out


def case(name):
    """(A, B, C) of a named case, built once and read-only; a Lyapunov case has B = A^T and C = Q."""
    if name not in _cache:
        _cache[name] = _frozen(*_BUILDERS[name]())
    return _cache[name]


# ------------------------------------------------------------------ constructed triangular cases
def tri(n, pairs, seed, cplx=False):
    rng = np.random.default_rng(seed)
    T = np.triu(rng.standard_normal((n, n)), 1) / np.sqrt(n)
    if cplx:
        assert not pairs
        T = T + 1j * np.triu(rng.standard_normal((n, n)), 1) / np.sqrt(n)
        return T + np.diag(rng.uniform(1.0, 2.0, n) + 1j * rng.uniform(-1.0, 1.0, n))
    T = T + np.diag(rng.uniform(1.0, 2.0, n))
    for k in pairs:
        assert 0 <= k and k + 1 < n and k + 1 not in pairs and k - 1 not in pairs
        T[k + 1, k + 1] = T[k, k]
        T[k, k + 1] = rng.uniform(0.5, 1.5)
        T[k + 1, k] = -rng.uniform(0.5, 1.5)
    return T


def _straddle(n):
    """pairs of an order-n real matrix: one across rows 63 | 64 where it fits (the first boundary moves up),
    one across rows 126 | 127 (the second boundary, 63 + 64, moves up too), two inside the first block"""
    return [k for k in (10, 30, 63, 126) if k + 1 < n] if n >= 65 else [n - 2]


_TRI_SPECS = {   # name: (m, pairs of R, n, pairs of S, complex)
    "pairs128": (128, list(range(0, 128, 2)), 128, list(range(0, 128, 2)), False),
    "odd129": (129, list(range(1, 129, 2)), 129, list(range(1, 129, 2)), False),
    "one_pair": (2, [0], 2, [0], False),
    "n1": (1, [], 1, [], False),
    "n3": (3, [0], 3, [1], False),
    "r200x7": (200, _straddle(200), 7, [2], False),
    "r7x200": (7, [4], 200, _straddle(200), False),
    "r130x66": (130, _straddle(130), 66, _straddle(66), False),
}
for _n in (63, 64, 65, 127, 129, 200):
    _TRI_SPECS[f"r{_n}"] = (_n, _straddle(_n), _n, _straddle(_n), False)
for _n in (31, 32, 33, 65, 100):
    _TRI_SPECS[f"c{_n}"] = (_n, [], _n, [], True)
TRI = list(_TRI_SPECS)
_tri_cache = {}


def tri_case(name):
    """(R, S, F) of a constructed case, built once and read-only."""
    if name not in _tri_cache:
        m, pr, n, ps, cplx = _TRI_SPECS[name]
        seed = 5000 + TRI.index(name) * 3
        F = np.random.default_rng(seed + 2).standard_normal((m, n))
        if cplx:
            F = F + 1j * np.random.default_rng(seed + 3).standard_normal((m, n))
        _tri_cache[name] = _frozen(tri(m, pr, seed, cplx), tri(n, ps, seed + 1, cplx), F)
    return _tri_cache[name]


def op(S, trans_b):
    return S.conj().T if trans_b else S


# ------------------------------------------------------------------ the partition and the schedule
def starts(T, nb=None):
    """Block starts of T: s_0 = 0, s_{b+1} = min(s_b + nb, n), one less where that would split a 2 x 2 block
    (T[s_{b+1}, s_{b+1} - 1] != 0); the last entry is n."""
    nb = nb_of(T) if nb is None else nb
    n = T.shape[0]
    s = [0]
    while s[-1] < n:
        e = min(s[-1] + nb, n)
        if e < n and T[e, e - 1] != 0:
            e -= 1
        s.append(e)
    return s


def check_partition(T, s, nb=None):
    """Raises AssertionError unless s partitions T's rows into blocks of nb - 1 or nb rows (the last one: 1 to
    nb) that split no 2 x 2 block."""
    nb = nb_of(T) if nb is None else nb
    n = T.shape[0]
    assert s[0] == 0 and s[-1] == n
    sizes = np.diff(s)
    assert np.all(sizes >= 1) and np.all(sizes <= nb)
    assert all(z in (nb - 1, nb) for z in sizes[:-1]), "an inner block is neither nb - 1 nor nb rows"
    for e in s[1:-1]:
        assert T[e, e - 1] == 0, f"the boundary at {e} splits a 2 x 2 block"


def lapack_trsyl(Rm, Sm, F, trans_b):
    """LAPACK xTRSYL (isgn = +1) with its scale factor divided out."""
    if np.iscomplexobj(Rm) or np.iscomplexobj(Sm) or np.iscomplexobj(F):
        x, scale, info = lapack.ztrsyl(Rm, Sm, F, tranb="C" if trans_b else "N")
    else:
        x, scale, info = lapack.dtrsyl(Rm, Sm, F, tranb="T" if trans_b else "N")
    assert info in (0, 1)
    return x / scale


def trsyl_ref(Rm, Sm, F, trans_b=False, nb=None):
    """R Y + Y op(S) = F by the device's partition and wavefront schedule: per wavefront all diagonal block
    solves (LAPACK's xTRSYL stands in for the one-workgroup kernel), then all column updates, then all row
    updates."""
    dt = np.result_type(Rm, Sm, F)
    nb = (NB_CPLX if np.issubdtype(dt, np.complexfloating) else NB_REAL) if nb is None else nb
    F = np.array(F, dtype=dt, order="F")
    rs, cs = starts(Rm, nb), starts(Sm, nb)
    p, q = len(rs) - 1, len(cs) - 1
    Sop = op(Sm, trans_b)
    for d in range(p + q - 1):
        blocks = []
        for t in range(q):
            i = p - 1 - (d - t)
            if 0 <= i < p:
                blocks.append((slice(rs[i], rs[i + 1]), (q - 1 - t) if trans_b else t))
        for ri, j in blocks:   # launch 1: the diagonal solves
            cj = slice(cs[j], cs[j + 1])
            F[ri, cj] = lapack_trsyl(Rm[ri, ri], Sm[cj, cj], F[ri, cj], trans_b)
        for ri, j in blocks:   # launch 2: the column updates
            cj = slice(cs[j], cs[j + 1])
            F[:ri.start, cj] -= Rm[:ri.start, ri] @ F[ri, cj]
        for ri, j in blocks:   # launch 3: the row updates
            cj = slice(cs[j], cs[j + 1])
            rest = slice(0, cs[j]) if trans_b else slice(cs[j + 1], None)
            F[ri, rest] -= F[ri, cj] @ Sop[cj, rest]
    return F


def bartels_stewart_ref(A, B, C, trans_b=False):
    """A X + X op(B) = C with LAPACK's Schur forms around trsyl_ref."""
    cplx = any(np.iscomplexobj(M) for M in (A, B, C))
    out = "complex" if cplx else "real"
    TA, U = sla.schur(np.array(A), output=out)
    TB, V = sla.schur(np.array(B), output=out)
    Y = trsyl_ref(TA, TB, U.conj().T @ C @ V, trans_b)
    return U @ Y @ V.conj().T


def bound(lapack_r):
    return max(2.0, 3.0 * lapack_r)
