"""Figure, cases and the NumPy restatement of the triangular stage for the Sylvester / Lyapunov tests
(csrc/sylvester.hip).

Figure of a solution X of A X + X op(B) = C (A m x m, B n x n; ``Bop`` below is op(B) itself):
    r = ||A X + X op(B) - C||_F / (max(m, n) eps ((||A||_F + ||B||_F) ||X||_F + ||C||_F))
``figure`` forms the norms as they stand; ``figure_scaled`` first takes an exact power of two out of each of
A, B, X and C (as schur_ref.figures does), for the scaled cases below whose norms would overflow or underflow.

Componentwise figure of the triangular stage R Y + Y op(S) = F (``figure_cw``), not divided by the order:
    w = max_ij |R Y + Y op(S) - F|_ij / (eps (|R| |Y| + |Y| |op(S)| + |F|)_ij)
with the residual and the denominator formed in numpy.longdouble.  It sees an error in an entry of Y that is
small against ||Y||_F, which r cannot.  Its bound (``bound_cw``) is max(3 x xTRSYL's w on the case, the floor of
the scalar type), the floor being 3 x the largest w of xTRSYL over all constructed cases of that type.

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

Hard constructed cases (``TRI_HARD``, seeds of their own so that TRI's bits stay; ``TRI_ALL`` is both lists):
  close<d> (real, order 130, pairs at _straddle(130); d = 1e-04, 1e-08, 1e-12): eigenvalue pairs of R and op(S)
    with lambda_i + mu_j = d.  R(5, 5) is set to R(10, 10), the real part of R's pair at row 10, and S is
    overwritten at the hits: 1 x 1 with 1 x 1 at (i, j) = (5, 7) and (100, 65); 2 x 2 with 2 x 2 at (10, 30),
    (63, 63), (126, 10), S's block becoming [-a + d, 2 g; -g / 2, -a + d] for R's [a b; -c a], g = sqrt(b c) (standard
    form, the same imaginary part); which makes (5, 30) a 1 x 2 and (10, 7) a 2 x 1 system whose real parts sum
    to d (their imaginary part keeps them regular: K has a diagonal of d and off-diagonal entries of order 1, so
    complete pivoting must exchange).  Row 65 and not 64 for the second 1 x 1 hit: S's rows 63, 64 are a pair.
  cclose<d> / cclose<d>h (complex, order 65): S(j, j) = -R(i, i) + d (its conjugate for the "h" names, so that
    S^H has the hit) at (3, 4), (31, 32), (40, 31), (64, 0).  Both names run with both trans_b.
  nonnormal65, nonnormal130 and nonnormal65p, nonnormal130p (pairs at _straddle(n)): the strict triangle is
    N(0, 1), undamped; Y spans many orders of magnitude.
  gradedF130x66: r130x66 with F(i, j) 2^-(i + j).
  mixed_up / mixed_down: r130x66 as (2^200 R, 2^-200 S, F) / (2^-200 R, 2^200 S, 2^200 F).

Scaled named cases (``SCALED``; "r65x63*A+B-" is (2^400 A, 2^-400 B, C) of r65x63, "*C+" is (A, B, 2^600 C)), on
r65x63, c33x65, and lyap65 with "*A+" / "*A-".
"""
import json
import os

import numpy as np
import scipy.linalg as sla
from scipy.linalg import lapack

import eig_ref as R

EPS = R.EPS
NB_REAL, NB_CPLX = 64, 32
ACCURACY_JSON = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "sylvester_accuracy.json")
_figures = {}


def record(key, **kw):
    """One case's measured figures into profiles/sylvester_accuracy.json (the GPU tests of both files)."""
    if not _figures and os.path.exists(ACCURACY_JSON):   # a partial run keeps the other cases' figures
        with open(ACCURACY_JSON) as f:
            _figures.update(json.load(f))
    _figures[key] = {k: float(v) for k, v in kw.items()}
    os.makedirs(os.path.dirname(ACCURACY_JSON), exist_ok=True)
    with open(ACCURACY_JSON, "w") as f:
        json.dump(_figures, f, indent=1, sort_keys=True)
        f.write("\n")


def nb_of(T):
    return NB_CPLX if np.iscomplexobj(T) else NB_REAL


def figure(A, Bop, C, X):
    m, n = C.shape
    den = (np.linalg.norm(A) + np.linalg.norm(Bop)) * np.linalg.norm(X) + np.linalg.norm(C)
    if den == 0.0:
        den = 1.0
    return float(np.linalg.norm(A @ X + X @ Bop - C)) / (max(m, n) * EPS * den)


def _pow2(M):
    """(e, 2^-e M) with max |M| in [0.5, 1): the scaling is exact"""
    M = np.asarray(M)
    big = float(np.max(np.abs(M.real) + np.abs(M.imag))) if M.size else 0.0
    e = int(np.frexp(big)[1]) if big > 0.0 else 0
    return e, np.ldexp(M.real, -e) + (1j * np.ldexp(M.imag, -e) if np.iscomplexobj(M) else 0.0)


def figure_scaled(A, Bop, C, X):
    """``figure`` after an exact power-of-two rescaling of each operand, so that the norms of A = 2^ea A' etc.
    can be formed at any scale: with E = max(ea + ex, eb + ex, ec) the residual is 2^E (2^(ea+ex-E) A' X' +
    2^(eb+ex-E) X' B' - 2^(ec-E) C') and the denominator scales alike; 2^E cancels."""
    m, n = C.shape
    (ea, As), (eb, Bs), (ec, Cs), (ex, Xs) = (_pow2(M) for M in (A, Bop, C, X))
    E = max(ea + ex, eb + ex, ec)
    fa, fb, fc = (float(np.ldexp(1.0, max(k - E, -1074))) for k in (ea + ex, eb + ex, ec))
    den = (fa * np.linalg.norm(As) + fb * np.linalg.norm(Bs)) * np.linalg.norm(Xs) + fc * np.linalg.norm(Cs)
    if den == 0.0:
        den = 1.0
    return float(np.linalg.norm(fa * (As @ Xs) + fb * (Xs @ Bs) - fc * Cs)) / (max(m, n) * EPS * den)


def figure_cw(Rm, Sop, F, Yv):
    """The componentwise backward error w of Y in R Y + Y op(S) = F (``Sop`` is op(S) itself), formed in
    long double; inf where an entry's denominator is 0 and its residual is not."""
    cplx = any(np.iscomplexobj(M) for M in (Rm, Sop, F, Yv))
    lt = np.clongdouble if cplx else np.longdouble
    Rl, Sl, Fl, Yl = (np.asarray(M).astype(lt) for M in (Rm, Sop, F, Yv))
    res = np.abs(Rl @ Yl + Yl @ Sl - Fl)
    aR, aS, aF, aY = (np.abs(M) for M in (Rl, Sl, Fl, Yl))
    den = aR @ aY + aY @ aS + aF
    if not (np.all(np.isfinite(res)) and np.all(np.isfinite(den))):
        return float("inf")
    zero = den == 0
    if np.any(res[zero] != 0):
        return float("inf")
    if np.all(zero):
        return 0.0
    return float(np.max(res[~zero] / den[~zero]) / np.longdouble(EPS))


def bound_cw(lapack_w, dtype_floor):
    return max(3.0 * lapack_w, dtype_floor)


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


SHAPES = [(1, 1), (2, 2), (1, 5), (3, 2), (63, 65), (64, 64), (65, 63), (33, 65), (66, 130), (130, 66), (97, 33), (200, 7), (450, 450)]
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
_SCALES = {"A+B+": (400, 400, 0), "A-B-": (-400, -400, 0), "A+B-": (400, -400, 0), "A-B+": (-400, 400, 0),
           "C+": (0, 0, 600), "C-": (0, 0, -600)}


def _scaled_case(base, ea, eb, ec):
    A, B, C = case(base)
    return np.ldexp(A.real, ea) + (1j * np.ldexp(A.imag, ea) if np.iscomplexobj(A) else 0.0), \
        np.ldexp(B.real, eb) + (1j * np.ldexp(B.imag, eb) if np.iscomplexobj(B) else 0.0), \
        np.ldexp(C.real, ec) + (1j * np.ldexp(C.imag, ec) if np.iscomplexobj(C) else 0.0)


SCALED = []
for _b in ("r65x63", "c33x65"):
    for _t, _e in _SCALES.items():
        _BUILDERS[f"{_b}*{_t}"] = (lambda b=_b, e=_e: _scaled_case(b, *e))
        SCALED.append(f"{_b}*{_t}")
SCALED_LYAPUNOV = []
for _t, _e in (("A+", 400), ("A-", -400)):
    _BUILDERS[f"lyap65*{_t}"] = (lambda e=_e: _scaled_case("lyap65", e, e, 0))
    SCALED_LYAPUNOV.append(f"lyap65*{_t}")
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


def _rhs(m, n, seed, cplx):
    F = np.random.default_rng(seed + 2).standard_normal((m, n))
    return F + 1j * np.random.default_rng(seed + 3).standard_normal((m, n)) if cplx else F


def _close(delta, seed):
    n, pr = 130, _straddle(130)
    Rm, Sm = tri(n, pr, seed), tri(n, pr, seed + 1)
    Rm[5, 5] = Rm[10, 10]
    for i, j in ((5, 7), (100, 65)):
        assert i not in pr and i - 1 not in pr and j not in pr and j - 1 not in pr
        Sm[j, j] = -Rm[i, i] + delta
    for i, j in ((10, 30), (63, 63), (126, 10)):
        assert i in pr and j in pr
        g = np.sqrt(-Rm[i, i + 1] * Rm[i + 1, i])
        Sm[j, j] = Sm[j + 1, j + 1] = -Rm[i, i] + delta
        Sm[j, j + 1], Sm[j + 1, j] = 2.0 * g, -g / 2.0
    return Rm, Sm, _rhs(n, n, seed, False)


def _cclose(delta, seed, trans_b):
    n = 65
    Rm, Sm = tri(n, [], seed, True), tri(n, [], seed + 1, True)
    for i, j in ((3, 4), (31, 32), (40, 31), (64, 0)):
        v = -Rm[i, i] + delta
        Sm[j, j] = np.conj(v) if trans_b else v
    return Rm, Sm, _rhs(n, n, seed, True)


def _nonnormal(n, pairs, seed):
    def one(sd):
        rng = np.random.default_rng(sd)
        T = np.triu(rng.standard_normal((n, n)), 1) + np.diag(rng.uniform(1.0, 2.0, n))
        for k in pairs:
            T[k + 1, k + 1] = T[k, k]
            T[k, k + 1] = rng.uniform(0.5, 1.5)
            T[k + 1, k] = -rng.uniform(0.5, 1.5)
        return T
    return one(seed), one(seed + 1), _rhs(n, n, seed, False)


def _graded():
    Rm, Sm, F = tri_case("r130x66")
    i, j = np.indices(F.shape)
    return Rm, Sm, np.ldexp(F, -(i + j))


def _mixed(up):
    Rm, Sm, F = tri_case("r130x66")
    e = 200 if up else -200
    return np.ldexp(Rm, e), np.ldexp(Sm, -e), F if up else np.ldexp(F, 200)


_HARD = {}   # name: builder taking the case's seed
for _d in (1e-4, 1e-8, 1e-12):
    _HARD[f"close{_d:.0e}"] = (lambda seed, d=_d: _close(d, seed))
    _HARD[f"cclose{_d:.0e}"] = (lambda seed, d=_d: _cclose(d, seed, False))
    _HARD[f"cclose{_d:.0e}h"] = (lambda seed, d=_d: _cclose(d, seed, True))
for _n in (65, 130):
    _HARD[f"nonnormal{_n}"] = (lambda seed, n=_n: _nonnormal(n, [], seed))
    _HARD[f"nonnormal{_n}p"] = (lambda seed, n=_n: _nonnormal(n, _straddle(n), seed))
_HARD["gradedF130x66"] = (lambda seed: _graded())
_HARD["mixed_up"] = (lambda seed: _mixed(True))
_HARD["mixed_down"] = (lambda seed: _mixed(False))
TRI_HARD = list(_HARD)
TRI_ALL = TRI + TRI_HARD


def is_complex_case(name):
    return np.iscomplexobj(tri_case(name)[0])


def tri_case(name):
    """(R, S, F) of a constructed case, built once and read-only."""
    if name not in _tri_cache and name in _HARD:
        _tri_cache[name] = _frozen(*_HARD[name](9000 + TRI_HARD.index(name) * 4))
    if name not in _tri_cache:
        m, pr, n, ps, cplx = _TRI_SPECS[name]
        seed = 5000 + TRI.index(name) * 3
        F = np.random.default_rng(seed + 2).standard_normal((m, n))
        if cplx:
            F = F + 1j * np.random.default_rng(seed + 3).standard_normal((m, n))
        _tri_cache[name] = _frozen(tri(m, pr, seed, cplx), tri(n, ps, seed + 1, cplx), F)
    return _tri_cache[name]


def ldexp(M, e):
    """2^e M, exactly (away from overflow and underflow)"""
    M = np.asarray(M)
    return np.ldexp(M.real, e) + 1j * np.ldexp(M.imag, e) if np.iscomplexobj(M) else np.ldexp(M, e)


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
