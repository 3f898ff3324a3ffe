"""NumPy / SciPy restatement of ``eig`` (csrc/eig.hip, steps a-f), the named test matrices and two figures.

The restatement follows the device code decision by decision, not bit by bit: ``scipy.linalg.hessenberg``
for the reduction, ``numpy.linalg.eigvals`` of every diagonal block of H for the eigenvalues, then the block
rule (H splits where h(i+1, i) == 0 exactly; the vector of an eigenvalue of the block [kl, kr) comes from
the leading kr x kr matrix and is zero below it), dhsein's perturbation by eps3 = eps ||H_block||_1,
xLAEIN's iteration (partial-pivot LU of the Hessenberg matrix whose multipliers are not applied to the
right-hand side, pivots below eps3 replaced by eps3, start vectors on the block's own rows, accepted at
||x||_1 >= 0.1 / sqrt(kr), at most kr - kl starts), Q, and the normalisation.

Figures of a set of eigenpairs (w, V) of A:
    r = max_j ||A v_j - w_j v_j||_2 / (n eps ||A||_F)   (||A||_F replaced by 1 for a zero matrix)
    c = cond_2(V)
"""
import numpy as np
import scipy.linalg as sla

EPS = float(np.finfo(np.float64).eps)
TINY = float(np.finfo(np.float64).tiny)
SMLNUM = np.sqrt(TINY) / EPS


def _abs1(z):
    return np.abs(z.real) + np.abs(z.imag)


# ------------------------------------------------------------------ the named matrices
def _rng(seed):
    return np.random.default_rng(seed)


def _gen(n, seed):
    return _rng(seed).standard_normal((n, n))


def _grcar(n, k=3):
    A = np.eye(n) - np.diag(np.ones(n - 1), -1)
    for q in range(1, k + 1):
        A += np.diag(np.ones(n - q), q)
    return A


def _jordan40():
    r = _rng(40)
    J = np.diag(np.concatenate([[2.0, 2.0, 2.0], np.linspace(-3.0, 5.0, 37) + 0.013]))
    J[0, 1] = J[1, 2] = 1.0
    Q, _ = np.linalg.qr(r.standard_normal((40, 40)))
    return Q @ J @ Q.T


def _graded60():
    d = 10.0 ** (-np.arange(60) / 10.0)
    return d[:, None] * _gen(60, 60) * d[None, :]


def _blk40():
    r = _rng(41)
    M, X = r.standard_normal((20, 20)), r.standard_normal((20, 20))
    return np.block([[M, X], [np.zeros((20, 20)), M]])


_BUILDERS = {
    "n1": lambda: np.array([[3.5]]),
    "n2rot": lambda: np.array([[0.0, -1.0], [1.0, 0.0]]),
    "n3": lambda: _gen(3, 3),
    "gen63": lambda: _gen(63, 63),
    "gen64": lambda: _gen(64, 64),
    "gen65": lambda: _gen(65, 65),
    "gen97": lambda: _gen(97, 97),
    "cgen70": lambda: _gen(70, 70) + 1j * _gen(70, 71),
    "gen1030": lambda: _gen(1030, 1030),
    "grcar100": lambda: _grcar(100),
    "jordan40": _jordan40,
    "graded60": _graded60,
    "tri30": lambda: np.triu(_gen(30, 30)),
    "eye7": lambda: np.eye(7),
    "zero5": lambda: np.zeros((5, 5)),
    "diag50": lambda: np.diag(np.linspace(-2.0, 3.0, 50) + 0.01 * np.arange(50) ** 2),
    "blk40": _blk40,
    "kron30": lambda: np.kron(np.eye(2), _gen(15, 15)),
    "sym65": lambda: (lambda G: G + G.T)(_gen(65, 65)),
    "gen97_big": lambda: np.ldexp(_gen(97, 97), 600),
    "gen97_small": lambda: np.ldexp(_gen(97, 97), -600),
}
NAMES = list(_BUILDERS)
# the normal and well-conditioned cases: every eigenvalue is compared with numpy.linalg.eigvals one to one
WELL_CONDITIONED = [k for k in NAMES if k.startswith("gen") or k in ("cgen70", "sym65", "diag50", "tri30")]
_cache = {}


def matrix(name):
    if name not in _cache:
        A = np.asfortranarray(_BUILDERS[name]())
        A.setflags(write=False)
        _cache[name] = A
    return _cache[name]


# ------------------------------------------------------------------ figures
def _in_range(A):
    """A scaled by a power of two (exactly) so that its norms can be formed; the figures do not change."""
    amax = float(np.max(np.abs(A))) if A.size else 0.0
    if amax > 0.0 and (amax < 1e-100 or amax > 1e100):
        return -int(np.floor(np.log2(amax)))
    return 0


def figures(A, w, V, cols=None):
    """(r, c) of the eigenpairs (w[cols], V) of A."""
    n = A.shape[0]
    e = _in_range(A)
    As = np.ldexp(A.real, e) + (1j * np.ldexp(A.imag, e) if np.iscomplexobj(A) else 0)
    ws = np.asarray(w)[np.arange(n) if cols is None else np.asarray(cols)]
    ws = np.ldexp(ws.real, e) + 1j * np.ldexp(ws.imag, e)
    fro = float(np.linalg.norm(As))
    if fro == 0.0:
        fro = 1.0
    R = As @ V - V * ws[None, :]
    r = float(np.max(np.linalg.norm(R, axis=0))) / (n * EPS * fro) if V.shape[1] else 0.0
    c = float(np.linalg.cond(V)) if V.shape[1] else 1.0
    return r, c


def lapack_figures(A):
    e = _in_range(A)
    As = np.ldexp(A.real, e) + (1j * np.ldexp(A.imag, e) if np.iscomplexobj(A) else 0)
    w, V = np.linalg.eig(As)
    return figures(As, w, V)


def match_one_to_one(a, b):
    """max |a_i - b_p(i)| over a greedy nearest pairing of two eigenvalue lists."""
    a = np.asarray(a, dtype=np.complex128)
    b = list(np.asarray(b, dtype=np.complex128))
    worst = 0.0
    for x in a[np.argsort(-np.abs(a))]:
        d = np.abs(np.asarray(b) - x)
        k = int(np.argmin(d))
        worst = max(worst, float(d[k]))
        b.pop(k)
    return worst


# ------------------------------------------------------------------ the restatement
def _blocks(H):
    n = H.shape[0]
    cuts = [0] + [i + 1 for i in range(n - 1) if H[i + 1, i] == 0] + [n]
    return list(zip(cuts[:-1], cuts[1:]))


def _laein_group(Hl, lams, eps3, kl):
    """xLAEIN's iteration for the shifts lams on the leading matrix Hl (kr x kr); the eigenvalues' own block
    starts at row kl.  Returns X (kr x g) and the number of shifts no start vector was accepted for."""
    kr = Hl.shape[0]
    g = len(lams)
    cplx = np.iscomplexobj(Hl) or np.iscomplexobj(lams)
    T = np.complex128 if cplx else np.float64
    B = np.empty((g, kr, kr), dtype=T)
    B[:] = Hl
    idx = np.arange(kr)
    B[:, idx, idx] -= np.asarray(lams, dtype=T)[:, None]
    with np.errstate(all="ignore"):
        for i in range(kr - 1):
            piv, sd = B[:, i, i].copy(), B[:, i + 1, i].copy()
            swap = _abs1(piv) < _abs1(sd)
            pivf = np.where(_abs1(piv) < eps3, eps3, piv)
            mult = np.where(swap, piv / np.where(swap, sd, 1), sd / pivf)
            r0, r1 = B[:, i, i + 1:].copy(), B[:, i + 1, i + 1:].copy()
            sw = swap[:, None]
            B[:, i, i + 1:] = np.where(sw, r1, r0)
            B[:, i + 1, i + 1:] = np.where(sw, r0 - mult[:, None] * r1, r1 - mult[:, None] * r0)
            B[:, i, i] = np.where(swap, sd, pivf)
            B[:, i + 1, i] = 0
        last = B[:, kr - 1, kr - 1]
        B[:, kr - 1, kr - 1] = np.where(_abs1(last) < eps3, eps3, last)
    rootn = np.sqrt(kr)
    growto = 0.1 / rootn
    rtemp = eps3 / (rootn + 1.0)
    X = np.zeros((kr, g), dtype=T)
    failed = 0
    for q in range(g):
        U = np.triu(B[q])
        ok = False
        for its in range(1, kr - kl + 1):
            v = np.zeros(kr, dtype=T)
            if its == 1:
                v[kl:] = eps3
            else:
                v[kl:] = rtemp
                v[kl] = eps3
                v[kr - its + 1] -= eps3 * rootn
            with np.errstate(all="ignore"):
                x = sla.solve_triangular(U, v, lower=False, check_finite=False)
            if np.sum(_abs1(x)) >= growto:
                ok = True
                break
        failed += 0 if ok else 1
        mx = np.max(_abs1(x))
        X[:, q] = x / mx if mx > 0 and np.isfinite(mx) else x
    return X, failed


def normalise(V):
    """unit 2-norm, the largest-modulus component (the first on ties) real and positive"""
    V = np.array(V, dtype=np.complex128, order="F")
    for j in range(V.shape[1]):
        a = np.abs(V[:, j])
        k = int(np.argmax(a))
        if a[k] > 0:
            V[:, j] *= np.conj(V[k, j]) / a[k]
            V[k, j] = a[k]
            V[:, j] /= np.linalg.norm(V[:, j])
    return V


def eig_ref(A, group=16):
    """(w, V, not_converged) by the scheme of csrc/eig.hip.  w is ordered block by block (numpy's order
    inside a block), V[:, j] belongs to w[j]."""
    A = np.asarray(A)
    n = A.shape[0]
    real = not np.iscomplexobj(A)
    amax = float(np.max(np.abs(A.real) if real else np.maximum(np.abs(A.real), np.abs(A.imag)))) if n else 0.0
    e = 0
    if np.isfinite(amax) and amax > 0.0 and (amax < SMLNUM or amax > 1.0 / SMLNUM):
        e = -int(np.floor(np.log2(amax)))
    As = np.ldexp(A, e) if real else np.ldexp(A.real, e) + 1j * np.ldexp(A.imag, e)
    if n >= 3:
        H, Q = sla.hessenberg(As, calc_q=True)
    else:
        H, Q = As.copy(), np.eye(n)
    w = np.zeros(n, dtype=np.complex128)
    Y = np.zeros((n, n), dtype=np.complex128)
    failed = 0
    for kl, kr in _blocks(H):
        Hb = H[kl:kr, kl:kr]
        wb = np.linalg.eigvals(Hb).astype(np.complex128)
        w[kl:kr] = wb
        hnorm = float(np.max(np.sum(np.abs(Hb), axis=0)))
        eps3 = hnorm * EPS if hnorm > 0 else TINY * ((kr - kl) / EPS)
        second = np.zeros(kr - kl, dtype=bool)   # the second member of a real matrix's conjugate pair
        if real:
            for k in range(kr - kl - 1):
                if (not second[k] and wb[k].imag != 0 and wb[k + 1].real == wb[k].real
                        and wb[k + 1].imag == -wb[k].imag):
                    second[k + 1] = True
        wp = wb.copy()
        for k in range(kr - kl):
            if second[k]:
                wp[k] = np.conj(wp[k - 1])
                continue
            x = wb[k]
            for _ in range(k + 1):
                close = [i for i in range(k - 1, -1, -1) if abs(wp[i].real - x.real) + abs(wp[i].imag - x.imag) < eps3]
                if not close:
                    break
                x = x + eps3
            wp[k] = x
        Hl = H[:kr, :kr]
        jobs_r = [k for k in range(kr - kl) if real and wb[k].imag == 0]
        jobs_c = [k for k in range(kr - kl) if not second[k] and not (real and wb[k].imag == 0)]
        for jobs, as_real in ((jobs_r, True), (jobs_c, False)):
            for g0 in range(0, len(jobs), group):
                ks = jobs[g0:g0 + group]
                lams = wp[ks].real if as_real else wp[ks]
                X, f = _laein_group(Hl, lams, eps3, kl)
                failed += f
                for q, k in enumerate(ks):
                    Y[:kr, kl + k] = X[:, q]
                    if real and not as_real and k + 1 < kr - kl and second[k + 1]:
                        Y[:kr, kl + k + 1] = np.conj(X[:, q])
    V = normalise(Q @ Y)
    if real:   # a conjugate partner: the bitwise conjugate; a real eigenvalue: a real vector
        for j in range(n):
            if w[j].imag == 0:
                V[:, j] = V[:, j].real
    return np.ldexp(w.real, -e) + 1j * np.ldexp(w.imag, -e), V, failed
