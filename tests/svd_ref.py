"""NumPy restatement of svd (csrc/svd.hip) and the named matrices its tests share.

svd_ref follows the device code step by step: the work on A^H for m < n, the power-of-two scaling, the column
blocks of 32 (real) / 16 (complex), the round-robin schedule of block pairs, tol = sqrt(m) eps, the skip test,
cyclic two-sided Jacobi on the pair's Gram matrix with the disjoint rotations of an inner step applied at
once, the Newton-Schulz polish of the accumulated rotation, and the finish (norms, stable descending sort,
completion of the columns whose singular value is exactly 0, phase convention).  Only the order of the
floating-point sums differs (BLAS here, MFMA tiles there).

hestenes_longdouble is a plain (not blocked) one-sided Jacobi in numpy.longdouble for small real matrices: the
reference for the relative accuracy of small singular values.
"""
import numpy as np

EPS = 2.0 ** -52
MAX_INNER = 30


# ------------------------------------------------------------------ named matrices
def _rng(seed):
    return np.random.default_rng(seed)


def _orth(rng, m, n):
    return np.linalg.qr(rng.standard_normal((m, n)))[0]


def _hilbert(n):
    i = np.arange(n)
    return 1.0 / (i[:, None] + i[None, :] + 1.0)


def _rand(seed, m, n, cplx=False):
    g = _rng(seed)
    A = g.standard_normal((m, n))
    if cplx:
        A = A + 1j * g.standard_normal((m, n))
    return A


def _cond1e12_96():
    g = _rng(112)
    return (_orth(g, 96, 96) * np.logspace(0, -12, 96)) @ _orth(g, 96, 96).T


def _rank20of72():
    g = _rng(120)
    return g.standard_normal((72, 20)) @ g.standard_normal((20, 72))


def _rank1_70():
    g = _rng(121)
    return np.outer(g.standard_normal(70), g.standard_normal(70))


def _dupcols50x40():
    A = _rand(123, 50, 40)
    A[:, 20:] = A[:, :20]   # every column twice: 20 singular values are 0, exactly or to rounding
    return A


def _diag50():
    d = np.arange(1, 51) * np.where(np.arange(50) % 3 == 0, -1.0, 1.0)
    return np.diag(_rng(124).permutation(d))


_BUILD = {
    "n1": lambda: np.array([[-3.0]]),
    "n2": lambda: np.array([[1.0, 2.0], [3.0, 4.0]]),
    "rand9": lambda: _rand(101, 9, 9),
    "rand33": lambda: _rand(102, 33, 33),
    "rand64": lambda: _rand(103, 64, 64),
    "rand65": lambda: _rand(104, 65, 65),
    "rand97": lambda: _rand(105, 97, 97),
    "tall130x70": lambda: _rand(106, 130, 70),
    "tall300x97": lambda: _rand(107, 300, 97),
    "wide70x130": lambda: _rand(108, 70, 130),
    "crand65": lambda: _rand(109, 65, 65, True),
    "ctall90x40": lambda: _rand(110, 90, 40, True),
    "cond1e12_96": _cond1e12_96,
    "hilbert64": lambda: _hilbert(64),
    "graded30x24": lambda: _rand(113, 30, 24) * np.logspace(0, -40, 24),
    "rank20of72": _rank20of72,
    "rank1_70": _rank1_70,
    "ones40": lambda: np.ones((40, 40)),
    "dupcols50x40": _dupcols50x40,
    "eye33": lambda: np.eye(33),
    "zero9x5": lambda: np.zeros((9, 5)),
    "diag50": _diag50,
    "rand97_big": lambda: np.ldexp(_rand(105, 97, 97), 600),
    "rand97_small": lambda: np.ldexp(_rand(105, 97, 97), -600),
}
NAMES = list(_BUILD)
RANK_DEFICIENT = ["rank20of72", "rank1_70", "ones40", "dupcols50x40", "zero9x5"]
_cache = {}


def matrix(name):
    if name not in _cache:
        A = np.asfortranarray(_BUILD[name]())
        A.setflags(write=False)
        _cache[name] = A
    return _cache[name]


# ------------------------------------------------------------------ the restatement
def block_width(A):
    return 16 if np.iscomplexobj(A) else 32


def round_robin(cnt, s, i):
    """pair i of step s of the circle schedule on cnt (even) players"""
    r = cnt - 1
    if i == 0:
        return r, s % r
    return (s + i) % r, (s - i + r) % r


def schedule(n, b):
    """the steps of one sweep: lists of (first column p, first column q, width p, width q)"""
    nb = -(-n // b)
    width = lambda k: min(b, n - k * b)
    if nb == 1:
        return [[(0, 0, n, 0)]]
    cnt = nb + (nb & 1)
    steps = []
    for s in range(cnt - 1):
        st = []
        for i in range(cnt // 2):
            a, c = round_robin(cnt, s, i)
            p, q = min(a, c), max(a, c)
            if q < nb:
                st.append((p * b, q * b, width(p), width(q)))
        steps.append(st)
    return steps


def _offmax(G):
    d = np.sqrt(np.maximum(np.diag(G).real, 0.0))
    D = np.outer(d, d)
    with np.errstate(divide="ignore", invalid="ignore"):
        R = np.where(D > 0, np.abs(G) / np.where(D > 0, D, 1.0), 0.0)
    np.fill_diagonal(R, 0.0)
    return float(R.max()) if R.size else 0.0


def pair_jacobi(G, tol):
    """(max of the skip test, J or None where the pair is skipped)"""
    P = G.shape[0]
    off = _offmax(G)
    if not off > tol:
        return off, None
    G = G.copy()
    J = np.eye(P, dtype=G.dtype)
    cnt = P + (P & 1)
    idx = []
    for s in range(cnt - 1):
        pq = [round_robin(cnt, s, i) for i in range(cnt // 2)]
        pq = [(min(a, c), max(a, c)) for a, c in pq if max(a, c) < P]
        idx.append((np.array([a for a, _ in pq], dtype=int), np.array([c for _, c in pq], dtype=int)))
    for _ in range(MAX_INNER):
        for p, q in idx:
            app, aqq, g = G[p, p].real, G[q, q].real, G[p, q]
            ag = np.abs(g)
            act = (app > 0) & (aqq > 0) & (ag > 0)   # plain cyclic Jacobi: every non-zero entry is rotated
            if not act.any():
                continue
            d = aqq - app
            ags = np.where(act, ag, 1.0)
            t = np.where(act, np.where(d < 0, -2.0, 2.0) * ags / (np.abs(d) + np.hypot(d, 2.0 * ags)), 0.0)
            c = 1.0 / np.sqrt(1.0 + t * t)
            sw = np.where(act, (g / ags) * (t * c), 0.0)
            Gp, Gq = G[:, p].copy(), G[:, q].copy()
            G[:, p] = c * Gp - np.conj(sw) * Gq
            G[:, q] = sw * Gp + c * Gq
            Gp, Gq = G[p, :].copy(), G[q, :].copy()
            G[p, :] = c[:, None] * Gp - sw[:, None] * Gq
            G[q, :] = np.conj(sw)[:, None] * Gp + c[:, None] * Gq
            pa, qa = p[act], q[act]
            G[pa, qa] = 0.0
            G[qa, pa] = 0.0
            G[pa, pa] = G[pa, pa].real
            G[qa, qa] = G[qa, qa].real
            Jp, Jq = J[:, p].copy(), J[:, q].copy()
            J[:, p] = c * Jp - np.conj(sw) * Jq
            J[:, q] = sw * Jp + c * Jq
        if not _offmax(G) > tol:
            break
    J = J @ (1.5 * np.eye(P) - 0.5 * (J.conj().T @ J))
    return off, J


def _complete(U, zero_cols):
    m = U.shape[0]
    nxt = 0
    thr = 0.5
    while nxt < len(zero_cols) and thr > 1e-3:
        for k in range(m):
            if nxt == len(zero_cols):
                break
            v = np.zeros(m, dtype=U.dtype)
            v[k] = 1.0
            for _ in range(2):
                v = v - U @ (U.conj().T @ v)
            nrm = np.linalg.norm(v)
            if nrm >= thr:
                U[:, zero_cols[nxt]] = v / nrm
                nxt += 1
        thr *= 0.25
    assert nxt == len(zero_cols)


def _phase(Z, Y):
    for j in range(Z.shape[1]):
        k = int(np.argmax(np.abs(Z[:, j])))
        pm = abs(Z[k, j])
        if pm > 0:
            u = np.conj(Z[k, j]) / pm
            Z[:, j] *= u
            Z[k, j] = pm
            if Y is not None:
                Y[:, j] *= u


def svd_ref(A, max_sweeps=60):
    """(U, s, V, sweeps, not_converged) with A = U diag(s) V^H, as eigsol_svd_dense returns them"""
    A = np.asarray(A)
    wide = A.shape[0] < A.shape[1]
    W = np.array(A.conj().T if wide else A, order="F", copy=True)
    m, n = W.shape
    amax = max(np.abs(W.real).max(), np.abs(W.imag).max()) if W.size else 0.0
    esc = -int(np.floor(np.log2(amax))) if amax > 0 else 0
    if amax > 0:
        W = np.ldexp(W.real, esc) + (1j * np.ldexp(W.imag, esc) if np.iscomplexobj(W) else 0)
    V = np.eye(n, dtype=W.dtype)
    b = block_width(W)
    tol = np.sqrt(m) * EPS
    steps = schedule(n, b)
    sweeps, above = 0, 0
    for sweep in range(1, max_sweeps + 1):
        above = 0
        for st in steps:
            for p, q, bp, bq in st:
                cols = np.r_[p:p + bp, q:q + bq]
                pos = np.r_[0:bp, b:b + bq]   # the pair's local columns: a ragged block leaves zero columns
                X = W[:, cols]
                G = np.zeros((2 * b, 2 * b), dtype=W.dtype)
                G[np.ix_(pos, pos)] = X.conj().T @ X
                off, J = pair_jacobi(G, tol)
                if off > tol:
                    above += 1
                if J is not None:
                    J = J[np.ix_(pos, pos)]
                    W[:, cols] = X @ J
                    V[:, cols] = V[:, cols] @ J
        sweeps = sweep
        if above == 0:
            break
    nrm = np.sqrt(np.sum(np.abs(W) ** 2, axis=0))
    perm = np.argsort(-nrm, kind="stable")
    s = np.ldexp(nrm[perm], -esc)
    U = np.zeros((m, n), dtype=W.dtype)
    for j, src in enumerate(perm):
        if nrm[src] > 0:
            U[:, j] = W[:, src] / nrm[src]
    Vo = V[:, perm].copy()
    zero_cols = [j for j, src in enumerate(perm) if nrm[src] == 0]
    if zero_cols:
        _complete(U, zero_cols)
    if wide:
        _phase(U, Vo)
        return Vo, s, U, sweeps, above
    _phase(Vo, U)
    return U, s, Vo, sweeps, above


# ------------------------------------------------------------------ figures
def _scaled(A, s):
    """A and s times one power of two that brings A's largest entry near 1 (the figures are scale free)"""
    amax = float(np.abs(A).max()) if A.size else 0.0
    if amax == 0 or not np.isfinite(amax):
        return A, s
    e = -int(np.floor(np.log2(amax)))
    As = np.ldexp(A.real, e) + (1j * np.ldexp(A.imag, e) if np.iscomplexobj(A) else 0)
    return As, np.ldexp(s, e)


def lapack_s(A):
    As, _ = _scaled(A, np.zeros(1))
    e = 0 if not A.size or np.abs(A).max() == 0 else -int(np.floor(np.log2(float(np.abs(A).max()))))
    return np.ldexp(np.linalg.svd(As, compute_uv=False), -e)


def figures(A, U, s, V, s_lapack):
    """r, o_u, o_v, e of the issue: N = max(m, n)"""
    N = max(A.shape)
    As, ss = _scaled(A, s)
    _, sl = _scaled(A, s_lapack)
    k = len(s)
    na = np.linalg.norm(As)
    num = np.linalg.norm(As @ V - U * ss)
    r = num / (N * EPS * na) if na > 0 else (0.0 if num == 0 else np.inf)
    ou = np.linalg.norm(U.conj().T @ U - np.eye(k)) / (N * EPS)
    ov = np.linalg.norm(V.conj().T @ V - np.eye(k)) / (N * EPS)
    e = float(np.max(np.abs(ss - sl)) / (N * EPS * sl[0])) if k and sl[0] > 0 else float(np.max(np.abs(ss), initial=0.0))
    return float(r), float(ou), float(ov), e


def lapack_figures(A):
    As, _ = _scaled(A, np.zeros(1))
    U, s, Vh = np.linalg.svd(As, full_matrices=False)
    return figures(As, U, s, Vh.conj().T, s)[:3]


def hestenes_longdouble(A, sweeps=60):
    """singular values (descending, float64) of a small real matrix by plain one-sided Jacobi in long double"""
    W = np.array(A, dtype=np.longdouble)
    n = W.shape[1]
    assert n <= 40 and not np.iscomplexobj(A)
    eps = np.finfo(np.longdouble).eps
    for _ in range(sweeps):
        rotated = False
        for p in range(n - 1):
            for q in range(p + 1, n):
                a, d, g = W[:, p] @ W[:, p], W[:, q] @ W[:, q], W[:, p] @ W[:, q]
                if a == 0 or d == 0 or abs(g) <= eps * np.sqrt(a) * np.sqrt(d):
                    continue
                rotated = True
                dl = d - a
                t = (2 if dl >= 0 else -2) * g / (abs(dl) + np.sqrt(dl * dl + 4 * g * g))
                c = 1 / np.sqrt(1 + t * t)
                sn = t * c
                wp = W[:, p].copy()
                W[:, p] = c * wp - sn * W[:, q]
                W[:, q] = sn * wp + c * W[:, q]
        if not rotated:
            break
    s = np.sqrt(np.sum(W * W, axis=0))
    return np.sort(s)[::-1].astype(np.float64)


def max_relative_error(s, s_ref):
    return float(np.max(np.abs(s - s_ref) / s_ref))
