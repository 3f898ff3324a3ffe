"""NumPy restatement of eigh(method="dc"): Cuppen's divide and conquer on the tridiagonal matrix of
eigh_ref.tridiagonal, with Gu and Eisenstat's stabilisation, step for step what csrc/eigh_dc.hip does:

  scale     every split block times the power of two that brings its largest entry into [1, 2), undone on the
            eigenvalues (exact);
  plan      every split block is halved down to leaves of order <= leaf; at a cut c: rho = e_c, d_c -= rho,
            d_{c+1} -= rho;
  leaves    any symmetric tridiagonal eigensolver (numpy.linalg.eigh here, implicit QL on the device);
  deflate   dlaed2's rules (deflate below): z normalised and ||z||^2 folded into rho, the poles sorted,
            tol = 8 u max(max |d|, max |z|), rho |z_j| <= tol dropped, close poles rotated together;
  secular   every root relative to its nearer pole (the origin o_i, chosen by the sign of f at the midpoint),
            by bisection on mu = lambda - d_o: geometric steps while the bracket spans more than a factor 4,
            stopped when the bracket cannot be halved;
  Loewner   zhat_j = sign(z_j) sqrt(prod_i (lambda_i - d_j) / prod_{i != j} (d_i - d_j) / rho), as a running
            product of ratios; every difference is (d_o - d_j) + mu, never d_j - lambda;
  vectors   u_ji = zhat_j / ((d_j - d_o) - mu_i), unit columns; Q <- Q U.

Shared by tests/test_eigh_dc_cpu.py and the GPU tests of the method.  References are computed once."""
import functools

import numpy as np

import eigh_ref as R

U_ROUND = 2.0 ** -53      # unit roundoff (dlamch('E'))
MAX_STEPS = 400           # the secular bisection's cap (the device kernel's)


def deflate(d, z, rho):
    """dlaed2's deflation of D + rho z z^T (d: the poles, any order).  Returns a dict: k, perm (new place ->
    old index; the k kept poles first, ascending), dk (n: kept poles, then the deflated values), zk (n: kept
    z, then zeros), rho (rho ||z||^2), rot (list of (a, b, c, s): columns a, b <- c a + s b, c b - s a), tol."""
    d = np.array(d, dtype=np.float64)
    z = np.array(z, dtype=np.float64)
    n = d.size
    nrm2 = 0.0
    for v in z:                       # a fixed order, as the C code
        nrm2 += v * v
    nrm = np.sqrt(nrm2)
    if nrm > 0:
        z = z / nrm
    rho = rho * nrm2
    order = np.argsort(d, kind="stable")
    tol = 8.0 * U_ROUND * max(np.abs(d).max(), np.abs(z).max())
    kept, gone, rot = [], [], []
    if rho * np.abs(z).max() <= tol:
        gone = list(order)
    else:
        pj = -1
        for j in order:
            if rho * abs(z[j]) <= tol:
                gone.append(j)
            elif pj < 0:
                pj = j
            else:
                s, c = z[pj], z[j]
                tau = np.hypot(c, s)
                t = d[j] - d[pj]
                c, s = c / tau, -s / tau
                if abs(t * c * s) <= tol:
                    z[j], z[pj] = tau, 0.0
                    rot.append((int(pj), int(j), float(c), float(s)))
                    t = d[pj] * c * c + d[j] * s * s
                    d[j] = d[pj] * s * s + d[j] * c * c
                    d[pj] = t
                    gone.append(pj)
                else:
                    kept.append(pj)
                pj = j
        kept.append(pj)
    perm = np.array(kept + gone, dtype=np.int64)
    k = len(kept)
    zk = np.zeros(n)
    zk[:k] = z[perm[:k]]
    return dict(k=k, perm=perm, dk=d[perm], zk=zk, rho=float(rho), rot=rot, tol=float(tol))


def _g(delta, z2, rho, orig, mu):
    """1 + rho sum_j z_j^2 / ((d_j - d_o) - mu), one value per root, summed in pole order."""
    den = (delta[None, :] - delta[orig][:, None]) - mu[:, None]
    return 1.0 + rho * np.cumsum(z2[None, :] / den, axis=1)[:, -1]


def secular(delta, z, rho):
    """(orig, mu, steps): root i = delta[orig[i]] + mu[i] of 1 + rho sum z_j^2 / (delta_j - x)."""
    k = delta.size
    z2 = z * z
    if k == 1:
        return np.zeros(1, dtype=np.int64), np.array([rho * z2[0]]), 0
    nrm2 = 0.0
    for v in z2:
        nrm2 += v
    idx = np.arange(k)
    half = np.empty(k)
    half[:-1] = 0.5 * (delta[1:] - delta[:-1])
    half[-1] = rho * nrm2
    orig = idx.copy()
    fm = _g(delta, z2, rho, idx[:-1], half[:-1])          # f at the midpoints, seen from the left pole
    right = np.r_[fm <= 0.0, False]                        # root in the right half: origin i + 1, mu < 0
    orig[right] += 1
    sgn = np.where(right, -1.0, 1.0)
    a, b = np.zeros(k), half.copy()                        # nu = |mu| in (a, b]
    steps = 0
    live = np.ones(k, dtype=bool)
    while live.any() and steps < MAX_STEPS:
        with np.errstate(over="ignore", invalid="ignore"):
            gm = np.sqrt(a * b)
            mid = a + 0.5 * (b - a)
            m = np.where(a == 0.0, b * 2.0 ** -20, np.where((b > 4.0 * a) & (a < gm) & (gm < b), gm, mid))
        live &= (a < m) & (m < b)
        if not live.any():
            break
        g = _g(delta, z2, rho, orig, sgn * m)
        up = np.where(right, g > 0.0, g <= 0.0)            # the root's |mu| is above m
        a = np.where(live & up, m, a)
        b = np.where(live & ~up, m, b)
        steps += 1
    nu = np.where(a == 0.0, b, a + 0.5 * (b - a))
    return orig, sgn * nu, steps


def loewner(delta, z, rho, orig, mu):
    k = delta.size
    w = np.empty(k)
    for j in range(k):
        lam_d = (delta[orig] - delta[j]) + mu              # lambda_i - d_j
        p = lam_d[j]
        for i in range(k):
            if i != j:
                p *= lam_d[i] / (delta[i] - delta[j])
        w[j] = p
    return np.where(z < 0, -1.0, 1.0) * np.sqrt(np.abs(w) / rho)


def _loewner_fast(delta, z, rho, orig, mu):
    """loewner() with the inner loop as one cumulative product per j (the same order of operations)."""
    k = delta.size
    lam_d = (delta[orig][None, :] - delta[:, None]) + mu[None, :]      # [j, i]
    den = delta[None, :] - delta[:, None]
    np.fill_diagonal(den, 1.0)
    ratio = lam_d / den
    diag = np.diagonal(lam_d).copy()
    np.fill_diagonal(ratio, 1.0)
    w = np.cumprod(np.c_[diag, ratio], axis=1)[:, -1]
    return np.where(z < 0, -1.0, 1.0) * np.sqrt(np.abs(w) / rho)


def merge(d, z, rho, Q, stats=None):
    """Eigenpairs of diag(d) + rho z z^T applied to the columns of Q: (values, Q_new), the kept roots first
    (ascending), then the deflated values."""
    D = deflate(d, z, rho)
    Q = Q.copy()
    for a, b, c, s in D["rot"]:
        qa, qb = Q[:, a].copy(), Q[:, b].copy()
        Q[:, a], Q[:, b] = c * qa + s * qb, c * qb - s * qa
    Q = Q[:, D["perm"]]
    k = D["k"]
    lam = D["dk"].copy()
    if stats is not None:
        stats["merges"] = stats.get("merges", 0) + 1
        stats["deflated"] = stats.get("deflated", 0) + d.size - k
        stats["poles"] = stats.get("poles", 0) + d.size
    if k:
        delta, zk = D["dk"][:k], D["zk"][:k]
        orig, mu, steps = secular(delta, zk, D["rho"])
        if stats is not None:
            stats["steps"] = max(stats.get("steps", 0), steps)
        zh = _loewner_fast(delta, zk, D["rho"], orig, mu)
        Um = zh[:, None] / ((delta[:, None] - delta[orig][None, :]) - mu[None, :])
        Um /= np.sqrt(np.cumsum(Um * Um, axis=0)[-1])[None, :]
        Q[:, :k] = Q[:, :k] @ Um
        lam[:k] = delta[orig] + mu
    return lam, Q


def _solve(d, e, leaf, stats):
    n = d.size
    if n <= leaf:
        if n == 1:
            return d.copy(), np.ones((1, 1))
        return np.linalg.eigh(np.diag(d) + np.diag(e, 1) + np.diag(e, -1))
    n1 = n // 2
    rho = e[n1 - 1]
    d = d.copy()
    d[n1 - 1] -= rho
    d[n1] -= rho
    w1, Q1 = _solve(d[:n1], e[:n1 - 1], leaf, stats)
    w2, Q2 = _solve(d[n1:], e[n1:], leaf, stats)
    Q = np.zeros((n, n))
    Q[:n1, :n1], Q[n1:, n1:] = Q1, Q2
    return merge(np.r_[w1, w2], np.r_[Q1[-1], Q2[0]], rho, Q, stats)


def split_blocks(d, e):
    """dstebz's splitting rule, as eigsol_tridiag_plan applies it: the block starts, with n appended."""
    starts = [0]
    for i in range(d.size - 1):
        ae = abs(e[i])
        if ae == 0 or ae <= R.EPS * np.sqrt(abs(d[i]) * abs(d[i + 1])) or ae * ae <= np.finfo(float).tiny:
            starts.append(i + 1)
    return starts + [d.size]


def block_exponent(d, e):
    """k with 2^k max(|d_i|, |e_i|) in [1, 2) (0 for a zero block): the exact scaling every split block gets
    before the plan, as dstedc scales to unit max-norm.  dlaed2's tol = 8 u max(max |d|, max |z|) takes
    |z| <= 1 as the scale of the poles; on an unscaled block of small norm it deflates what matters."""
    amax = max(np.abs(d).max(), np.abs(e).max() if e.size else 0.0)
    return 0 if amax == 0 else 1 - int(np.frexp(amax)[1])


def tridiagonal_dc(d, e, leaf=64, stats=None, scale=True):
    """(w ascending, Z) of tridiag(d, e) by divide and conquer; equal values in block order.  scale=False
    leaves the blocks at their own scale (what the tests show to be wrong for small norms)."""
    n = d.size
    starts = split_blocks(d, e)
    w = np.empty(n)
    Z = np.zeros((n, n))
    blk = np.empty(n, dtype=np.int64)
    for b in range(len(starts) - 1):
        b0, b1 = starts[b], starts[b + 1]
        k = block_exponent(d[b0:b1], e[b0:b1 - 1]) if scale else 0
        wb, Z[b0:b1, b0:b1] = _solve(np.ldexp(d[b0:b1], k), np.ldexp(e[b0:b1 - 1], k), leaf, stats)
        w[b0:b1] = np.ldexp(wb, -k)
        blk[b0:b1] = b
    order = np.lexsort((np.arange(n), blk, w))
    return w[order], Z[:, order]


def restatement(A, leaf=64, stats=None, scale=True):
    """(w, Z) of the Hermitian matrix whose lower triangle is A's, all pairs."""
    d, e, D, Q = R.tridiagonal(A)
    w, z = tridiagonal_dc(d, e, leaf, stats, scale)
    return w, Q @ (D[:, None] * z)


@functools.lru_cache(maxsize=None)
def reference(name, leaf=64):
    w, Z = restatement(R.matrix(name), leaf)
    w.setflags(write=False)
    Z.setflags(write=False)
    return w, Z


@functools.lru_cache(maxsize=None)
def evd(name):
    """(w, Z, r, o) of scipy.linalg.eigh(driver="evd") on the named matrix: LAPACK's divide and conquer."""
    import scipy.linalg as sl
    A = R.mirror_lower(R.matrix(name))
    w, Z = sl.eigh(A, driver="evd")
    w.setflags(write=False)
    Z.setflags(write=False)
    return w, Z, R.r_figure(A, w, Z), R.o_figure(Z)
