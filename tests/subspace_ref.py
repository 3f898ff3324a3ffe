"""numpy restatement of the block subspace iteration (csrc/subspace.hip) and the test matrices it is
pinned on.  Same steps and the same stopping rules as the device driver; only the rounding of the
reductions and of eig(B) differs (numpy.linalg.eig here, the library's own small QR there)."""
import numpy as np
import scipy.sparse as sp

N = 1500
TOL = 1e-12
RTOL = 1e-9
MAXIT = 500


def is_close_relative(a, b, tol):
    return abs(a - b) <= tol * (1 + abs(a))


def ritz_order(w):
    """|theta| descending; inside a run of neighbours whose moduli agree to 1e-12 relative, the larger
    imaginary part first."""
    p = sorted(range(len(w)), key=lambda i: -abs(w[i]))
    i = 0
    while i < len(p):
        j = i + 1
        while j < len(p) and abs(w[p[j - 1]]) - abs(w[p[j]]) <= 1e-12 * abs(w[p[j - 1]]):
            j += 1
        p[i:j] = sorted(p[i:j], key=lambda t: -w[t].imag)
        i = j
    return p


class RankLoss(Exception):
    pass


def _chol_upper(G):
    m = G.shape[0]
    thr = m * 2.0 ** -52 * np.max(np.diag(G).real)
    G = G.copy()
    R = np.zeros_like(G)
    for k in range(m):
        d = G[k, k].real
        if not d > 0 or d < thr:
            raise RankLoss(k)
        R[k, k] = np.sqrt(d)
        R[k, k + 1:] = G[k, k + 1:] / R[k, k]
        G[k + 1:, k + 1:] -= np.outer(R[k, k + 1:].conj(), R[k, k + 1:])
    return R


def cholqr2(Z, G=None):
    for p in range(2):
        if G is None:
            G = Z.conj().T @ Z
        R = _chol_upper(G)
        Z = np.linalg.solve(R.T, Z.T).T          # Z R^-1
        G = None
    return Z


def subspace_iteration(A, k, X0, tol=TOL, rtol=RTOL, max_iterations=MAXIT):
    """Returns dict(eigenvalues, eigenvectors, residuals, iterations, converged, Q)."""
    Q = cholqr2(np.array(X0))
    old = None
    conv = False
    it = 0
    for it in range(1, max_iterations + 1):
        Z = A @ Q
        B = Q.conj().T @ Z
        G = Z.conj().T @ Z
        w, Y = np.linalg.eig(B)
        p = ritz_order(w)
        theta, Y = w[p].astype(complex), Y[:, p].astype(complex)
        if it > 1:
            used = set()
            ok = True
            for j in range(k):
                cand = [l for l in range(k) if l not in used]
                best = min(cand, key=lambda l: abs(theta[j] - old[l]))
                used.add(best)
                if not is_close_relative(theta[j], old[best], tol):
                    ok = False
                    break
            if ok and rtol != 0:
                for j in range(k):
                    x = Q @ Y[:, j]
                    r = Z @ Y[:, j] - theta[j] * x
                    if not np.linalg.norm(r) / np.linalg.norm(x) <= rtol * (1 + abs(theta[j])):
                        ok = False
                        break
            if ok:
                conv = True
                break
        old = theta[:k].copy()
        if it == max_iterations:
            break
        Q = cholqr2(Z, G)
    X = Q @ Y[:, :k]
    nrm = np.linalg.norm(X, axis=0)
    Ys = Y[:, :k] / nrm
    X = Q @ Ys
    res = np.linalg.norm(Z @ Ys - X * theta[:k], axis=0)
    return dict(eigenvalues=theta[:k], eigenvectors=X, residuals=res, iterations=it, converged=conv, Q=Q)


# ------------------------------------------------------------------ the pinned inputs (a) - (c)
def case_a():
    """Symmetric f64: diag(d) + 0.05 (S + S^T); k = 4, m = 8."""
    rng = np.random.default_rng(101)
    d = rng.uniform(0, 3, N)
    d[:5] = [10, 9, 8, 7, 6.5]
    S = sp.random(N, N, density=4 / N, random_state=np.random.default_rng(102), format="csr")
    A = (sp.diags(d) + 0.05 * (S + S.T)).tocsr()
    X0 = np.random.default_rng(103).uniform(-1, 1, (N, 8))
    return A, 4, 8, X0


def case_b():
    """Nonsymmetric f64, dominant conjugate pair 6 +- 8i, then 8 and -7; k = 4, m = 8."""
    rng = np.random.default_rng(201)
    d = rng.uniform(-3, 3, N)
    d[2], d[3] = 8, -7
    D = sp.lil_matrix((N, N))
    D.setdiag(d)
    D[0, 0], D[0, 1], D[1, 0], D[1, 1] = 6, 8, -8, 6
    S = sp.random(N, N, density=4 / N, random_state=np.random.default_rng(202), format="csr")
    A = (D.tocsr() + 0.05 * S).tocsr()
    X0 = np.random.default_rng(203).uniform(-1, 1, (N, 8))
    return A, 4, 8, X0


def case_c():
    """c128 upper triangular; the eigenvalues are the diagonal; k = 4, m = 6, complex X0."""
    rng = np.random.default_rng(301)
    diag = rng.uniform(0, 3, N) * np.exp(2j * np.pi * rng.uniform(0, 1, N))
    diag[:4] = [10j, -9, 8, 5 + 5j]
    S = sp.random(N, N, density=6 / N, random_state=np.random.default_rng(302), format="csr")
    A = (sp.diags(diag) + (0.1 + 0.1j) * sp.triu(S, 1)).tocsr()
    r = np.random.default_rng(303)
    X0 = r.uniform(-1, 1, (N, 6)) + 1j * r.uniform(-1, 1, (N, 6))
    return A, 4, 6, X0


CASES = {"a": case_a, "b": case_b, "c": case_c}


def dominant(A, k):
    """The k eigenvalues of largest modulus by numpy.linalg.eigvals."""
    w = np.linalg.eigvals(A.toarray())
    return w[np.argsort(-abs(w))][:k]


def match_error(got, want):
    """max over want of the distance to its nearest not-yet-used value of got, scaled by 1 + |want|."""
    got = list(got)
    worst = 0.0
    for z in want:
        j = min(range(len(got)), key=lambda i: abs(got[i] - z))
        worst = max(worst, abs(got[j] - z) / (1 + abs(z)))
        got.pop(j)
    return worst
