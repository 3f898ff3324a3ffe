"""Selections, the expected order, the constructed inputs and the LAPACK reference of the ``ordschur`` tests
(csrc/ordschur.hip).

A selection is defined on the diagonal blocks of a given (quasi-)triangular T, so a conjugate pair is always
taken or left as a whole.  The expected order after reordering is the stable partition of
``schur_ref.block_eigenvalues(T)``: the selected eigenvalues in their order, then the others in theirs, which
is LAPACK xTRSEN's order.

The constructed inputs ``pairs(n, first)`` are quasi-triangular with a 2 x 2 block on every row pair, after an
optional leading 1 x 1 block, so that pairs sit on even rows in one variant and on odd rows in the other and
straddle every nominal window boundary of the device code in one of the two.  Their orders are 3 and 4 (with
n2real and n3 of schur_ref: the four kinds of swap) and the window sizes' edges for the half-window H_REAL
the device code uses.
"""
import numpy as np
import scipy.linalg.lapack as lapack

import eig_ref as R
import schur_ref as S

EPS = S.EPS
H_REAL, H_CPLX = 47, 32   # csrc/ordschur.hpp, OrdDims
SELECTIONS = ["lhp", "alt", "last", "bottomhalf", "inside", "all", "none"]
PAIR_ORDERS = [3, 4, H_REAL, 2 * H_REAL, 2 * H_REAL - 1, 2 * H_REAL + 1, 4 * H_REAL + 1]
_pairs = {}


def blocks(T):
    """[(first row, rows)] of T's diagonal blocks."""
    T = np.asarray(T)
    n = T.shape[0]
    out, k = [], 0
    while k < n:
        two = k + 1 < n and not np.iscomplexobj(T) and T[k + 1, k] != 0
        out.append((k, 2 if two else 1))
        k += 2 if two else 1
    return out


def selection(T, name):
    """The boolean mask, one flag per row of T, of the named selection."""
    T = np.asarray(T)
    n = T.shape[0]
    w = S.block_eigenvalues(T)
    bl = blocks(T)
    mask = np.zeros(n, dtype=bool)
    if name == "lhp":
        take = [w[k].real < 0 for k, _ in bl]
    elif name == "alt":
        take = [i % 2 == 1 for i in range(len(bl))]
    elif name == "last":
        take = [i == len(bl) - 1 for i in range(len(bl))]
    elif name == "bottomhalf":
        take = [k >= n / 2 for k, _ in bl]
    elif name == "inside":
        med = float(np.median(np.abs(w))) if n else 0.0
        take = [abs(w[k]) < med for k, _ in bl]
    elif name == "all":
        take = [True] * len(bl)
    elif name == "none":
        take = [False] * len(bl)
    else:
        raise KeyError(name)
    for (k, sz), t in zip(bl, take):
        mask[k:k + sz] = t
    return mask


def pair_rule(T, mask):
    """LAPACK's rule: a flag on either row of a 2 x 2 block selects the pair."""
    out = np.array(mask, dtype=bool)
    for k, sz in blocks(T):
        out[k:k + sz] = np.any(out[k:k + sz])
    return out


def expected_order(T, mask):
    """The stable partition of T's eigenvalues by the mask (after the pair rule)."""
    w = S.block_eigenvalues(T)
    m = pair_rule(T, mask)
    return np.concatenate([w[m], w[~m]])


def pairs(n, first):
    """Quasi-triangular T of order n: strictly upper part N(0, 1) / sqrt(n); 2 x 2 blocks [a b; -c a] with
    b, c in [0.1, 1.1) on every row pair from row ``1 if first else 0`` on; 1 x 1 blocks elsewhere."""
    key = (n, bool(first))
    if key not in _pairs:
        rng = np.random.default_rng(1000 * n + int(first))
        T = np.triu(rng.standard_normal((n, n)), 1) / np.sqrt(n)
        d = rng.standard_normal(n)
        k = 1 if first else 0
        T[np.arange(n), np.arange(n)] = d
        while k + 1 < n:
            T[k + 1, k + 1] = T[k, k]
            T[k, k + 1] = 0.1 + rng.random()
            T[k + 1, k] = -(0.1 + rng.random())
            k += 2
        T = np.asfortranarray(T)
        T.setflags(write=False)
        _pairs[key] = T
    return _pairs[key]


def pairs_cases():
    return [(n, first) for n in PAIR_ORDERS for first in (False, True)]


def trsen(T, Z, mask):
    """LAPACK xTRSEN (no condition estimates) on (T, Z): (T', Z', w', m, info)."""
    T = np.asarray(T)
    sel = np.asarray(mask).astype(np.int32)
    if np.iscomplexobj(T):
        ts, qs, w, m, _, _, info = lapack.ztrsen(sel, np.array(T, order="F"), np.array(Z, order="F"), job="N", wantq=1)
        return ts, qs, np.asarray(w, dtype=np.complex128), int(m), int(info)
    ts, qs, wr, wi, m, _, _, info = lapack.dtrsen(sel, np.array(T, order="F"), np.array(Z, order="F"), job="N", wantq=1,
                                                  lwork=max(1, T.shape[0]), liwork=1)
    return ts, qs, wr + 1j * wi, int(m), int(info)


def order_error(A, w_new, w_expected):
    """max |w_new - w_expected|, position by position, formed under eig_ref._in_range's scaling of A."""
    if len(w_new) == 0:
        return 0.0
    e = R._in_range(A)
    d = S._scaled(np.asarray(w_new), e) - S._scaled(np.asarray(w_expected), e)
    return float(np.ldexp(np.max(np.abs(d)), -e))
