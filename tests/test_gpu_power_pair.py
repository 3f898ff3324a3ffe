"""The pair path of the fused power iteration: two reference iterations per pass over a windowed
CSR matrix (csr_pair_kernel), against the single-launch path (EIGSOL_POWER_PAIR=0)
and the CPU oracle.

The first product of a pair launch is bitwise a single launch's; the second defers the division
by the norm (y = A (s w1) / (s ||w1||), s a power of two), so only the rounding of that division
moves: traces agree to the existing trace test's bound (rtol 1e-13, atol 1e-13 max|trace|),
iterates to |x^H x'| >= 1 - 1e-12, and every count is equal.
"""
import numpy as np
import pytest
import scipy.sparse as sp

import pcsc_eigenvalue_solver_project_amd as E
from pcsc_eigenvalue_solver_project_amd import synthetic as S
from oracle import oracle as O

pytestmark = pytest.mark.gpu

PAIR_T = 16  # kPairT of csrc/csr_power.hip: slices per tile


def _session(ctx, csr, monkeypatch, pair, want_pass=None):
    """(matrix, session) built with the pair path on or forced off."""
    if pair:
        monkeypatch.delenv("EIGSOL_POWER_PAIR", raising=False)
    else:
        monkeypatch.setenv("EIGSOL_POWER_PAIR", "0")
    rp, ci, v, n = csr
    A = E.CsrMatrix(ctx, rp, ci, v, (n, n))
    s = E.PowerSession(A, trace_capacity=64)
    ipp = s.kernel_info()["iterations_per_pass"]
    assert ipp == (want_pass if want_pass is not None else (2 if pair else 1)), ipp
    assert ("csr_pair_kernel" in s.kernel_name()) == (ipp == 2)
    assert s.kernel_info()["variant"] == 5 and s.kernel_info()["iterations_per_launch"] == 1
    return A, s


def _fixed(ctx, csr, x0, iters, monkeypatch, pair, steps=None, want_pass=None):
    """iters iterations with tol < 0: (result, trace, launches)."""
    A, s = _session(ctx, csr, monkeypatch, pair, want_pass)
    s.begin(E.SolverOptions(iters, -1.0), x0)
    for k in (steps or [iters + 2]):
        s.step(k)
    done, launches = s.query()
    while not done:
        s.step(5)
        done, launches = s.query()
    res = s.finish()
    tr = s.trace(64)
    s.close()
    A.close()
    return res, tr, launches


def _assert_same_run(a, b):
    (ra, ta, la), (rb, tb, lb) = a, b
    assert ra.iterations == rb.iterations and la == lb and len(ta) == len(tb)
    assert ra.converged == rb.converged
    print("max trace diff", np.max(np.abs(ta - tb)) if len(ta) else 0.0, "of", np.max(np.abs(tb)) if len(tb) else 0.0)
    np.testing.assert_allclose(ta, tb, rtol=1e-13, atol=1e-13 * np.max(np.abs(tb)))
    ov = abs(np.vdot(ra.eigenvector, rb.eigenvector))
    print("overlap deficit", 1 - ov)
    assert ov >= 1 - 1e-12


def _band(n, w=64):
    rp, ci, v = S.band(n, 10, w=w)
    return rp, ci, v, n


@pytest.mark.parametrize("n,w", [(64 * 3 + 5, 64), (64 * 3 + 6, 64), (2 * PAIR_T * 64 + 64 + 17, 64),
                                 (2 * PAIR_T * 64 + 64 + 18, 64), (20000, 90)])
@pytest.mark.parametrize("iters", [30, 31])
def test_pair_matches_single_path(ctx, monkeypatch, n, w, iters):
    """Less than one tile; a tile boundary with a partial last slice; two halo slices per side.

    The sliced layout loads real windows in aligned pairs, so with an odd n the last slice's window
    cannot be padded to an even length inside x and the slice gathers: those matrices are not
    eligible and keep single launches (iterations_per_pass == 1).  Each odd shape therefore has
    an even neighbour with the same tile structure that does run the pair kernel."""
    csr = _band(n, w)
    x0 = S.start_vector(n)
    one = _fixed(ctx, csr, x0, iters, monkeypatch, pair=False)
    two = _fixed(ctx, csr, x0, iters, monkeypatch, pair=True, want_pass=2 if n % 2 == 0 else 1)
    assert two[0].iterations == iters and two[2] == iters + 2 and len(two[1]) == iters
    _assert_same_run(two, one)


def _assert_power_parity(res, ref, tol):
    lam, lam_ref = res.eigenvalue, ref["eigenvalue"]
    assert abs(lam - lam_ref) <= 1e-10 * (1 + abs(lam_ref)), (lam, lam_ref)
    assert res.converged == ref["converged"]
    if res.iterations != ref["iterations"]:
        assert abs(res.iterations - ref["iterations"]) == 1
        tr = ref["trace"]
        k = min(res.iterations, ref["iterations"]) - 1
        assert abs(tr[k] - tr[k - 1]) <= 10 * tol * (1 + abs(tr[k]))
    x, xr = res.eigenvector, ref["eigenvector"]
    assert abs(np.vdot(x, xr)) >= 1 - 1e-10
    assert abs(np.linalg.norm(x) - 1) <= 1e-12


@pytest.fixture(scope="module")
def band20k():
    n = 20000
    rp, ci, v = S.band(n, 10)
    x0 = S.start_vector(n)
    cp, ri, vv = O.csr_to_csc(rp, ci, v, n)
    return (rp, ci, v, n), x0, (cp, ri, vv)


# The oracle stops after 16 iterations at tol 1e-12 and after 15 at 3e-11 (its successive
# differences there are 9.8e-11, 9.8e-12, 5.6e-13 relative: a factor 3 from either tolerance), so
# the stop falls on a pair launch's own first iteration in one case and on the deferred second
# iteration of the previous pair in the other.
@pytest.mark.parametrize("tol,want_iters", [(1e-12, 16), (3e-11, 15)])
def test_pair_oracle_parity_stop_on_either_half(ctx, monkeypatch, band20k, tol, want_iters):
    csr, x0, (cp, ri, vv) = band20k
    ref = O.power_csc(cp, ri, vv, x0, 1000, tol, want_trace=True)
    assert ref["converged"] and ref["iterations"] == want_iters
    A, s = _session(ctx, csr, monkeypatch, pair=True)
    s.close()
    res = E.power_method(A, E.SolverOptions(1000, tol), x0)
    A.close()
    assert res.iterations == want_iters
    _assert_power_parity(res, ref, tol)


@pytest.mark.parametrize("max_iter", [0, 1, 2, 3])
def test_pair_small_max_iter(ctx, monkeypatch, band20k, max_iter):
    csr, x0, (cp, ri, vv) = band20k
    ref = O.power_csc(cp, ri, vv, x0, max_iter, 1e-12, want_trace=True)
    A, s = _session(ctx, csr, monkeypatch, pair=True)
    s.close()
    res = E.power_method(A, E.SolverOptions(max_iter, 1e-12), x0)
    A.close()
    assert res.iterations == ref["iterations"] == max_iter and not res.converged
    assert abs(res.eigenvalue - ref["eigenvalue"]) <= 1e-10 * (1 + abs(ref["eigenvalue"]))
    assert abs(np.vdot(res.eigenvector, ref["eigenvector"])) >= 1 - 1e-10


@pytest.fixture(scope="module")
def single30(ctx, band20k):
    """The single path's 30 fixed iterations on band20k (shared reference of the stepping tests)."""
    mp = pytest.MonkeyPatch()
    try:
        csr, x0, _ = band20k
        return _fixed(ctx, csr, x0, 30, mp, pair=False)
    finally:
        mp.undo()


@pytest.mark.parametrize("steps", [[1] * 7, [7], [3, 4], [40]], ids=["1x7", "7", "3+4", "40"])
def test_pair_stepping_patterns(ctx, monkeypatch, band20k, single30, steps):
    """Singles only, pairs with a single remainder, a pair split across two step() calls, and one
    call past the end: the same counts and, to 1e-13, the same eigenvalue."""
    csr, x0, _ = band20k
    run = _fixed(ctx, csr, x0, 30, monkeypatch, pair=True, steps=steps)
    assert run[0].iterations == 30 and run[2] == 32 and len(run[1]) == 30
    _assert_same_run(run, single30)
    assert abs(run[0].eigenvalue - single30[0].eigenvalue) <= 1e-13 * abs(single30[0].eigenvalue)


def _local(n, seed, min_len, max_len, empty_slice=None, reach=60):
    """Positive entries within `reach` columns of the diagonal, row lengths min_len..max_len (the
    sliced layout takes a matrix only while its padding stays small) and a few empty rows."""
    rng = np.random.default_rng(seed)
    rows, cols = [], []
    for i in range(n):
        L = int(rng.integers(min_len, max_len + 1))
        if i % 97 == 5 or (empty_slice is not None and i // 64 == empty_slice):
            L = 0
        lo, hi = max(0, i - reach), min(n, i + reach + 1)
        c = np.sort(rng.choice(np.arange(lo, hi), size=min(L, hi - lo), replace=False))
        rows.append(np.full(len(c), i))
        cols.append(c)
    rows, cols = np.concatenate(rows), np.concatenate(cols)
    M = sp.csr_matrix((rng.uniform(0.1, 1.0, len(rows)), (rows, cols)), shape=(n, n))
    M.sort_indices()
    return M.indptr, M.indices, M.data, n


@pytest.mark.parametrize("kind", ["long_rows", "empty_slice", "ragged"])
def test_pair_edges_of_the_layout(ctx, monkeypatch, kind):
    """Rows longer than the 12 and 16 register entries inside the window, an empty slice, ragged
    rows: the pair path runs (iterations_per_pass == 2) and matches the single path."""
    n = 64 * 21 + 10
    csr = {"long_rows": _local(n, 1, 27, 30), "empty_slice": _local(n, 2, 7, 10, empty_slice=5),
           "ragged": _local(n, 3, 8, 11)}[kind]
    if kind == "long_rows":
        assert np.max(np.diff(csr[0])) > 16
    x0 = S.start_vector(n)
    one = _fixed(ctx, csr, x0, 21, monkeypatch, pair=False)
    two = _fixed(ctx, csr, x0, 21, monkeypatch, pair=True)
    _assert_same_run(two, one)


def test_pair_zero_start_vector(ctx, monkeypatch, band20k):
    csr, _, _ = band20k
    x0 = np.zeros(csr[3])
    for pair in (False, True):
        A, s = _session(ctx, csr, monkeypatch, pair)
        s.close()
        res = E.power_method(A, E.SolverOptions(50, 1e-12), x0)
        A.close()
        assert res.iterations == 1 and not res.converged and res.eigenvalue == 0.0
        assert np.array_equal(res.eigenvector, x0)


def test_pair_first_product_zero(ctx, monkeypatch):
    """A = superdiagonal, x0 = e_0: A x0 = 0 (normY == 0 in iteration 0), and x0 = e_1: the norm
    vanishes one iteration later, on the other half."""
    n = 64 * 20 + 4
    i = np.arange(n - 1)
    M = sp.csr_matrix((np.full(n - 1, 2.0), (i, i + 1)), shape=(n, n))
    csr = (M.indptr, M.indices, M.data, n)
    for j in (0, 1, 2, 3):
        x0 = np.zeros(n)
        x0[j] = 1.0
        out = []
        for pair in (False, True):
            A, s = _session(ctx, csr, monkeypatch, pair)
            s.close()
            out.append(E.power_method(A, E.SolverOptions(50, 1e-12), x0))
            A.close()
        one, two = out
        assert two.iterations == one.iterations and two.converged == one.converged
        if j < 2:   # later starts stop on two equal (zero) Rayleigh quotients instead
            assert one.iterations == j + 1 and not one.converged
        assert two.eigenvalue == one.eigenvalue
        assert np.array_equal(two.eigenvector, one.eigenvector)


def test_pair_stream_segments_bitwise(ctx, monkeypatch):
    """4 MiB stream segments: the same path (iterations_per_pass == 2) and the same bits."""
    n = 200_000
    csr = _band(n)
    x0 = S.start_vector(n)
    opts = E.SolverOptions(300, 1e-12)
    out = []
    for seg in (None, 1 << 22):
        if seg:
            monkeypatch.setenv("EIGSOL_SLICE_SEG_BYTES", str(seg))
        A, s = _session(ctx, csr, monkeypatch, pair=True)
        s.close()
        out.append(E.power_method(A, opts, x0))
        A.close()
    assert out[0].iterations == out[1].iterations and out[0].eigenvalue == out[1].eigenvalue
    assert np.array_equal(out[0].eigenvector, out[1].eigenvector)


def test_pair_fallback_matrices_keep_the_single_path(ctx, monkeypatch):
    """Gather slices (uniform columns) are not eligible: one iteration per pass with or without the
    switch, and the same bits.  A rectangular matrix has no power session at all (powerMethod
    requires a square matrix), so there its product is compared instead."""
    n = 20000
    rp, ci, v = S.uniform(n, 16)
    x0 = S.start_vector(n)
    out = [_fixed(ctx, (rp, ci, v, n), x0, 12, monkeypatch, pair=p, want_pass=1) for p in (False, True)]
    assert out[0][2] == out[1][2] and out[0][0].iterations == out[1][0].iterations
    assert np.array_equal(out[0][1], out[1][1]) and out[0][0].eigenvalue == out[1][0].eigenvalue
    assert np.array_equal(out[0][0].eigenvector, out[1][0].eigenvector)
    m = 5000
    rp, ci, v = S.band(n, 10, nrows=m)          # m x n: the first m rows of the band matrix
    ys = []
    for pair in (False, True):
        if pair:
            monkeypatch.delenv("EIGSOL_POWER_PAIR", raising=False)
        else:
            monkeypatch.setenv("EIGSOL_POWER_PAIR", "0")
        A = E.CsrMatrix(ctx, rp, ci, v, (m, n))
        with pytest.raises(Exception):
            E.PowerSession(A)
        xd = ctx.malloc(x0.nbytes)
        ctx.h2d(xd, x0)
        yd = ctx.malloc(m * 8)
        A.spmv(xd, yd)
        ys.append(ctx.d2h(np.empty(m), yd))
        ctx.free(xd)
        ctx.free(yd)
        A.close()
    assert np.array_equal(ys[0], ys[1])
