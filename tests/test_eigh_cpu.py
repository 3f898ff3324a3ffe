"""CPU: the symmetric / Hermitian eigensolver's restatement (tests/eigh_ref.py) meets its own bounds, the
new C entries are exported and bound, eigsol_eigh_dense decides every status before any device call, and
eigsol_tridiag_plan (host only) returns the split blocks and clusters the device driver uses."""
import ctypes as C

import numpy as np
import pytest

import pcsc_eigenvalue_solver_project_amd as E
from pcsc_eigenvalue_solver_project_amd import _capi

import eigh_ref as R


@pytest.mark.parametrize("name", R.NAMES)
def test_restatement_bounds(name):
    """r <= 2 and o <= 2 for the restatement itself: the device conditions max(2, 3 ref) can be met."""
    A = R.matrix(name)
    w, Z, wl = R.reference(name)
    r, o = R.r_figure(A, w, Z), R.o_figure(Z)
    dw = float(np.abs(w - wl).max())
    print(f"{name}: r={r:.3f} o={o:.3f} |w-w_lapack|={dw:.3e} (bound {R.value_bound(A):.3e})")
    assert np.all(np.diff(w) >= 0)
    assert r <= 2 and o <= 2
    assert dw <= R.value_bound(A)


def test_lap300_closed_form():
    w = R.reference("lap300")[0]
    k = np.arange(1, 301)
    assert np.abs(w - (2 - 2 * np.cos(k * np.pi / 301))).max() <= R.value_bound(R.matrix("lap300"))


def test_symbols_exported_and_bound():
    L = C.CDLL(_capi.LIB_PATH)
    for s in ("eigsol_eigh_dense", "eigsol_tridiag_plan", "eigsol_eigh_stage_times"):
        assert hasattr(L, s), s
        assert s in _capi.SIGNATURES, s
    for s in ("eigh", "eigvalsh", "EighResult", "tridiag_plan"):
        assert hasattr(E, s), s


def _call(ctx, dtype, n, A, opts, w, m, Z=None):
    return E.lib().eigsol_eigh_dense(ctx, dtype, n, A, opts, w, Z, m, None)


def test_statuses_decided_without_a_device():
    fake = C.create_string_buffer(512)   # never dereferenced: every status below is decided first
    ctx = C.cast(fake, C.c_void_p)
    A = np.asfortranarray(np.eye(4))
    Ap = A.ctypes.data_as(C.c_void_p)
    w = np.zeros(4)
    wp = w.ctypes.data_as(C.c_void_p)
    m = C.c_int64(-1)
    INV, UNS = _capi.EIGSOL_E_INVALID, _capi.EIGSOL_E_UNSUPPORTED
    # null pointers with n > 0
    assert _call(None, 0, 4, Ap, None, wp, C.byref(m)) == INV
    assert _call(ctx, 0, 4, None, None, wp, C.byref(m)) == INV
    assert _call(ctx, 0, 4, Ap, None, None, C.byref(m)) == INV
    assert _call(ctx, 0, 4, Ap, None, wp, None) == INV
    assert _call(ctx, 0, -1, Ap, None, wp, C.byref(m)) == INV
    # n == 0: success, m = 0, even with a null context
    assert _call(None, 0, 0, None, None, None, C.byref(m)) == _capi.EIGSOL_OK and m.value == 0
    # selections
    O = _capi.EighOptionsC
    nan = float("nan")
    for bad in (O(3, 0, 0, 0.0, 1.0), O(-1, 0, 0, 0.0, 1.0), O(1, 2, 1, 0.0, 0.0), O(1, -1, 2, 0.0, 0.0),
                O(1, 0, 4, 0.0, 0.0), O(1, 4, 4, 0.0, 0.0), O(2, 0, 0, 1.0, 1.0), O(2, 0, 0, 2.0, 1.0),
                O(2, 0, 0, nan, 1.0), O(2, 0, 0, 0.0, nan)):
        assert _call(ctx, 0, 4, Ap, C.byref(bad), wp, C.byref(m)) == INV, tuple(getattr(bad, f[0]) for f in O._fields_)
    # scalar types without kernels, and orders above the blocked reduction's
    for dt in (_capi.EIGSOL_F32, _capi.EIGSOL_C64, _capi.EIGSOL_DD, _capi.EIGSOL_CDD):
        assert _call(ctx, dt, 4, Ap, None, wp, C.byref(m)) == UNS
    assert _call(ctx, 17, 4, Ap, None, wp, C.byref(m)) == INV
    assert _call(ctx, _capi.EIGSOL_F64, 16385, Ap, None, wp, C.byref(m)) == UNS
    assert _call(ctx, _capi.EIGSOL_C128, 8193, Ap, None, wp, C.byref(m)) == UNS
    assert b"order" in E.lib().eigsol_last_error()


def test_python_wrappers_validate():
    class Fake:
        handle = None
    with pytest.raises(E.EigSolError) as e:
        E.eigh(Fake(), np.zeros((3, 4)))
    assert e.value.status == _capi.EIGSOL_E_NOT_SQUARE
    with pytest.raises(E.EigSolError) as e:
        E.eigvalsh(Fake(), np.eye(3), select=("x", 0, 1))
    assert e.value.status == _capi.EIGSOL_E_INVALID
    with pytest.raises(E.EigSolError) as e:
        E.eigvalsh(Fake(), np.eye(3, dtype=np.float32))
    assert e.value.status in (_capi.EIGSOL_E_INVALID, _capi.EIGSOL_E_UNSUPPORTED)   # null context first
    assert E.eigvalsh(Fake(), np.zeros((0, 0))).size == 0


def _plan(name):
    d, e, _, _ = R.tridiagonal(R.matrix(name))
    w = R.reference(name)[0]
    return (d, e, w) + E.tridiag_plan(d, e, w)


def test_plan_blockdiag_two_blocks():
    d, e, w, block_of, cluster_of, nb, ncl = _plan("blockdiag")
    assert nb == 2
    assert np.array_equal(block_of, np.r_[np.zeros(33, np.int64), np.ones(31, np.int64)])
    # every eigenvalue goes to the block it is an eigenvalue of: clusters never mix blocks
    w0 = np.linalg.eigvalsh(R.matrix("blockdiag")[:33, :33])
    owner = np.array([int(np.abs(w0 - x).min() > 1e-10) for x in w])
    assert owner.sum() == 31
    for c in range(ncl):
        assert len(set(owner[cluster_of == c])) == 1
    assert sorted(set(cluster_of)) == list(range(ncl))


def test_plan_identity_all_split():
    d, e, w, block_of, cluster_of, nb, ncl = _plan("eye40")
    assert nb == 40 and ncl == 40
    assert np.array_equal(block_of, np.arange(40)) and np.array_equal(cluster_of, np.arange(40))


def test_plan_wilkinson_top_pairs():
    d, e, w, block_of, cluster_of, nb, ncl = _plan("wilk21")
    assert nb == 1 and not block_of.any()
    assert cluster_of[20] == cluster_of[19] and cluster_of[18] == cluster_of[17]
    assert cluster_of[20] != cluster_of[18] and cluster_of[17] != cluster_of[16]
    # the rule itself: a new cluster exactly where the gap exceeds 1e-3 ||T||_1
    nrm = max(abs(d[i]) + (e[i - 1] if i else 0) + (e[i] if i < 20 else 0) for i in range(21))
    want = np.r_[0, np.cumsum(np.diff(w) > 1e-3 * nrm)]
    assert np.array_equal(cluster_of, want) and ncl == want[-1] + 1


def test_plan_loose72_one_cluster_of_twelve():
    d, e, w, block_of, cluster_of, nb, ncl = _plan("loose72")
    assert nb == 1
    assert len(set(cluster_of[60:])) == 1 and cluster_of[59] != cluster_of[60]


@pytest.mark.parametrize("name", R.STRUCTURED)
def test_structured_matrices_have_their_structure(name):
    """weak*: one block, one cluster of n; twins1040: 520 clusters of 2; pairs2200: 2200 clusters of 1 in 1100
    blocks; mixed2100: 2100 clusters of 1 in 700 blocks of order 1 and 700 of order 2; wilk41: a pair closer than 10 eps |lambda| in one block; glued105: unsplit, clusters of 5."""
    R.check_structure(name)


CLOSED_FORM = {"twins1040": R.twins1040_closed_form, "pairs2200": R.pairs2200_closed_form,
               "mixed2100": R.mixed2100_closed_form}


@pytest.mark.parametrize("name", ["weak600", "twins1040", "pairs2200", "mixed2100"])
def test_large_restatement_bounds(name):
    """The large matrices (not in NAMES) under the conditions of test_restatement_bounds."""
    A = R.matrix(name)
    w, Z, wl = R.reference(name)
    r, o = R.r_figure(A, w, Z), R.o_figure(Z)
    dw = float(np.abs(w - wl).max())
    print(f"{name}: r={r:.3f} o={o:.3f} |w-w_lapack|={dw:.3e} (bound {R.value_bound(A):.3e})")
    assert r <= 2 and o <= 2 and dw <= R.value_bound(A)
    if name in CLOSED_FORM:
        assert np.abs(wl - CLOSED_FORM[name]()).max() <= R.value_bound(A)


def test_plan_hand_made():
    # rows 0-2 and 3-5: e[2] = 1e-18 <= eps sqrt(|2 * 3|) is negligible.  ||T_0||_1 = 1 + 4 + 1 = 6 (row 1),
    # ||T_1||_1 = 0.01 + 7 = 7.01 (row 5).  Eigenvalues of block 1, [[3, 1e-4, 0], [1e-4, 3, 0.01], [0, 0.01, -7]]:
    # two about 2e-4 apart near 3 (inside 7.01e-3), one near -7.
    d = np.array([1.0, 4.0, 2.0, 3.0, 3.0, -7.0])
    e = np.array([1.0, 1.0, 1e-18, 1e-4, 0.01])
    T = np.diag(d) + np.diag(e, 1) + np.diag(e, -1)
    w0 = np.linalg.eigvalsh(T[:3, :3])
    w1 = np.linalg.eigvalsh(T[3:, 3:])
    assert abs(w1[2] - w1[1]) < 7.01e-3 < abs(w1[1] - w1[0])
    w = np.sort(np.r_[w0, w1])
    block_of, cluster_of, nb, ncl = E.tridiag_plan(d, e, w)
    assert nb == 2 and list(block_of) == [0, 0, 0, 1, 1, 1]
    # ascending: w1[0] (-7.02), w0[0] (0.55), w0[1] (2.2), w1[1], w1[2] (about 3), w0[2] (4.2)
    assert np.argsort(np.r_[w0, w1], kind="stable").tolist() == [3, 0, 1, 4, 5, 2]
    assert list(cluster_of) == [0, 1, 2, 3, 3, 4] and ncl == 5
    # a subset, and bad arguments
    assert list(E.tridiag_plan(d, e, w[3:5])[1]) == [0, 0]
    with pytest.raises(E.EigSolError) as ex:
        E.tridiag_plan(d, e, w[::-1])
    assert ex.value.status == _capi.EIGSOL_E_INVALID
    with pytest.raises(E.EigSolError) as ex:
        E.tridiag_plan(d, e, np.array([100.0]))
    assert ex.value.status == _capi.EIGSOL_E_INVALID
