"""GPU: eig (eigsol_eig_dense, csrc/eig.hip) on the named matrices of tests/eig_ref.py.

Conditions, for every matrix (r = max_j ||A v_j - w_j v_j||_2 / (n eps ||A||_F), c = cond_2(V); the
restatement's figures are the ones tests/test_eig_cpu.py recorded in tests/golden/eig_ref_figures.json):
    r <= max(2, 3 r_restatement);   not_converged == 0;   c <= 10 c_restatement wherever c_restatement < 1e8;
    every eigenvalue matches numpy.linalg.eigvals one to one within 2 n eps ||A||_F on the normal and
    well-conditioned cases (gen*, cgen70, sym65, diag50, tri30);
    for n >= 64 the eigenvalues are bitwise qr_eigenvalues'.
Every measured figure is written to profiles/eig_accuracy.json."""
import ctypes as C
import json
import os

import numpy as np
import pytest

import pcsc_eigenvalue_solver_project_amd as E
from pcsc_eigenvalue_solver_project_amd import _capi

import eig_ref as R

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ACCURACY_JSON = os.path.join(ROOT, "profiles", "eig_accuracy.json")
GOLDEN = os.path.join(ROOT, "tests", "golden", "eig_ref_figures.json")
_figures = {}
_full = {}
_eigvals = {}


def _record(key, **kw):
    if not _figures and os.path.exists(ACCURACY_JSON):   # a partial run keeps the other cases' figures
        with open(ACCURACY_JSON) as f:
            _figures.update(json.load(f))
    _figures[key] = {k: float(v) for k, v in kw.items()}
    os.makedirs(os.path.dirname(ACCURACY_JSON), exist_ok=True)
    with open(ACCURACY_JSON, "w") as f:
        json.dump(_figures, f, indent=1, sort_keys=True)
        f.write("\n")


def restatement():
    with open(GOLDEN) as f:
        return json.load(f)


def full_run(ctx, name):
    """eig(select=None, batch=0), computed once per session and left unchanged."""
    if name not in _full:
        res = E.eig(ctx, R.matrix(name))
        res.values.setflags(write=False)
        res.vectors.setflags(write=False)
        _full[name] = res
    return _full[name]


def bits(a):
    return np.ascontiguousarray(a).view(np.uint64)


def value_bound(A):
    """2 n eps ||A||_F, formed without overflow"""
    e = R._in_range(A)
    As = np.ldexp(A.real, e) + (1j * np.ldexp(A.imag, e) if np.iscomplexobj(A) else 0)
    return float(np.ldexp(2 * A.shape[0] * R.EPS * np.linalg.norm(As), -e))


@pytest.mark.parametrize("name", R.NAMES)
def test_conditions(ctx, name):
    A = R.matrix(name)
    n = A.shape[0]
    ref = restatement()[name]
    res = full_run(ctx, name)
    w, V = res.values, res.vectors
    assert w.shape == (n,) and V.shape == (n, n) and V.dtype == np.complex128
    assert np.all(np.isfinite(w)) and np.all(np.isfinite(V))
    r, c = R.figures(A, w, V)
    rec = dict(r=r, c=c, r_restatement=ref["r"], c_restatement=ref["c"], not_converged=res.not_converged)
    dw = bound = None
    if name in R.WELL_CONDITIONED:
        if name not in _eigvals:
            _eigvals[name] = np.linalg.eigvals(A)
        dw, bound = R.match_one_to_one(w, _eigvals[name]), value_bound(A)
        rec.update(eigenvalue_difference=dw, eigenvalue_bound=bound)
    _record(name, **rec)
    print(f"{name}: r={r:.3g} (restatement {ref['r']:.3g}) c={c:.3g} (restatement {ref['c']:.3g}) "
          f"not_converged={res.not_converged} |w - w_numpy|={dw} (bound {bound})")
    assert res.converged
    assert res.not_converged == 0
    assert r <= max(2.0, 3.0 * ref["r"])
    if ref["c"] < 1e8:
        assert c <= 10.0 * ref["c"]
    if dw is not None:
        assert dw <= bound
    if n >= 64:
        q = E.qr_eigenvalues(ctx, A)
        assert np.array_equal(bits(q.eigenvalues_complex), bits(w))


@pytest.mark.parametrize("name", ["gen97", "gen1030", "jordan40", "kron30", "sym65"])
def test_real_matrix_pairs_and_real_vectors(ctx, name):
    """conjugate pairs are bitwise conjugate; the vector of a real eigenvalue has imaginary part exactly 0"""
    res = full_run(ctx, name)
    w, V = res.values, res.vectors
    n = w.size
    pairs = 0
    j = 0
    while j < n:
        if w[j].imag == 0:
            assert not np.any(V[:, j].imag), f"column {j}"
            j += 1
            continue
        assert j + 1 < n and w[j + 1] == np.conj(w[j]), f"eigenvalue {j} has no conjugate neighbour"
        assert np.array_equal(bits(V[:, j + 1]), bits(np.conj(V[:, j]))), f"columns {j}, {j + 1}"
        pairs += 1
        j += 2
    if name in ("gen97", "gen1030"):
        assert pairs > 0 and 2 * pairs < n   # both kinds are exercised


@pytest.mark.parametrize("name", ["gen97", "cgen70", "tri30", "eye7", "n1", "n2rot", "blk40"])
def test_normalisation(ctx, name):
    """unit 2-norm; the largest-modulus component real and positive"""
    V = full_run(ctx, name).vectors
    for j in range(V.shape[1]):
        a = np.abs(V[:, j])
        assert abs(np.linalg.norm(V[:, j]) - 1.0) <= 8 * R.EPS
        k = int(np.argmax(np.where((V[:, j].imag == 0) & (V[:, j].real > 0), a, -1.0)))
        assert V[k, j].imag == 0 and V[k, j].real > 0 and a[k] >= a.max() * (1 - 4 * R.EPS), f"column {j}"


@pytest.mark.parametrize("name", ["eye7", "zero5", "diag50"])
def test_unit_vectors_of_diagonal_matrices(ctx, name):
    res = full_run(ctx, name)
    n = res.values.size
    assert np.array_equal(res.vectors, np.eye(n))
    assert np.array_equal(res.values, np.diag(R.matrix(name)).astype(np.complex128))


@pytest.mark.parametrize("name", ["gen97", "cgen70"])
def test_two_runs_same_bits(ctx, name):
    a, b = full_run(ctx, name), E.eig(ctx, R.matrix(name))
    assert np.array_equal(bits(a.values), bits(b.values))
    assert np.array_equal(bits(a.vectors), bits(b.vectors))


def test_batch_of_seven_same_bits(ctx):
    """97 eigenvalues, 7 resident at a time: the launches reuse the workspace, the bits are the full call's"""
    a, b = full_run(ctx, "gen97"), E.eig(ctx, R.matrix("gen97"), batch=7)
    assert b.not_converged == 0
    assert np.array_equal(bits(a.values), bits(b.values))
    assert np.array_equal(bits(a.vectors), bits(b.vectors))


@pytest.mark.parametrize("name", ["gen97", "cgen70", "blk40"])
def test_selection_same_bits(ctx, name):
    full = full_run(ctx, name)
    n = full.values.size
    sel = [0, 5, n - 1]
    part = E.eig(ctx, R.matrix(name), select=sel)
    assert part.vectors.shape == (n, 3) and part.not_converged == 0
    assert np.array_equal(bits(part.values), bits(full.values))
    assert np.array_equal(bits(part.vectors), bits(full.vectors[:, sel]))


def test_selecting_one_of_a_pair(ctx):
    """the member with the negative imaginary part alone, then both in reverse order"""
    full = full_run(ctx, "gen97")
    w = full.values
    j = next(k for k in range(w.size) if w[k].imag < 0)
    p = j - 1 if j and w[j - 1] == np.conj(w[j]) else j + 1
    one = E.eig(ctx, R.matrix("gen97"), select=[j])
    assert np.array_equal(bits(one.vectors[:, 0]), bits(full.vectors[:, j]))
    both = E.eig(ctx, R.matrix("gen97"), select=[j, p, j])
    assert np.array_equal(bits(both.vectors), bits(full.vectors[:, [j, p, j]]))


def test_values_only(ctx):
    full = full_run(ctx, "gen97")
    res = E.eig(ctx, R.matrix("gen97"), select=[])
    assert res.vectors.shape == (97, 0)
    assert np.array_equal(bits(res.values), bits(full.values))


def test_stage_times(ctx):
    E.eig(ctx, R.matrix("gen97"))
    t = E.eig_stage_times(ctx)
    assert list(t) == ["reduction", "francis", "inverse_iteration", "back_transform"]
    assert all(v > 0 for v in t.values())


def _raw(ctx, dtype, n, A, opts, w, V, m):
    return _capi.lib().eigsol_eig_dense(None if ctx is None else ctx.handle, dtype, n, A, opts, w, V, m, None, None, None)


def test_status_codes(ctx):
    A = np.asfortranarray(R.matrix("gen64"))
    w = np.zeros(64, dtype=np.complex128)
    V = np.zeros((64, 64), dtype=np.complex128, order="F")
    m = C.c_int64(-1)
    pA, pw, pV = (x.ctypes.data_as(C.c_void_p) for x in (A, w, V))
    inv, uns = _capi.EIGSOL_E_INVALID, _capi.EIGSOL_E_UNSUPPORTED
    assert _raw(ctx, _capi.EIGSOL_F64, 64, None, None, pw, pV, C.byref(m)) == inv
    assert _raw(ctx, _capi.EIGSOL_F64, 64, pA, None, None, pV, C.byref(m)) == inv
    assert _raw(ctx, _capi.EIGSOL_F64, 64, pA, None, pw, pV, None) == inv
    assert _raw(None, _capi.EIGSOL_F64, 64, pA, None, pw, pV, C.byref(m)) == inv
    assert _raw(ctx, _capi.EIGSOL_F64, -1, pA, None, pw, pV, C.byref(m)) == inv
    for bad in ([64], [-1], [0, 5, 64]):
        sel = np.array(bad, dtype=np.int64)
        o = _capi.EigOptionsC(1000, 0, sel.size, sel.ctypes.data_as(C.POINTER(C.c_int64)))
        assert _raw(ctx, _capi.EIGSOL_F64, 64, pA, C.byref(o), pw, pV, C.byref(m)) == inv
    o = _capi.EigOptionsC(1000, -1, 0, None)
    assert _raw(ctx, _capi.EIGSOL_F64, 64, pA, C.byref(o), pw, pV, C.byref(m)) == inv
    o = _capi.EigOptionsC(0, 0, 0, None)
    assert _raw(ctx, _capi.EIGSOL_F64, 64, pA, C.byref(o), pw, pV, C.byref(m)) == inv
    for dt in (_capi.EIGSOL_F32, _capi.EIGSOL_C64, _capi.EIGSOL_DD, _capi.EIGSOL_CDD):
        assert _raw(ctx, dt, 64, pA, None, pw, pV, C.byref(m)) == uns
    assert _raw(ctx, 77, 64, pA, None, pw, pV, C.byref(m)) == inv
    # above the reduction's order limit: decided before A is read
    assert _raw(ctx, _capi.EIGSOL_F64, 16385, pA, None, pw, pV, C.byref(m)) == uns
    assert _raw(ctx, _capi.EIGSOL_C128, 8193, pA, None, pw, pV, C.byref(m)) == uns
    assert m.value == -1
    assert _raw(ctx, _capi.EIGSOL_F64, 0, None, None, None, None, C.byref(m)) == _capi.EIGSOL_OK and m.value == 0
    with pytest.raises(E.EigSolError) as e:
        E.eig(ctx, np.eye(4, dtype=np.float32))
    assert e.value.status == uns
    with pytest.raises(E.EigSolError):
        E.eig(ctx, np.zeros((3, 4)))
    res = E.eig(ctx, np.zeros((0, 0)))
    assert res.values.shape == (0,) and res.vectors.shape == (0, 0)
