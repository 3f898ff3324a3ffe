"""GPU: eigh(method="dc") (eigsol_eigh_dense_m, csrc/eigh_dc.hip) on the matrices of tests/eigh_ref.py.

Accuracy conditions, the project's usual ones:
    r <= max(2, 3 r_ref),   o <= max(2, 3 o_ref),   max |w - w_LAPACK| <= 2 n eps ||A||_F
"ref" is LAPACK's divide and conquer (scipy.linalg.eigh(driver="evd")) up to order 1000 and the NumPy
restatement (tests/eigh_dc_ref.py) above it, each computed once per matrix.  Every measured figure is written
to profiles/eigh_dc_accuracy.json."""
import ctypes as C
import json
import os

import numpy as np
import pytest

import pcsc_eigenvalue_solver_project_amd as E
from pcsc_eigenvalue_solver_project_amd import _capi

import eigh_dc_ref as DC
import eigh_ref as R
from test_gpu_eigh import check_phase

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ACCURACY_JSON = os.path.join(ROOT, "profiles", "eigh_dc_accuracy.json")
_figures = {}
_full = {}
_ref = {}


def _record(key, **kw):
    if not _figures and os.path.exists(ACCURACY_JSON):   # a partial run keeps the other cases' figures
        with open(ACCURACY_JSON) as f:
            _figures.update(json.load(f))
    _figures[key] = {k: float(v) for k, v in kw.items()}
    os.makedirs(os.path.dirname(ACCURACY_JSON), exist_ok=True)
    with open(ACCURACY_JSON, "w") as f:
        json.dump(_figures, f, indent=1, sort_keys=True)
        f.write("\n")


def full_run(ctx, name):
    """eigh(method="dc", select=None) at the default leaf order, computed once per session and left unchanged."""
    if name not in _full:
        res = E.eigh(ctx, R.matrix(name), method="dc")
        res.eigenvalues.setflags(write=False)
        res.eigenvectors.setflags(write=False)
        _full[name] = res
    return _full[name]


def ref_figures(name):
    """(r_ref, o_ref, w_LAPACK), once per matrix."""
    if name not in _ref:
        A = R.matrix(name)
        if A.shape[0] <= 1000:
            w, _, r, o = DC.evd(name)
            wl = R.reference(name)[2] if name in R.NAMES else w
        else:
            w, Z = DC.reference(name)
            r, o = R.r_figure(A, w, Z), R.o_figure(Z)
            wl = np.linalg.eigvalsh(R.mirror_lower(A))
        _ref[name] = (r, o, wl)
    return _ref[name]


def check_conditions(key, A, res, r_ref, o_ref, w_lapack):
    n = A.shape[0]
    w, Z = res.eigenvalues, res.eigenvectors
    assert w.shape == w_lapack.shape and Z.shape == (n, w.size) and Z.dtype == A.dtype
    r, o = R.r_figure(A, w, Z), R.o_figure(Z)
    dw = float(np.abs(w - w_lapack).max()) if w.size else 0.0
    bound = R.value_bound(A)
    _record(key, r=r, o=o, eigenvalue_difference=dw, eigenvalue_bound=bound, r_ref=r_ref, o_ref=o_ref,
            not_converged=res.not_converged)
    print(f"{key}: r={r:.3f} (ref {r_ref:.3f}) o={o:.3f} (ref {o_ref:.3f}) |w-w_lapack|={dw:.3e} (bound {bound:.3e}) "
          f"not_converged={res.not_converged}")
    assert np.all(np.isfinite(w)) and np.all(np.isfinite(Z))
    assert np.all(np.diff(w) >= 0)
    assert res.not_converged == 0
    assert r <= max(2, 3 * r_ref)
    assert o <= max(2, 3 * o_ref)
    assert dw <= bound
    check_phase(Z)


@pytest.mark.parametrize("name", R.NAMES)
def test_all_eigenpairs(ctx, name):
    check_conditions(name, R.matrix(name), full_run(ctx, name), *ref_figures(name))


@pytest.mark.parametrize("name", R.NAMES)
def test_all_eigenpairs_leaf4(ctx, name, monkeypatch):
    """EIGSOL_DC_LEAF=4: trees of 5 to 7 levels on the small matrices."""
    monkeypatch.setenv("EIGSOL_DC_LEAF", "4")
    res = E.eigh(ctx, R.matrix(name), method="dc")
    check_conditions(name + "@leaf4", R.matrix(name), res, *ref_figures(name))


# sym1030: the top merge keeps more than 1024 roots (one LDS pole chunk).  lap1025: odd orders at every level.
# weak600: the spectrum that is one dstein cluster.  twins1040, mixed2100: 1 x 1 and 2 x 2 blocks only, no merge.
CLOSED_FORM = {"twins1040": R.twins1040_closed_form, "mixed2100": R.mixed2100_closed_form}


@pytest.mark.parametrize("name", ["sym1030", "lap1025", "weak600", "twins1040", "mixed2100"])
def test_large(ctx, name):
    A = R.matrix(name)
    res = full_run(ctx, name)
    check_conditions(name, A, res, *ref_figures(name))
    if name in CLOSED_FORM:
        assert np.abs(res.eigenvalues - CLOSED_FORM[name]()).max() <= R.value_bound(A)
    if name == "sym1030":
        assert E.eigh_dc_stage_times(ctx)["merge_gemm"] >= 0


@pytest.mark.parametrize("name,il,iu", [("sym200", 0, 9), ("sym200", 90, 130), ("sym200", 199, 199), ("weak600", 250, 262)])
def test_index_selection(ctx, name, il, iu):
    A = R.matrix(name)
    full = full_run(ctx, name)
    res = E.eigh(ctx, A, select=("i", il, iu), method="dc")
    assert res.eigenvalues.tobytes() == full.eigenvalues[il:iu + 1].tobytes()
    assert res.eigenvectors.tobytes() == np.asfortranarray(full.eigenvectors[:, il:iu + 1]).tobytes()
    assert res.not_converged == 0
    o = R.o_figure(res.eigenvectors)
    print(f"{name}[i,{il},{iu}]: o={o:.3f}")
    assert o <= max(2, 3 * ref_figures(name)[1])


@pytest.mark.parametrize("vl,vu", [(0.5, 1.25), (-1.0, 0.01), (3.9, 10.0), (4.5, 5.0), (1.0, 1.0 + 1e-13)])
def test_value_selection(ctx, vl, vu):
    """lap300, half-open (vl, vu] on the computed values; the last two intervals are empty."""
    A = R.matrix("lap300")
    full = full_run(ctx, "lap300")
    keep = (full.eigenvalues > vl) & (full.eigenvalues <= vu)
    res = E.eigh(ctx, A, select=("v", vl, vu), method="dc")
    assert res.eigenvalues.tobytes() == full.eigenvalues[keep].tobytes()
    assert res.eigenvectors.shape == (300, int(keep.sum()))
    assert res.eigenvectors.tobytes() == np.asfortranarray(full.eigenvectors[:, keep]).tobytes()
    if vl >= 4.5 or vu - vl < 1e-12:
        assert res.eigenvalues.size == 0
    assert R.o_figure(res.eigenvectors) <= max(2, 3 * ref_figures("lap300")[1])


@pytest.mark.parametrize("name", ["sym200", "herm70"])
def test_two_runs_bitwise_equal(ctx, name):
    a = full_run(ctx, name)
    b = E.eigh(ctx, R.matrix(name), method="dc")
    assert a.eigenvalues.tobytes() == b.eigenvalues.tobytes()
    assert a.eigenvectors.tobytes() == b.eigenvectors.tobytes()


@pytest.mark.parametrize("name", ["sym97", "herm70"])
def test_only_lower_triangle_read(ctx, name):
    A = R.matrix(name).copy()
    iu = np.triu_indices(A.shape[0], 1)
    A[iu] = np.nan
    if np.iscomplexobj(A):
        A[np.diag_indices(A.shape[0])] += 3j
    res = E.eigh(ctx, A, method="dc")
    full = full_run(ctx, name)
    assert res.eigenvalues.tobytes() == full.eigenvalues.tobytes()
    assert res.eigenvectors.tobytes() == full.eigenvectors.tobytes()


def test_non_finite_entry(ctx):
    A = R.matrix("sym97").copy()
    A[50, 20] = np.inf
    with pytest.raises(E.EigSolError, match="the lower triangle holds a non-finite entry"):
        E.eigh(ctx, A, method="dc")


def _entry(ctx, A, name, method=None):
    """(w, Z, not_converged) straight from the C entry `name` (all pairs)."""
    n = A.shape[0]
    Af = np.asfortranarray(A)
    w = np.zeros(n)
    Z = np.zeros((n, n), dtype=A.dtype, order="F")
    m, nc = C.c_int64(0), C.c_int64(0)
    vp = lambda a: a.ctypes.data_as(C.c_void_p)
    code = E.EIGSOL_C128 if np.iscomplexobj(A) else E.EIGSOL_F64
    args = [ctx.handle, code, n, vp(Af), None] + ([] if method is None else [method]) + [vp(w), vp(Z), C.byref(m), C.byref(nc)]
    _capi.call(name, *args)
    assert m.value == n
    return w, Z, nc.value


@pytest.mark.parametrize("name", ["sym97", "herm70"])
def test_stein_and_default_are_the_existing_call(ctx, name):
    A = R.matrix(name)
    w0, Z0, nc0 = _entry(ctx, A, "eigsol_eigh_dense")
    w1, Z1, nc1 = _entry(ctx, A, "eigsol_eigh_dense_m", 0)
    assert w0.tobytes() == w1.tobytes() and Z0.tobytes() == Z1.tobytes() and nc0 == nc1
    for res in (E.eigh(ctx, A), E.eigh(ctx, A, method="stein")):
        assert res.eigenvalues.tobytes() == w0.tobytes() and res.eigenvectors.tobytes() == Z0.tobytes()
    # eigvalsh takes the argument and ignores it: the bisection values
    assert E.eigvalsh(ctx, A, method="dc").tobytes() == w0.tobytes()
    # the stage times of a "dc" call: the whole tridiagonal stage in the third slot
    E.eigh(ctx, A, method="dc")
    t = E.eigh_stage_times(ctx)
    assert t["bisection"] == 0 and t["inverse_iteration"] > 0
    t6 = E.eigh_dc_stage_times(ctx)
    assert all(v >= 0 for v in t6.values()) and t6["leaves"] > 0 and t6["reduction"] > 0


def test_unknown_method(ctx):
    A = R.matrix("sym97")
    with pytest.raises(E.EigSolError) as e:
        _entry(ctx, A, "eigsol_eigh_dense_m", 2)
    assert e.value.status == E.EIGSOL_E_INVALID
    with pytest.raises(E.EigSolError):
        E.eigh(ctx, A, method="qr")


# 2^+-600: eigh_rescale acts on A.  2^+-40, 2^-20, 2^-100: inside the range eigh_rescale leaves alone, where only
# the per-block scaling of T keeps dlaed2's tolerance (8 u max(max |d|, max |z|), |z| <= 1) meaningful: without it
# 2^-40 sym97 has r = 4.7e8 and at 2^-60 every pole deflates (tests/test_eigh_dc_cpu.py shows both).
@pytest.mark.parametrize("name", ["sym97", "herm70", "sym200", "lap300"])
@pytest.mark.parametrize("k", [600, -600, 40, -20, -40, -100])
def test_scale_extremes(ctx, name, k):
    """2^k A: every scaling is a power of two, so the unscaled values and the vectors are those of scale 1, bit for
    bit; the accuracy conditions then hold at every scale because test_all_eigenpairs holds them at scale 1."""
    A = R.matrix(name)
    full = full_run(ctx, name)
    res = E.eigh(ctx, np.ldexp(A.real, k) + (1j * np.ldexp(A.imag, k) if np.iscomplexobj(A) else 0), method="dc")
    assert res.not_converged == 0
    assert np.ldexp(res.eigenvalues, -k).tobytes() == full.eigenvalues.tobytes()
    assert res.eigenvectors.tobytes() == full.eigenvectors.tobytes()


@pytest.mark.parametrize("name,k", [("sym97", -60), ("graded80", -30), ("blockdiag", -45), ("herm200", -70)])
def test_small_norm_conditions(ctx, name, k):
    """The accuracy conditions themselves on matrices of small norm (not only the bits of scale 1)."""
    A = R.matrix(name)
    As = np.ldexp(A.real, k) + (1j * np.ldexp(A.imag, k) if np.iscomplexobj(A) else 0)
    r_ref, o_ref, wl = ref_figures(name)
    check_conditions(f"{name}*2^{k}", As, E.eigh(ctx, As, method="dc"), r_ref, o_ref, np.ldexp(wl, k))
