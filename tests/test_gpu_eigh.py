"""GPU: eigh / eigvalsh (eigsol_eigh_dense) on the matrices of tests/eigh_ref.py.

Accuracy conditions, with "ref" the CPU restatement's figure on the same matrix and selection:
    r <= max(2, 3 r_ref),   o <= max(2, 3 o_ref),   max |w - w_LAPACK| <= 2 n eps ||A||_F
(r = ||A Z - Z L||_F / (n eps ||A||_F), o = ||Z^H Z - I||_F / (n eps)).  Every measured figure is written to
profiles/eigh_accuracy.json."""
import json
import os
import types

import numpy as np
import pytest

import pcsc_eigenvalue_solver_project_amd as E

import eigh_ref as R

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ACCURACY_JSON = os.path.join(ROOT, "profiles", "eigh_accuracy.json")
_figures = {}
_full = {}


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
    """eigh(select=None) of the matrix, computed once per session and left unchanged."""
    if name not in _full:
        res = E.eigh(ctx, R.matrix(name))
        res.eigenvalues.setflags(write=False)
        res.eigenvectors.setflags(write=False)
        _full[name] = res
    return _full[name]


def check_conditions(key, A, res, w_ref, Z_ref, w_lapack):
    n = A.shape[0]
    w, Z = res.eigenvalues, res.eigenvectors
    assert w.shape == w_ref.shape and Z.shape == (n, w.size) and Z.dtype == A.dtype
    r, o = R.r_figure(A, w, Z), R.o_figure(Z)
    r_ref, o_ref = R.r_figure(A, w_ref, Z_ref), R.o_figure(Z_ref)
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


def check_phase(Z):
    """Unit columns whose largest-modulus component (the first on ties) is real and positive."""
    for j in range(Z.shape[1]):
        z = Z[:, j]
        assert abs(np.linalg.norm(z) - 1) <= 8 * Z.shape[0] * R.EPS
        a = np.abs(z)
        if np.isrealobj(z):
            assert z[int(np.argmax(a))] > 0     # argmax: the first of equal maxima
        else:                                   # moduli are rounded: any component within rounding of the largest
            near = np.nonzero(a >= a.max() * (1 - 8 * R.EPS))[0]
            assert any(z[k].imag == 0 and z[k].real > 0 for k in near)


@pytest.mark.parametrize("name", R.NAMES)
def test_all_eigenpairs(ctx, name):
    A = R.matrix(name)
    if name in R.STRUCTURED:
        R.check_structure(name)
    w_ref, Z_ref, w_lapack = R.reference(name)
    check_conditions(name, A, full_run(ctx, name), w_ref, Z_ref, w_lapack)


def test_laplacian_closed_form(ctx):
    w = full_run(ctx, "lap300").eigenvalues
    k = np.arange(1, 301)
    assert np.abs(w - (2 - 2 * np.cos(k * np.pi / 301))).max() <= R.value_bound(R.matrix("lap300"))


# cluster99's eight values 1.5 + 1e-12 j are the eigenvalues 69 .. 76 (66 of the 88 spread values and the triple
# 0.25 lie below 1.5)
@pytest.mark.parametrize("name,il,iu", [
    ("sym97", 0, 9), ("sym97", 90, 96), ("sym97", 40, 40), ("sym97", 31, 64),
    ("herm70", 0, 0), ("herm70", 69, 69), ("herm70", 10, 30),
    ("cluster99", 0, 71), ("cluster99", 72, 80), ("cluster99", 74, 98), ("cluster99", 75, 75),
])
def test_index_selection(ctx, name, il, iu):
    A = R.matrix(name)
    full = full_run(ctx, name)
    res = E.eigh(ctx, A, select=("i", il, iu))
    assert res.eigenvalues.tobytes() == full.eigenvalues[il:iu + 1].tobytes()
    w_ref, Z_ref = R.restatement(A, ("i", il, iu))
    check_conditions(f"{name}[i,{il},{iu}]", A, res, w_ref, Z_ref, R.reference(name)[2][il:iu + 1])
    assert E.eigvalsh(ctx, A, select=("i", il, iu)).tobytes() == res.eigenvalues.tobytes()


def test_sym1030_selected_pairs(ctx):
    A = R.matrix("sym1030")
    sel = ("i", 500, 531)
    res = E.eigh(ctx, A, select=sel)
    w_ref, Z_ref = R.restatement(A, sel)
    check_conditions("sym1030[i,500,531]", A, res, w_ref, Z_ref, np.linalg.eigvalsh(A)[500:532])


# weak600: one block, one cluster of 600, three projection batches (256 + 256 + 88).  twins1040: 520 clusters of
# two, more than the 512 workgroups the cluster kernel gets.  pairs2200: 2200 clusters of one in blocks of
# order 2, more than the 2048 waves the single-eigenvalue kernel gets.  mixed2100: 2100 clusters of one, every
# third a 1 x 1 block, so a wave that takes a second cluster meets the unit-vector shortcut beside real blocks.
# check_structure asserts each of these.
CLOSED_FORM = {"twins1040": R.twins1040_closed_form, "pairs2200": R.pairs2200_closed_form,
               "mixed2100": R.mixed2100_closed_form}


@pytest.mark.parametrize("name", ["weak600", "twins1040", "pairs2200", "mixed2100"])
def test_large_structured(ctx, name):
    A = R.matrix(name)
    R.check_structure(name)
    w_ref, Z_ref, w_lapack = R.reference(name)
    res = full_run(ctx, name)
    check_conditions(name, A, res, w_ref, Z_ref, w_lapack)
    if name in CLOSED_FORM:
        closed = CLOSED_FORM[name]()
        dc = float(np.abs(res.eigenvalues - closed).max())
        print(f"{name}: |w - closed form| = {dc:.3e}")
        assert dc <= R.value_bound(A)


# a selection projects only against the selected members of the cluster: 13 of them (one batch, cut out of the
# middle), and all 600 through the index path
@pytest.mark.parametrize("il,iu", [(250, 262), (0, 599)])
def test_weak600_selection_cuts_the_cluster(ctx, il, iu):
    A = R.matrix("weak600")
    R.check_structure("weak600")
    full = full_run(ctx, "weak600")
    res = E.eigh(ctx, A, select=("i", il, iu))
    assert res.eigenvalues.tobytes() == full.eigenvalues[il:iu + 1].tobytes()
    w_ref, Z_ref = R.restatement(A, ("i", il, iu))
    check_conditions(f"weak600[i,{il},{iu}]", A, res, w_ref, Z_ref, R.reference("weak600")[2][il:iu + 1])


# block orders around kBisectChunk = 1024 (the staging chunk of the Sturm count): one chunk, one chunk and a
# row, two chunks and a row (one unsplit block each), and the dense sym1030
@pytest.mark.parametrize("name", ["sym1030", "lap1024", "lap1025", "lap2049"])
def test_all_values_past_one_bisection_chunk(ctx, name):
    A = R.matrix(name)
    w = E.eigvalsh(ctx, A)
    w_lapack = np.linalg.eigvalsh(A)
    assert w.shape == w_lapack.shape and np.all(np.isfinite(w)) and np.all(np.diff(w) >= 0)
    dw, bound = float(np.abs(w - w_lapack).max()), R.value_bound(A)
    _record(f"{name}[values]", eigenvalue_difference=dw, eigenvalue_bound=bound)
    print(f"{name}: |w-w_lapack|={dw:.3e} (bound {bound:.3e})")
    assert dw <= bound


# eigh(s A) for exact scalings s = 2^p: s^-1 w and Z must meet the conditions of A itself (LAPACK returns s w
# for these, so the references are those of A, and the test's own arithmetic stays in range).  |p| = 400 is
# inside the range the solver takes as it is (e^2 = 2^+-800 is representable); |p| = 600 is outside it.
SCALE_SELECTION = {"sym97": (31, 64), "herm70": (10, 30), "cluster99": (72, 80)}


def _unscaled(res, s):
    return types.SimpleNamespace(eigenvalues=res.eigenvalues / s, eigenvectors=res.eigenvectors,
                                 not_converged=res.not_converged)


@pytest.mark.parametrize("p", [-600, -400, 400, 600])
@pytest.mark.parametrize("name", ["sym97", "herm70", "cluster99"])
def test_scale_extremes(ctx, name, p):
    A = R.matrix(name)
    s = 2.0 ** p
    sA = s * A
    assert np.array_equal(sA / s, A)                       # the scaling is exact
    w_ref, Z_ref, w_lapack = R.reference(name)
    res = E.eigh(ctx, sA)
    check_conditions(f"{name}*2^{p}", A, _unscaled(res, s), w_ref, Z_ref, w_lapack)
    # values only: against s w_LAPACK(A), and the same bits as the full run
    wv = E.eigvalsh(ctx, sA)
    assert wv.shape == w_lapack.shape and np.all(np.isfinite(wv))
    assert np.abs(wv - s * w_lapack).max() <= s * R.value_bound(A)
    assert wv.tobytes() == res.eigenvalues.tobytes()
    # an index selection: a slice of the full run, under the conditions of the same selection on A
    il, iu = SCALE_SELECTION[name]
    sel = E.eigh(ctx, sA, select=("i", il, iu))
    assert sel.eigenvalues.tobytes() == res.eigenvalues[il:iu + 1].tobytes()
    ws_ref, Zs_ref = R.restatement(A, ("i", il, iu))
    check_conditions(f"{name}*2^{p}[i,{il},{iu}]", A, _unscaled(sel, s), ws_ref, Zs_ref, w_lapack[il:iu + 1])


# a value selection is taken on the caller's scale
@pytest.mark.parametrize("p", [-600, 600])
def test_scale_extremes_value_selection(ctx, p):
    A = R.matrix("sym97")
    s = 2.0 ** p
    full = full_run(ctx, "sym97").eigenvalues
    vl, vu = -3.0, 2.5
    keep = (full > vl) & (full <= vu)
    assert 0 < keep.sum() < 97
    res = E.eigh(ctx, s * A, select=("v", s * vl, s * vu))
    w_ref, Z_ref = R.restatement(A, ("v", vl, vu))
    check_conditions(f"sym97*2^{p}[v,{vl},{vu}]", A, _unscaled(res, s), w_ref, Z_ref, R.reference("sym97")[2][keep])


# both scalings are brought to the same matrix (largest entry in [1, 2)) by exact multiplications, so everything
# but the eigenvalues' exponent agrees to the bit
@pytest.mark.parametrize("name", ["sym97", "herm70"])
def test_scale_extremes_same_bits_up_and_down(ctx, name):
    A = R.matrix(name)
    up, down = E.eigh(ctx, 2.0 ** 600 * A), E.eigh(ctx, 2.0 ** -600 * A)
    assert (up.eigenvalues / 2.0 ** 600).tobytes() == (down.eigenvalues * 2.0 ** 600).tobytes()
    assert up.eigenvectors.tobytes() == down.eigenvectors.tobytes()
    assert up.not_converged == down.not_converged == 0


@pytest.mark.parametrize("p", [0, 600])
@pytest.mark.parametrize("bad", [np.inf, np.nan])
def test_non_finite_entry_fails_at_any_scale(ctx, bad, p):
    A = 2.0 ** p * R.matrix("sym97")
    A[50, 3] = bad
    with pytest.raises(E.EigSolError) as e:
        E.eigh(ctx, A)
    assert "non-finite" in str(e.value)
    H = 2.0 ** p * R.matrix("herm70")
    H[69, 69] = bad
    with pytest.raises(E.EigSolError) as e:
        E.eigvalsh(ctx, H)
    assert "non-finite" in str(e.value)


@pytest.mark.parametrize("name,vl,vu", [("lap300", 4.5, 5.0), ("lap300", -1.0, -0.5), ("wilk21", 0.4, 0.6)])
def test_value_selection_empty_interval(ctx, name, vl, vu):
    w_lapack = R.reference(name)[2]
    assert not np.any((w_lapack > vl) & (w_lapack <= vu))
    res = E.eigh(ctx, R.matrix(name), select=("v", vl, vu))
    assert res.eigenvalues.size == 0 and res.eigenvectors.shape == (R.matrix(name).shape[0], 0)
    assert res.not_converged == 0
    assert E.eigvalsh(ctx, R.matrix(name), select=("v", vl, vu)).size == 0


@pytest.mark.parametrize("name,vl,vu", [("lap300", 1.0, 1.5), ("wilk21", 5.5, 11.0)])
def test_value_selection(ctx, name, vl, vu):
    A = R.matrix(name)
    full = full_run(ctx, name)
    keep = (full.eigenvalues > vl) & (full.eigenvalues <= vu)
    assert 0 < keep.sum() < A.shape[0]
    res = E.eigh(ctx, A, select=("v", vl, vu))
    assert res.eigenvalues.tobytes() == full.eigenvalues[keep].tobytes()
    w_ref, Z_ref = R.restatement(A, ("v", vl, vu))
    check_conditions(f"{name}[v,{vl},{vu}]", A, res, w_ref, Z_ref, R.reference(name)[2][keep])


def test_value_selection_half_open_at_exact_eigenvalues(ctx):
    A = R.matrix("diag50")
    dv = np.sort(np.diag(A))
    u = np.unique(dv)
    vl, vu = float(u[2]), float(u[5])            # both are eigenvalues, exactly
    want = dv[(dv > vl) & (dv <= vu)]
    assert vl not in want and vu in want
    res = E.eigh(ctx, A, select=("v", vl, vu))
    assert res.eigenvalues.tobytes() == want.tobytes()
    assert R.r_figure(A, res.eigenvalues, res.eigenvectors) == 0 and R.o_figure(res.eigenvectors) == 0
    assert full_run(ctx, "diag50").eigenvalues.tobytes() == dv.tobytes()


@pytest.mark.parametrize("name", ["sym97", "herm70", "cluster99", "lap300", "blockdiag", "eye40", "n2"])
def test_values_only_equals_full_run(ctx, name):
    assert E.eigvalsh(ctx, R.matrix(name)).tobytes() == full_run(ctx, name).eigenvalues.tobytes()


@pytest.mark.parametrize("name", ["sym200", "herm70"])
def test_two_runs_identical_bits(ctx, name):
    a, b = E.eigh(ctx, R.matrix(name)), E.eigh(ctx, R.matrix(name))
    assert a.eigenvalues.tobytes() == b.eigenvalues.tobytes()
    assert a.eigenvectors.tobytes() == b.eigenvectors.tobytes()
    assert a.eigenvalues.tobytes() == full_run(ctx, name).eigenvalues.tobytes()


def test_only_the_lower_triangle_is_read(ctx):
    A = R.matrix("sym97").copy()
    iu = np.triu_indices(97, 1)
    g = np.random.default_rng(11).standard_normal(iu[0].size) * 1e6
    g[::3] = np.nan
    g[1::7] = np.inf
    A[iu] = g
    res = E.eigh(ctx, A)
    full = full_run(ctx, "sym97")
    assert res.eigenvalues.tobytes() == full.eigenvalues.tobytes()
    assert res.eigenvectors.tobytes() == full.eigenvectors.tobytes()
    # C128: the diagonal's imaginary part is ignored too
    H = R.matrix("herm70").copy()
    H[np.triu_indices(70, 1)] = np.nan
    H[np.diag_indices(70)] += 3j
    rh = E.eigh(ctx, H)
    assert rh.eigenvalues.tobytes() == full_run(ctx, "herm70").eigenvalues.tobytes()
    assert rh.eigenvectors.tobytes() == full_run(ctx, "herm70").eigenvectors.tobytes()


def test_hessenberg_unchanged_by_eigh(ctx):
    """The reduction's optional reflector outputs leave the existing path bitwise as it was."""
    A = R.matrix("sym97")
    before = E.to_hessenberg(ctx, A)
    E.eigh(ctx, A)
    after = E.to_hessenberg(ctx, A)
    assert before.tobytes() == after.tobytes()


def test_empty_matrix_and_stage_times(ctx):
    r = E.eigh(ctx, np.zeros((0, 0)))
    assert r.eigenvalues.size == 0 and r.not_converged == 0
    E.eigh(ctx, R.matrix("sym97"))
    t = E.eigh_stage_times(ctx)
    assert set(t) == {"reduction", "bisection", "inverse_iteration", "back_transform"}
    assert all(v > 0 for v in t.values())
