"""CPU: the cases, the figure and the restated schedule of the Sylvester tests (tests/sylvester_ref.py) are sound
with the reference alone.

``scipy.linalg.solve_sylvester`` / ``solve_continuous_lyapunov`` (LAPACK xGEES + xTRSYL) run on every named
case: the figure r = ||A X + X op(B) - C||_F / (max(m, n) eps ((||A||_F + ||B||_F) ||X||_F + ||C||_F)) must be at
most 2/3, so that the GPU tests' bound max(2, 3 x LAPACK's figure) is its floor 2 wherever LAPACK is that good; a
case above 2/3 must stay within 1.25 of what tests/golden/sylvester_ref_figures.json records for it (the rule of
tests/test_schur_cpu.py).  On the constructed triangular cases LAPACK's figure is xTRSYL's own, also recorded.
``trsyl_ref``, the NumPy statement of the device's partition and three-launch wavefront schedule, must meet
the GPU tests' bound on every named and every constructed case.

The componentwise figure w of tests/sylvester_ref.py (``figure_cw``) on every constructed case, hard ones
included: xTRSYL's w is finite and within 1.25 of its recorded value, and ``trsyl_ref`` meets ``bound_cw``.  The
golden file's "tri_cw" table and "cw_floor" (3 x the largest recorded w per scalar type) are written by the
same command as the rest.  The scaled named cases use ``figure_scaled``.

    python tests/test_sylvester_cpu.py        # rewrites tests/golden/sylvester_ref_figures.json
"""
import json
import os

import numpy as np
import pytest
import scipy.linalg as sla

import sylvester_ref as Y

LYAP = Y.LYAPUNOV + Y.SCALED_LYAPUNOV
ALL_NAMED = Y.NAMES + Y.SCALED + LYAP
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "sylvester_ref_figures.json")
_runs = {}


def lapack_named(name):
    """LAPACK's figure on one named case, once per session."""
    if name not in _runs:
        A, B, C = Y.case(name)
        X = sla.solve_continuous_lyapunov(np.array(A), np.array(C)) if name in LYAP else sla.solve_sylvester(A, B, C)
        _runs[name] = fig(name)(A, B, C, X)
    return _runs[name]


def fig(name):
    return Y.figure_scaled if "*" in name else Y.figure


def lapack_tri_cw(name, trans_b):
    key = f"cw:{name}/{'H' if trans_b else 'N'}"
    if key not in _runs:
        Rm, Sm, F = Y.tri_case(name)
        _runs[key] = Y.figure_cw(Rm, Y.op(Sm, trans_b), F, Y.lapack_trsyl(Rm, Sm, F, trans_b))
    return _runs[key]


def ref_tri(name, trans_b):
    """trsyl_ref on one constructed case, once per session."""
    key = f"ref:{name}/{'H' if trans_b else 'N'}"
    if key not in _runs:
        Rm, Sm, F = Y.tri_case(name)
        _runs[key] = Y.trsyl_ref(Rm, Sm, F, trans_b)
        _runs[key].setflags(write=False)
    return _runs[key]


def lapack_tri(name, trans_b):
    key = f"{name}/{'H' if trans_b else 'N'}"
    if key not in _runs:
        Rm, Sm, F = Y.tri_case(name)
        _runs[key] = Y.figure(Rm, Y.op(Sm, trans_b), F, Y.lapack_trsyl(Rm, Sm, F, trans_b))
    return _runs[key]


def recorded():
    with open(GOLDEN) as f:
        return json.load(f)


@pytest.mark.parametrize("name", ALL_NAMED)
def test_lapack_on_the_named_cases(name):
    r, rec = lapack_named(name), recorded()["named"][name]
    print(f"{name}: r={r:.3g} recorded {rec:.3g}")
    assert np.isfinite(r)
    assert r <= 2.0 / 3.0 or r <= 1.25 * rec


@pytest.mark.parametrize("name", ALL_NAMED)
def test_trsyl_ref_on_the_named_cases(name):
    A, B, C = Y.case(name)
    lyap = name in LYAP
    X = Y.bartels_stewart_ref(A, A if lyap else B, C, trans_b=lyap)
    r, rec = fig(name)(A, B, C, X), recorded()["named"][name]
    print(f"{name}: r={r:.3g} LAPACK {rec:.3g}")
    assert X.dtype == np.result_type(A, B, C)
    assert r <= Y.bound(rec)


@pytest.mark.parametrize("trans_b", [False, True])
@pytest.mark.parametrize("name", Y.TRI_ALL)
def test_trsyl_ref_on_the_constructed_cases(name, trans_b):
    Rm, Sm, F = Y.tri_case(name)
    key = f"{name}/{'H' if trans_b else 'N'}"
    rl, rec = lapack_tri(name, trans_b), recorded()["tri"][key]
    assert rl <= 2.0 / 3.0 or rl <= 1.25 * rec
    for T in (Rm, Sm):
        Y.check_partition(T, Y.starts(T))
    X = ref_tri(name, trans_b)
    r = Y.figure(Rm, Y.op(Sm, trans_b), F, X)
    print(f"{key}: r={r:.3g} LAPACK {rl:.3g} recorded {rec:.3g}")
    assert r <= Y.bound(rec)


@pytest.mark.parametrize("trans_b", [False, True])
@pytest.mark.parametrize("name", Y.TRI_ALL)
def test_componentwise_figure_on_the_constructed_cases(name, trans_b):
    Rm, Sm, F = Y.tri_case(name)
    key = f"{name}/{'H' if trans_b else 'N'}"
    rec = recorded()
    wl, wrec = lapack_tri_cw(name, trans_b), rec["tri_cw"][key]
    floor = rec["cw_floor"]["complex" if np.iscomplexobj(Rm) else "real"]
    w = Y.figure_cw(Rm, Y.op(Sm, trans_b), F, ref_tri(name, trans_b))
    print(f"{key}: w={w:.3g} LAPACK {wl:.3g} recorded {wrec:.3g} floor {floor:.3g}")
    assert np.isfinite(wl) and wl <= 1.25 * wrec
    assert w <= Y.bound_cw(wrec, floor)


def test_the_floors_are_three_times_the_largest_recorded_w():
    rec = recorded()
    for kind in ("real", "complex"):
        ws = [rec["tri_cw"][f"{nm}/{t}"] for nm in Y.TRI_ALL for t in "NH" if Y.is_complex_case(nm) == (kind == "complex")]
        assert rec["cw_floor"][kind] == 3.0 * max(ws)
    assert set(rec["tri_cw"]) == set(rec["tri"]) == {f"{nm}/{t}" for nm in Y.TRI_ALL for t in "NH"}


def test_figure_cw_sees_what_the_normwise_figure_cannot():
    """A relative error of 1e-8 (half the digits) in the smallest entry of Y of close1e-08: r does not move, w
    leaves its bound by orders of magnitude; a zero denominator with a non-zero residual gives inf."""
    Rm, Sm, F = Y.tri_case("close1e-08")
    X = np.array(ref_tri("close1e-08", False))
    k = np.unravel_index(np.argmin(np.abs(X)), X.shape)
    r0, w0 = Y.figure(Rm, Sm, F, X), Y.figure_cw(Rm, Sm, F, X)
    X[k] *= 1.0 + 1e-8
    r1, w1 = Y.figure(Rm, Sm, F, X), Y.figure_cw(Rm, Sm, F, X)
    print(f"r {r0:.3g} -> {r1:.3g}, w {w0:.3g} -> {w1:.3g}")
    assert r1 <= 1.01 * r0 and w0 <= 6.0 and w1 > 1e3 * 6.0
    Z = np.zeros((2, 2))
    assert Y.figure_cw(Z, Z, Z, np.ones((2, 2))) == 0.0
    assert Y.figure_cw(Z, Z, np.ones((2, 2)) - 1.0, Z) == 0.0
    assert Y.figure_cw(np.eye(2), Z, np.diag([1.0, 1.0]), np.eye(2)) == 0.0
    assert Y.figure_cw(Z, Z, np.ones((2, 2)), Z) == 1.0 / Y.EPS


def test_figure_scaled_equals_figure_where_both_can_be_formed():
    for name in ("r65x63", "c33x65", "r3x2", "lyap65"):
        A, B, C = Y.case(name)
        X = sla.solve_sylvester(A, B, C)
        a, b = Y.figure(A, B, C, X), Y.figure_scaled(A, B, C, X)
        assert abs(a - b) <= 1e-12 * a
    A, B, C = Y.case("r65x63*C+")
    assert not np.isfinite(np.linalg.norm(C))     # the plain figure cannot be formed here
    assert np.isfinite(Y.figure_scaled(A, B, C, sla.solve_sylvester(A, B, C)))


@pytest.mark.parametrize("trans_b", [False, True])
@pytest.mark.parametrize("name", ["r130x66", "odd129", "c65"])
def test_trsyl_ref_commutes_with_powers_of_two(name, trans_b):
    """the property tests/test_gpu_trsyl.py asks of the device, bit for bit"""
    Rm, Sm, F = Y.tri_case(name)
    X = ref_tri(name, trans_b)
    for e in (-300, 300):
        assert np.array_equal(Y.trsyl_ref(Y.ldexp(Rm, e), Y.ldexp(Sm, e), Y.ldexp(F, e), trans_b), X)
        assert np.array_equal(Y.trsyl_ref(Rm, Sm, Y.ldexp(F, e), trans_b), Y.ldexp(X, e))


def test_dtrsyl_smin_is_global():
    """R = diag(1, .., 1, 4) of order 65, S = [-1 + 2 eps]: LAPACK's smin = eps max(||R||, ||S||) = 4 eps is above
    every pivot 2 eps of the first 64 rows, so dtrsyl perturbs them (info = 1).  The device's smin is per diagonal
    block (eps in the first block, rows 0 .. 63), which tests/test_gpu_trsyl.py pins."""
    d = np.ones(65)
    d[64] = 4.0
    x, scale, info = Y.lapack.dtrsyl(np.diag(d), np.array([[-1.0 + 2 * Y.EPS]]), np.ones((65, 1)))
    assert info == 1
    assert np.all(x[:64, 0] / scale == 1.0 / (4 * Y.EPS))


def test_the_constructed_cases_reach_the_partition_paths():
    assert Y.starts(Y.tri_case("pairs128")[0]) == [0, 64, 128]          # no boundary moves
    assert Y.starts(Y.tri_case("odd129")[0]) == [0, 63, 127, 129]       # pairs at odd rows: 64 would split one, 127 does not
    assert Y.starts(Y.tri_case("r200")[0]) == [0, 63, 126, 190, 200]    # pairs across rows 63 | 64 and 126 | 127
    assert Y.starts(Y.tri_case("r65")[0]) == [0, 63, 65]
    assert Y.starts(Y.tri_case("r64")[0]) == [0, 64]
    assert Y.starts(Y.tri_case("c65")[0]) == [0, 32, 64, 65]
    assert Y.starts(Y.tri_case("c33")[0]) == [0, 32, 33]
    Rm, Sm, _ = Y.tri_case("close1e-12")
    assert Y.starts(Rm) == Y.starts(Sm) == [0, 63, 126, 130]            # the hits at 63 and 126 sit across boundaries
    assert Y.starts(Y.tri_case("nonnormal130p")[0]) == [0, 63, 126, 130]
    assert Y.starts(Y.tri_case("cclose1e-12")[0]) == [0, 32, 64, 65]


def test_the_close_cases_have_their_hits():
    for d in (1e-4, 1e-8, 1e-12):
        Rm, Sm, _ = Y.tri_case(f"close{d:.0e}")
        for T in (Rm, Sm):   # still schur's standard form
            for k in np.flatnonzero(np.diagonal(T, -1)):
                assert T[k, k] == T[k + 1, k + 1] and T[k, k + 1] * T[k + 1, k] < 0
        lam, mu = np.linalg.eigvals(Rm), np.linalg.eigvals(Sm)
        gaps = np.sort(np.abs(lam[:, None] + mu[None, :]).ravel())
        # 2 one-by-one hits and 3 x 2 conjugate pairs of two-by-two hits; rounding of order eps moves a sum
        assert np.count_nonzero(np.abs(gaps - d) <= 64 * Y.EPS) == 8 and gaps[0] >= d - 64 * Y.EPS
        for tb, nm in ((False, f"cclose{d:.0e}"), (True, f"cclose{d:.0e}h")):
            Rc, Sc, _ = Y.tri_case(nm)
            g = np.sort(np.abs(np.diagonal(Rc)[:, None] + np.diagonal(Y.op(Sc, tb))[None, :]).ravel())
            assert np.count_nonzero(np.abs(g - d) <= 8 * Y.EPS) == 4 and g[0] >= d - 8 * Y.EPS


@pytest.mark.parametrize("pattern", ["pairs", "odd", "none"])
def test_check_partition(pattern):
    for n in range(1, 201):
        T = np.triu(np.ones((n, n)))
        first = {"pairs": 0, "odd": 1, "none": n}[pattern]
        for k in range(first, n - 1, 2):
            T[k + 1, k] = -1.0
        for nb in (64, 32, 2):
            s = Y.starts(T, nb)
            Y.check_partition(T, s, nb)
            if pattern == "none":
                assert s == list(range(0, n, nb)) + [n]


def test_check_partition_rejects():
    T = np.triu(np.ones((130, 130)))
    T[64, 63] = -1.0
    with pytest.raises(AssertionError):
        Y.check_partition(T, [0, 64, 128, 130], 64)     # splits the pair
    Y.check_partition(T, [0, 63, 127, 130], 64)
    with pytest.raises(AssertionError):
        Y.check_partition(T, [0, 62, 126, 130], 64)     # a block of nb - 2 rows
    with pytest.raises(AssertionError):
        Y.check_partition(T, [0, 63, 127], 64)          # does not reach n


if __name__ == "__main__":
    out = {"named": {nm: lapack_named(nm) for nm in ALL_NAMED}, "tri": {}, "tri_cw": {}}
    worst = {"real": 0.0, "complex": 0.0}
    for nm in Y.TRI_ALL:
        for tb in (False, True):
            k = f"{nm}/{'H' if tb else 'N'}"
            out["tri"][k] = lapack_tri(nm, tb)
            out["tri_cw"][k] = lapack_tri_cw(nm, tb)
            kind = "complex" if Y.is_complex_case(nm) else "real"
            worst[kind] = max(worst[kind], out["tri_cw"][k])
    out["cw_floor"] = {kind: 3.0 * v for kind, v in worst.items()}
    for kind, figs in out.items():
        for nm, v in figs.items():
            print(kind, nm, f"{v:.3g}")
    with open(GOLDEN, "w") as fh:
        json.dump(out, fh, indent=1, sort_keys=True)
        fh.write("\n")
