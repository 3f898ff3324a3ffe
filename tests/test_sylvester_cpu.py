"""CPU: the cases, the figure and the restated schedule of the Sylvester tests (tests/sylvester_ref.py) are sound
with the reference alone.

``scipy.linalg.solve_sylvester`` / ``solve_continuous_lyapunov`` (LAPACK xGEES + xTRSYL) run on every named
case: the figure r = ||A X + X op(B) - C||_F / (max(m, n) eps ((||A||_F + ||B||_F) ||X||_F + ||C||_F)) must be at
most 2/3, so that the GPU tests' bound max(2, 3 x LAPACK's figure) is its floor 2 wherever LAPACK is that good; a
case above 2/3 must stay within 1.25 of what tests/golden/sylvester_ref_figures.json records for it (the rule of
tests/test_schur_cpu.py).  On the constructed triangular cases LAPACK's figure is xTRSYL's own, also recorded.
``trsyl_ref``, the NumPy statement of the device's partition and three-launch wavefront schedule, must meet
the GPU tests' bound on every named and every constructed case.

    python tests/test_sylvester_cpu.py        # rewrites tests/golden/sylvester_ref_figures.json
"""
import json
import os

import numpy as np
import pytest
import scipy.linalg as sla

import sylvester_ref as Y

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "sylvester_ref_figures.json")
_runs = {}


def lapack_named(name):
    """LAPACK's figure on one named case, once per session."""
    if name not in _runs:
        A, B, C = Y.case(name)
        X = sla.solve_continuous_lyapunov(np.array(A), np.array(C)) if name in Y.LYAPUNOV else sla.solve_sylvester(A, B, C)
        _runs[name] = Y.figure(A, B, C, X)
    return _runs[name]


def lapack_tri(name, trans_b):
    key = f"{name}/{'H' if trans_b else 'N'}"
    if key not in _runs:
        Rm, Sm, F = Y.tri_case(name)
        _runs[key] = Y.figure(Rm, Y.op(Sm, trans_b), F, Y.lapack_trsyl(Rm, Sm, F, trans_b))
    return _runs[key]


def recorded():
    with open(GOLDEN) as f:
        return json.load(f)


@pytest.mark.parametrize("name", Y.NAMES + Y.LYAPUNOV)
def test_lapack_on_the_named_cases(name):
    r, rec = lapack_named(name), recorded()["named"][name]
    print(f"{name}: r={r:.3g} recorded {rec:.3g}")
    assert np.isfinite(r)
    assert r <= 2.0 / 3.0 or r <= 1.25 * rec


@pytest.mark.parametrize("name", Y.NAMES + Y.LYAPUNOV)
def test_trsyl_ref_on_the_named_cases(name):
    A, B, C = Y.case(name)
    lyap = name in Y.LYAPUNOV
    X = Y.bartels_stewart_ref(A, A if lyap else B, C, trans_b=lyap)
    r, rec = Y.figure(A, B, C, X), recorded()["named"][name]
    print(f"{name}: r={r:.3g} LAPACK {rec:.3g}")
    assert X.dtype == np.result_type(A, B, C)
    assert r <= Y.bound(rec)


@pytest.mark.parametrize("trans_b", [False, True])
@pytest.mark.parametrize("name", Y.TRI)
def test_trsyl_ref_on_the_constructed_cases(name, trans_b):
    Rm, Sm, F = Y.tri_case(name)
    key = f"{name}/{'H' if trans_b else 'N'}"
    rl, rec = lapack_tri(name, trans_b), recorded()["tri"][key]
    assert rl <= 2.0 / 3.0 or rl <= 1.25 * rec
    for T in (Rm, Sm):
        Y.check_partition(T, Y.starts(T))
    X = Y.trsyl_ref(Rm, Sm, F, trans_b)
    r = Y.figure(Rm, Y.op(Sm, trans_b), F, X)
    print(f"{key}: r={r:.3g} LAPACK {rl:.3g} recorded {rec:.3g}")
    assert r <= Y.bound(rec)


def test_the_constructed_cases_reach_the_partition_paths():
    assert Y.starts(Y.tri_case("pairs128")[0]) == [0, 64, 128]          # no boundary moves
    assert Y.starts(Y.tri_case("odd129")[0]) == [0, 63, 127, 129]       # pairs at odd rows: 64 would split one, 127 does not
    assert Y.starts(Y.tri_case("r200")[0]) == [0, 63, 126, 190, 200]    # pairs across rows 63 | 64 and 126 | 127
    assert Y.starts(Y.tri_case("r65")[0]) == [0, 63, 65]
    assert Y.starts(Y.tri_case("r64")[0]) == [0, 64]
    assert Y.starts(Y.tri_case("c65")[0]) == [0, 32, 64, 65]
    assert Y.starts(Y.tri_case("c33")[0]) == [0, 32, 33]


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
    out = {"named": {nm: lapack_named(nm) for nm in Y.NAMES + Y.LYAPUNOV}, "tri": {}}
    for nm in Y.TRI:
        for tb in (False, True):
            out["tri"][f"{nm}/{'H' if tb else 'N'}"] = lapack_tri(nm, tb)
    for kind, figs in out.items():
        for nm, v in figs.items():
            print(kind, nm, f"{v:.3g}")
    with open(GOLDEN, "w") as fh:
        json.dump(out, fh, indent=1, sort_keys=True)
        fh.write("\n")
