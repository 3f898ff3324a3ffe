"""CPU: the cases, the figures and the restatements of the matrix square root tests (tests/sqrtm_ref.py) are
sound with the references alone.

``scipy.linalg.sqrtm`` runs on every named case: its figure r = ||X^2 - A||_F / (n eps ||X||_F^2) must be at most
2/3, so that the GPU tests' bound max(2, 3 x SciPy's figure) is its floor 2 wherever SciPy is that good; a case
above 2/3 must stay within 1.25 of what tests/golden/sqrtm_ref_figures.json records for it (the rule of
tests/test_sylvester_cpu.py).  On the constructed triangular cases, hard ones included, the unblocked recurrence
``sqrt_recurrence`` is the reference: its componentwise figure w is finite and within 1.25 of its recorded value,
and ``trsqrt_ref``, the NumPy statement of the device's partition and two-launch schedule, meets the GPU tests'
bounds on r and on w.  The golden file also holds "cw_floor" (3 x the recurrence's largest w per scalar type) and
"mp_gap": ||X_scipy - X_mp||_F / ||X_mp||_F for the named cases of order <= 65, X_mp being the root recomputed in
mpmath at 50 digits (minutes of host time, so only the command below computes it).

    python tests/test_sqrtm_cpu.py        # rewrites tests/golden/sqrtm_ref_figures.json
"""
import json

import numpy as np
import pytest

import sqrtm_ref as Q
import sylvester_ref as Y

_runs = {}


def scipy_named(name):
    """SciPy's root of one named case, once per session."""
    if name not in _runs:
        _runs[name] = Q.scipy_root(Q.case(name), name in Q.REAL_ROOT)
        _runs[name].setflags(write=False)
    return _runs[name]


def recurrence(name):
    key = "rec:" + name
    if key not in _runs:
        _runs[key] = Q.sqrt_recurrence(Q.tri_case(name))
    return _runs[key]


def blocked(name):
    key = "blk:" + name
    if key not in _runs:
        _runs[key] = Q.trsqrt_ref(Q.tri_case(name))
    return _runs[key]


@pytest.mark.parametrize("name", Q.NAMES)
def test_scipy_on_the_named_cases(name):
    A, X = Q.case(name), scipy_named(name)
    r, rec = Q.figure(A, X), Q.golden()["named"][name]
    print(f"{name}: r={r:.3g} recorded {rec:.3g}")
    assert X.dtype == (np.float64 if name in Q.REAL_ROOT else np.complex128)
    assert np.isfinite(r)
    assert r <= 2.0 / 3.0 or r <= 1.25 * rec


def test_the_unshifted_real_cases_have_negative_real_eigenvalues():
    for name, count in zip(Q.NEEDS_COMPLEX, (2, 3, 5)):
        ev = np.linalg.eigvals(Q.case(name))
        assert np.count_nonzero((ev.imag == 0) & (ev.real < 0)) == count


@pytest.mark.parametrize("name", Q.TRI_ALL)
def test_the_recurrence_on_the_constructed_cases(name):
    T, U = Q.tri_case(name), recurrence(name)
    rec = Q.golden()
    w, r = Q.figure_cw(T, U), Q.figure(T, U)
    print(f"{name}: w={w:.3g} recorded {rec['tri_cw'][name]:.3g}; r={r:.3g} recorded {rec['tri'][name]:.3g}")
    assert U.dtype == T.dtype and np.all(np.isfinite(U))
    assert np.isfinite(w) and w <= 1.25 * rec["tri_cw"][name]
    assert r <= 2.0 / 3.0 or r <= 1.25 * rec["tri"][name]
    assert np.all(Q.group_eigenvalues(U).real >= 0)


@pytest.mark.parametrize("name", Q.TRI_ALL)
def test_trsqrt_ref_on_the_constructed_cases(name):
    T, U = Q.tri_case(name), blocked(name)
    rec = Q.golden()
    Y.check_partition(T, Y.starts(T))
    floor = rec["cw_floor"]["complex" if Q.is_complex_case(name) else "real"]
    w, r = Q.figure_cw(T, U), Q.figure(T, U)
    print(f"{name}: w={w:.3g} (recurrence {rec['tri_cw'][name]:.3g}, floor {floor:.3g}) r={r:.3g}")
    assert U.dtype == T.dtype
    assert np.array_equal(U[~Q.quasi_mask(T)], np.zeros(np.count_nonzero(~Q.quasi_mask(T))))
    assert r <= Q.bound(rec["tri"][name])
    assert w <= Q.bound_cw(rec["tri_cw"][name], floor)


def test_the_floors_are_three_times_the_largest_recorded_w():
    rec = Q.golden()
    for kind in ("real", "complex"):
        ws = [rec["tri_cw"][nm] for nm in Q.TRI_ALL if Q.is_complex_case(nm) == (kind == "complex")]
        assert rec["cw_floor"][kind] == 3.0 * max(ws)


def test_the_gap_table_covers_the_small_named_cases():
    rec = Q.golden()["mp_gap"]
    assert sorted(rec) == sorted(Q.MP_NAMES)
    assert all(np.isfinite(v) and 0.0 <= v < 1e-6 for v in rec.values())


def test_r_is_nearly_blind_on_triangular_input():
    """an error of 1e3 eps in one entry of U far from the diagonal: w sees it, r does not"""
    T = Q.tri_case("r130")
    U = np.array(recurrence("r130"))
    U[3, 120] *= 1.0 + 1e3 * Q.EPS
    assert Q.figure(T, U) < 1.0
    assert Q.figure_cw(T, U) > 30.0


if __name__ == "__main__":
    out = {"named": {}, "mp_gap": {}, "tri": {}, "tri_cw": {}, "cw_floor": {}}
    for nm in Q.TRI_ALL:
        out["tri"][nm] = Q.figure(Q.tri_case(nm), recurrence(nm))
        out["tri_cw"][nm] = Q.figure_cw(Q.tri_case(nm), recurrence(nm))
        print(nm, out["tri"][nm], out["tri_cw"][nm], flush=True)
    for kind in ("real", "complex"):
        out["cw_floor"][kind] = 3.0 * max(out["tri_cw"][nm] for nm in Q.TRI_ALL
                                          if Q.is_complex_case(nm) == (kind == "complex"))
    for nm in Q.NAMES:
        out["named"][nm] = Q.figure(Q.case(nm), scipy_named(nm))
        print(nm, out["named"][nm], flush=True)
    for nm in Q.MP_NAMES:
        out["mp_gap"][nm] = Q.gap(scipy_named(nm), Q.mp_root(Q.case(nm)))
        print(nm, "gap", out["mp_gap"][nm], flush=True)
    with open(Q.GOLDEN, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")
