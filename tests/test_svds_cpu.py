"""CPU: the NumPy restatement of svds (tests/svds_ref.py) on its named cases.  The golden file pins the
restatement's figures, cycles and products; r and e are held to 1.5 on the restatement itself (den carries the
stopping tolerance and the rounding term n eps s_0, so a converged run sits below 1 in both up to the small SVD's
own error)."""
import numpy as np
import pytest

import svds_ref as R

NAMES = list(R.CASES) + ["big"]


@pytest.fixture(scope="module")
def golden():
    return R.load_golden()


def test_golden_holds_every_case(golden):
    assert sorted(golden) == sorted(R.key(nm, dt) for nm in NAMES for dt in R.DTYPES)


@pytest.mark.parametrize("dtype", R.DTYPES)
@pytest.mark.parametrize("name", NAMES)
def test_restatement_matches_golden(golden, name, dtype):
    res, rec = R.run_case(name, dtype)
    pin = golden[R.key(name, dtype)]
    print(R.key(name, dtype), {q: rec[q] for q in rec if q != "s_ref"})
    assert res["converged"] and pin["converged"]
    assert np.all(np.diff(res["s"]) <= 0)
    assert rec["r"] <= 1.5 and rec["e"] <= 1.5
    assert pin["r"] <= 1.5 and pin["e"] <= 1.5
    # the reference values are recomputed by the LAPACK at hand: equal to the pinned ones to rounding
    assert np.allclose(rec["s_ref"], pin["s_ref"], rtol=1e-13, atol=0)
    if name.startswith("rank3"):
        return   # whether the alpha floor trips at step 3 is a matter of rounding: only the results are pinned
    # cycles and products: a BLAS with another summation order may move a slow case by a cycle
    assert abs(rec["restarts"] - pin["restarts"]) <= 1
    assert abs(rec["applications"] - pin["applications"]) <= 2 * R.CASES.get(name, R.BIG)[2]
    for q in ("o_u", "o_v"):
        assert rec[q] <= max(2.0, 3.0 * pin[q])


@pytest.mark.parametrize("dtype", R.DTYPES)
@pytest.mark.parametrize("kind", ["beta", "alpha"])
def test_breakdown_cases(kind, dtype):
    A, v0, ncv, apps = R.breakdown_case(kind, dtype)
    for nsv in (1, 2):
        res = R.svds(R.DenseOp(A), nsv, ncv, v0)
        assert res["converged"] and res["applications"] == apps and res["restarts"] == 1
        assert np.all(np.abs(res["s"] - np.array([3.0, 2.0])[:nsv]) <= 1e-14)
        assert np.all(res["residuals"] <= 1e-13)
    with pytest.raises(ArithmeticError, match="dimension 2 < nsv"):
        R.svds(R.DenseOp(A), 3, ncv, v0)
    A, v0, ncv, _ = R.breakdown_case(kind, dtype, fail=True)
    with pytest.raises(ArithmeticError, match="dimension 2 < nsv"):
        R.svds(R.DenseOp(A), 3, ncv, v0)


def test_one_cycle_and_negative_tolerance():
    shape, nsv, ncv = R.CASES["slow"]
    op = R.operator("slow", np.float64)
    res = R.svds(op, nsv, ncv, R.start_vector(shape[1], np.float64), max_restarts=1)
    assert res["restarts"] == 1 and res["applications"] == 2 * ncv and not res["converged"]
    res = R.svds(op, nsv, ncv, R.start_vector(shape[1], np.float64), tol=-1.0, max_restarts=3)
    assert res["restarts"] == 3 and not res["converged"]
