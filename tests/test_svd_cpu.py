"""CPU: pins the NumPy restatement of svd (tests/svd_ref.py) that the GPU tests measure the device code against.

Figures, for A (m x n), N = max(m, n), eps = 2^-52:
    r   = ||A V - U diag(s)||_F / (N eps ||A||_F)        o_u = ||U^H U - I||_F / (N eps)
    o_v = ||V^H V - I||_F / (N eps)                      e   = max |s - s_LAPACK| / (N eps s_1)
For every named matrix the restatement converges inside the 60-sweep cap with not_converged == 0, and each
figure is <= max(2, 3 x LAPACK's own figure) or <= the ``*_max`` recorded in tests/golden/svd_ref_figures.json
(the measured value x 1.25, rounded up to three digits: the allowance covers BLAS libraries that sum in another
order; for e, whose LAPACK figure is 0 by definition, the bound is max(2, recorded)).  The file also records the sweeps, and for
graded30x24 the largest relative error of a singular value against the long-double Hestenes Jacobi, with
LAPACK's beside it; tests/test_gpu_svd.py takes all of these as the restatement's.

    python tests/test_svd_cpu.py        # rewrites tests/golden/svd_ref_figures.json
"""
import json
import math
import os

import numpy as np
import pytest

import svd_ref as R

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "svd_ref_figures.json")
FIGS = ("r", "ou", "ov", "e")
_runs = {}


def run(name):
    """The restatement and LAPACK on one matrix, once per session: dict of figures, and (U, s, V)."""
    if name not in _runs:
        A = R.matrix(name)
        U, s, V, sweeps, nc = R.svd_ref(A)
        sl = R.lapack_s(A)
        r, ou, ov, e = R.figures(A, U, s, V, sl)
        rl, oul, ovl = R.lapack_figures(A)
        fig = {"r": r, "ou": ou, "ov": ov, "e": e, "sweeps": sweeps, "not_converged": nc, "r_lapack": rl,
               "ou_lapack": oul, "ov_lapack": ovl, "e_lapack": 0.0}
        if name == "graded30x24":
            ld = R.hestenes_longdouble(A)
            fig["rel"] = R.max_relative_error(s, ld)
            fig["rel_lapack"] = R.max_relative_error(sl, ld)
        _runs[name] = (fig, U, s, V)
    return _runs[name]


def recorded():
    with open(GOLDEN) as f:
        return json.load(f)


@pytest.mark.parametrize("name", R.NAMES)
def test_restatement_figures(name):
    fig = run(name)[0]
    rec = recorded()[name]
    print(name, {k: (f"{v:.3g}" if isinstance(v, float) else v) for k, v in fig.items()})
    assert fig["not_converged"] == 0
    assert fig["sweeps"] <= 60
    for k in FIGS:
        assert np.isfinite(fig[k])
        assert fig[k] <= max(2.0, 3.0 * fig[k + "_lapack"]) or fig[k] <= rec[k + "_max"], k


def test_descending_and_phase():
    for name in ("rand97", "crand65", "wide70x130", "rank1_70"):
        _, U, s, V = run(name)
        assert np.all(s[:-1] >= s[1:])
        for j in range(V.shape[1]):
            k = int(np.argmax(np.abs(V[:, j])))
            assert V[k, j].imag == 0 and V[k, j].real > 0


def test_graded_relative_accuracy():
    """column scaling keeps the relative accuracy of every singular value; LAPACK's gesdd loses the small ones"""
    fig = run("graded30x24")[0]
    print(f"graded30x24: rel={fig['rel']:.3g} rel_lapack={fig['rel_lapack']:.3g}")
    # Demmel and Veselic: the relative error of every singular value is of order eps cond(B), B = A with its
    # columns scaled to unit norm; m eps cond(B) allows the length-m sums their worst case
    A = R.matrix("graded30x24")
    B = A / np.linalg.norm(A, axis=0)
    assert fig["rel"] <= A.shape[0] * R.EPS * np.linalg.cond(B)
    assert fig["rel"] < fig["rel_lapack"]


def test_eye_is_exact():
    fig, U, s, V = run("eye33")
    assert fig["sweeps"] == 1
    assert np.array_equal(U, np.eye(33)) and np.array_equal(V, np.eye(33)) and np.array_equal(s, np.ones(33))


def test_zero_matrix_completes_u():
    fig, U, s, V = run("zero9x5")
    assert np.array_equal(s, np.zeros(5)) and np.array_equal(V, np.eye(5))
    assert fig["ou"] <= 1.0
    assert np.array_equal(U, np.eye(9)[:, :5])


def test_diag_gives_a_permutation():
    fig, U, s, V = run("diag50")
    d = np.diag(R.matrix("diag50"))
    assert fig["sweeps"] == 1
    assert np.array_equal(s, np.sort(np.abs(d))[::-1])
    assert np.array_equal(np.sort(V, axis=0)[-1], np.ones(50)) and np.count_nonzero(V) == 50
    assert np.array_equal(U * s @ V.T, R.matrix("diag50"))


@pytest.mark.parametrize("name", ["ones40", "zero9x5"])
def test_exact_zero_columns_are_met(name):
    """these inputs reach the completion of U: some singular values are exactly 0 (dupcols50x40's null singular
    values come out at rounding level here, so it tests the other branch: tiny columns that are normalised)"""
    _, U, s, V = run(name)
    assert np.count_nonzero(s == 0.0) > 0


def test_scaling_by_a_power_of_two():
    """2^600 A and 2^-600 A: s scales, U and V stay"""
    _, U0, s0, V0 = run("rand97")
    for name, e in (("rand97_big", 600), ("rand97_small", -600)):
        _, U, s, V = run(name)
        assert np.array_equal(np.ldexp(s, -e), s0)
        assert np.max(np.abs(U - U0)) <= 1e-10 and np.max(np.abs(V - V0)) <= 1e-10


def _round_up(x, digits=3):
    if x == 0 or not math.isfinite(x):
        return x
    q = 10.0 ** (digits - 1 - math.floor(math.log10(abs(x))))
    return math.ceil(x * q) / q


if __name__ == "__main__":
    out = {}
    for nm in R.NAMES:
        f = dict(run(nm)[0])
        for k in FIGS:
            f[k + "_max"] = _round_up(1.25 * f[k])
        out[nm] = f
        print(nm, f)
    with open(GOLDEN, "w") as fh:
        json.dump(out, fh, indent=1, sort_keys=True)
        fh.write("\n")
