"""CPU: the checker and the inputs of the schur tests (tests/schur_ref.py) are sound with the reference alone.

``scipy.linalg.schur`` (LAPACK xGEES; ``output="real"`` for a real matrix) runs on every named matrix:
``check_structure`` must accept its T, and its figures r = ||A - Z T Z^H||_F / (n eps ||A||_F) and
o = ||Z^H Z - I||_F / (n eps) must be at most 2/3, so that the bound of tests/test_gpu_schur.py,
max(2, 3 x LAPACK's figure), is its floor 2 wherever LAPACK is that good.  A case above 2/3 with LAPACK alone
is kept: it must then stay within 1.25 of what tests/golden/schur_ref_figures.json records for it (the
allowance covers BLAS libraries that sum in another order), and the GPU bound is 3 x the recorded figure.

    python tests/test_schur_cpu.py        # rewrites tests/golden/schur_ref_figures.json
"""
import json
import os

import numpy as np
import pytest
import scipy.linalg as sla

import eig_ref as R
import schur_ref as S

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "schur_ref_figures.json")
_runs = {}


def run(name):
    """LAPACK on one matrix, once per session: (T, Z, r, o)."""
    if name not in _runs:
        A = S.matrix(name)
        real = not np.iscomplexobj(A)
        T, Z = sla.schur(np.array(A), output="real" if real else "complex")
        r, o = S.figures(A, T, Z)
        _runs[name] = (T, Z, r, o)
    return _runs[name]


def recorded():
    with open(GOLDEN) as f:
        return json.load(f)


@pytest.mark.parametrize("name", S.NAMES)
def test_lapack_passes_the_checker(name):
    A = S.matrix(name)
    T, Z, r, o = run(name)
    rec = recorded()[name]
    print(f"{name}: r={r:.3g} o={o:.3g} recorded r={rec['r']:.3g} o={rec['o']:.3g}")
    assert T.dtype == A.dtype and Z.dtype == A.dtype
    S.check_structure(T, not np.iscomplexobj(A))
    for fig, key in ((r, "r"), (o, "o")):
        assert np.isfinite(fig)
        assert fig <= 2.0 / 3.0 or fig <= 1.25 * rec[key]


@pytest.mark.parametrize("name", [k for k in S.NAMES if k in S.WELL_CONDITIONED])
def test_block_eigenvalues_are_the_eigenvalues(name):
    A = S.matrix(name)
    w = S.block_eigenvalues(run(name)[0])
    if not np.iscomplexobj(A):
        assert S.pairs_conjugate(w)
    assert R.match_one_to_one(w, np.linalg.eigvals(A)) <= S.value_bound(A)


def test_the_checker_rejects():
    T = np.triu(np.ones((4, 4)))
    S.check_structure(T, True)
    S.check_structure(T.astype(np.complex128), False)
    for i, j, v in ((2, 0, 1e-300), (1, 0, 1.0)):   # below the sub-diagonal; a block with b c > 0
        B = T.copy()
        B[i, j] = v
        with pytest.raises(AssertionError):
            S.check_structure(B, True)
    B = T.copy()
    B[1, 0] = B[2, 1] = -1.0   # consecutive sub-diagonal entries
    with pytest.raises(AssertionError):
        S.check_structure(B, True)
    B = T.copy()
    B[1, 0], B[1, 1] = -1.0, 1.0 + 2 * S.EPS   # unequal diagonal entries
    with pytest.raises(AssertionError):
        S.check_structure(B, True)
    B = T.astype(np.complex128)
    B[1, 0] = 1e-300j
    with pytest.raises(AssertionError):
        S.check_structure(B, False)


if __name__ == "__main__":
    out = {}
    for nm in S.NAMES:
        _, _, r_, o_ = run(nm)
        out[nm] = {"r": r_, "o": o_}
        print(nm, out[nm])
    with open(GOLDEN, "w") as fh:
        json.dump(out, fh, indent=1, sort_keys=True)
        fh.write("\n")
