"""GPU: EigSol::expm and EigSol::solve through the C++ façade (tests/cpp/test_expm.cpp) on r65_40 and c65_40 of
tests/expm_ref.py under the bound of tests/test_gpu_expm.py, and on r65_40 rounded to float (promoted to fp64 by
the façade).  Each case file carries the plan, the bound and scipy.linalg.expm's result, and for A Y = exp(A) the
bound of tests/test_gpu_solve.py: 3 max(NumPy's figure on that system, NumPy's largest over the type's cases)."""
import os
import subprocess

import numpy as np
import pytest

from cpp_build import ROOT, build

import expm_ref as X
import test_gpu_solve as TS

pytestmark = pytest.mark.gpu

CASES = ("r65_40", "c65_40")


def _write_case(path, name):
    """"n degree squarings bound solve_bound", then A and X_scipy as lines "re im", column-major."""
    A, B = X.case(name), X.scipy_expm(name)
    m, s = X.PLAN_OF_TARGET[X.target_of(name)]
    cx = name[0] == "c"
    floor = max(TS.numpy_figure(*c) for c in TS.CASES if c[2] == cx)
    solve_bound = 3.0 * max(TS.figure(A, np.linalg.solve(A, B), B), floor)
    with open(path, "w") as f:
        f.write(f"{A.shape[0]} {m} {s} {X.bound(name)!r} {solve_bound!r}\n")
        for M in (A, X.scipy_expm(name)):
            for v in np.asarray(M).ravel(order="F"):
                f.write(f"{complex(v).real!r} {complex(v).imag!r}\n")


def test_cpp_expm(tmp_path):
    exe = build(os.path.join(ROOT, "tests", "cpp", "test_expm.cpp"), str(tmp_path / "test_expm"))
    args = [str(tmp_path / f"{nm}.txt") for nm in CASES]
    for path, name in zip(args, CASES):
        _write_case(path, name)
    r = subprocess.run([exe] + args, capture_output=True, text=True, timeout=120)
    print(r.stdout)
    assert r.returncode == 0 and "ALL PASSED" in r.stdout, r.stdout[-3000:] + r.stderr[-2000:]
