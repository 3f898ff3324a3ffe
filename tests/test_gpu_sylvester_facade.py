"""GPU: EigSol::solve_sylvester / solve_lyapunov through the C++ façade (tests/cpp/test_sylvester.cpp) on r65x63,
c63x65 and lyap65 of tests/sylvester_ref.py under the bound of tests/test_gpu_sylvester.py, and on r65x63 rounded to
float (promoted to fp64 by the façade).  The bounds max(2, 3 r_LAPACK) are passed in a file."""
import os
import subprocess

import numpy as np
import pytest

from cpp_build import ROOT, build

import sylvester_ref as Y
from test_gpu_sylvester import lapack

pytestmark = pytest.mark.gpu

CASES = ("r65x63", "c63x65", "lyap65")


def _write_case(path, name):
    """"m n" (n = 0: a Lyapunov case, no B), then A, B and C as lines "re im", column-major."""
    A, B, Cm = Y.case(name)
    lyap = name in Y.LYAPUNOV
    with open(path, "w") as f:
        f.write(f"{A.shape[0]} {0 if lyap else B.shape[0]}\n")
        for M in (A, Cm) if lyap else (A, B, Cm):
            for v in np.asarray(M).ravel(order="F"):
                f.write(f"{complex(v).real!r} {complex(v).imag!r}\n")


def test_cpp_sylvester(tmp_path):
    exe = build(os.path.join(ROOT, "tests", "cpp", "test_sylvester.cpp"), str(tmp_path / "test_sylvester"))
    args = [str(tmp_path / f"{nm}.txt") for nm in CASES] + [str(tmp_path / "bounds.txt")]
    for path, name in zip(args, CASES):
        _write_case(path, name)
    with open(args[-1], "w") as f:
        f.write(" ".join(repr(Y.bound(lapack()[nm])) for nm in CASES) + "\n")
    r = subprocess.run([exe] + args, capture_output=True, text=True, timeout=120)
    print(r.stdout)
    assert r.returncode == 0 and "ALL PASSED" in r.stdout, r.stdout[-3000:] + r.stderr[-2000:]
