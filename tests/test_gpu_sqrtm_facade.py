"""GPU: EigSol::sqrtm through the C++ façade (tests/cpp/test_sqrtm.cpp) on r65, c65 and ur65 of tests/sqrtm_ref.py
(a real root, a complex matrix, a real matrix whose root is complex) under the bound of tests/test_gpu_sqrtm.py,
and on r65 rounded to float (promoted to fp64 by the façade).  The bounds max(2, 3 r_SciPy) are passed in a file."""
import os
import subprocess

import numpy as np
import pytest

from cpp_build import ROOT, build

import sqrtm_ref as Q

pytestmark = pytest.mark.gpu

CASES = ("r65", "c65", "ur65")


def _write_case(path, name):
    """"n", then A as lines "re im", column-major."""
    A = Q.case(name)
    with open(path, "w") as f:
        f.write(f"{A.shape[0]}\n")
        for v in np.asarray(A).ravel(order="F"):
            f.write(f"{complex(v).real!r} {complex(v).imag!r}\n")


def test_cpp_sqrtm(tmp_path):
    exe = build(os.path.join(ROOT, "tests", "cpp", "test_sqrtm.cpp"), str(tmp_path / "test_sqrtm"))
    args = [str(tmp_path / f"{nm}.txt") for nm in CASES] + [str(tmp_path / "bounds.txt")]
    for path, name in zip(args, CASES):
        _write_case(path, name)
    rec = Q.golden()["named"]
    with open(args[-1], "w") as f:
        f.write(" ".join(repr(Q.bound(rec[nm])) for nm in CASES) + "\n")
    r = subprocess.run([exe] + args, capture_output=True, text=True, timeout=120)
    print(r.stdout)
    assert r.returncode == 0 and "ALL PASSED" in r.stdout, r.stdout[-3000:] + r.stderr[-2000:]
