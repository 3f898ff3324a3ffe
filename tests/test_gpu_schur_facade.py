"""GPU: EigSol::schur through the C++ façade (tests/cpp/test_schur.cpp) on gen65 and cgen70 of tests/schur_ref.py
under the conditions of tests/test_gpu_schur.py, and on gen65 rounded to float (promoted to fp64 by the
façade): the program checks the structure of T, both figures, the eigenvalues and the call without vectors."""
import os
import subprocess

import numpy as np
import pytest

from cpp_build import ROOT, build

import schur_ref as S
from test_gpu_eigh_facade import _write_matrix
from test_gpu_schur import lapack

pytestmark = pytest.mark.gpu


def _write_expect(path, name):
    """"value_bound r_bound o_bound", then numpy.linalg.eigvals' eigenvalues "re im"."""
    A = S.matrix(name)
    ref = lapack()[name]
    with open(path, "w") as f:
        f.write(f"{S.value_bound(A)!r} {max(2.0, 3.0 * ref['r'])!r} {max(2.0, 3.0 * ref['o'])!r}\n")
        for v in np.linalg.eigvals(A):
            f.write(f"{complex(v).real!r} {complex(v).imag!r}\n")


def test_cpp_schur(tmp_path):
    exe = build(os.path.join(ROOT, "tests", "cpp", "test_schur.cpp"), str(tmp_path / "test_schur"))
    names = ("gen65", "cgen70")
    args = [str(tmp_path / f"{nm}{suffix}.txt") for nm in names for suffix in ("", "_expect")]
    for i, name in enumerate(names):
        _write_matrix(args[2 * i], S.matrix(name))
        _write_expect(args[2 * i + 1], name)
    r = subprocess.run([exe] + args, capture_output=True, text=True, timeout=120)
    print(r.stdout)
    assert r.returncode == 0 and "ALL PASSED" in r.stdout, r.stdout[-3000:] + r.stderr[-2000:]
