"""GPU: EigSol::krylovSchur through the C++ façade (tests/cpp/test_krylov.cpp) on case a (largest
modulus) and the shifted Laplacian (shift-invert about 0) of tests/krylov_ref.py."""
import os
import subprocess

import pytest
import scipy.sparse as sp

from cpp_build import ROOT, build

import krylov_ref as K

pytestmark = pytest.mark.gpu


def _write_matrix(path, A):
    A = sp.coo_matrix(A)
    with open(path, "w") as f:
        f.write(f"sparse\n{A.shape[0]} {A.shape[1]}\n{A.nnz}\n")
        for r, c, v in zip(A.row, A.col, A.data):
            f.write(f"{r} {c} {float(v)!r}\n")


def _write_values(path, w):
    with open(path, "w") as f:
        for z in w:
            f.write(f"{complex(z).real!r} {complex(z).imag!r}\n")


def test_cpp_krylov_schur(tmp_path):
    exe = build(os.path.join(ROOT, "tests", "cpp", "test_krylov.cpp"), str(tmp_path / "test_krylov"))
    args = [str(tmp_path / f) for f in ("a.txt", "a_eigs.txt", "lap.txt", "lap_eigs.txt")]
    _write_matrix(args[0], K.matrix("a"))
    _write_values(args[1], K.wanted("a_lm"))
    _write_matrix(args[2], K.matrix("lap"))
    _write_values(args[3], K.wanted("lap_si"))
    r = subprocess.run([exe] + args, capture_output=True, text=True, timeout=120)
    print(r.stdout)
    assert r.returncode == 0 and "ALL PASSED" in r.stdout, r.stdout[-3000:] + r.stderr[-2000:]
