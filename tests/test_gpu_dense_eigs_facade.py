"""GPU: EigSol::subspaceIteration_dense and EigSol::krylovSchur_dense through the C++ façade
(tests/cpp/test_dense_eigs.cpp) on the densified case a, shifted Laplacian (shift-invert about 0)
and complex case c of tests/krylov_ref.py."""
import os
import subprocess

import pytest
import scipy.sparse as sp

from cpp_build import ROOT, build

import krylov_ref as K

pytestmark = pytest.mark.gpu


def _write_matrix(path, A):
    """"n nnz", then "row col re im" per entry: the C++ test fills a DenseMatrix from it."""
    A = sp.coo_matrix(A)
    with open(path, "w") as f:
        f.write(f"{A.shape[0]} {A.nnz}\n")
        for r, c, v in zip(A.row, A.col, A.data):
            f.write(f"{r} {c} {complex(v).real!r} {complex(v).imag!r}\n")


def _write_values(path, w):
    with open(path, "w") as f:
        for z in w:
            f.write(f"{complex(z).real!r} {complex(z).imag!r}\n")


def test_cpp_dense_eigs(tmp_path):
    exe = build(os.path.join(ROOT, "tests", "cpp", "test_dense_eigs.cpp"), str(tmp_path / "test_dense_eigs"))
    args = [str(tmp_path / f) for f in ("a.txt", "a_eigs.txt", "lap.txt", "lap_eigs.txt", "c.txt", "c_eigs.txt")]
    for i, (key, case) in enumerate((("a", "a_lm"), ("lap", "lap_si"), ("c", "c_lm"))):
        _write_matrix(args[2 * i], K.matrix(key))
        _write_values(args[2 * i + 1], K.wanted(case))
    r = subprocess.run([exe] + args, capture_output=True, text=True, timeout=120)
    print(r.stdout)
    assert r.returncode == 0 and "ALL PASSED" in r.stdout, r.stdout[-3000:] + r.stderr[-2000:]
