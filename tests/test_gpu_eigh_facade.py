"""GPU: EigSol::eigh and EigSol::eigvalsh through the C++ façade (tests/cpp/test_eigh.cpp) on sym97 and
herm70 of tests/eigh_ref.py: all pairs, an index and a value selection, and the façade's error messages."""
import os
import subprocess

import numpy as np
import pytest

from cpp_build import ROOT, build

import eigh_ref as R

pytestmark = pytest.mark.gpu


def _write_matrix(path, A):
    """"n", then n * n lines "re im", column-major."""
    with open(path, "w") as f:
        f.write(f"{A.shape[0]}\n")
        for v in np.asarray(A).ravel(order="F"):
            f.write(f"{complex(v).real!r} {complex(v).imag!r}\n")


def _write_expect(path, name):
    """"value_bound r_bound o_bound" (the accuracy conditions of tests/test_gpu_eigh.py), then LAPACK's eigenvalues."""
    A = R.matrix(name)
    w_ref, Z_ref, w_lapack = R.reference(name)
    with open(path, "w") as f:
        bounds = (R.value_bound(A), max(2.0, 3 * R.r_figure(A, w_ref, Z_ref)), max(2.0, 3 * R.o_figure(Z_ref)))
        f.write(" ".join(repr(float(b)) for b in bounds) + "\n")
        for v in w_lapack:
            f.write(f"{float(v)!r}\n")


def test_cpp_eigh(tmp_path):
    exe = build(os.path.join(ROOT, "tests", "cpp", "test_eigh.cpp"), str(tmp_path / "test_eigh"))
    args = [str(tmp_path / f) for f in ("sym97.txt", "sym97_expect.txt", "herm70.txt", "herm70_expect.txt")]
    for i, name in enumerate(("sym97", "herm70")):
        _write_matrix(args[2 * i], R.matrix(name))
        _write_expect(args[2 * i + 1], name)
    r = subprocess.run([exe] + args, capture_output=True, text=True, timeout=120)
    print(r.stdout)
    assert r.returncode == 0 and "ALL PASSED" in r.stdout, r.stdout[-3000:] + r.stderr[-2000:]
