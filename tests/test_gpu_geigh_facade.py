"""GPU: EigSol::eigh(A, B), EigSol::eigvalsh(A, B) and EigSol::cholesky(B) through the C++ façade
(tests/cpp/test_geigh.cpp) on gsym97 and gherm70 of tests/geigh_ref.py, and the façade's error messages."""
import os
import subprocess

import numpy as np
import pytest

from cpp_build import ROOT, build

import geigh_ref as G

pytestmark = pytest.mark.gpu


def _write_matrix(path, A):
    """"n", then n * n lines "re im", column-major."""
    with open(path, "w") as f:
        f.write(f"{A.shape[0]}\n")
        for v in np.asarray(A).ravel(order="F"):
            f.write(f"{complex(v).real!r} {complex(v).imag!r}\n")


def _write_expect(path, name):
    """"value_bound r_bound o_bound c_bound cond_B" (the conditions of tests/test_gpu_geigh.py and
    tests/test_gpu_cholesky.py), then the reference eigenvalues."""
    A, B = G.pair(name)
    w_ref, X_ref, w_np = G.reference(name)
    bounds = (G.value_bound(A, B, w_np), max(2.0, 3 * G.r_figure(A, B, w_ref, X_ref)),
              max(2.0, 3 * G.o_figure(B, X_ref)), max(2.0, 3 * G.c_figure(B, np.linalg.cholesky(B))),
              float(np.linalg.cond(B, 2)))
    with open(path, "w") as f:
        f.write(" ".join(repr(float(b)) for b in bounds) + "\n")
        for v in w_np:
            f.write(f"{float(v)!r}\n")


def test_cpp_geigh(tmp_path):
    exe = build(os.path.join(ROOT, "tests", "cpp", "test_geigh.cpp"), str(tmp_path / "test_geigh"))
    args = []
    for name in ("gsym97", "gherm70"):
        A, B = G.pair(name)
        paths = [str(tmp_path / f"{name}_{s}.txt") for s in ("A", "B", "expect")]
        _write_matrix(paths[0], A)
        _write_matrix(paths[1], B)
        _write_expect(paths[2], name)
        args += paths
    r = subprocess.run([exe] + args, capture_output=True, text=True, timeout=120)
    print(r.stdout)
    assert r.returncode == 0 and "ALL PASSED" in r.stdout, r.stdout[-3000:] + r.stderr[-2000:]
