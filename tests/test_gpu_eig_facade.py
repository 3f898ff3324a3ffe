"""GPU: EigSol::eig through the C++ façade (tests/cpp/test_eig.cpp) on gen97 and cgen70 of tests/eig_ref.py
under the conditions of tests/test_gpu_eig.py: the program checks the residual, the eigenvalues, the vectors'
conventions, a selection and the eigenvalues-only call; cond(V) is formed here from the vectors it writes."""
import os
import subprocess

import numpy as np
import pytest

from cpp_build import ROOT, build

import eig_ref as R
from test_gpu_eig import restatement, value_bound
from test_gpu_eigh_facade import _write_matrix

pytestmark = pytest.mark.gpu


def _write_expect(path, name):
    """"value_bound r_bound", then numpy.linalg.eigvals' eigenvalues "re im"."""
    A = R.matrix(name)
    with open(path, "w") as f:
        f.write(f"{value_bound(A)!r} {max(2.0, 3.0 * restatement()[name]['r'])!r}\n")
        for v in np.linalg.eigvals(A):
            f.write(f"{complex(v).real!r} {complex(v).imag!r}\n")


def _read_vectors(path):
    with open(path) as f:
        n = int(f.readline())
        a = np.loadtxt(f).reshape(n * n, 2)
    return (a[:, 0] + 1j * a[:, 1]).reshape((n, n), order="F")


def test_cpp_eig(tmp_path):
    exe = build(os.path.join(ROOT, "tests", "cpp", "test_eig.cpp"), str(tmp_path / "test_eig"))
    names = ("gen97", "cgen70")
    args = [str(tmp_path / f"{nm}{suffix}.txt") for nm in names for suffix in ("", "_expect", "_vectors")]
    for i, name in enumerate(names):
        _write_matrix(args[3 * i], R.matrix(name))
        _write_expect(args[3 * i + 1], name)
    r = subprocess.run([exe] + args, capture_output=True, text=True, timeout=120)
    print(r.stdout)
    assert r.returncode == 0 and "ALL PASSED" in r.stdout, r.stdout[-3000:] + r.stderr[-2000:]
    for i, name in enumerate(names):
        c = float(np.linalg.cond(_read_vectors(args[3 * i + 2])))
        c_ref = restatement()[name]["c"]
        print(f"{name}: c={c:.4g} (restatement {c_ref:.4g})")
        assert c <= 10.0 * c_ref
