"""GPU: EigSol::svd and EigSol::svdvals through the C++ façade (tests/cpp/test_svd.cpp) on rand97 and crand65 of
tests/svd_ref.py under the bounds of tests/test_gpu_svd.py: the program checks shapes, order, conventions, the
values-only call and the argument checks; the four figures are formed here from the factors it writes."""
import os
import subprocess

import numpy as np
import pytest

from cpp_build import ROOT, build

import svd_ref as R
from test_gpu_svd import FIGS, restatement
from test_gpu_eigh_facade import _write_matrix

pytestmark = pytest.mark.gpu


def _read_result(path, cplx):
    with open(path) as f:
        n, sweeps = (int(x) for x in f.readline().split())
        s = np.array([float(f.readline()) for _ in range(n)])
        a = np.loadtxt(f).reshape(2 * n * n, 2)
    z = a[:, 0] + 1j * a[:, 1]
    U, V = z[:n * n].reshape((n, n), order="F"), z[n * n:].reshape((n, n), order="F")
    if not cplx:
        assert np.all(U.imag == 0) and np.all(V.imag == 0)
        U, V = U.real, V.real
    return U, s, V, sweeps


def test_cpp_svd(tmp_path):
    exe = build(os.path.join(ROOT, "tests", "cpp", "test_svd.cpp"), str(tmp_path / "test_svd"))
    names = ("rand97", "crand65")
    args = [str(tmp_path / f"{nm}{suffix}.txt") for nm in names for suffix in ("", "_out")]
    for i, name in enumerate(names):
        _write_matrix(args[2 * i], R.matrix(name))
    r = subprocess.run([exe] + args, capture_output=True, text=True, timeout=120)
    print(r.stdout)
    assert r.returncode == 0 and "ALL PASSED" in r.stdout, r.stdout[-3000:] + r.stderr[-2000:]
    for i, name in enumerate(names):
        A = R.matrix(name)
        ref = restatement()[name]
        U, s, V, sweeps = _read_result(args[2 * i + 1], np.iscomplexobj(A))
        fig = dict(zip(FIGS, R.figures(A, U, s, V, R.lapack_s(A))))
        print(name, f"sweeps={sweeps}", " ".join(f"{q}={fig[q]:.3g} (restatement {ref[q]:.3g})" for q in FIGS))
        assert sweeps <= ref["sweeps"] + 2
        for q in FIGS:
            assert fig[q] <= max(2.0, 3.0 * ref[q]), q
