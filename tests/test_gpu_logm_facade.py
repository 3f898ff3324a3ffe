"""GPU: EigSol::logm through the C++ façade (tests/cpp/test_logm.cpp) on r65, c65 and ur65 of tests/sqrtm_ref.py (a
real logarithm, a complex matrix, a real matrix whose logarithm is complex) and on r65 rounded to float (promoted to
fp64 by the façade).  The program checks shapes, flags, bitwise repeatability and the reruns itself and writes its
logarithms to files; the figure e of tests/logm_ref.py is formed here, under the bound of tests/test_gpu_logm.py."""
import os
import subprocess

import numpy as np
import pytest

from cpp_build import ROOT, build

import logm_ref as G

pytestmark = pytest.mark.gpu

CASES = ("r65", "c65", "ur65")
OUT = ("real.txt", "complex.txt", "real_complex_log.txt")


def _write_case(path, name):
    """"n", then A as lines "re im", column-major."""
    A = G.case(name)
    with open(path, "w") as f:
        f.write(f"{A.shape[0]}\n")
        for v in np.asarray(A).ravel(order="F"):
            f.write(f"{complex(v).real!r} {complex(v).imag!r}\n")


def _read_result(path):
    with open(path) as f:
        n = int(f.readline())
        v = np.array([[float(t) for t in ln.split()] for ln in f])
    return (v[:, 0] + 1j * v[:, 1]).reshape((n, n), order="F")


def test_cpp_logm(tmp_path):
    exe = build(os.path.join(ROOT, "tests", "cpp", "test_logm.cpp"), str(tmp_path / "test_logm"))
    args = [str(tmp_path / f"{nm}.txt") for nm in CASES] + [str(tmp_path / "out_")]
    for path, name in zip(args, CASES):
        _write_case(path, name)
    r = subprocess.run([exe] + args, capture_output=True, text=True, timeout=120)
    print(r.stdout)
    assert r.returncode == 0 and "ALL PASSED" in r.stdout, r.stdout[-3000:] + r.stderr[-2000:]
    rec = G.golden()["named"]
    for name, tag in zip(CASES, OUT):
        X = _read_result(str(tmp_path / ("out_" + tag)))
        if name in G.REAL_LOG:
            assert not np.any(X.imag)
            X = X.real
        e = G.figure_e(G.case(name), X)
        print(f"{name}: e={e:.3g} (SciPy {rec[name]:.3g})")
        assert e <= G.bound(rec[name])
