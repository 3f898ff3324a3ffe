"""GPU: EigSol::eigh with EighOptions::Method::DC through the C++ façade (tests/cpp/test_eigh_dc.cpp) on sym97
and herm70 of tests/eigh_ref.py: residual, orthogonality and eigenvalues against LAPACK's divide and conquer."""
import os
import subprocess

import pytest

from cpp_build import ROOT, build

import eigh_dc_ref as DC
import eigh_ref as R
from test_gpu_eigh_facade import _write_matrix

pytestmark = pytest.mark.gpu


def _write_expect(path, name):
    """"value_bound r_bound o_bound" (the conditions of tests/test_gpu_eigh_dc.py), then LAPACK's eigenvalues."""
    A = R.matrix(name)
    _, _, r_evd, o_evd = DC.evd(name)
    with open(path, "w") as f:
        f.write(" ".join(repr(float(b)) for b in (R.value_bound(A), max(2.0, 3 * r_evd), max(2.0, 3 * o_evd))) + "\n")
        for v in R.reference(name)[2]:
            f.write(f"{float(v)!r}\n")


def test_cpp_eigh_dc(tmp_path):
    exe = build(os.path.join(ROOT, "tests", "cpp", "test_eigh_dc.cpp"), str(tmp_path / "test_eigh_dc"))
    args = [str(tmp_path / f) for f in ("sym97.txt", "sym97_expect.txt", "herm70.txt", "herm70_expect.txt")]
    for i, name in enumerate(("sym97", "herm70")):
        _write_matrix(args[2 * i], R.matrix(name))
        _write_expect(args[2 * i + 1], name)
    r = subprocess.run([exe] + args, capture_output=True, text=True, timeout=120)
    print(r.stdout)
    assert r.returncode == 0 and "ALL PASSED" in r.stdout, r.stdout[-3000:] + r.stderr[-2000:]
