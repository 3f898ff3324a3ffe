"""GPU: EigSol::subspaceIteration through the C++ façade (tests/cpp/test_subspace.cpp)."""
import os
import subprocess

import pytest

from cpp_build import ROOT, build

pytestmark = pytest.mark.gpu


def test_cpp_subspace_iteration(tmp_path):
    exe = build(os.path.join(ROOT, "tests", "cpp", "test_subspace.cpp"), str(tmp_path / "test_subspace"))
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    print(r.stdout)
    assert r.returncode == 0 and "ALL PASSED" in r.stdout, r.stdout[-3000:] + r.stderr[-2000:]
