"""GPU: EigSol::svds and EigSol::svds_dense through the C++ façade (tests/cpp/test_svds.cpp) on sp_tall (double,
sparse) and planted (complex, dense) of tests/svds_ref.py under the bounds of tests/test_gpu_svds.py: the program
checks shapes, order, the phase convention, the values-only call and the argument checks; the four figures are
formed here from the factors it writes."""
import os
import subprocess

import numpy as np
import pytest
import scipy.sparse as sp

from cpp_build import ROOT, build

import svds_ref as R

pytestmark = pytest.mark.gpu


def _write_sparse(path, A):
    A = sp.coo_matrix(A)
    with open(path, "w") as f:
        f.write(f"sparse\n{A.shape[0]} {A.shape[1]}\n{A.nnz}\n")
        for r, c, v in zip(A.row, A.col, A.data):
            f.write(f"{r} {c} {float(v)!r}\n")


def _write_dense(path, A):
    with open(path, "w") as f:
        f.write(f"{A.shape[0]} {A.shape[1]}\n")
        for z in np.asarray(A).ravel(order="F"):
            f.write(f"{complex(z).real!r} {complex(z).imag!r}\n")


def _write_vector(path, v):
    with open(path, "w") as f:
        for z in v:
            f.write(f"{complex(z).real!r} {complex(z).imag!r}\n")


def _read_result(path, cplx):
    with open(path) as f:
        M, N, k, restarts, apps, conv = (int(x) for x in f.readline().split())
        s = np.array([float(f.readline()) for _ in range(k)])
        res = np.array([float(f.readline()) for _ in range(k)])
        a = np.loadtxt(f).reshape((M + N) * k, 2)
    z = a[:, 0] + 1j * a[:, 1]
    U, V = z[:M * k].reshape((M, k), order="F"), z[M * k:].reshape((N, k), order="F")
    if not cplx:
        assert np.all(U.imag == 0) and np.all(V.imag == 0)
        U, V = U.real, V.real
    return s, res, U, V, restarts, apps, bool(conv)


def test_cpp_svds(tmp_path):
    exe = build(os.path.join(ROOT, "tests", "cpp", "test_svds.cpp"), str(tmp_path / "test_svds"))
    cases = (("sp_tall", np.float64), ("planted", np.complex128))
    args = [str(tmp_path / f"{nm}{suffix}.txt") for nm, _ in cases for suffix in ("", "_v0", "_out")]
    for i, (name, dt) in enumerate(cases):
        A = R.matrix(name, dt)
        (_write_sparse if name == "sp_tall" else _write_dense)(args[3 * i], A)
        _write_vector(args[3 * i + 1], R.start_vector(A.shape[1], dt))
    r = subprocess.run([exe] + args, capture_output=True, text=True, timeout=120)
    print(r.stdout)
    assert r.returncode == 0 and "ALL PASSED" in r.stdout, r.stdout[-3000:] + r.stderr[-2000:]
    golden = R.load_golden()
    for i, (name, dt) in enumerate(cases):
        ref = golden[R.key(name, dt)]
        s, res, U, V, restarts, apps, conv = _read_result(args[3 * i + 2], dt == np.complex128)
        fig = dict(zip(R.FIGS, R.figures(R.CASES[name][0], s, U, V, res, np.array(ref["s_ref"]))))
        print(name, f"restarts={restarts} applications={apps}",
              " ".join(f"{q}={fig[q]:.3g} (restatement {ref[q]:.3g})" for q in R.FIGS))
        assert conv and restarts <= ref["restarts"] + 2
        assert fig["r"] <= 2 and fig["e"] <= 2
        assert fig["o_u"] <= max(2.0, 3.0 * ref["o_u"]) and fig["o_v"] <= max(2.0, 3.0 * ref["o_v"])
