"""Krylov-Schur: time per operator application and per restart cycle, and applications x time
against block subspace iteration to the same residual.

Workloads (synthetic.py): the 1M x 1M matrices of DESIGN §11's table (16 nnz/row, uniform and band
columns; f64; largest modulus) and the 1M convection-diffusion matrix of the bench's config 5
(complex; shift-invert about 4 + 0.5i).  nev = 4, ncv = 20.

  per application / per cycle   the difference of two tolerance < 0 runs (which never converge) with
                                different max_restarts, over the difference in applications / cycles:
                                the set-up (upload, factorisation, Ritz vectors, residuals) cancels.
                                An application is one Arnoldi step: the operator plus its
                                orthogonalisation.
  to convergence                one run at tolerance 1e-10: wall time, restarts, applications, residuals.
  against subspace_iteration    (largest modulus) the same matrix in the same process, block 8, stopped
                                by residual_tolerance = the worst ||r|| / (1 + |theta|) the Krylov run
                                returned: products (iterations x block) and wall time.

Writes one JSON document (default profiles/krylov_bench.json) and prints it.

  python tools/bench_krylov.py [--workloads uniform1m,band1m,convdiff1m] [--out FILE]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import pcsc_eigenvalue_solver_project_amd as E  # noqa: E402
from pcsc_eigenvalue_solver_project_amd import synthetic as S  # noqa: E402

NEV, NCV = 4, 20


def step_bytes(n, nnz, ncv, p, sb, op_bytes):
    """Algorithmic bytes of the steps j = p .. ncv - 1 of one cycle: per step against j + 1 columns,
    two passes of (dots: j + 1 columns and w; update: j + 1 columns, w read and written), then the
    normalisation (w read and written): (4 (j + 1) + 8) n s, plus the operator."""
    orth = sum((4 * (j + 1) + 8) * n * sb for j in range(p, ncv))
    return {"orthogonalisation": orth, "operator": op_bytes * (ncv - p), "steps": ncv - p}


def timed(fn):
    t = time.perf_counter()
    r = fn()
    return time.perf_counter() - t, r


def per_step(A, v0, sigma, lo, hi):
    run = lambda c: E.krylov_schur(A, NEV, E.KrylovOptions(c, -1.0), sigma=sigma, ncv=NCV, v0=v0)  # noqa: E731
    timed(lambda: run(lo))                                   # warm-up: kernels loaded, layouts chosen
    tl, rl = min((timed(lambda: run(lo)) for _ in range(2)), key=lambda x: x[0])
    th, rh = min((timed(lambda: run(hi)) for _ in range(2)), key=lambda x: x[0])
    da, dc = rh.applications - rl.applications, rh.restarts - rl.restarts
    return {"application_ms": round(1e3 * (th - tl) / da, 4), "cycle_ms": round(1e3 * (th - tl) / dc, 3),
            "applications_timed": da, "cycles_timed": dc, "applications_per_restarted_cycle": da // dc}


def spmv_ms(ctx, A, n, dtype):
    s = E.PowerSession(A)
    s.begin(E.SolverOptions(2 ** 31 - 1, -1.0), S.start_vector(n, dtype))
    s.step(20)
    ctx.synchronize()
    t = time.perf_counter()
    s.step(200)
    ctx.synchronize()
    ms = 1e3 * (time.perf_counter() - t) / 200
    info = s.kernel_info()
    s.close()
    return ms, info


def largest_modulus(ctx, kind, n, k):
    rp, ci, v = S.uniform(n, k) if kind == "uniform" else S.band(n, k)
    A = E.CsrMatrix(ctx, rp, ci, v, (n, n))
    nnz = len(ci)
    del rp, ci, v
    v0 = S.start_vector(n)
    sms, info = spmv_ms(ctx, A, n, np.float64)
    w = {"n": n, "nnz": nnz, "dtype": "f64", "mode": "largest modulus", "nev": NEV, "ncv": NCV,
         "power_iteration_ms": round(sms, 4), "power_kernel": info["kernel"]}
    w.update(per_step(A, v0, None, 2, 6))
    w["bytes_per_restarted_cycle"] = step_bytes(n, nnz, NCV, NEV, 8, info["bytes_per_iteration"])
    t, r = timed(lambda: E.krylov_schur(A, NEV, E.KrylovOptions(300, 1e-10), ncv=NCV, v0=v0))
    rel = float(np.max(r.residuals / (1 + np.abs(r.eigenvalues))))
    w["to_convergence"] = {"seconds": round(t, 4), "converged": r.converged, "restarts": r.restarts,
                           "applications": r.applications, "residuals": [float(x) for x in r.residuals],
                           "eigenvalues": [[z.real, z.imag] for z in r.eigenvalues],
                           "worst_relative_residual": rel}
    X0 = np.asfortranarray(np.random.default_rng(7).uniform(-1, 1, (n, 8)))
    so = E.SubspaceOptions(3000, 1e-14, max(rel, 1e-13))
    ts, rs = timed(lambda: E.subspace_iteration(A, NEV, so, block=8, X0=X0))
    w["subspace_iteration_to_the_same_residual"] = {
        "seconds": round(ts, 4), "converged": rs.converged, "iterations": rs.iterations, "block": 8,
        "products": rs.iterations * 8, "residuals": [float(x) for x in rs.residuals],
        "max_iterations": 3000}
    w["krylov_over_subspace_seconds"] = round(t / ts, 4)
    A.close()
    return w


def convdiff(ctx, nx=1000):
    rp, ci, v = S.convdiff_complex(nx)
    n = nx * nx
    A = E.CsrMatrix(ctx, rp, ci, v, (n, n))
    nnz = len(ci)
    del rp, ci, v
    sigma = 4.0 + 0.5j
    v0 = S.start_vector(n, np.complex128)
    w = {"n": n, "nnz": nnz, "dtype": "c128", "mode": "shift-invert", "sigma": [sigma.real, sigma.imag],
         "nev": NEV, "ncv": NCV}
    w.update(per_step(A, v0, sigma, 1, 3))
    t, r = timed(lambda: E.krylov_schur(A, NEV, E.KrylovOptions(60, 1e-10), sigma=sigma, ncv=NCV, v0=v0))
    w["to_convergence"] = {"seconds_with_factorisation": round(t, 4), "converged": r.converged,
                           "restarts": r.restarts, "applications": r.applications,
                           "residuals": [float(x) for x in r.residuals],
                           "eigenvalues": [[z.real, z.imag] for z in r.eigenvalues]}
    A.close()
    return w


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workloads", default="uniform1m,band1m,convdiff1m")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "krylov_bench.json"))
    a = ap.parse_args()
    ctx = E.Context(0)
    out = {"metric": "Krylov-Schur: ms per application (operator + orthogonalisation), ms per restart cycle, "
                     "and to convergence against block subspace iteration", "workloads": {}}
    for name in a.workloads.split(","):
        if name == "convdiff1m":
            out["workloads"][name] = convdiff(ctx)
        else:
            out["workloads"][name] = largest_modulus(ctx, "uniform" if name == "uniform1m" else "band", 1_000_000, 16)
        print(name, json.dumps(out["workloads"][name]), flush=True)
    ctx.close()
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
