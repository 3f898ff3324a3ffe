"""Dense symmetric / Hermitian eigensolver (eigvalsh, eigh): seconds per call, host buffers in and out.

Workloads: a random symmetric f64 matrix of order 4096 and a random Hermitian c128 matrix of order 2048
(seeded).  Per workload:

  eigvalsh         all eigenvalues (reduction + bisection)
  eigh             all eigenpairs, with the call's stages by stream events (eigsol_eigh_stage_times):
                   reduction, bisection, inverse iteration, back-transformation
  eigh_32          32 selected pairs from the middle of the spectrum
  qr_eigenvalues   the Francis path on the same matrix: the only way to these eigenvalues without eigvalsh
  numpy_eigh       numpy.linalg.eigh / eigvalsh on the host cores this process may use

Every entry is warmed once (code objects loaded), then timed REPS times with a host clock around the
whole call, which ends synchronised (results are on the host); the figure is the median, the fastest and
the slowest are listed too.  The eigenvalues of the paths are compared.

Writes one JSON document (default profiles/eigh_bench.json) and prints it.

  python tools/eigh_bench.py [--n-real 4096] [--n-complex 2048] [--reps 5] [--out FILE]
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import pcsc_eigenvalue_solver_project_amd as E  # noqa: E402


def matrix(n, dtype, seed):
    g = np.random.default_rng(seed)
    B = g.standard_normal((n, n))
    if dtype == np.complex128:
        B = B + 1j * g.standard_normal((n, n))
    return np.asfortranarray((B + B.conj().T) / 2)


def timed(fn, reps):
    fn()                                        # warm-up
    ts, r = [], None
    for _ in range(reps):
        t = time.perf_counter()
        r = fn()
        ts.append(time.perf_counter() - t)
    return {"s": round(statistics.median(ts), 5), "s_fastest": round(min(ts), 5), "s_slowest": round(max(ts), 5),
            "calls": reps}, r


def workload(ctx, n, dtype, seed, reps):
    A = matrix(n, dtype, seed)
    fro = float(np.linalg.norm(A))
    out = {"n": n, "dtype": np.dtype(dtype).name}
    out["eigvalsh"], w = timed(lambda: E.eigvalsh(ctx, A), reps)
    out["eigh"], res = timed(lambda: E.eigh(ctx, A), reps)
    out["eigh"]["stages_s"] = {k: round(v, 5) for k, v in E.eigh_stage_times(ctx).items()}
    out["eigh"]["not_converged"] = res.not_converged
    lo = n // 2 - 16
    out["eigh_32"], part = timed(lambda: E.eigh(ctx, A, select=("i", lo, lo + 31)), reps)
    out["eigh_32"]["stages_s"] = {k: round(v, 5) for k, v in E.eigh_stage_times(ctx).items()}
    out["qr_eigenvalues"], q = timed(lambda: E.qr_eigenvalues(ctx, A), max(2, reps // 2))
    out["qr_eigenvalues"]["converged"] = bool(q.converged)
    out["numpy_eigvalsh"], wn = timed(lambda: np.linalg.eigvalsh(A), max(2, reps // 2))
    out["numpy_eigh"], _ = timed(lambda: np.linalg.eigh(A), max(2, reps // 2))
    out["host_threads"] = int(os.environ.get("OMP_NUM_THREADS", "0")) or len(os.sched_getaffinity(0))
    Z = res.eigenvectors
    eps = np.finfo(float).eps
    out["checks"] = {
        "eigvalsh_vs_numpy_over_n_eps_fro": float(np.abs(w - wn).max() / (n * eps * fro)),
        "eigh_values_bitwise_eigvalsh": bool(res.eigenvalues.tobytes() == w.tobytes()),
        "eigh_32_values_bitwise_full": bool(part.eigenvalues.tobytes() == w[lo:lo + 32].tobytes()),
        "francis_vs_numpy_over_n_eps_fro": float(np.abs(np.sort(q.eigenvalues_complex.real) - wn).max() / (n * eps * fro)),
        "r": float(np.linalg.norm(A @ Z - Z * res.eigenvalues) / (n * eps * fro)),
        "o": float(np.linalg.norm(Z.conj().T @ Z - np.eye(n)) / (n * eps)),
    }
    out["eigvalsh_over_qr_eigenvalues"] = round(out["eigvalsh"]["s"] / out["qr_eigenvalues"]["s"], 4)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n-real", type=int, default=4096)
    ap.add_argument("--n-complex", type=int, default=2048)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "eigh_bench.json"))
    a = ap.parse_args()
    ctx = E.Context(0)
    out = {"metric": "seconds per call, host buffers in and out (median of the timed calls after one warm-up call)"}
    out["f64"] = workload(ctx, a.n_real, np.float64, 1, a.reps)
    print(json.dumps(out["f64"]), flush=True)
    out["c128"] = workload(ctx, a.n_complex, np.complex128, 2, a.reps)
    print(json.dumps(out["c128"]), flush=True)
    ctx.close()
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
