"""Dense block product and the dense k-eigenpair solvers: time per eigsol_dense_gemm against one
eigsol_dense_gemv, per dense block iteration against power-iteration steps, and per Krylov-Schur
application in both modes.

Workloads: uniform(-1, 1) matrices, 16384^2 f64 and 8192^2 c128 (the sizes of DESIGN §13).

  product     m in {1, 4, 8, 16, 32}: ms per eigsol_dense_gemm and per eigsol_dense_gemv, measured in
              the same process in alternating rounds (every round times REPS launches of each variant
              between two stream synchronisations; the figure is the median round, the fastest is
              listed too), and the bytes/s of the model that reads A once (8 n^2, 16 n^2 complex).
  subspace    (f64) ms per block iteration at block 16: the difference of two tolerance < 0 runs with
              different max_iterations over the difference in iterations, against 16 steps of a dense
              PowerSession.
  krylov      (f64) ms per application at ncv = 20, largest modulus and shift-invert: the difference
              of two tolerance < 0 runs with different max_restarts (set-up and factorisation
              cancel); the factorisation is timed alone through a ShiftedSession's creation.

Writes one JSON document (default profiles/dense_block_bench.json) and prints it.

  python tools/bench_dense_block.py [--n-real 16384] [--n-complex 8192] [--out FILE]
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

WIDTHS = (1, 4, 8, 16, 32)
REPS, ROUNDS = 200, 7
NEV, NCV = 4, 20


def matrix(n, dtype, seed):
    """Column-major uniform(-1, 1) entries (the transpose view of a C-ordered draw: no second copy)."""
    rng = np.random.default_rng(seed)
    A = rng.uniform(-1, 1, (n, n))
    if dtype == np.complex128:
        A = A + 1j * rng.uniform(-1, 1, (n, n))
    return A.T


def values(n, m, dtype, seed):
    rng = np.random.default_rng(seed)
    X = rng.uniform(-1, 1, (n, m))
    if dtype == np.complex128:
        X = X + 1j * rng.uniform(-1, 1, (n, m))
    return np.ascontiguousarray(X.astype(dtype))


def window(ctx, launch, reps):
    ctx.synchronize()
    t = time.perf_counter()
    for _ in range(reps):
        launch()
    ctx.synchronize()
    return 1e3 * (time.perf_counter() - t) / reps


def product(ctx, D, n, dtype):
    sb = np.dtype(dtype).itemsize
    dx, dy = ctx.malloc(n * 32 * sb), ctx.malloc(n * 32 * sb)
    ctx.h2d(dx, values(n, 32, dtype, 3))
    variants = {"gemv": lambda: D.gemv(dx, dy)}
    for m in WIDTHS:
        variants[f"gemm_m{m}"] = (lambda m=m: D.gemm(dx, dy, m))
    for fn in variants.values():              # warm-up: code objects loaded, workspaces allocated
        window(ctx, fn, 10)
    times = {k: [] for k in variants}
    for _ in range(ROUNDS):                   # alternating: every round times every variant once
        for k, fn in variants.items():
            times[k].append(window(ctx, fn, REPS))
    ctx.free(dx)
    ctx.free(dy)
    model = sb * n * n
    gv = statistics.median(times["gemv"])
    out = {"n": n, "dtype": np.dtype(dtype).name, "model_bytes": model, "launches_per_round": REPS, "rounds": ROUNDS,
           "gemv_ms": round(gv, 4), "gemv_ms_fastest": round(min(times["gemv"]), 4),
           "gemv_model_TBps": round(model / gv / 1e9, 3), "gemm": {}}
    for m in WIDTHS:
        t = statistics.median(times[f"gemm_m{m}"])
        out["gemm"][str(m)] = {"ms": round(t, 4), "ms_fastest": round(min(times[f"gemm_m{m}"]), 4),
                               "over_one_gemv": round(t / gv, 3), "over_m_gemvs": round(t / (m * gv), 4),
                               "model_TBps": round(model / t / 1e9, 3),
                               "TFLOPs": round((8 if sb == 16 else 2) * n * n * m / t / 1e9, 3)}
    return out


def timed(fn):
    t = time.perf_counter()
    r = fn()
    return time.perf_counter() - t, r


def subspace(ctx, D, n):
    X0 = np.asfortranarray(np.random.default_rng(7).uniform(-1, 1, (n, 16)))
    run = lambda c: E.subspace_iteration(D, NEV, E.SubspaceOptions(c, -1.0, 0.0), block=16, X0=X0)  # noqa: E731
    timed(lambda: run(3))
    tl, rl = min((timed(lambda: run(3)) for _ in range(3)), key=lambda x: x[0])
    th, rh = min((timed(lambda: run(23)) for _ in range(3)), key=lambda x: x[0])
    it_ms = 1e3 * (th - tl) / (rh.iterations - rl.iterations)
    s = E.PowerSession(D)
    s.begin(E.SolverOptions(2 ** 31 - 1, -1.0), np.random.default_rng(8).uniform(-1, 1, n))
    s.step(20)
    ctx.synchronize()
    t = time.perf_counter()
    s.step(320)
    ctx.synchronize()
    p_ms = 1e3 * (time.perf_counter() - t) / 320
    s.close()
    return {"n": n, "dtype": "float64", "block": 16, "nev": NEV, "block_iteration_ms": round(it_ms, 4),
            "iterations_timed": rh.iterations - rl.iterations, "power_iteration_ms": round(p_ms, 4),
            "sixteen_power_iterations_ms": round(16 * p_ms, 4),
            "block_iteration_over_16_power_iterations": round(it_ms / (16 * p_ms), 4)}


def krylov(ctx, D, n, sigma):
    v0 = np.random.default_rng(9).uniform(-1, 1, n)
    out = {"n": n, "dtype": "float64", "nev": NEV, "ncv": NCV}
    for mode, sg in (("largest_modulus", None), ("shift_invert", sigma)):
        run = lambda c: E.krylov_schur(D, NEV, E.KrylovOptions(c, -1.0), sigma=sg, ncv=NCV, v0=v0)  # noqa: E731
        timed(lambda: run(2))
        tl, rl = min((timed(lambda: run(2)) for _ in range(2)), key=lambda x: x[0])
        th, rh = min((timed(lambda: run(12)) for _ in range(2)), key=lambda x: x[0])
        da = rh.applications - rl.applications
        out[mode] = {"application_ms": round(1e3 * (th - tl) / da, 4), "applications_timed": da,
                     "run_of_2_cycles_s": round(tl, 4)}
    def factor():
        s = E.ShiftedSession(D, sigma)
        ctx.synchronize()
        s.close()
    timed(factor)
    out["shift_invert"]["sigma"] = sigma
    out["shift_invert"]["factorisation_s"] = round(min(timed(factor)[0] for _ in range(2)), 4)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n-real", type=int, default=16384)
    ap.add_argument("--n-complex", type=int, default=8192)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "dense_block_bench.json"))
    a = ap.parse_args()
    ctx = E.Context(0)
    out = {"metric": "dense block product (ms per eigsol_dense_gemm against eigsol_dense_gemv), dense block "
                     "subspace iteration and dense Krylov-Schur (ms per iteration / application)"}
    D = E.DenseMatrix(ctx, matrix(a.n_real, np.float64, 1))
    out["product_f64"] = product(ctx, D, a.n_real, np.float64)
    print(json.dumps(out["product_f64"]), flush=True)
    out["subspace_f64"] = subspace(ctx, D, a.n_real)
    print(json.dumps(out["subspace_f64"]), flush=True)
    out["krylov_f64"] = krylov(ctx, D, a.n_real, 0.5)
    print(json.dumps(out["krylov_f64"]), flush=True)
    D.close()
    D = E.DenseMatrix(ctx, matrix(a.n_complex, np.complex128, 2))
    out["product_c128"] = product(ctx, D, a.n_complex, np.complex128)
    print(json.dumps(out["product_c128"]), flush=True)
    D.close()
    ctx.close()
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
