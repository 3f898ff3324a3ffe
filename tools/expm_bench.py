"""expm at 4096^2 float64 and 2048^2 complex128 with its stage times, the LDS-tiled GEMM alone against the product
path of sqrtm and solve_sylvester, and scipy.linalg.expm on the host beside them.

Per workload (a Gaussian matrix scaled to 1-norm 40: degree 13, three squarings) the legs alternate in one process
after one warm-up call each:
  expm     X = exp(A), host buffers in and out; the six stage times of every call (eigsol_expm_stage_times)
  sqrtm    the call whose "transform" stage is two syl_product calls of n^3 multiply-adds each with the copy of
           the result to the host: half of it is the earlier product path's cost per product
The new kernel's cost per product is a third of expm's "squarings" stage (three gemm_device calls and nothing
else); the Pade stage holds six more with the linear combinations between them and is listed for comparison.
Medians of the timed calls, with the fastest and the slowest; per pair of alternating calls the difference
(earlier path - new kernel) per product, whose smallest value must be positive for the new kernel to count as
faster.  "factor_share" is the LU factorisation's part of the call: its panel issues two launches per column.
scipy.linalg.expm runs once on 16 host threads.

Writes one JSON document after every workload (default profiles/expm_bench.json).

  python tools/expm_bench.py [--reps 5] [--scipy-reps 1] [--only f64|c128] [--out FILE]
"""
import argparse
import json
import os
import statistics
import sys
import time

HOST_THREADS = 16
for _v in ("OMP_NUM_THREADS", "OPENBLAS_NUM_THREADS", "MKL_NUM_THREADS"):
    os.environ[_v] = str(HOST_THREADS)

import numpy as np  # noqa: E402
import scipy.linalg as sla  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import pcsc_eigenvalue_solver_project_amd as E  # noqa: E402

STAGES = ("norm", "pade", "factor", "substitution", "squarings", "total")


def summary(ts, digits=6):
    return {"s": round(statistics.median(ts), digits), "s_fastest": round(min(ts), digits), "s_slowest": round(max(ts), digits),
            "calls": len(ts)}


def workload(ctx, A, As, reps, scipy_reps):
    n, cplx = A.shape[0], np.iscomplexobj(A)
    flops = (8.0 if cplx else 2.0) * n ** 3          # one product, real operations
    res = E.expm(ctx, A)                              # warm-up
    E.sqrtm(ctx, As)
    wall, stages, parent, diffs = [], {k: [] for k in STAGES}, [], []
    for _ in range(reps):
        t = time.perf_counter()
        res = E.expm(ctx, A)
        wall.append(time.perf_counter() - t)
        st = E.expm_stage_times(ctx)
        for k in STAGES:
            stages[k].append(st[k])
        E.sqrtm(ctx, As)
        parent.append(E.sqrtm_stage_times(ctx)["transform"] / 2.0)
        diffs.append(parent[-1] - st["squarings"] / res.squarings)
        print("  call", wall[-1], st["squarings"] / res.squarings, parent[-1], flush=True)
    new = [v / res.squarings for v in stages["squarings"]]
    out = {"degree": res.degree, "squarings": res.squarings, "expm": summary(wall, 5),
           "stages_s": {k: summary(v) for k, v in stages.items()},
           "factor_share": round(statistics.median(stages["factor"]) / statistics.median(stages["total"]), 4),
           "factor_launches_about": 2 * n,
           "gemm_new": {**summary(new), "tflops": round(flops / statistics.median(new) * 1e-12, 2)},
           "gemm_in_pade_stage_upper": {"s": round(statistics.median(stages["pade"]) / 6.0, 6),
                                        "note": "the Pade stage over its six products; the linear combinations are in it"},
           "product_earlier_path": {**summary(parent), "tflops": round(flops / statistics.median(parent) * 1e-12, 2),
                                    "note": "half of sqrtm's transform stage, which also holds the copy of X to the host"},
           "earlier_minus_new_s": {"median": round(statistics.median(diffs), 6), "smallest": round(min(diffs), 6),
                                   "largest": round(max(diffs), 6)},
           "new_is_faster_beyond_spread": bool(min(diffs) > 0.0 and max(new) < min(parent))}
    if scipy_reps > 0:
        st = []
        for _ in range(scipy_reps):
            t = time.perf_counter()
            Xs = sla.expm(A)
            st.append(time.perf_counter() - t)
        out["scipy"] = {**summary(st, 4), "host_threads": HOST_THREADS, "host_cpus": os.cpu_count(),
                        "gap_to_expm": float(np.linalg.norm(res.X - Xs) / np.linalg.norm(Xs))}
        out["scipy_over_expm"] = round(out["scipy"]["s"] / out["expm"]["s"], 2)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--scipy-reps", type=int, default=1)
    ap.add_argument("--only", choices=("f64", "c128"))
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "expm_bench.json"))
    a = ap.parse_args()
    doc = {}
    if os.path.exists(a.out):
        with open(a.out) as f:
            doc = json.load(f)
    doc["metric"] = ("seconds (median of the timed calls after one warm-up call; expm and sqrtm alternate in one process; "
                     "stage times by stream events; scipy on the host afterwards, once)")
    ctx = E.Context(0)
    for idx, (key, n, cplx) in enumerate((("f64", 4096, False), ("c128", 2048, True))):
        if a.only and a.only != key:
            continue
        rng = np.random.default_rng(20261021 + idx)
        G = rng.standard_normal((n, n))
        # sqrtm's matrix as in tools/sqrtm_bench.py (a real one shifted to a real root); expm's scaled to 1-norm 40
        As = G + 1j * rng.standard_normal((n, n)) if cplx else G + (2.0 * np.sqrt(n) + 1.0) * np.eye(n)
        A = As if cplx else G
        A = np.asfortranarray(A * (40.0 / np.abs(A).sum(axis=0).max()))
        print(key, "start", flush=True)
        doc[key] = {"n": n, "dtype": "complex128" if cplx else "float64", "norm1": 40.0,
                    **workload(ctx, A, np.asfortranarray(As), a.reps, a.scipy_reps)}
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(doc, f, indent=1)
            f.write("\n")
        print(key, "done", flush=True)
    ctx.close()
    print(json.dumps(doc, indent=1))


if __name__ == "__main__":
    main()
