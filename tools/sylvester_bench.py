"""solve_sylvester against the two schur calls it contains, and scipy.linalg.solve_sylvester on the host beside
them: seconds per call, host buffers in and out.

Workloads (seeded standard normal entries): A and B of order 4096 in f64, A and B of order 2048 in c128, and a
rectangular pair in f64, A of order 4096 with B of order 512.  Per workload:

  solve_sylvester   A X + X B = C, everything between the uploads and the download on the device
  two_schur         schur(A) then schur(B), each with its own upload and download (what the solver's first two
                    stages do without the copies of T and Z back to the host)
  scipy             scipy.linalg.solve_sylvester (LAPACK xGEES twice, xTRSYL, four GEMMs) on HOST_THREADS threads

The two device measurements are timed ALTERNATELY in one process after one warm-up of each, REPS times with a
host clock around the whole call, which ends synchronised (results on the host).  The figure is the median; the
fastest and the slowest are listed.  The five stage times of the last solve_sylvester call are listed
(eigsol_sylvester_stage_times), their non-Schur part against one schur(A) call, and the residual figure
r = ||A X + X B - C||_F / (max(m, n) eps ((||A||_F + ||B||_F) ||X||_F + ||C||_F)).  scipy runs once, afterwards.
LAPACK's xTRSYL is unblocked: at order 4096 the scipy call takes tens of minutes, nearly all of it in xTRSYL, so
--scipy-only runs that leg alone, without a device, on the same seeded matrices and merges it into the document
(the host it ran on is recorded with it); --scipy-reps 0 leaves it out of a device run.

Writes one JSON document after every workload (default profiles/sylvester_bench.json; an existing document keeps
the workloads this run does not time) and prints it at the end.

  python tools/sylvester_bench.py [--reps 5] [--scipy-reps 1] [--scipy-only] [--only f64|c128|rect] [--out FILE]
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

EPS = np.finfo(float).eps


def summary(ts):
    return {"s": round(statistics.median(ts), 5), "s_fastest": round(min(ts), 5), "s_slowest": round(max(ts), 5),
            "calls": len(ts)}


def figure(A, B, C, X):
    m, n = C.shape
    den = (np.linalg.norm(A) + np.linalg.norm(B)) * np.linalg.norm(X) + np.linalg.norm(C)
    return float(np.linalg.norm(A @ X + X @ B - C) / (max(m, n) * EPS * den))


def scipy_leg(A, B, C, scipy_reps):
    st = []
    for _ in range(scipy_reps):
        t = time.perf_counter()
        Xs = sla.solve_sylvester(A, B, C)
        st.append(time.perf_counter() - t)
    return {**summary(st), "host_threads": HOST_THREADS, "host_cpus": os.cpu_count(), "r": figure(A, B, C, Xs)}


def workload(ctx, A, B, C, reps, scipy_reps):
    ts = {"solve_sylvester": [], "two_schur": [], "schur_a": []}
    E.solve_sylvester(ctx, A, B, C)             # warm-up
    E.schur(ctx, A)
    E.schur(ctx, B)
    res = stages = None
    for _ in range(reps):
        t = time.perf_counter()
        res = E.solve_sylvester(ctx, A, B, C)
        ts["solve_sylvester"].append(time.perf_counter() - t)
        stages = E.sylvester_stage_times(ctx)
        t = time.perf_counter()
        E.schur(ctx, A)
        t1 = time.perf_counter()
        E.schur(ctx, B)
        ts["two_schur"].append(time.perf_counter() - t)
        ts["schur_a"].append(t1 - t)
        print("  call", ts["solve_sylvester"][-1], ts["two_schur"][-1], flush=True)
    out = {k: summary(v) for k, v in ts.items()}
    rest = stages["transform_in"] + stages["triangular"] + stages["transform_out"]
    out["solve_sylvester"].update(stages_s={k: round(v, 5) for k, v in stages.items()}, r=figure(A, B, C, res.X),
                                  perturbed=res.perturbed, converged=res.converged)
    out["non_schur_stages_s"] = round(rest, 5)
    out["non_schur_stages_over_schur_a"] = round(rest / out["schur_a"]["s"], 4)
    out["solve_sylvester_over_two_schur"] = round(out["solve_sylvester"]["s"] / out["two_schur"]["s"], 3)
    if scipy_reps > 0:
        out["scipy"] = scipy_leg(A, B, C, scipy_reps)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--scipy-reps", type=int, default=1)
    ap.add_argument("--scipy-only", action="store_true")
    ap.add_argument("--only", choices=("f64", "c128", "rect"))
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sylvester_bench.json"))
    a = ap.parse_args()
    doc = {}
    if os.path.exists(a.out):
        with open(a.out) as f:
            doc = json.load(f)
    doc["metric"] = ("seconds per call, host buffers in and out (median of the timed calls after one warm-up call; "
                     "solve_sylvester and the two schur calls timed alternately in one process; scipy on the host "
                     "afterwards)")
    ctx = None if a.scipy_only else E.Context(0)

    for idx, (key, m, n, cplx) in enumerate((("f64", 4096, 4096, False), ("c128", 2048, 2048, True), ("rect", 4096, 512, False))):
        if a.only and a.only != key:
            continue
        rng = np.random.default_rng(20261020 + idx)   # per workload, so that --only and --scipy-only see the same matrices

        def gen(r, c):
            M = rng.standard_normal((r, c))
            return np.asfortranarray(M + 1j * rng.standard_normal((r, c)) if cplx else M)

        A, B, C = gen(m, m), gen(n, n), gen(m, n)
        print(key, "start", flush=True)
        if a.scipy_only:
            doc.setdefault(key, {"m": m, "n": n, "dtype": "complex128" if cplx else "float64"})
            doc[key]["scipy"] = scipy_leg(A, B, C, max(a.scipy_reps, 1))
        else:
            kept = doc.get(key, {}).get("scipy") if a.scipy_reps == 0 else None
            doc[key] = {"m": m, "n": n, "dtype": "complex128" if cplx else "float64",
                        **workload(ctx, A, B, C, a.reps, a.scipy_reps)}
            if kept:
                doc[key]["scipy"] = kept
        if "scipy" in doc[key] and "solve_sylvester" in doc[key]:
            doc[key]["scipy_over_solve_sylvester"] = round(doc[key]["scipy"]["s"] / doc[key]["solve_sylvester"]["s"], 3)
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(doc, f, indent=1)
            f.write("\n")
        print(key, "done", flush=True)
    if ctx is not None:
        ctx.close()
    print(json.dumps(doc, indent=1))


if __name__ == "__main__":
    main()
