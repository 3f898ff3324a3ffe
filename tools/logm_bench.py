"""logm against the schur call it contains, and scipy.linalg.logm on the host beside them: seconds per call,
host buffers in and out.

Workloads (seeded standard normal entries): order 4096 in f64 with (2 sqrt(n) + 1) I added, which is above the
spectral radius of such a matrix (about sqrt(n)), so that the logarithm is real; order 2048 in c128, unshifted.  Per
workload:

  logm     X = log A, everything between the upload and the download on the device
  schur    schur(A) with its own upload and download (the solver's first stage plus the copies of T and Z)
  scipy    scipy.linalg.logm on HOST_THREADS threads, once

The two device measurements are timed ALTERNATELY in one process after one warm-up of each, REPS times with a
host clock around the whole call, which ends synchronised (results on the host).  The figure is the median; the
fastest and the slowest are listed.  The stage times of the last logm call are listed (eigsol_logm_stage_times:
Schur, roots, Pade, transform, total), their non-Schur part against one schur(A) call, the roots and the degree, the
seconds per root, the Pade stage's rate over its m n^3 / 3 flops (complex: four real flops per multiply and two per
add, 4 m n^3 / 3) and e = ||exp(X) - A||_F / (n eps ||A||_F) with the device's own expm.
--scipy-only runs the host leg alone, without a device, on the same seeded matrices and merges it into the
document; --scipy-reps 0 leaves it out of a device run.

Writes one JSON document after every workload (default profiles/logm_bench.json; an existing document keeps the
workloads this run does not time) and prints it at the end.

  python tools/logm_bench.py [--reps 5] [--scipy-reps 1] [--scipy-only] [--only f64|c128] [--out FILE]
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

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import pcsc_eigenvalue_solver_project_amd as E  # noqa: E402

EPS = np.finfo(float).eps


def summary(ts):
    return {"s": round(statistics.median(ts), 5), "s_fastest": round(min(ts), 5), "s_slowest": round(max(ts), 5),
            "calls": len(ts)}


def scipy_leg(A, scipy_reps):
    try:
        import scipy.linalg as sla
    except ImportError:
        return None
    st = []
    for _ in range(scipy_reps):
        t = time.perf_counter()
        Xs = sla.logm(A)
        st.append(time.perf_counter() - t)
    return {**summary(st), "host_threads": HOST_THREADS, "host_cpus": os.cpu_count(), "dtype": str(np.asarray(Xs).dtype)}


def workload(ctx, A, reps, scipy_reps):
    n, cplx = A.shape[0], np.iscomplexobj(A)
    ts = {"logm": [], "schur": []}
    E.logm(ctx, A)             # warm-up
    E.schur(ctx, A)
    res = stages = None
    for _ in range(reps):
        t = time.perf_counter()
        res = E.logm(ctx, A)
        ts["logm"].append(time.perf_counter() - t)
        stages = E.logm_stage_times(ctx)
        t = time.perf_counter()
        E.schur(ctx, A)
        ts["schur"].append(time.perf_counter() - t)
        print("  call", ts["logm"][-1], ts["schur"][-1], flush=True)
    out = {k: summary(v) for k, v in ts.items()}
    rest = stages["roots"] + stages["pade"] + stages["transform"]
    back = E.expm(ctx, res.X).X
    e = float(np.linalg.norm(back - A) / (n * EPS * np.linalg.norm(A)))
    flops = (4.0 if cplx else 1.0) * res.degree * float(n) ** 3 / 3.0
    out["logm"].update(stages_s={k: round(v, 5) for k, v in stages.items()}, e_device_expm=e, dtype=str(res.X.dtype),
                       roots=res.roots, degree=res.degree, perturbed=res.perturbed, converged=res.converged)
    out["roots_s_per_root"] = round(stages["roots"] / max(res.roots, 1), 5)
    out["pade_tflops"] = round(flops / max(stages["pade"], 1e-12) * 1e-12, 3)
    out["non_schur_stages_s"] = round(rest, 5)
    out["non_schur_stages_over_schur"] = round(rest / out["schur"]["s"], 4)
    out["logm_over_schur"] = round(out["logm"]["s"] / out["schur"]["s"], 3)
    if scipy_reps > 0:
        leg = scipy_leg(A, scipy_reps)
        if leg:
            out["scipy"] = leg
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--scipy-reps", type=int, default=1)
    ap.add_argument("--scipy-only", action="store_true")
    ap.add_argument("--only", choices=("f64", "c128"))
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "logm_bench.json"))
    a = ap.parse_args()
    doc = {}
    if os.path.exists(a.out):
        with open(a.out) as f:
            doc = json.load(f)
    doc["metric"] = ("seconds per call, host buffers in and out (median of the timed calls after one warm-up call; logm "
                     "and schur timed alternately in one process; scipy on the host, once)")
    ctx = None if a.scipy_only else E.Context(0)

    for idx, (key, n, cplx) in enumerate((("f64", 4096, False), ("c128", 2048, True))):
        if a.only and a.only != key:
            continue
        rng = np.random.default_rng(20261021 + idx)   # per workload, so that --only and --scipy-only see the same matrices
        A = rng.standard_normal((n, n))
        A = A + 1j * rng.standard_normal((n, n)) if cplx else A + (2.0 * np.sqrt(n) + 1.0) * np.eye(n)
        A = np.asfortranarray(A)
        print(key, "start", flush=True)
        if a.scipy_only:
            doc.setdefault(key, {"n": n, "dtype": "complex128" if cplx else "float64"})
            leg = scipy_leg(A, max(a.scipy_reps, 1))
            if leg:
                doc[key]["scipy"] = leg
        else:
            kept = doc.get(key, {}).get("scipy") if a.scipy_reps == 0 else None
            doc[key] = {"n": n, "dtype": "complex128" if cplx else "float64", **workload(ctx, A, a.reps, a.scipy_reps)}
            if kept:
                doc[key]["scipy"] = kept
        if "scipy" in doc[key] and "logm" in doc[key]:
            doc[key]["scipy_over_logm"] = round(doc[key]["scipy"]["s"] / doc[key]["logm"]["s"], 3)
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
