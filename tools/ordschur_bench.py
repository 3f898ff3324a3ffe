"""schur(A, sort="lhp") against schur(A) on the same matrix, the reordering stage on its own, and
scipy.linalg.schur(sort="lhp") on the host beside them: seconds per call, host buffers in and out.

Workloads: a random f64 matrix of order 4096 and a random c128 matrix of order 2048 (seeded standard normal
entries).  Per workload:

  schur            T, Z and the eigenvalues, unsorted
  schur_lhp        the same with sort="lhp": the reordering runs on the device before anything is copied back
  reorder          the reordering stage of the last schur_lhp call by stream events (ordschur_stats), with its
                   rounds, windows that did work and swaps, and as a share of the schur call measured beside it
  last             ordschur of the unsorted result with the bottom block alone selected: one eigenvalue (or
                   pair) crosses every window, the latency-bound extreme
  scipy_schur_lhp  scipy.linalg.schur(sort="lhp") (LAPACK xGEES with its select function) on HOST_THREADS threads

schur and schur_lhp are timed ALTERNATELY in one process after one warm-up call of each, REPS times with a host
clock around the whole call, which ends synchronised (results on the host).  The figure is the median; the
fastest and the slowest are listed.  r = ||A - Z T Z^H||_F / (n eps ||A||_F) and o = ||Z^H Z - I||_F / (n eps)
of the sorted result are listed.  scipy is timed SCIPY_REPS times (default 1).

Writes one JSON document (default profiles/ordschur_bench.json; an existing document keeps the workloads this
run does not time) and prints it.

  python tools/ordschur_bench.py [--n-real 4096] [--n-complex 2048] [--reps 5] [--scipy-reps 1] [--only f64|c128]
                                 [--out FILE]
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


def figures(A, T, Z):
    n = A.shape[0]
    r = float(np.linalg.norm(A - Z @ T @ Z.conj().T) / (n * EPS * np.linalg.norm(A)))
    o = float(np.linalg.norm(Z.conj().T @ Z - np.eye(n)) / (n * EPS))
    return r, o


def workload(ctx, A, reps, scipy_reps):
    n = A.shape[0]
    calls = {"schur": lambda: E.schur(ctx, A), "schur_lhp": lambda: E.schur(ctx, A, sort="lhp")}
    out = {k: {} for k in calls}
    ts = {k: [] for k in calls}
    reorder = []
    last = {}
    for fn in calls.values():
        fn()                                    # warm-up
    for _ in range(reps):
        for k, fn in calls.items():
            t = time.perf_counter()
            last[k] = fn()
            ts[k].append(time.perf_counter() - t)
            if k == "schur_lhp":
                reorder.append(E.ordschur_stats(ctx))
    for k in calls:
        out[k].update(summary(ts[k]))
    plain, srt = last["schur"], last["schur_lhp"]
    r, o = figures(A, srt.T, srt.Z)
    out["schur_lhp"].update(r=r, o=o, converged=srt.converged, ordered=srt.ordered, sdim=srt.sdim,
                            leading_all_lhp=bool(np.all(srt.eigenvalues[:srt.sdim].real < 0) and
                                                 np.all(srt.eigenvalues[srt.sdim:].real >= 0)))
    st = reorder[-1]
    out["reorder"] = {"s": round(statistics.median(x["seconds"] for x in reorder), 5), "rounds": st["rounds"],
                      "windows": st["windows"], "swaps": st["swaps"]}
    out["reorder"]["share_of_schur"] = round(out["reorder"]["s"] / out["schur"]["s"], 4)
    out["schur_lhp_over_schur"] = round(out["schur_lhp"]["s"] / out["schur"]["s"], 3)
    # the bottom block alone to the top
    mask = np.zeros(n, dtype=bool)
    mask[-1] = True
    tl, sl = [], []
    for _ in range(1 + reps):                   # the first call is the warm-up
        t = time.perf_counter()
        res = E.ordschur(ctx, plain.T, plain.Z, mask)
        tl.append(time.perf_counter() - t)
        sl.append(E.ordschur_stats(ctx))
    r, o = figures(A, res.T, res.Z)
    out["last"] = {**summary(tl[1:]), "reorder_s": round(statistics.median(x["seconds"] for x in sl[1:]), 5),
                   "rounds": sl[-1]["rounds"], "windows": sl[-1]["windows"], "swaps": sl[-1]["swaps"], "sdim": res.sdim,
                   "ordered": res.ordered, "r": r, "o": o}
    out["last"]["reorder_share_of_schur"] = round(out["last"]["reorder_s"] / out["schur"]["s"], 4)
    if scipy_reps > 0:
        real = not np.iscomplexobj(A)
        st = []
        for _ in range(scipy_reps):
            t = time.perf_counter()
            Ts, Zs, sd = sla.schur(A, output="real" if real else "complex", sort="lhp")
            st.append(time.perf_counter() - t)
        rs, os_ = figures(A, Ts, Zs)
        out["scipy_schur_lhp"] = {**summary(st), "host_threads": HOST_THREADS, "r": rs, "o": os_, "sdim": int(sd)}
        out["scipy_schur_lhp_over_schur_lhp"] = round(out["scipy_schur_lhp"]["s"] / out["schur_lhp"]["s"], 3)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n-real", type=int, default=4096)
    ap.add_argument("--n-complex", type=int, default=2048)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--scipy-reps", type=int, default=1)
    ap.add_argument("--only", choices=("f64", "c128"))
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ordschur_bench.json"))
    a = ap.parse_args()
    doc = {}
    if os.path.exists(a.out):
        with open(a.out) as f:
            doc = json.load(f)
    doc["metric"] = ("seconds per call, host buffers in and out (median of the timed calls after one warm-up call; schur "
                     "and schur_lhp timed alternately in one process; reorder by stream events; scipy on the host afterwards)")
    ctx = E.Context(0)
    rng = np.random.default_rng(20251020)
    if a.only != "c128":
        A = np.asfortranarray(rng.standard_normal((a.n_real, a.n_real)))
        doc["f64"] = {"n": a.n_real, "dtype": "float64", **workload(ctx, A, a.reps, a.scipy_reps)}
    if a.only != "f64":
        n = a.n_complex
        A = np.asfortranarray(rng.standard_normal((n, n)) + 1j * rng.standard_normal((n, n)))
        doc["c128"] = {"n": n, "dtype": "complex128", **workload(ctx, A, a.reps, a.scipy_reps)}
    ctx.close()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    print(json.dumps(doc, indent=1))


if __name__ == "__main__":
    main()
