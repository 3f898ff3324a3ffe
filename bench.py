#!/usr/bin/env python3
"""Benchmark of the MI355X power-iteration hot path (BASELINE.json metric).

metric : "power-iteration SpMV GB/s vs HBM roofline + eigvals/sec (QR), 1/2/4/8 GPU"
step   : one fused power iteration (y = A x / ||.||, ||y||^2, x^H y, device-side convergence
         test) over the workload's CSR matrix — powerMethodImpl's loop body
         (src/power_method/power_method.hpp:68-96) with the redundant second product fused away.
workload (default): BASELINE config 4 "10M x 10M CSR ~10 nnz/row fp64, power_method row-sharded"
         — ONE 10,000,000 x 10,000,000 band matrix (SURVEY §8d generator, partition-invariant) split
         into N contiguous row blocks, one per rank (strong scaling; --scaling weak gives every
         rank a 10M-row block of an (N*10M)-row matrix instead).  Per iteration the ranks exchange
         halo rows and partial sums device to device (EIGSOL_TRANSPORT_PEER: the SpMV epilogue
         stores into the peers' IPC-mapped inboxes over xGMI, the next launch waits on their flags).
value  : algorithmic bytes (12 nnz + 4 (n+1) + 16 n per iteration, summed over the
         ranks' blocks) x iterations / max-over-ranks wall time of the K timed iterations; inputs
         resident in HBM.

Run: python bench.py [--gpus N --steps K --warmup W] [--dump-outputs DIR] [--full].  A plain run sets
up, warms up, times the K steps and prints the line; --dump-outputs DIR then also writes what the
timed steps computed as DIR/<name>.npy (same arguments: same inputs, so two builds compare output
for output); --full adds the measured HBM ceilings, the extras and the CPU baselines to the line
(N = 1; --no-extras / --no-cpu-baseline drop either again).  N>1 runs one rank per GPU: either launched
by torch.distributed.run (WORLD_SIZE set), or, when started directly, bench.py starts the N ranks
itself as a child torch.distributed.run over 127.0.0.1 before importing torch and relays rank 0's
line and exit code.
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

METRIC = "power-iteration SpMV GB/s vs HBM roofline + eigvals/sec (QR), 1/2/4/8 GPU"
HBM_PEAK_GBS = 8000.0   # MI355X HBM3E spec (MI355X_MICROARCH.md chip table)

WORKLOADS = {
    # name: (generator, rows (global for strong scaling, per rank for weak), nnz per row)
    "band10m": ("band", 10_000_000, 10),
    "uniform10m": ("uniform", 10_000_000, 10),
    "uniform1m": ("uniform", 1_000_000, 16),
    "band1m": ("band", 1_000_000, 16),
}


def parse():
    p = argparse.ArgumentParser()
    p.add_argument("--gpus", type=int, default=1)
    p.add_argument("--steps", type=int, default=200)
    p.add_argument("--warmup", type=int, default=20)
    p.add_argument("--workload", default="band10m", choices=sorted(WORKLOADS))
    p.add_argument("--scaling", default="strong", choices=["strong", "weak"],
                   help="strong: one global matrix split over the ranks (BASELINE config 4); "
                        "weak: a full-size block per rank")
    p.add_argument("--full", action="store_true",
                   help="after the headline run, also measure what the line reports beside it: the STREAM-like "
                        "HBM ceilings, the extras (configs 1, 2, 3, 5, other precisions and sizes) and the CPU "
                        "baselines (N = 1 only).  Off by default: a plain run sets up, warms up, times the steps "
                        "and prints the line")
    p.add_argument("--dump-outputs", metavar="DIR", default=None,
                   help="after the timed steps, write what they computed (eigenvalue estimate, iteration count, "
                        "iterate) as DIR/<name>.npy in float64; an iterate above the size cap is written as a "
                        "fixed seeded sample of its entries")
    p.add_argument("--no-cpu-baseline", action="store_true", help="with --full: skip the CPU baselines")
    p.add_argument("--cpu-seconds", type=float, default=12.0)
    p.add_argument("--no-extras", action="store_true",
                   help="with --full: skip configs 2 (QR 4096^2), 3 (1M x 16 CSR) and 5 (shifted inverse, "
                        "1M complex)")
    p.add_argument("--check", action="store_true",
                   help="after the timed region, run the power method to convergence (tol 1e-12, at most 300 "
                        "iterations) on the same sharded matrix and report lambda / iterations in the line")
    p.add_argument("--bootstrap", default="auto", choices=["auto", "rccl", "host"],
                   help="N > 1: the library's communicator. rccl: an RCCL communicator (one GPU per rank); "
                        "host: set-up over torch.distributed (gloo), per-iteration exchange device to device "
                        "(peer inboxes). auto: rccl on distinct GPUs (a rank whose peer set-up fails falls back to "
                        "RCCL's collective exchange), host when ranks share a GPU (RCCL refuses duplicate devices)")
    return p.parse_args()


def device_map(world, local_world=None):
    """GPU of each local rank: EIGSOL_BENCH_DEVICES="0,0,1,1" when set (rehearsing N ranks on fewer
    GPUs), else local rank r on GPU r.  torch.cuda.device_count() does not initialise the GPU."""
    spec = os.environ.get("EIGSOL_BENCH_DEVICES")
    n = local_world or world
    if spec:
        devs = [int(t) for t in spec.split(",") if t.strip()]
        if len(devs) < n:
            raise SystemExit(f"EIGSOL_BENCH_DEVICES names {len(devs)} devices for {n} local ranks")
        return devs[:n]
    return list(range(n))


def gen(kind, n_global, k, row0, nrows):
    from pcsc_eigenvalue_solver_project_amd import synthetic as S
    if kind == "band":
        return S.band(n_global, k, row0=row0, nrows=nrows)
    return S.uniform(n_global, k, row0=row0, nrows=nrows)


def kernel_key(name):
    """'void eigsol::dev::csr_slice_kernel<double, true, 12, false, false>(eigsol::dev::CsrArgs<double>, int)'
    -> 'csr_slice_kernel<double, true, 12, false, false>' (template instantiation, no scope/arguments)."""
    name = (name or "").strip()
    if name.startswith("void "):
        name = name[5:]
    depth, cut = 0, len(name)
    for i, ch in enumerate(name):          # drop the argument list: first '(' outside the template brackets
        if ch == "<":
            depth += 1
        elif ch == ">":
            depth -= 1
        elif ch == "(" and depth == 0:
            cut = i
            break
    name = name[:cut]
    head = name.split("<", 1)
    return head[0].split("::")[-1] + ("<" + head[1] if len(head) > 1 else "")


def pmc_traffic(workload, kernel_name):
    """HBM bytes per launch of the SAME kernel instantiation on the same workload, from the
    committed rocprofv3 PMC summary (profiles/, FETCH_SIZE x 2 + WRITE_SIZE per MI355X_MICROARCH.md);
    PMC counters cannot be read from inside a timed run, so the profile is a separate pass of this
    workload.  A summary whose kernel string is a different instantiation is not used."""
    import glob
    best = None
    want = kernel_key(kernel_name)
    for f in sorted(glob.glob(os.path.join(ROOT, "profiles", f"r*_{workload}_*.json"))):
        try:
            d = json.load(open(f))
        except (OSError, ValueError):
            continue
        if "hbm_traffic_bytes_per_launch" in d and want and kernel_key(d.get("kernel")) == want:
            best = {"hbm_traffic_bytes_per_launch": round(d["hbm_traffic_bytes_per_launch"]),
                    "source": os.path.relpath(f, ROOT), "kernel": d.get("kernel")}
    return best


def cpu_baseline(kind, k, budget_s, n, mat=None):
    """Reference algorithm (two CSC products per iteration, single thread) on the same matrix as
    the GPU run (n = the workload's global size), a bounded number of iterations."""
    from oracle import oracle as O
    from pcsc_eigenvalue_solver_project_amd import synthetic as S
    rp, ci, v = mat if mat is not None else gen(kind, n, k, 0, n)
    cp, ri, vv = O.csr_to_csc(rp, ci, v, n)
    x0 = S.start_vector(n)
    t = time.perf_counter()
    O.power_csc(cp, ri, vv, x0, 2, -1.0)
    per_iter = (time.perf_counter() - t) / 2
    iters = max(3, int(budget_s / max(per_iter, 1e-6)))
    t = time.perf_counter()
    O.power_csc(cp, ri, vv, x0, iters, -1.0)
    dt = time.perf_counter() - t
    nbytes = S.csr_bytes_per_iteration(n, len(ci))
    # BASELINE.md §2's secondary run: the same restatement at the reference's as-shipped flags (its
    # CMake sets no build type: -O0, no -march), a few iterations of the same loop
    with O.as_shipped():
        t = time.perf_counter()
        O.power_csc(cp, ri, vv, x0, 1, -1.0)
        per0 = time.perf_counter() - t
        it0 = max(1, min(5, int(0.5 * budget_s / max(per0, 1e-6))))
        t = time.perf_counter()
        O.power_csc(cp, ri, vv, x0, it0, -1.0)
        dt0 = time.perf_counter() - t
    as_shipped = {"value": round(nbytes * it0 / dt0 / 1e9, 3), "unit": "GB/s", "cores": 1, "kind": "port",
                  "ms_per_iteration": round(1e3 * dt0 / it0, 1),
                  "sample": f"the same matrix, {it0} reference power iterations, oracle compiled -O0 without -march "
                            f"(the reference's CMake sets no build type), {dt0:.1f}s; a baseline only, never a target"}
    return {
        "as_shipped_O0": as_shipped,
        "value": nbytes * iters / dt / 1e9,
        "unit": "GB/s",
        "cores": 1,
        "kind": "port",
        "sample": f"the same {kind} {n}x{n} matrix, {k} nnz/row, {iters} reference power "
                  f"iterations (2 CSC-scatter products each, oracle/eigsol_oracle.cpp, -O3, 1 thread), "
                  f"{dt:.1f}s",
        "ms_per_iteration": 1e3 * dt / iters,
    }


def host_cpu():
    """Core model and the CPU share this process may use (the GPU box exports OMP_NUM_THREADS)."""
    model = "?"
    try:
        for line in open("/proc/cpuinfo"):
            if line.startswith("model name"):
                model = line.split(":", 1)[1].strip()
                break
    except OSError:
        pass
    return {"model": model, "nproc": os.cpu_count(),
            "threads_allowed": int(os.environ.get("OMP_NUM_THREADS", os.cpu_count() or 1))}


def cpu_allcores(kind, k, budget_s, n, mat=None):
    """Stronger CPU figure: one fused CSR product per iteration on all allowed cores,
    on the SAME n x n matrix as the GPU run (context only, never a target)."""
    from oracle import oracle as O
    from pcsc_eigenvalue_solver_project_amd import synthetic as S
    rp, ci, v = mat if mat is not None else gen(kind, n, k, 0, n)
    x0 = S.start_vector(n)
    th = host_cpu()["threads_allowed"]
    t = time.perf_counter()
    O.power_csr_omp(rp, ci, v, x0, 2, th)
    per_iter = (time.perf_counter() - t) / 2
    iters = max(3, int(budget_s / max(per_iter, 1e-6)))
    t = time.perf_counter()
    O.power_csr_omp(rp, ci, v, x0, iters, th)
    dt = time.perf_counter() - t
    return {"value": round(S.csr_bytes_per_iteration(n, len(ci)) * iters / dt / 1e9, 2), "unit": "GB/s",
            "cores": th, "kind": "port",
            "sample": f"the same {kind} {n}x{n} matrix, {k} nnz/row ({S.csr_bytes_per_iteration(n, len(ci)) / 1e9:.2f} GB "
                      f"per iteration, beyond the host caches): {iters} fused CSR power iterations, OpenMP rows "
                      f"(oracle power_csr_omp_f64, -O3), {dt:.1f}s; context only, not a target",
            "ms_per_iteration": round(1e3 * dt / iters, 3)}


def measured_hbm(torch, stream, ctx=None):
    """STREAM-like figures on this GPU (report beside the 8 TB/s spec): the library's
    hand-written gfx950 streaming kernels (eigsol_hbm_probe: non-temporal dwordx4 and dwordx2 reads,
    dwordx4 copy / write, 2 GiB, best of 1/2/4/8 workgroups per CU) and, for comparison, a torch copy_ and a torch read-only reduction."""
    a = torch.empty(2 << 30, dtype=torch.uint8, device="cuda").view(torch.float64)
    b = torch.empty_like(a)
    a.fill_(1.0)
    b.copy_(a)
    a.sum()
    torch.cuda.synchronize()
    reps = 10
    ms_copy = _events(torch, stream, lambda: [b.copy_(a) for _ in range(reps)]) / reps
    ms_read = _events(torch, stream, lambda: [a.sum() for _ in range(reps)]) / reps
    nb = a.numel() * 8
    del a, b
    torch.cuda.empty_cache()
    out = {"torch_copy_GBps": round(2 * nb / ms_copy / 1e6, 1), "torch_read_GBps": round(nb / ms_read / 1e6, 1)}
    if ctx is not None:
        import ctypes as C
        from pcsc_eigenvalue_solver_project_amd import lib
        rd, cp, wr, bpc = C.c_double(), C.c_double(), C.c_double(), C.c_int()
        st = lib().eigsol_hbm_probe(ctx.handle, C.c_size_t(2 << 30), 10, C.byref(rd), C.byref(cp), C.byref(wr),
                                    C.byref(bpc))
        if st == 0:
            out.update({"kernel_read_GBps": round(rd.value, 1), "kernel_copy_GBps": round(cp.value, 1),
                        "kernel_write_GBps": round(wr.value, 1), "kernel_read_blocks_per_cu": bpc.value,
                        "kernel": "eigsol::pdev::read_kernel, read8_kernel / copy_kernel / write_kernel (probe.hip, "
                                  "libeigsol_hip.so)"})
        mx, mb = C.c_double(), C.c_int()
        if lib().eigsol_hbm_probe_mix(ctx.handle, C.c_size_t(2 << 30), 10, C.byref(mx), C.byref(mb)) == 0:
            out.update({"kernel_mix12_GBps": round(mx.value, 1), "kernel_mix12_blocks_per_cu": mb.value,
                        "mix12_kernel": "eigsol::pdev::mix_kernel: the headline's read/write mix, 12 16-byte "
                                        "non-temporal reads per 16-byte write"})
    out["note"] = ("practical ceilings of this box; the roofline peak stays the 8 TB/s spec.  kernel_read_GBps is "
                   "the better of the 16-byte and the 8-byte non-temporal read kernels (each at 1/2/4/8 workgroups "
                   "per CU).  The headline's actual DRAM rate (PMC traffic / event time) is compared against it below")
    return out


def _events(torch, stream, fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(stream)
    fn()
    e1.record(stream)
    torch.cuda.synchronize()
    return e0.elapsed_time(e1)


def run_config3(E, S, ctx, torch, stream, opts):
    """BASELINE config 3: 1M x 1M CSR, 16 nnz/row (uniform columns: the gather-bound case)."""
    res = {}
    for kind in ("uniform", "band"):
        rp, ci, v = S.uniform(1_000_000, 16) if kind == "uniform" else S.band(1_000_000, 16)
        A = E.CsrMatrix(ctx, rp, ci, v, (1_000_000, 1_000_000))
        s = E.PowerSession(A)
        s.begin(opts, S.start_vector(1_000_000))
        s.step(20)
        torch.cuda.synchronize()
        ms = _events(torch, stream, lambda: s.step(200)) / 200
        info = s.kernel_info()
        res[kind] = {"GB/s": round(info["bytes_per_iteration"] / (ms / 1e3) / 1e9, 2),
                     "ms_per_iteration": round(ms, 5), "kernel": info["kernel"]}
        s.close()
        A.close()
    res["note"] = "212 MB per iteration fits the 256 MB Infinity Cache: can exceed the HBM bound"
    return res


def run_single_band10m(E, S, ctx, torch, stream):
    """float (ScalarConcept admits it, types.hpp:28-30): the config-4 band matrix stored and multiplied
    in single precision on the device.  Algorithmic bytes (SURVEY §8d with 4-byte values):
    8 nnz + 4 (n + 1) + 8 n per fused iteration."""
    n, k = 10_000_000, 10
    rp, ci, v = S.band(n, k)
    A = E.CsrMatrix(ctx, rp, ci, v.astype(np.float32), (n, n))
    del rp, ci, v
    sess = E.PowerSession(A)
    sess.begin(E.SolverOptions(2**31 - 1, -1.0), S.start_vector(n, np.float32))
    sess.step(10)
    torch.cuda.synchronize()
    ms = _events(torch, stream, lambda: sess.step(100)) / 100
    info = sess.kernel_info()
    out = {"GB/s": round(info["bytes_per_iteration"] / (ms / 1e3) / 1e9, 2), "ms_per_iteration": round(ms, 4),
           "bytes_per_iteration": info["bytes_per_iteration"],
           "roofline_frac": round(info["bytes_per_iteration"] / (ms / 1e3) / 1e9 / HBM_PEAK_GBS, 4),
           "kernel": info["kernel"], "dtype": "f32"}
    sess.close()
    A.close()
    return out


def run_long_double_power(E, S, ctx, torch, n=1_000_000, k=10):
    """long double (x87 in the reference, double-double on the device, wide.hip): powerMethod's
    fused step on a 1M band matrix with 10 entries per row.  One reference iteration is the
    double-double pass (x = y / normY, A x, the norm / Rayleigh partials) and the host's stopping
    test (one host wait).  Algorithmic bytes per iteration (kernel_info): (16 + 4) nnz + 4 (n + 1)
    + 48 n (y read, x and A x written)."""
    rp, ci, v = S.band(n, k)
    A = E.CsrMatrix(ctx, rp, ci, v.astype(np.longdouble), (n, n))
    del v
    sess = E.PowerSession(A)
    sess.begin(E.SolverOptions(2**31 - 1, -1.0), S.start_vector(n).astype(np.longdouble))
    sess.step(3)
    torch.cuda.synchronize()
    iters = 30
    t = time.perf_counter()
    sess.step(iters)
    torch.cuda.synchronize()
    ms = (time.perf_counter() - t) / iters * 1e3
    nnz = len(ci)
    info = sess.kernel_info()
    b = info["bytes_per_iteration"]
    sess.close()
    A.close()
    return {"n": n, "nnz": nnz, "dtype": "double-double", "ms_per_iteration": round(ms, 4),
            "GB/s": round(b / (ms / 1e3) / 1e9, 1), "roofline_frac": round(b / (ms / 1e3) / 1e9 / HBM_PEAK_GBS, 4),
            "kernel": info["kernel"]}


def run_uniform10m(E, S, ctx, torch, stream, opts):
    """Config 4's honest gather figure (SURVEY §8d "uniform also reported"): the same fused
    iteration on a 10M x 10M matrix with 10 uniform random columns per row, one GPU."""
    n = 10_000_000
    rp, ci, v = S.uniform(n, 10)
    A = E.CsrMatrix(ctx, rp, ci, v, (n, n))
    del rp, ci, v
    s = E.PowerSession(A)
    s.begin(opts, S.start_vector(n))
    s.step(5)
    torch.cuda.synchronize()
    ms = _events(torch, stream, lambda: s.step(40)) / 40
    info = s.kernel_info()
    s.close()
    A.close()
    return {"GB/s": round(info["bytes_per_iteration"] / (ms / 1e3) / 1e9, 2), "ms_per_iteration": round(ms, 4),
            "roofline_frac": round(info["bytes_per_iteration"] / (ms / 1e3) / 1e9 / HBM_PEAK_GBS, 4),
            "kernel": info["kernel"], "bytes_per_iteration": info["bytes_per_iteration"]}


def run_config2(E, ctx, no_cpu):
    """BASELINE config 2: 4096^2 N(0,1) (seed 20251226), Hessenberg + Francis multishift QR."""
    n = 4096
    A = np.asfortranarray(np.random.default_rng(20251226).standard_normal((n, n)))   # column-major, like Matrix::Dense
    E.qr_eigenvalues(ctx, A[:256, :256].copy())          # warm-up (module load)
    t = time.perf_counter()
    r = E.qr_eigenvalues(ctx, A)
    dt = time.perf_counter() - t
    out = {"eigvals_per_s": round(n / dt, 1), "seconds": round(dt, 3), "converged": r.converged,
           "iterations": r.iterations, "dtype": "f64",
           "includes": "host->device copy of A, blocked Hessenberg, multishift sweeps, eigenvalue copy-back"}
    fx = os.path.join(ROOT, "tests", "golden", "cfg2_eigvals_4096.npy")
    if os.path.exists(fx):
        from scipy.spatial import cKDTree
        ref = np.load(fx)
        ev = r.eigenvalues_complex
        d, j = cKDTree(np.c_[ref.real, ref.imag]).query(np.c_[ev.real, ev.imag], k=1)
        out["vs_lapack_fixture"] = {"max_abs_diff": float(d.max()), "one_to_one": bool(len(np.unique(j)) == n)}
    prof = os.path.join(ROOT, "profiles", "r06_qr4096_mfma.json")
    if os.path.exists(prof):
        d = json.load(open(prof))
        out["mfma"] = {"gemm_TFLOPs": round(d["gemm_TFLOPs"], 2), "peak_TFLOPs": d["mfma_peak_TFLOPs"],
                       "utilisation": round(d["mfma_utilisation"], 4), "gemm_flops": d["gemm_flops"],
                       "rank_update_TFLOPs": round(d.get("rank_update_TFLOPs") or 0.0, 2),
                       "rank_update_utilisation": round(d.get("rank_update_mfma_utilisation") or 0.0, 4),
                       "francis_window_gemm_share": round(d.get("francis_window_gemm_share") or 0.0, 4),
                       "source": "profiles/r06_qr4096_mfma.json from profiles/r06_qr4096_kernel_stats.csv "
                                 "(rocprofv3 kernel times of the shipped path: hess_panel_coop2<double> issued by "
                                 "an ordinary launch of the same kernel, gemm_mfma_f64 / gemm_reduce / "
                                 "rankk_mfma<double, false> on v_mfma_f64_16x16x4_f64 - the whole trailing-update "
                                 "set incl. the split-K W = V^T A, and the single rank-2nb update alone; "
                                 "win_gemm_mfma for the sweeps' share)",
                       "kernels": sorted(k for k in d.get("kernels", {}) if "mfma" in k or "hess_panel" in k)}
    if not no_cpu:
        from oracle import oracle as O
        m = 1024
        B = np.random.default_rng(20251226).standard_normal((m, m))
        t = time.perf_counter()
        O.hqr_francis(O.hessenberg(B))
        dc = time.perf_counter() - t
        th = host_cpu()["threads_allowed"]
        t = time.perf_counter()
        np.linalg.eigvals(A)
        dl = time.perf_counter() - t
        out["cpu_allcores"] = {"value": round(n / dl, 1), "unit": "eigvals/s", "cores": th, "kind": "lapack",
                               "sample": f"numpy.linalg.eigvals (LAPACK dgeev: dgehrd + multishift dhseqr with AED, "
                                         f"the implicit-shift algorithm class the device runs) on the same 4096^2 "
                                         f"matrix, {dl:.2f}s, BLAS threads = OMP_NUM_THREADS"}
        out["cpu_baseline"] = {
            "value": round(m / dc, 1), "unit": "eigvals/s", "cores": 1, "kind": "port", "measured_at_n": m,
            "extrapolated_to_n": n, "extrapolation": "n^3",
            "extrapolated_value": round(n / (dc * (n / m) ** 3), 1),
            "sample": f"{m}x{m} N(0,1) (not the 4096 config: measured at n = {m}): oracle Hessenberg + textbook "
                      f"Francis double shift (oracle/eigsol_oracle.cpp, 1 thread) {dc:.2f}s; extrapolated_value is "
                      f"that time scaled by n^3 to 4096.  The reference's own unshifted iteration does not converge "
                      f"on this input"}
    return out


def run_qr_complex(E, ctx, no_cpu, n=1024):
    """qr_eigenvalues_dense<std::complex<double>> on an n^2 complex N(0,1) matrix (seed n, n = 1024 or
    4096): blocked complex Hessenberg + complex AED and multishift sweeps (zfrancis.hip), matched to
    the zgeev fixture (tests/golden/qr_c<n>_eigvals.npy)."""
    rng = np.random.default_rng(n)
    # column-major (Matrix::Dense's layout) before the clock starts: a C-ordered 4096^2 complex input
    # costs ~1.1 s of numpy transposition inside the call (round-4 kernel trace, tools/gap_analysis.py)
    A = np.asfortranarray(rng.standard_normal((n, n)) + 1j * rng.standard_normal((n, n)))
    E.qr_eigenvalues(ctx, np.asfortranarray(A[:512, :512]))   # warm-up: every kernel of the path loaded
    t = time.perf_counter()
    r = E.qr_eigenvalues(ctx, A)
    dt = time.perf_counter() - t
    out = {"eigvals_per_s": round(n / dt, 1), "seconds": round(dt, 3), "converged": r.converged,
           "iterations": r.iterations, "dtype": "c128"}
    fx = os.path.join(ROOT, "tests", "golden", f"qr_c{n}_eigvals.npy")
    if os.path.exists(fx):
        from scipy.spatial import cKDTree
        ref = np.load(fx)
        ev = r.eigenvalues_complex
        d, j = cKDTree(np.c_[ref.real, ref.imag]).query(np.c_[ev.real, ev.imag], k=1)
        out["vs_lapack_fixture"] = {"max_abs_diff": float(d.max()), "one_to_one": bool(len(np.unique(j)) == n)}
    if not no_cpu and n <= 1024:   # (zgeev at 4096 takes ~40 s of host time: timed at 1024 only)
        t = time.perf_counter()
        np.linalg.eigvals(A)
        dl = time.perf_counter() - t
        out["cpu_allcores"] = {"value": round(n / dl, 1), "unit": "eigvals/s", "cores": host_cpu()["threads_allowed"],
                               "kind": "lapack", "sample": f"numpy.linalg.eigvals (zgeev) on the same matrix, {dl:.2f}s"}
    return out


def _convdiff_run(E, ctx, torch, stream, A, sigma, x0, max_iter, tol=1e-10):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    sess = E.ShiftedSession(A, sigma)
    t_factor = time.perf_counter() - t0
    info0 = sess.kernel_info()
    sess.begin(E.ShiftedSolverOptions(max_iter, tol, sigma), x0)
    t = time.perf_counter()
    done = False
    while not done:
        sess.step(1)
        done, _ = sess.query()
    res = sess.finish()
    t_solve = time.perf_counter() - t
    t_e2e = time.perf_counter() - t0
    info = sess.kernel_info()
    sess.begin(E.ShiftedSolverOptions(2**31 - 1, -1.0, sigma), x0)
    sess.step(1)
    torch.cuda.synchronize()
    ms = _events(torch, stream, lambda: sess.step(3)) / 3
    sess.close()
    paths = {7: "ILU(0) + restarted GMRES", 8: "RCM + banded partial-pivot LU",
             18: "exact sparse LU (complete fill, no pivoting) + residual check", 4: "densified partial-pivot LU",
             19: "nested-dissection multifrontal LU (front-restricted pivoting) + residual check"}
    return res, {"solver_path": paths.get(info0["variant"], str(info0["variant"])), "variant": info0["variant"],
                 "factor_seconds": round(t_factor, 3), "ms_per_iteration": round(ms, 3),
                 "iterations": res.iterations, "converged": res.converged,
                 "eigenvalue": [float(np.real(res.eigenvalue)), float(np.imag(res.eigenvalue))],
                 "arnoldi_steps_last_solve": info["tiles"] if info["variant"] in (7, 18, 19) else None,
                 "band_kl_plus_ku": info["tiles"] if info["variant"] == 8 else None,
                 "solve_seconds": round(t_solve, 3), "end_to_end_seconds": round(t_e2e, 3)}


def run_config5_convdiff(E, S, ctx, torch, stream, nx=1000, max_iter=8):
    """The general-sparse shifted inverse on a matrix whose LU has real fill:
    synthetic.convdiff_complex(1000), a 2-D convection-diffusion stencil on a 1000 x 1000 grid with
    complex perturbations under a random symmetric permutation (n = 1M, ~5M nnz; neither banded nor
    triangular as stored; the exact LU's fill passes the 3 x nnz cap).  Reported for the path the
    library chooses by default (a direct factor, like the reference's SparseLU: since round 5 the
    nested-dissection multifrontal LU, multifrontal.hip; round 5's first figure was the RCM band LU:
    13.8 s set-up, 1.37 s per iteration) and for ILU(0) + GMRES forced (EIGSOL_LU_FILL_CAP=0): set-up
    time, steady-state ms per iteration, Arnoldi steps / band width, and the end-to-end time of a run
    (plus the default path on the values rounded to complex<float>)
    of at most max_iter iterations (sigma sits inside a clustered spectrum, so the iteration itself
    converges slowly: `converged` says whether it did).  solve_shifted.hpp:85-117 is the reference
    path (SparseLU, refactored every iteration)."""
    import scipy.sparse as sp
    rp, ci, v = S.convdiff_complex(nx)
    n = nx * nx
    sigma = 4.0 + 0.5j                      # inside the stencil's spectrum (around (0, 8))
    x0 = S.start_vector(n, np.complex128)
    A = E.CsrMatrix(ctx, rp, ci, v, (n, n))
    M = sp.csr_matrix((v, ci, rp), shape=(n, n))
    out = {"n": n, "nnz": int(len(ci)), "sigma": [sigma.real, sigma.imag]}
    for label, forced in (("default", None), ("ilu0_gmres_forced", {"EIGSOL_SPARSE_SOLVER": "gmres",
                                                                     "EIGSOL_LU_FILL_CAP": "0"})):
        old = {k: os.environ.get(k) for k in (forced or {})}
        os.environ.update(forced or {})
        try:
            res, d = _convdiff_run(E, ctx, torch, stream, A, sigma, x0, max_iter)
        finally:
            for k, val in old.items():
                if val is None:
                    os.environ.pop(k, None)
                else:
                    os.environ[k] = val
        x = res.eigenvector
        d["eigen_residual"] = float(np.linalg.norm(M @ x - res.eigenvalue * x) / np.linalg.norm(x))
        # the same 8 iterations of the reference loop run with SciPy's SuperLU on the host
        # (tests/golden/convdiff1000_fixed.json): lambda after them, and the iteration count
        fxp = os.path.join(ROOT, "tests", "golden", "convdiff1000_fixed.json")
        if os.path.exists(fxp) and nx == 1000 and max_iter == 8:
            fx = json.load(open(fxp))
            if complex(*fx["sigma"]) == sigma:
                d["vs_superlu_fixture"] = {"abs_error": float(abs(res.eigenvalue - complex(*fx["lambda"]))),
                                           "fixture_iterations": fx["iterations"],
                                           "source": "tests/golden/convdiff1000_fixed.json"}
        out[label] = d
    A.close()
    # complex<float>: the same family on the values widened to double, the iterate in complex<float>
    A32 = E.CsrMatrix(ctx, rp, ci, v.astype(np.complex64), (n, n))
    res, d = _convdiff_run(E, ctx, torch, stream, A32, np.complex64(sigma), x0.astype(np.complex64), max_iter)
    x = res.eigenvector.astype(np.complex128)
    d["eigen_residual"] = float(np.linalg.norm(M @ x - res.eigenvalue * x) / np.linalg.norm(x))
    out["complex64_default"] = d
    A32.close()
    return out


def run_dense_power(E, S, ctx, torch, stream):
    """Dense branch of powerMethod (power_method.hpp:141-143): column-major fp64 GEMV fused with the
    norm and Rayleigh partials, 16384^2 (2 GiB, HBM-bound: 8 n^2 + 16 n bytes per iteration)."""
    n = 16384
    A = np.random.default_rng(1).standard_normal((n, n))
    D = E.DenseMatrix(ctx, A)
    del A
    s = E.PowerSession(D)
    s.begin(E.SolverOptions(2**31 - 1, -1.0), S.start_vector(n))
    s.step(5)
    torch.cuda.synchronize()
    ms = _events(torch, stream, lambda: s.step(50)) / 50
    info = s.kernel_info()
    gbs = info["bytes_per_iteration"] / (ms / 1e3) / 1e9
    s.close()
    # the same matrix through the dense shifted inverse (shifted_inverse_power_solver.hpp:49-76): the
    # partial-pivot LU once, then per iteration both triangular solves (dense_trsv2_kernel) and the
    # partials; steady state with tol < 0, like the power method above
    t = time.perf_counter()
    sh = E.ShiftedSession(D, 0.5)
    t_factor = time.perf_counter() - t
    sh.begin(E.ShiftedSolverOptions(2**31 - 1, -1.0, 0.5), S.start_vector(n))
    sh.step(3)
    torch.cuda.synchronize()
    ms_sh = _events(torch, stream, lambda: sh.step(20)) / 20
    info_sh = sh.kernel_info()
    sh.close()
    D.close()
    return {"n": n, "dtype": "f64", "ms_per_iteration": round(ms, 4), "GB/s": round(gbs, 1),
            "roofline_frac": round(gbs / HBM_PEAK_GBS, 4), "kernel": info["kernel"],
            "shifted_inverse": {"sigma": 0.5, "factor_seconds": round(t_factor, 3),
                                "ms_per_iteration": round(ms_sh, 4),
                                "GB/s": round(info_sh["bytes_per_iteration"] / (ms_sh / 1e3) / 1e9, 1),
                                "kernel": info_sh["kernel"]}}


def run_config1(E, S, ctx):
    """BASELINE config 1: data/A.txt read as double (the reference's text format), power method."""
    path = os.path.join(ROOT, "tests", "golden", "A.txt")
    tok = open(path).read().split()
    r_, c_ = int(tok[1]), int(tok[2])
    A = np.array([float(t) for t in tok[3:3 + r_ * c_]]).reshape(r_, c_)   # row by row, like the reader
    res = E.power_method(E.DenseMatrix(ctx, A), E.SolverOptions(1000, 1e-10), S.start_vector(r_))
    exact = 1.0 + np.sqrt(15.0)
    return {"eigenvalue": res.eigenvalue, "iterations": res.iterations, "converged": res.converged,
            "abs_error_vs_1_plus_sqrt15": abs(res.eigenvalue - exact)}


def run_config5(E, S, ctx, torch, stream, no_cpu):
    """BASELINE config 5: 1M x 1M complex upper-triangular CSR (16 nnz/row), shifted inverse
    iteration with sigma next to the planted interior eigenvalue."""
    n = 1_000_000
    rp, ci, v, _ = S.triu_complex(n, 16)
    target = 1.5 * np.exp(0.7j)
    sigma = target + 1e-3
    x0 = S.start_vector(n, np.complex128)
    A = E.CsrMatrix(ctx, rp, ci, v, (n, n))
    # warm-up: a small factor of the same kind loads every kernel of the path (module load is a
    # one-off of the process, not of a solve)
    wr, wc, wv, _ = S.triu_complex(4096, 16)
    W = E.CsrMatrix(ctx, wr, wc, wv, (4096, 4096))
    E.shifted_inverse_power_method(W, E.ShiftedSolverOptions(50, 1e-12, sigma), x0[:4096])
    W.close()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    sess = E.ShiftedSession(A, sigma)
    t_factor = time.perf_counter() - t0
    sess.begin(E.ShiftedSolverOptions(1000, 1e-12, sigma), x0)
    t = time.perf_counter()
    sess.step(3)
    done, _ = sess.query()
    while not done:
        sess.step(2)
        done, _ = sess.query()
    res = sess.finish()
    t_solve = time.perf_counter() - t
    t_e2e = time.perf_counter() - t0
    sess.begin(E.ShiftedSolverOptions(2**31 - 1, -1.0, sigma), x0)
    sess.step(3)
    torch.cuda.synchronize()
    info = sess.kernel_info()
    ms = _events(torch, stream, lambda: sess.step(30)) / (30 * info["iterations_per_launch"])
    out = {"ms_per_iteration": round(ms, 4), "GB/s": round(info["bytes_per_iteration"] / (ms / 1e3) / 1e9, 2),
           "dependency_levels": info["tiles"], "kernel": info["kernel"], "iterations": res.iterations,
           "converged": res.converged, "abs_error_vs_planted_eigenvalue": float(abs(res.eigenvalue - target)),
           "analysis_seconds": round(t_factor, 4), "solve_seconds": round(t_solve, 4),
           "end_to_end_seconds": round(t_e2e, 4),
           "end_to_end_includes": "ShiftedSession create (device-side level analysis + layout of A - sigma I, "
                                  "matrix already resident) + begin (x0 upload) + launches to convergence + "
                                  "finish (eigenvector download)"}
    sess.close()
    # the same complex matrix in the fused power iteration: the complex SpMV rate (SURVEY §8d asks
    # for both the SpMV and the SpTRSV GB/s of config 5)
    ps = E.PowerSession(A)
    ps.begin(E.SolverOptions(2**31 - 1, -1.0), x0)
    ps.step(5)
    torch.cuda.synchronize()
    ms_mv = _events(torch, stream, lambda: ps.step(50)) / 50
    pinfo = ps.kernel_info()
    out["spmv"] = {"ms_per_iteration": round(ms_mv, 4),
                   "GB/s": round(pinfo["bytes_per_iteration"] / (ms_mv / 1e3) / 1e9, 2), "kernel": pinfo["kernel"]}
    ps.close()
    if not no_cpu:
        from oracle import oracle as O
        t = time.perf_counter()
        O.shifted_triu_csr(rp, ci, v, sigma, x0, 3, -1.0)
        dc = (time.perf_counter() - t) / 3
        out["cpu_end_to_end_seconds"] = round(dc * res.iterations, 3)
        out["cpu_baseline"] = {"value": round(dc * 1e3, 2), "unit": "ms/iteration", "cores": 1, "kind": "port",
                               "sample": "same matrix, 3 iterations of the reference loop with a CSR triangular "
                                         "solve + CSC product (oracle, 1 thread); the reference itself refactors "
                                         "with SparseLU every iteration (slower still)"}
    A.close()
    return out


def run_config5_general(E, S, ctx, torch, stream):
    """Config 5's matrix made non-triangular (synthetic.general_complex; eigenvalues = diagonal):
    the general-sparse shifted inverse on the device: GMRES over the exact
    sparse LU of A - sigma I (complete fill, ~1.4 x nnz here; a direct solve checked by its true
    residual), or over ILU(0) where the fill would exceed 3 x nnz.  solve_seconds is the converged
    run's wall clock (session begin to finish, incl. the eigenvector download); ms_per_iteration is
    the steady state, HIP events around 10 host-driven iterations."""
    n = 1_000_000
    rp, ci, v, _ = S.general_complex(n, 16)
    target = 1.5 * np.exp(0.7j)
    sigma = target + 1e-3
    x0 = S.start_vector(n, np.complex128)
    A = E.CsrMatrix(ctx, rp, ci, v, (n, n))
    t = time.perf_counter()
    sess = E.ShiftedSession(A, sigma)
    t_factor = time.perf_counter() - t
    sess.begin(E.ShiftedSolverOptions(1000, 1e-12, sigma), x0)
    t = time.perf_counter()
    done, launches = False, 0
    while not done:
        sess.step(1)
        done, launches = sess.query()
    res = sess.finish()
    t_solve = time.perf_counter() - t
    info = sess.kernel_info()
    sess.begin(E.ShiftedSolverOptions(2**31 - 1, -1.0, sigma), x0)
    sess.step(2)
    torch.cuda.synchronize()
    ms = _events(torch, stream, lambda: sess.step(10)) / 10
    out = {"ms_per_iteration": round(ms, 3), "iterations": res.iterations,
           "converged": res.converged, "abs_error_vs_planted_eigenvalue": float(abs(res.eigenvalue - target)),
           "gmres_steps_last_solve": info["tiles"],
           "last_solve_algorithmic_GB": round(info["bytes_per_iteration"] / 1e9, 3),
           "kernel": info["kernel"], "factor_seconds": round(t_factor, 3), "solve_seconds": round(t_solve, 3),
           "nnz": int(len(ci))}
    sess.close()
    A.close()
    return out


DUMP_MAX_ENTRIES = 4_000_000   # float64 entries of the iterate over all ranks (32 MB of the 64 MB cap)
DUMP_SEED = 20251226


def dump_outputs(path, res, rank, world):
    """--dump-outputs: what a caller of the timed path receives after its last step (the session's
    finish(): Rayleigh-quotient estimate, iteration count, normalised iterate), as float64 .npy
    files.  Every rank writes its own row block of the iterate (eigenvector.npy at N = 1, else
    eigenvector_rank<r>.npy); a block above its share of DUMP_MAX_ENTRIES is written as the entries
    at a sorted index sample drawn from default_rng([DUMP_SEED, rank]), the same from run to run."""
    os.makedirs(path, exist_ok=True)
    x = np.asarray(res.eigenvector, dtype=np.float64)
    cap = max(1, DUMP_MAX_ENTRIES // world)
    if x.size > cap:
        idx = np.sort(np.random.default_rng([DUMP_SEED, rank]).choice(x.size, size=cap, replace=False))
        x = x[idx]
    np.save(os.path.join(path, "eigenvector.npy" if world == 1 else f"eigenvector_rank{rank}.npy"), x)
    if rank == 0:
        np.save(os.path.join(path, "eigenvalue.npy"), np.array([float(res.eigenvalue)], dtype=np.float64))
        np.save(os.path.join(path, "iterations.npy"), np.array([float(res.iterations)], dtype=np.float64))


def launcher_cmd(argv, n, port, python=None):
    """The child command that starts N ranks of this script, one per GPU of this node (the
    contract's own form: torch.distributed.run over 127.0.0.1, arguments forwarded unchanged)."""
    return [python or sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={n}",
            "--master-addr", "127.0.0.1", f"--master-port={port}", os.path.abspath(__file__)] + list(argv)


def launch_ranks(argv, n, cmd=None):
    """`python bench.py --gpus N` with N > 1 outside torch.distributed.run: start the N ranks as a
    CHILD process (never exec: nothing here has imported torch or touched a GPU), relay rank 0's
    JSON line to stdout and everything else to stderr as it arrives, and return the child's exit
    code."""
    import socket
    import subprocess
    if cmd is None:
        with socket.socket(socket.AF_INET, socket.SOCK_STREAM) as s:
            s.bind(("127.0.0.1", 0))
            port = s.getsockname()[1]
        cmd = launcher_cmd(argv, n, port)
    env = dict(os.environ)
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")   # dmabuf IPC only on this host driver
    p = subprocess.Popen(cmd, stdout=subprocess.PIPE, env=env, text=True, bufsize=1)
    for line in p.stdout:
        s = line.strip()
        if s.startswith("{") and '"metric"' in s:
            print(s, flush=True)
        else:
            sys.stderr.write(line)
            sys.stderr.flush()
    return p.wait()


def main():
    args = parse()
    if "WORLD_SIZE" not in os.environ and args.gpus > 1:
        raise SystemExit(launch_ranks(sys.argv[1:], args.gpus))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    import torch
    import torch.distributed as dist

    if world > 1:
        dist.init_process_group("gloo")
    devs = device_map(world, int(os.environ.get("LOCAL_WORLD_SIZE", world)))
    device = devs[local_rank]
    shared = len(set(devs)) < len(devs)
    bootstrap = args.bootstrap
    if bootstrap == "auto":
        bootstrap = "host" if shared else "rccl"
    if world > 1 and shared and bootstrap == "rccl" and os.environ.get("EIGSOL_BENCH_FORCE_RCCL") != "1":
        # (EIGSOL_BENCH_FORCE_RCCL=1, tests only: let RCCL refuse them, exercising the host fallback)
        raise SystemExit("--bootstrap rccl with ranks sharing a GPU: RCCL refuses duplicate devices")
    torch.cuda.set_device(device)

    import pcsc_eigenvalue_solver_project_amd as E
    from pcsc_eigenvalue_solver_project_amd import synthetic as S

    kind, rows_cfg, k = WORKLOADS[args.workload]
    if args.scaling == "strong":
        n_global = rows_cfg
        rb = np.linspace(0, n_global, world + 1).astype(np.int64)
    else:
        n_global = rows_cfg * world
        rb = np.arange(world + 1, dtype=np.int64) * rows_cfg
    row0, rows = int(rb[rank]), int(rb[rank + 1] - rb[rank])
    # A dedicated (non-default) torch stream: the library's work and torch's timing events share it.
    torch_stream = torch.cuda.Stream()
    torch.cuda.set_stream(torch_stream)
    rp, ci, v = gen(kind, n_global, k, row0, rows)
    if world > 1:
        from pcsc_eigenvalue_solver_project_amd import dist as D
        ctx = None
        if bootstrap == "rccl":
            # one communicator per rank owned by the library (RCCL over xGMI); gloo only ships the id
            try:
                ctx = D.torch_dist_context(device, stream=torch_stream.cuda_stream)
            except E.EigSolError as e:
                sys.stderr.write(f"[bench] rank {rank}: RCCL bootstrap failed ({e}); trying the host bootstrap\n")
            # every rank takes the same bootstrap: RCCL only where all of them have a communicator
            ok = torch.tensor([1 if ctx is not None else 0], dtype=torch.int32)
            dist.all_reduce(ok, op=dist.ReduceOp.MIN)
            if int(ok[0]) == 0:
                if ctx is not None:
                    ctx.close()
                ctx = None
                bootstrap = "host (RCCL bootstrap failed)"
        if ctx is None:
            # set-up all-gathers over gloo; the exchange itself is the same device-side peer push
            ctx = D.torch_host_context(device, stream=torch_stream.cuda_stream)
        A = D.DistCsrMatrix(ctx, rb, rp, ci, v)
        sess = E.PowerSession(A)
    else:
        ctx = E.Context(device, stream=torch_stream.cuda_stream)
        A = E.CsrMatrix(ctx, rp, ci, v, (rows, rows))
        sess = E.PowerSession(A)
    nnz = len(ci)
    del rp, ci, v
    x0 = S.start_vector(rows, np.float64, row0=row0)
    transport = sess.transport()
    opts = E.SolverOptions(2**31 - 1, -1.0)   # tol < 0: the reference loop never stops early
    # --dump-outputs: finish() hands out results only once the reference loop has ended, so its
    # iteration budget is set to end with the last timed launch: reference iteration k completes
    # with launch k + 1 (its second product is the next iteration's first), so W + K launches are
    # W + K - 1 iterations; the launches themselves are the same, and the one after them only decides
    head_opts = E.SolverOptions(max(1, args.warmup + args.steps - 1), -1.0) if args.dump_outputs else opts

    def warm(s):
        s.begin(head_opts, x0)
        s.step(args.warmup)
        torch.cuda.synchronize()
        s.query()   # raises on a peer-wait fault (bounded waits: every rank gets here)

    werr = None
    try:
        warm(sess)
    except E.EigSolError as e:
        werr = e
    if world > 1:
        # a device-side peer exchange that does not work between these GPUs (every wait is bounded,
        # so all ranks return): all ranks rebuild the session on RCCL's collective exchange together
        okt = torch.tensor([0 if werr is not None else 1], dtype=torch.int32)
        dist.all_reduce(okt, op=dist.ReduceOp.MIN)
        if int(okt[0]) == 0 and transport == 2 and bootstrap == "rccl":
            sys.stderr.write(f"[bench] rank {rank}: peer exchange failed in the warm-up ({werr}); "
                             "rebuilding the session on the collective transport\n")
            sess.close()
            os.environ["EIGSOL_DIST_TRANSPORT"] = "collective"
            sess = E.PowerSession(A)
            transport = sess.transport()
            bootstrap = "rccl (peer exchange failed: collective transport)"
            warm(sess)
        elif int(okt[0]) == 0:
            raise werr if werr is not None else SystemExit("another rank failed its warm-up")
    elif werr is not None:
        raise werr
    info = sess.kernel_info()
    kname = sess.kernel_name()
    if world > 1:
        dist.barrier()
    torch.cuda.synchronize()
    ev0 = torch.cuda.Event(enable_timing=True)
    ev1 = torch.cuda.Event(enable_timing=True)
    t0 = time.perf_counter()
    ev0.record(torch_stream)
    sess.step(args.steps)
    ev1.record(torch_stream)
    torch.cuda.synchronize()
    t1 = time.perf_counter()
    if world > 1:
        dist.barrier()
    elapsed = t1 - t0
    ev_ms = ev0.elapsed_time(ev1)
    done, launches = sess.query()
    assert not done, "tol < 0 must never terminate"
    el = torch.tensor([elapsed, ev_ms / 1e3], dtype=torch.float64)
    tot = torch.tensor([info["bytes_per_iteration"], float(nnz)], dtype=torch.float64)
    if world > 1:
        dist.all_reduce(el, op=dist.ReduceOp.MAX)
        dist.all_reduce(tot, op=dist.ReduceOp.SUM)
    elapsed_max, ev_max = float(el[0]), float(el[1])
    transport_names = {0: "none", 1: "collective", 2: "peer"}
    transports = [transport_names[transport]]
    if world > 1:
        transports = [None] * world
        dist.all_gather_object(transports, transport_names[transport])
    if args.dump_outputs:
        # untimed: the state the timed steps left (every rank downloads its own row block); one more
        # launch sees the budget used up and ends the loop without iterating (a run of fewer than
        # two launches in all is topped up to the one iteration a result needs)
        for _ in range(3):
            sess.step(1)
            if sess.query()[0]:
                break
        else:
            raise SystemExit("--dump-outputs: the loop did not end after the timed steps")
        dump_outputs(args.dump_outputs, sess.finish(), rank, world)
    check = None
    if args.check:
        # untimed: the same session run to convergence (every rank takes part: the exchange is per
        # iteration); lambda of every rank gathered so the line shows they are bitwise identical
        sess.begin(E.SolverOptions(300, 1e-12), x0)
        done = False
        while not done:
            sess.step(16)
            done = sess.query()[0]
        res = sess.finish()
        mine = [float(res.eigenvalue), int(res.iterations), bool(res.converged)]
        per_rank = [mine]
        if world > 1:
            per_rank = [None] * world
            dist.all_gather_object(per_rank, mine)
        check = {"eigenvalue": per_rank[0][0], "iterations": per_rank[0][1], "converged": per_rank[0][2],
                 "tolerance": 1e-12, "max_iterations": 300,
                 "ranks_bitwise_equal": all(p == per_rank[0] for p in per_rank),
                 "eigenvector_norm2_rank0": float(np.linalg.norm(res.eigenvector))}

    bytes_iter = info["bytes_per_iteration"]          # this rank's algorithmic bytes
    total_bytes = float(tot[0]) * args.steps          # all ranks' blocks
    value = total_bytes / elapsed_max / 1e9
    achieved = bytes_iter / (ev_ms / 1e3 / args.steps) / 1e9

    out = None
    if rank == 0:
        out = {
            "metric": METRIC,
            "value": round(value, 2),
            "unit": "GB/s",
            "n_gpus": world,
            "steps": args.steps,
            "warmup": args.warmup,
            "ms_per_step": round(1e3 * elapsed_max / args.steps, 4),
            "higher_is_better": True,
            "scaling": args.scaling,
            "vs_baseline": None,
            "dtype": "f64",
            "data": "synthetic (seeded generators of SURVEY §8d; x0 seed 7)",
            "config": {
                "workload": (f"power_method CSR {args.workload}: one {n_global}x{n_global} matrix, {k} nnz/row "
                             f"({kind} columns), split into {world} row blocks of ~{rows} rows"
                             if args.scaling == "strong" else
                             f"power_method CSR {args.workload}: {rows} rows x {k} nnz/row per GPU "
                             f"({kind} columns), global {n_global}x{n_global} (weak scaling)"),
                "rows_per_gpu": rows,
                "nnz_per_gpu": nnz,
                "nnz_global": int(tot[1]),
                "n_global": n_global,
                "parallelism": f"row-block x{world}" if world > 1 else "single GPU",
                "exchange": {0: "none (one GPU)", 1: "collective (pack kernel + RCCL group per iteration)",
                             2: "peer (SpMV epilogue stores halo + partial into the peers' IPC inboxes, "
                                "epoch flags, no host round trip)"}[transport],
                "bytes_per_iteration_per_gpu": bytes_iter,
                "grid_blocks": info["grid"],
                "row_tiles": info["tiles"],
            },
            "roofline": {
                "bound": "hbm",
                "kernel": kname or info["kernel"],
                "kernel_role": info["kernel"] + ", fused power iteration",
                "achieved": round(achieved, 2),
                "peak": HBM_PEAK_GBS,
                "unit": "GB/s",
                "frac": round(achieved / HBM_PEAK_GBS, 4),
                "traffic": None,
                "event_ms_per_launch": round(ev_ms / args.steps, 5),
                "algorithmic_bytes_per_launch": bytes_iter,
            },
            "cpu_baseline": None,
        }
        if check is not None:
            out["check"] = check
        out["config"]["bootstrap"] = bootstrap if world > 1 else "none"
        out["config"]["devices"] = devs if world > 1 else [device]
    if rank == 0:
        pmc = pmc_traffic(args.workload, kname)
        if pmc:
            t = pmc["hbm_traffic_bytes_per_launch"]
            out["roofline"]["traffic"] = t
            out["roofline"]["traffic_source"] = pmc["source"]
            out["roofline"]["traffic_kernel"] = pmc["kernel"]
            # frac is EFFECTIVE: algorithmic bytes count int32 columns, the sliced layout
            # streams 8-bit window offsets; frac_dram is what the DRAM actually moved per launch
            out["roofline"]["frac_basis"] = (
                "effective: algorithmic CSR bytes (12 B per f64 nonzero with an int32 column, SURVEY §8d) / kernel "
                "time; the shipped slices stream 8-bit column offsets, so fewer bytes reach DRAM — frac_dram is the "
                "PMC traffic (FETCH_SIZE x 2 + WRITE_SIZE, profiles/) / the same kernel time / 8 TB/s")
            out["roofline"]["frac_dram"] = round(t / (ev_ms / 1e3 / args.steps) / 1e9 / HBM_PEAK_GBS, 4)
    if rank == 0:
        import ctypes as C
        dv, rk, nr, ck = C.c_int(), C.c_int(), C.c_int(), C.c_int()
        if E.lib().eigsol_ctx_info(ctx.handle, C.byref(dv), C.byref(rk), C.byref(nr), C.byref(ck)) == 0:
            out["config"]["communicator"] = {
                "library_ranks": nr.value, "library_rank": rk.value, "transport_per_rank": transports,
                "kind": {0: "none (one GPU)", 1: "RCCL communicator", 2: "loopback", 3: "host all-gather + peer inboxes"}[ck.value],
                "note": "from eigsol_ctx_info: the ranks the library itself exchanges with (no 8-GPU run of "
                        "this line has been recorded by the builder; the driver's SCALE record is the measurement)"}
    if args.full and world == 1 and rank == 0:
        out["roofline"]["measured_hbm"] = measured_hbm(torch, torch_stream, ctx)
        t = out["roofline"].get("traffic")
        kr = out["roofline"]["measured_hbm"].get("kernel_read_GBps")
        if t and kr:
            actual = t / (ev_ms / 1e3 / args.steps) / 1e9
            out["roofline"]["actual_dram_GBps"] = round(actual, 1)
            out["roofline"]["actual_over_kernel_read_ceiling"] = round(actual / kr, 4)
            km = out["roofline"]["measured_hbm"].get("kernel_mix12_GBps")
            if km:
                out["roofline"]["actual_over_kernel_mix12_ceiling"] = round(actual / km, 4)
    if args.full and not args.no_extras and world == 1:
        out["extras"] = {
            "config3_csr_1Mx16": run_config3(E, S, ctx, torch, torch_stream, opts),
            "config4_uniform10m": run_uniform10m(E, S, ctx, torch, torch_stream, opts),
            "band10m_float32": run_single_band10m(E, S, ctx, torch, torch_stream),
            "long_double_band1m": run_long_double_power(E, S, ctx, torch),
            "config1_A_txt": run_config1(E, S, ctx),
            "config2_qr_4096": run_config2(E, ctx, args.no_cpu_baseline),
            "qr_complex_1024": run_qr_complex(E, ctx, args.no_cpu_baseline),
            "qr_complex_4096": run_qr_complex(E, ctx, args.no_cpu_baseline, 4096),
            "config5_shifted_inverse_1M": run_config5(E, S, ctx, torch, torch_stream, args.no_cpu_baseline),
            "config5_general_sparse_1M": run_config5_general(E, S, ctx, torch, torch_stream),
            "config5_convdiff_1M": run_config5_convdiff(E, S, ctx, torch, torch_stream),
            "dense_power_16384": run_dense_power(E, S, ctx, torch, torch_stream),
        }
    sess.close()
    A.close()
    ctx.close()
    if rank == 0:
        if args.full and world == 1 and not args.no_cpu_baseline:
            mat = gen(kind, n_global, k, 0, n_global)
            out["cpu_baseline"] = cpu_baseline(kind, k, args.cpu_seconds, n_global, mat)
            out["cpu_baseline"]["host"] = host_cpu()
            out["cpu_allcores"] = cpu_allcores(kind, k, min(args.cpu_seconds, 10.0), n_global, mat)
            del mat
        print(json.dumps(out), flush=True)
    if world > 1:
        dist.barrier()
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
