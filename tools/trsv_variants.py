"""Config-5 triangular solve under factor-time knobs: one line per variant.

usage: python tools/trsv_variants.py 'EIGSOL_TRSV_HEAD=block' 'EIGSOL_TRSV_TWO=0' ...
(each argument is a space-separated list of VAR=value applied before the factor is built)."""
import json, os, sys
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch
import pcsc_eigenvalue_solver_project_amd as E
from pcsc_eigenvalue_solver_project_amd import synthetic as S

st = torch.cuda.Stream()
torch.cuda.set_stream(st)
ctx = E.Context(0, stream=st.cuda_stream)
n = int(os.environ.get("TRSV_N", 1_000_000))
rp, ci, v, _ = S.triu_complex(n, 16)
target = 1.5 * np.exp(0.7j)
M = E.CsrMatrix(ctx, rp, ci, v, (n, n))
x0 = S.start_vector(n, np.complex128)
for spec in (sys.argv[1:] or [""]):
    saved = dict(os.environ)
    for kv in spec.split():
        k, val = kv.split("=", 1)
        os.environ[k] = val
    s = E.ShiftedSession(M, target + 1e-3)
    s.begin(E.ShiftedSolverOptions(2**31 - 1, -1.0, target + 1e-3), x0)
    s.step(3)
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    steps = 20
    e0.record(st)
    s.step(steps)
    e1.record(st)
    torch.cuda.synchronize()
    ms = e0.elapsed_time(e1) / (steps * s.kernel_info()["iterations_per_launch"])
    s.close()
    r = E.shifted_inverse_power_method(M, E.ShiftedSolverOptions(100, 1e-12, target + 1e-3), x0)
    print(json.dumps({"variant": spec or "default", "ms": round(ms, 4), "lambda_err": abs(r.eigenvalue - target),
                      "iters": r.iterations, "converged": r.converged}), flush=True)
    os.environ.clear()
    os.environ.update(saved)
M.close()
ctx.close()
