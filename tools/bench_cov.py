"""Cost of the covariance at query times (tools only): BatchSolver.covariance with one
query and with 8 queries, beside one Gauss-Newton iteration of the same build at the
same shape.

    python tools/bench_cov.py [C2|C3] [B] [reps]

HIP events around the calls, inputs resident on the device, one warm-up call of each
kind first.  The covariance is timed as the median of `reps` calls; the GN iteration by
differencing a (k + 1)-iteration and a 1-iteration solve with tol = 0 (same staging, same
epilogue), as tools/bench_big.py does.  The work of a covariance call is one assembly,
one factorization and the forward sweep of the query panels -- no back substitution --
so a figure above roughly two iterations points at the sweep.  One JSON line, stamped
with the library's digest.
"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "nlp-filter_amd"))
import numpy as np  # noqa: E402
import torch  # noqa: E402
from mhe import _lib, configs, solver  # noqa: E402

cfg = sys.argv[1] if len(sys.argv) > 1 else "C2"
B = int(sys.argv[2]) if len(sys.argv) > 2 else {"C2": 1024, "C3": 4096}[cfg]
reps = int(sys.argv[3]) if len(sys.argv) > 3 else 5
K_IT = 10 if cfg == "C2" else 3
w = configs.CONFIGS[cfg](B=B)
s = solver.from_workload(w)
dev = s.device
X = torch.as_tensor(w.X_init, device=dev)
U = torch.as_tensor(w.U, device=dev)
Y = torch.as_tensor(w.Y, device=dev)
PAR = None if w.PAR is None else torch.as_tensor(w.PAR, device=dev)
nodes = w.cpm.tau2t(w.cpm.tau)
t8 = np.concatenate([[0.0, 0.37 * w.T, w.T, nodes[len(nodes) // 2]], np.linspace(0.1, 0.9, 4) * w.T])
Phi = {k: torch.as_tensor(w.cpm.lagrange_matrix(t8[:k]), device=dev) for k in (1, 8)}
e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)


def timed(f):
    e0.record()
    out = f()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1), out


def solve(k):
    return s.solve(X, U, Y, PAR, max_iter=k, tol=0.0)


# one GN iteration of this build: the point of the covariance calls is the iterate after it
_, out = timed(lambda: solve(1))
X1 = out[0]
t1 = min(timed(lambda: solve(1))[0] for _ in range(3))
tk = min(timed(lambda: solve(K_IT + 1))[0] for _ in range(3))
ms_iter = (tk - t1) / K_IT

res = {"config": cfg, "workload": w.name, "B": B, "d": w.P * w.n, "lib": _lib.lib_digest(),
       "large_system": bool(s.large_system), "ms_per_gn_iter": ms_iter, "gn_iters_differenced": K_IT, "reps": reps}
for k in (1, 8):
    cov = lambda: s.covariance(X1, U, Y, PAR, Phi=Phi[k])  # noqa: E731
    _, (C, st) = timed(cov)  # warm-up (allocations, first launch)
    ts = sorted(timed(cov)[0] for _ in range(reps))
    res[f"ms_cov_{k}q"] = ts[len(ts) // 2]
    res[f"ms_cov_{k}q_min_max"] = [ts[0], ts[-1]]
    res[f"cov_{k}q_in_gn_iters"] = ts[len(ts) // 2] / ms_iter
    res[f"status_{k}q"] = sorted(set(st.cpu().numpy().tolist()))
    res[f"scratch_gib_{k}q"] = s.lib.mhe_cov_scratch_bytes(s.dims, s._chunk(B, torch.cuda.current_stream()), k) / 2 ** 30
print(json.dumps(res))
