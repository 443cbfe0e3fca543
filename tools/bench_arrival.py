"""Cost of the on-device arrival-cost update (tools only): one BatchSolver.arrival call
beside one Gauss-Newton iteration and one single-query BatchSolver.covariance of the same
build at the same shape, every trajectory with its own prior weight.

    python tools/bench_arrival.py [C2|C3] [B] [reps]

HIP events around the calls, inputs resident on the device, one warm-up call of each kind
first; arrival and covariance are timed as the median of `reps` calls, the GN iteration by
differencing a (k + 1)-iteration and a 1-iteration solve with tol = 0, as tools/bench_cov.py
does.  An arrival call is the single-query covariance plus an n^3 step per trajectory
(k_arrival: one wavefront each), so the figure to hold it against is this build's own
single-query covariance time: an excess beyond the spread of the repetitions points at
k_arrival.  One JSON line, stamped with the library's digest (appended to
profiles/arrival_cost.jsonl by the caller).
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
reps = int(sys.argv[3]) if len(sys.argv) > 3 else 7
K_IT = 10 if cfg == "C2" else 3
w = configs.CONFIGS[cfg](B=B)
n = w.n
# a prior per trajectory: Pw_b = d S_b d, S_b = G_b G_b^T / n + I / 2, around the initial state
rng = np.random.default_rng(7)
G = rng.normal(size=(B, n, n))
d = np.sqrt(np.array([10.0, 10.0] if n == 2 else [1e-2, 1e-2, 1e-2, 1e-2, 1.0]))
S = G @ np.swapaxes(G, 1, 2) / n + 0.5 * np.eye(n)
S = 0.5 * (S + np.swapaxes(S, 1, 2))
w.Pw = np.zeros((n, n))  # the constants carry no prior weight: it travels per solve
s = solver.from_workload(w)
dev = s.device
Pw = torch.as_tensor(d[None, :, None] * S * d[None, None, :], device=dev)
x0 = torch.as_tensor(w.X_init[:, 0] + 0.1 * rng.normal(size=(B, n)), device=dev)
X = torch.as_tensor(w.X_init, device=dev)
U = torch.as_tensor(w.U, device=dev)
Y = torch.as_tensor(w.Y, device=dev)
PAR = None if w.PAR is None else torch.as_tensor(w.PAR, device=dev)
phi = torch.as_tensor(w.cpm.lagrange_matrix(np.array([0.25 * w.T])), device=dev)
e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)


def timed(f):
    e0.record()
    out = f()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1), out


def solve(k):
    return s.solve(X, U, Y, PAR, x0, max_iter=k, tol=0.0, Pw=Pw)


def median(f):
    timed(f)  # warm-up (allocations, first launch)
    ts = sorted(timed(f)[0] for _ in range(reps))
    return ts[len(ts) // 2], [ts[0], ts[-1]]


_, out = timed(lambda: solve(1))
X1 = out[0]
t1 = min(timed(lambda: solve(1))[0] for _ in range(3))
tk = min(timed(lambda: solve(K_IT + 1))[0] for _ in range(3))
ms_iter = (tk - t1) / K_IT

cov = lambda: s.covariance(X1, U, Y, PAR, x0, Phi=phi, Pw=Pw)  # noqa: E731
arr = lambda: s.arrival(X1, U, Y, PAR, x0, Phi=phi, Pw=Pw)  # noqa: E731
ms_cov, cov_mm = median(cov)
ms_arr, arr_mm = median(arr)
ms_cov2, cov2_mm = median(cov)  # the covariance again after the arrival calls: its own drift
st = arr()[2]
torch.cuda.synchronize()
res = {"config": cfg, "workload": w.name, "B": B, "d": w.P * n, "lib": _lib.lib_digest(),
       "large_system": bool(s.large_system), "ms_per_gn_iter": ms_iter, "gn_iters_differenced": K_IT, "reps": reps,
       "ms_cov_1q": ms_cov, "ms_cov_1q_min_max": cov_mm, "ms_cov_1q_again": ms_cov2, "ms_cov_1q_again_min_max": cov2_mm,
       "ms_arrival": ms_arr, "ms_arrival_min_max": arr_mm, "arrival_minus_cov_ms": ms_arr - 0.5 * (ms_cov + ms_cov2),
       "arrival_in_gn_iters": ms_arr / ms_iter, "status": sorted(set(st.cpu().numpy().tolist())),
       "note": "host-side Pw symmetry check (one device reduction and sync per call) is inside all three timings"}
print(json.dumps(res))
