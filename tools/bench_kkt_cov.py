"""Cost of the covariance of mixed-row / bordered problems (tools only): mhe_kkt_cov through
BatchSolver.covariance with 1 and 4 queries, beside one Gauss-Newton iteration of the same
build at the same shape -- tools/bench_cov.py's method on the general problems.

    python tools/bench_kkt_cov.py [two_rx|two_rx_noeq|C5s] [B] [reps] [N]

two_rx: the two-receiver problem of tests/general_problems.py at the script's order N = 10
with the script's range / heading rate (51 + 51 rows, 6 GNSS epochs of 16 rows: M = 198),
zA = zB at every node (K = 11); eight seeded trajectories tiled to B.  two_rx_noeq: the same
without the equality rows (K = 0, k_big_cov).  C5s: mhe.configs.make_c5_small (n = 8, three
extra variables) at N (default 40).

HIP events around the calls, inputs resident on the device, one warm-up call of each kind.
The covariance: median, min and max of `reps` calls.  The GN iteration: a (k + 1)-iteration
minus a 1-iteration solve with tol = 0, over k.  A bordered iteration holds the same assembly
and factorization and the border's two-sided sweep; the covariance call sweeps the border and
the query columns forward only and forms the Gram products.  One JSON line, stamped with the
library's digest.
"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "nlp-filter_amd"))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np  # noqa: E402
import torch  # noqa: E402
from mhe import _lib, configs, solver  # noqa: E402

cfg = sys.argv[1] if len(sys.argv) > 1 else "two_rx"
B = int(sys.argv[2]) if len(sys.argv) > 2 else 1024
reps = int(sys.argv[3]) if len(sys.argv) > 3 else 7
K_IT = 4

if cfg in ("two_rx", "two_rx_noeq"):
    from general_problems import two_receiver_problem
    N = int(sys.argv[4]) if len(sys.argv) > 4 else 10
    pb, X0, U, Y, PAR, x0, _ = two_receiver_problem(N=N, B=8, M_range=51, with_eq=cfg == "two_rx")
    tile = lambda a: np.concatenate([a] * (-(-B // 8)))[:B]  # noqa: E731
    X0, U, Y, PAR, x0, Z0 = tile(X0), tile(U), tile(Y), tile(PAR), tile(x0), None
    s = solver.BatchSolver(pb.N, pb.T, pb.dyn, "mixed", pb.D, pb.c, pb.Phi, pb.Qw, pb.Rw, Pw=pb.Pw,
                           eq=pb.eq if pb.eq.size else None)
    name, T, P, n, M = f"two_receiver_N{N}", pb.T, pb.P, pb.n, pb.M
    from oracle import collocation as oc
    rows = lambda t: oc.interp_matrix(N, T, np.asarray(t))  # noqa: E731
else:
    N = int(sys.argv[4]) if len(sys.argv) > 4 else 40
    w = configs.make_c5_small(B=B, N=N)
    s = solver.from_workload(w)
    X0, U, Y, PAR, x0, Z0 = w.X_init, w.U, w.Y, w.PAR, w.x0, w.Z_init
    name, T, P, n, M = w.name + f"_N{N}", w.T, w.P, w.n, w.M
    rows = lambda t: w.cpm.lagrange_matrix(np.asarray(t))  # noqa: E731

dev = s.device
dv = lambda a: None if a is None else torch.as_tensor(np.ascontiguousarray(a), device=dev)  # noqa: E731
X0, U, Y, PAR, x0, Z0 = dv(X0), dv(U), dv(Y), dv(PAR), dv(x0), dv(Z0)
t4 = np.array([0.0, 0.37 * T, T, 0.2 * T])
Phi = {k: dv(rows(t4[:k])) for k in (1, 4)}
e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)


def timed(f):
    e0.record()
    out = f()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1), out


def solve(k):
    return s.solve(X0, U, Y, PAR, x0, max_iter=k, tol=0.0, Z0=Z0)


_, out = timed(lambda: solve(1))  # warm-up; the covariance is formed at the iterate after one step
X1, Z1 = out[0], (out[4] if s.n_extra else None)
t1 = sorted(timed(lambda: solve(1))[0] for _ in range(reps))
tk = sorted(timed(lambda: solve(K_IT + 1))[0] for _ in range(reps))
ms_iter = (tk[len(tk) // 2] - t1[len(t1) // 2]) / K_IT

res = {"config": cfg, "workload": name, "B": B, "d": P * n, "dp": s.dp, "M": M, "K": s.n_extra + s.n_eq,
       "lib": _lib.lib_digest(), "ms_per_gn_iter": ms_iter, "gn_iters_differenced": K_IT,
       "ms_per_gn_iter_min_max": [(tk[0] - t1[-1]) / K_IT, (tk[-1] - t1[0]) / K_IT], "reps": reps}
for k in (1, 4):
    cov = lambda: s.covariance(X1, U, Y, PAR, x0, Phi=Phi[k], Z=Z1)  # noqa: E731
    _, (C, st) = timed(cov)  # warm-up (allocations, first launch)
    ts = sorted(timed(cov)[0] for _ in range(reps))
    res[f"ms_cov_{k}q"] = ts[len(ts) // 2]
    res[f"ms_cov_{k}q_min_max"] = [ts[0], ts[-1]]
    res[f"cov_{k}q_in_gn_iters"] = ts[len(ts) // 2] / ms_iter
    res[f"status_{k}q"] = sorted(set(st.cpu().numpy().tolist()))
print(json.dumps(res))
