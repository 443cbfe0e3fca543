"""Cost of a Gauss-Newton iteration of a small general problem on the fused single-launch
kernel (BatchSolver(fused_general=True), k_gn_general) beside the default (large-system) path
of the same build at the same shape (tools only).

    python tools/bench_fused_general.py [two_rx|multi] [B] [reps] [N]

two_rx: gnss-multi-receiver.py's window -- N = 10, range and heading rows at 10 Hz (51 + 51),
6 GNSS epochs of 10 satellite slots for each receiver (M = 222, 51 epochs), zA = zB at every
node (K = 11) -- with seeded satellites and a seeded truth; eight trajectories tiled to B.
multi: tests/general_problems.multi_receiver_problem at N (default 7; three extra variables).

HIP events around the calls, inputs resident on the device, one warm-up call of each kind and
path.  The two paths alternate inside every repetition.  The GN iteration: a 5-iteration minus
a 1-iteration solve with tol = 0, over 4 (medians; min / max from the extreme pairs).  One JSON
line per path, stamped with the library's digest, and the largest difference of the two paths'
iterates after 5 iterations.
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
from mhe import _lib, solver  # noqa: E402
from oracle import collocation as oc  # noqa: E402
from oracle import gn_general as gg  # noqa: E402
import general_problems as gp  # noqa: E402

cfg = sys.argv[1] if len(sys.argv) > 1 else "two_rx"
B = int(sys.argv[2]) if len(sys.argv) > 2 else 1024
reps = int(sys.argv[3]) if len(sys.argv) > 3 else 7
K_IT = 4


def two_rx_script_window(B0=8, seed=0):
    c = dict(gp.TWO_RX)
    N, T, n, m = c["N"], c["T"], c["n"], c["m"]
    P = N + 1
    rng = np.random.default_rng(seed)
    sats = [rng.normal(size=(c["N_sat"], 3)) * 1.5e7 + np.array([0, 0, 2e7]) for _ in range(6)]
    zero = [np.zeros(c["N_sat"])] * 6
    t, rows, Rw, _ = gp.two_rx_window_rows(c, sats, zero, sats, zero)
    order = np.argsort(t, kind="stable")
    t, rows, Rw = t[order], rows[order], Rw[order]
    Phi = oc.interp_matrix(N, T, t)
    t_nodes = oc.tau2t(oc.nodes(N), 0.0, T)
    xt = np.zeros((B0, P, n))
    for b in range(B0):
        pa, va = rng.normal(size=3) * 30, rng.normal(size=3)
        off = np.array([30.0, -33.0, 0.0])
        for k, tk in enumerate(t_nodes):
            xt[b, k, 0:3], xt[b, k, 5:8] = pa + va * tk, pa + off + va * tk
            xt[b, k, 2] = xt[b, k, 7]
            xt[b, k, 3], xt[b, k, 4] = 1e3 + 0.5 * tk, 0.5
            xt[b, k, 8], xt[b, k, 9] = -2e3 + 0.2 * tk, 0.2
    U = np.zeros((B0, P, m))
    U[:, :, 0:3] = U[:, :, 3:6] = np.array([1.0, 0.5, 0.0])
    Y = np.zeros((B0, len(t), 1))
    for b in range(B0):
        for i in range(len(t)):
            Y[b, i, 0] = gg.mixed_row(rows[i], Phi[i] @ xt[b])[0] + rng.normal() * 0.01
    Qw, Pw = gp.two_rx_weights()
    eq = np.array([[k * n + 2, k * n + 7] for k in range(P)])
    pb = gg.GeneralProblem(N, T, n, m, "gnss_two_receiver", "mixed", oc.diff_matrix(N), (T / 2.0) * oc.quad_weights(N),
                           Phi, Qw, Rw, Pw=Pw, eq=eq)
    x0 = xt[:, 0] + rng.normal(size=(B0, n)) * 0.5
    X0 = xt + rng.normal(size=xt.shape) * 2.0
    return pb, X0, None, U, Y, np.tile(rows[None], (B0, 1, 1)), x0


if cfg == "two_rx":
    pb, X0, Z0, U, Y, PAR, x0 = two_rx_script_window()
    name = "two_receiver_script_window_N10"
else:
    N = int(sys.argv[4]) if len(sys.argv) > 4 else 7
    pb, X0, Z0, U, Y, PAR, _, _ = gp.multi_receiver_problem(N=N, B=8)
    x0 = None
    name = f"multi_receiver_N{N}"
tile = lambda a: None if a is None else np.concatenate([a] * (-(-B // 8)))[:B]  # noqa: E731
X0, Z0, U, Y, PAR, x0 = tile(X0), tile(Z0), tile(U), tile(Y), tile(PAR), tile(x0)

mk = lambda fused: solver.BatchSolver(pb.N, pb.T, pb.dyn, "mixed", pb.D, pb.c, pb.Phi, pb.Qw, pb.Rw, Pw=pb.Pw,  # noqa: E731
                                      n_extra=pb.n_extra, eq=pb.eq if pb.eq.size else None, fused_general=fused)
paths = {"fused": mk(True), "default": mk(False)}
assert paths["fused"].fused_general and paths["default"].large_system
dev = paths["fused"].device
dv = lambda a: None if a is None else torch.as_tensor(np.ascontiguousarray(a), device=dev)  # noqa: E731
X0, Z0, U, Y, PAR, x0 = dv(X0), dv(Z0), dv(U), dv(Y), dv(PAR), dv(x0)
e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)


def timed(s, k):
    e0.record()
    out = s.solve(X0, U, Y, PAR, x0, max_iter=k, tol=0.0, Z0=Z0)
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1), out


X5 = {}
for key, s in paths.items():  # warm-up of each kind
    timed(s, 1)
    X5[key] = timed(s, K_IT + 1)[1][0]
t1, tk = {k: [] for k in paths}, {k: [] for k in paths}
for _ in range(reps):
    for key, s in paths.items():  # alternating
        t1[key].append(timed(s, 1)[0])
        tk[key].append(timed(s, K_IT + 1)[0])
diff = float((X5["fused"] - X5["default"]).abs().max())
med = lambda v: sorted(v)[len(v) // 2]  # noqa: E731
for key, s in paths.items():
    a, b = sorted(t1[key]), sorted(tk[key])
    buf = __import__("ctypes").create_string_buffer(256)
    s.lib.mhe_solve_kernel_name(s.dims, B, None, buf, 256)
    print(json.dumps({
        "config": cfg, "workload": name, "path": key, "B": B, "d": pb.P * pb.n, "dp": s.dp, "M": pb.M,
        "K": s.n_extra + s.n_eq, "lib": _lib.lib_digest(), "ms_per_gn_iter": (med(b) - med(a)) / K_IT,
        "ms_per_gn_iter_min_max": [(b[0] - a[-1]) / K_IT, (b[-1] - a[0]) / K_IT],
        "ms_solve_1_iter": med(a), "ms_solve_1_iter_min_max": [a[0], a[-1]],
        "ms_solve_5_iter": med(b), "ms_solve_5_iter_min_max": [b[0], b[-1]],
        "gn_iters_differenced": K_IT, "reps": reps, "max_abs_diff_X_vs_other_path_5_iters": diff,
        "kernel": buf.value.decode()}))
