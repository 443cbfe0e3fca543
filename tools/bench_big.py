"""Large-system path timing (tools only): C3 / C4 / C5 shapes of BASELINE.json.

    python tools/bench_big.py [C3|C4|C5] [B] [iters] [meas_delta]

meas_delta (optional, a scale in the rows' units): the same solve with pseudo-Huber
measurement rows (mhe_solve_args.meas_delta, one shared (M,) array) -- the cost of the
per-row reweighting against the run without it.

GN collocation-point updates/s = B * P * iters / device time (HIP events around one
mhe_solve call with tol = 0, inputs resident; a batch whose workspace exceeds the free
HBM is streamed through one workspace in chunks), and the algorithmic FP64 rate by
SURVEY.md §8(d)'s count per trajectory-iteration:
    F = d^3/3 + 2 d^2 + sum_e P^2 nnz(G_e) + 2 P^2 n^2 + 4 P n^3
(nnz(G_e): the component pairs the epoch's unmasked rows couple).  The split
factorization skips the tiles outside the factor's envelope (mhe_big_envelope: each tile
row's first nonzero tile column, from the component pairs the assembled H couples), so the
executed count replaces d^3/3 by the envelope's share of it -- the tile-level left-looking
count on the envelope over the same count dense -- and the line carries both bases
(executed_*: what ran; achieved_tflops / frac_fp64_peak: the §8(d) dense count, which
exceeds the peak where the envelope is narrow, C5).
"""
import ctypes
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "nlp-filter_amd"))
import numpy as np  # noqa: E402
import torch  # noqa: E402
from mhe import configs, solver  # noqa: E402

cfg = sys.argv[1] if len(sys.argv) > 1 else "C3"
B = int(sys.argv[2]) if len(sys.argv) > 2 else 256
it = int(sys.argv[3]) if len(sys.argv) > 3 else 3
meas_delta = float(sys.argv[4]) if len(sys.argv) > 4 else None
w = configs.CONFIGS[cfg](B=B)
s = solver.from_workload(w)
P, n = w.P, w.n
d = P * n
E = np.unique(w.t_meas).shape[0]


def nnz_g_sum():
    """sum over epochs of nnz(G_e): the (a, b) component pairs some unmasked row of the
    epoch couples (pseudorange: x, y, z, b; mixed rows: the row's state indices)."""
    t, Rw = w.t_meas, np.asarray(w.Rw).reshape(len(w.t_meas), -1)
    total = 0
    for te in np.unique(t):
        pairs = set()
        for i in np.nonzero(t == te)[0]:
            if not np.any(Rw[i]):
                continue
            if w.meas == "mixed":
                ids = [int(v) for v in w.PAR[0, i, 1:8] if 0 <= v < n]
            elif w.meas == "pseudorange":
                ids = list(w.meas_static["idx"])
            else:
                ids = list(range(n))
            pairs |= {(a, b) for a in ids for b in ids}
        total += len(pairs)
    return total


F = d ** 3 / 3 + 2 * d * d + nnz_g_sum() * P * P + 2 * P * P * n * n + 4 * P * n ** 3
Z0 = getattr(w, "Z_init", None)
KW = {} if meas_delta is None else {"meas_delta": torch.full((w.M,), meas_delta, dtype=torch.float64, device=s.device)}


def run(k):
    return s.solve(w.X_init, w.U, w.Y, w.PAR, max_iter=k, tol=0.0, Z0=Z0, **KW)


run(1)
torch.cuda.synchronize()
e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
# inputs are staged inside solve() before the first launch; time the GN launches only
# by differencing an iters-long and a 1-iteration solve (same staging, same epilogue)
e0.record(); run(1); e1.record(); torch.cuda.synchronize(); t1 = e0.elapsed_time(e1)
e0.record(); out = run(it + 1); e1.record(); torch.cuda.synchronize(); tk = e0.elapsed_time(e1)
dt = (tk - t1) / 1e3
st = out[3].cpu().numpy()


def chol_tile_count(f):
    """Left-looking tile Cholesky on an envelope f (first nonzero tile column per tile row):
    per off-diagonal tile (I, J) its updates over k in [max(f_I, f_J), J) and its TRSM, per
    diagonal tile its updates over [f_I, I) and its panel, in 16^3 units."""
    f = np.asarray(f, dtype=np.int64)
    tot = 0.0
    for i in range(f.shape[0]):
        j = np.arange(f[i], i)
        tot += 2.0 * np.maximum(j - np.maximum(f[i], f[j]), 0).sum() + j.shape[0] + (i - f[i]) + 1.0 / 3.0
    return tot


def envelope_share():
    """Executed share of the dense factorization (1.0 when the build has no envelope)."""
    NT = s.lib.mhe_padded_dim(s.dims) // 16
    fc = (ctypes.c_int32 * NT)()
    ws = list(s._ws.values())[-1]
    nb = ws.numel()
    rc = s.lib.mhe_big_envelope(s.dims, ctypes.c_void_p(ws.data_ptr()), nb, 0, fc, NT,
                                ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    if rc < 0:
        return 1.0, None
    f = np.array(fc[:NT])
    return chol_tile_count(f) / chol_tile_count(np.zeros(NT, dtype=np.int64)), f


share, fenv = envelope_share()
Fx = F - d ** 3 / 3 + share * d ** 3 / 3
res = {"config": cfg, "workload": w.name, "B": B, "iters": it, "meas_delta": meas_delta, "d": d, "P": P, "n": n, "E": int(E),
       "ms_per_iter": dt / it * 1e3, "pt_updates_per_s": B * P * it / dt,
       "mflop_per_traj_iter": F / 1e6, "achieved_tflops": F * B * it / dt / 1e12,
       "frac_fp64_peak": F * B * it / dt / 1e12 / 78.6,
       "envelope_share": share, "executed_mflop_per_traj_iter": Fx / 1e6,
       "executed_tflops": Fx * B * it / dt / 1e12, "executed_frac": Fx * B * it / dt / 1e12 / 78.6,
       "workspace_gib": s.lib.mhe_workspace_bytes(s.dims, B) / 2 ** 30,
       "chunk": s._chunk(B, torch.cuda.current_stream()),  # as solve() sizes it (its own workspace counted free)
       "status": sorted(set(st.tolist()))}
print(json.dumps(res))
