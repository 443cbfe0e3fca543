"""NumPy reference of the iterated EKF with pseudo-Huber measurement rows
(utils.ekf.run_batch(iterations=..., huber=...), mhe_iekf_run_robust), for
tests/test_robust_iekf_host.py and tests/test_gpu_robust_iekf.py -- TEST INFRASTRUCTURE ONLY.

tests/iekf_reference.py's run (its plug-ins, Cholesky and forward substitution by import, generic
in dtype, vectorised over the batch) with three changes.  Per pass, with r = z - h at the iterate:

    t_j = r_j / delta_j,  s_j = sqrt(1 + t_j t_j),  g_j = sqrt(s_j)
    1. P = H S- H^T + R~,  R~_jl = R_jl * (g_j * g_l)        (R itself in iekf_reference.run)
    2. the gate of pass 0 tests the UNWEIGHTED diagonal (H S- H^T)_jj + R_jj, the sum the plain
       run forms, so the mask is the plain run's at the same prediction
    3. om = 1 / s of the last pass on the rows that were applied, 0 on every other row.

nis and loglik are pass 0's w and L of the sweep that used R~ at x_0: the reweighted model's.
delta = +inf gives s = g = 1 exactly, R~ = R bitwise, and the run is iekf_reference.run's bitwise.

Inputs: tests/ukf_gate_reference.py's sets (consistent prior, 8 % of the rows shifted by +400 m),
B = 70 -- 17 workgroups and a partial one.  The cap on the passes is 64, which no step of the
cases below reaches.  Per case and output, floor = max |float64 run - longdouble run| and
    bound = 8 * floor + 1e-10 * (1 + max |ref|)
(tests/ukf_reference.py's form); `weights` is among the outputs.  reference() asserts what lets the
device's counts and masks be compared exactly: n_iter, rej and status equal in both precisions,
every pass of every step |step / tol - 1| >= iekf_reference.STEP_MARGIN (1e-3), every valid row
|d2 / gate - 1| >= 1e-6.
"""
import functools

import numpy as np

import iekf_reference as ir
import ukf_gate_reference as ug
import ukf_reference as ur
from iekf_reference import dyn_jac, meas_jac
from ukf_reference import cholesky, forward

B = ir.B
CAP = 64
KIND = ir.KIND
OUTPUTS = ir.OUTPUTS + ("weights",)
GATE = ug.GATES[0]          # 10.83
GATE_MARGIN = 1e-6
# (case, gate, delta, tol): pairs whose step and gate margins hold in both precisions
# (tests/test_robust_iekf_host.py re-verifies them and prints the margins)
PARITY = (("gnss", None, 5.0, 3e-4), ("corr", None, 15.0, 1e-4), ("bias", None, 15.0, 1e-4),
          ("car", None, 15.0, 1e-6), ("gnss", GATE, 15.0, 3e-4), ("car", GATE, 15.0, 1e-6))
# the per-row case: `bias` with the pseudoranges' delta and another one for the bias row (the
# last row of a step, in seconds of clock bias times c: metres as well)
ROWS = ("bias", None, (5.0, 15.0), 1e-4)


def inputs(name):
    """tests/ukf_gate_reference.py's input set of a case.  Treat as read-only."""
    return ug.inputs(name)


def delta_array(inp, delta, dtype=np.float64):
    """delta (B,T,P): a scalar for every row, or (rows', last row's) with the last row of each
    step (row nz - 1) given its own value."""
    shape = inp["Z"].shape
    if not isinstance(delta, tuple):
        return np.full(shape, delta, dtype=dtype)
    out = np.full(shape, delta[0], dtype=dtype)
    last = np.arange(shape[2])[None, None, :] == (inp["nz"] - 1)[:, :, None]
    out[last] = delta[1]
    return out


# ---------------------------------------------------------------- the filter
def run(inp, kind, iterations, tol, delta, gate=np.inf, dtype=np.float64, pmax=None):
    """iekf_reference.run with pseudo-Huber rows: delta a scalar or an array of Z's shape.  Returns
    its dict and om (B,T,P), the last pass's 1 / s on the applied rows and 0 elsewhere."""
    f = lambda a: np.asarray(a, dtype=dtype)                      # noqa: E731
    mu, S = f(inp["mu0"]).copy(), f(inp["S0"]).copy()
    U, Z, sat, Q, Rall, nzall = f(inp["U"]), f(inp["Z"]), f(inp["sat"]), f(inp["Q"]), f(inp["R"]), inp["nz"]
    Bn, T = nzall.shape
    n, P = mu.shape[1], Z.shape[2]
    pmax = P if pmax is None else pmax
    tol, gate = dtype(tol), dtype(gate)
    D = np.broadcast_to(f(delta), Z.shape)
    Q = np.triu(Q) + np.triu(Q, 1).T                             # only the upper triangle is read
    bit = np.uint64(1) << np.arange(P, dtype=np.uint64)
    out = {"mu": np.zeros((Bn, T, n), dtype), "S": np.zeros((Bn, T, n, n), dtype), "nis": np.zeros((Bn, T), dtype),
           "loglik": np.zeros((Bn, T), dtype), "n_iter": np.zeros((Bn, T), np.int32),
           "rej": np.zeros((Bn, T), np.uint32), "nkept": np.zeros((Bn, T), int), "mp": np.zeros((Bn, T, n), dtype),
           "SP": np.zeros((Bn, T, n, n), dtype), "step_last": np.zeros((Bn, T), dtype), "step_margin": np.inf,
           "gate_margin": np.inf, "margin": np.inf, "om": np.zeros((Bn, T, P), dtype)}
    status = np.zeros(Bn, dtype=np.int32)
    with np.errstate(all="ignore"):
        for k in range(T):
            mp, G = dyn_jac(kind, mu, U[:, k], inp, dtype)
            SP = G @ (S @ np.swapaxes(G, 1, 2)) + Q[None]
            SP = np.triu(SP) + np.swapaxes(np.triu(SP, 1), 1, 2)   # an entry below the diagonal is its mirror image
            out["mp"][:, k], out["SP"][:, k] = mp, SP
            nz = nzall[:, k].astype(np.int64)
            status[(nz > pmax) & (status == 0)] = 2
            rows = np.where((nz > 0) & (nz <= pmax), nz, 0)
            act = np.arange(P)[None, :] < rows[:, None]
            keep, go = act, rows > 0
            going = go.copy()                                      # instances still iterating
            x, Yl, sl = mp.copy(), np.zeros((Bn, P, n), dtype), np.ones((Bn, P), dtype)
            R = Rall[:, k] if Rall.ndim == 4 else np.broadcast_to(Rall[k], (Bn, P, P))
            for i in range(iterations):
                if not going.any():
                    break
                h, H = meas_jac(kind, x, sat[:, k], rows)
                r = Z[:, k] - h
                t = r / D[:, k]
                s = np.sqrt(1 + t * t)
                g = np.where(act, np.sqrt(s), 1)                   # a lane without a row holds g = 1
                e = r
                for c in range(n):
                    e = e - H[:, :, c] * (mp[:, c] - x[:, c])[:, None]
                T1 = H @ SP
                HSH = T1 @ np.swapaxes(H, 1, 2)
                Pm = HSH + R * (g[:, :, None] * g[:, None, :])
                if i == 0:
                    den = np.einsum("bii->bi", HSH) + np.einsum("bii->bi", R)     # the unweighted diagonal
                    d2 = e * e / den
                    rej = act & (den > 0) & (d2 > gate)
                    if np.isfinite(gate):
                        dist = np.where(act, np.abs(d2 / gate - 1).astype(np.float64), np.inf)
                        out["gate_margin"] = min(out["gate_margin"], float(np.fmin.reduce(dist, axis=None)))
                    out["rej"][:, k] = (rej * bit).sum(axis=1).astype(np.uint32)
                    keep = act & ~rej
                    out["nkept"][:, k] = keep.sum(axis=1)
                    go = keep.any(axis=1)
                    going = going & go
                L, ok, margin = cholesky(Pm, keep)
                out["margin"] = min(out["margin"], float(np.min(margin[going], initial=np.inf)))
                status[going & ~ok & (status != 2)] = 1
                Yw = forward(L, np.concatenate([np.where(keep[:, :, None], T1, 0),
                                                np.where(keep, e, 0)[:, :, None]], axis=2))
                Yw = np.where(keep[:, :, None], Yw, 0)
                Y, w = Yw[:, :, :n], Yw[:, :, n]
                dmu = np.zeros_like(mp)
                for rr in range(P):                                # the rows in increasing order
                    dmu = dmu + Y[:, rr, :] * w[:, rr, None]
                xn = mp + dmu
                step = np.max(np.abs(xn - x), axis=1)              # NaN if any component is
                if i == 0:
                    nis = (w * w).sum(axis=1)
                    logdet = np.where(keep, np.log(np.where(keep, np.einsum("bii->bi", L), 1)), 0).sum(axis=1)
                    out["nis"][:, k] = np.where(go, nis, 0)
                    out["loglik"][:, k] = np.where(go, -(nis + 2 * logdet + keep.sum(axis=1) * dtype(ir.LOG_2PI)) / 2, 0)
                if tol > 0:
                    dist = np.where(going, np.abs(step / tol - 1).astype(np.float64), np.inf)
                    out["step_margin"] = min(out["step_margin"], float(np.fmin.reduce(dist, axis=None)))
                x = np.where(going[:, None], xn, x)
                Yl = np.where(going[:, None, None], Y, Yl)
                sl = np.where(going[:, None], s, sl)
                out["n_iter"][:, k] += going
                out["step_last"][:, k] = np.where(going, step, out["step_last"][:, k])
                going = going & ((step > tol) if tol > 0 else True)    # tol = 0: the step is not tested
            dS = np.zeros_like(SP)
            for rr in range(P):
                dS = dS + Yl[:, rr, :, None] * Yl[:, rr, None, :]
            mu = np.where(go[:, None], x, mp)
            S = np.where(go[:, None, None], SP - dS, SP)
            out["mu"][:, k], out["S"][:, k] = mu, S
            out["om"][:, k] = np.where(go[:, None] & keep, 1 / np.where(keep, sl, 1), 0)
    out["status"] = status
    out["rej"] = out["rej"].view(np.int32)
    return out


@functools.lru_cache(maxsize=None)
def reference(name, delta, tol, gate=None):
    """Both runs of a case on tests/ukf_gate_reference.py's inputs, computed once and shared
    (read-only).  delta: a float, or (rows', last row's) for delta_array.  ref = the longdouble run
    rounded to float64 (`weights` = its om), floor and bound per output, the float64 run under
    "f64", and n_iter / rej / nkept / status, asserted equal in the two precisions, with the
    margins (the smaller of the two runs')."""
    ur.require_extended()
    inp = inputs(name)
    g = np.inf if gate is None else gate
    lo = run(inp, KIND[name], CAP, tol, delta_array(inp, delta), g, np.float64)
    hi = run(inp, KIND[name], CAP, tol, delta_array(inp, delta, np.longdouble), g, np.longdouble)
    for key in ("n_iter", "rej", "status", "nkept"):
        np.testing.assert_array_equal(lo[key], hi[key], err_msg=f"{name}: {key} differs between the precisions")
    lo["weights"], hi["weights"] = lo["om"], hi["om"]
    res = {"f64": lo, "floor": {}, "bound": {}, "iterations": CAP, "tol": tol, "delta": delta}
    for key in ("n_iter", "rej", "status", "nkept"):
        res[key] = hi[key]
    for key in ("step_margin", "gate_margin", "margin"):
        res[key] = min(lo[key], hi[key])
    assert res["step_margin"] >= ir.STEP_MARGIN, (name, delta, tol, gate, res["step_margin"])
    assert res["gate_margin"] >= GATE_MARGIN, (name, delta, tol, gate, res["gate_margin"])
    for key in OUTPUTS + ("mp", "SP", "step_last"):
        res[key] = hi[key].astype(np.float64)
        res[key].setflags(write=False)
    for key in OUTPUTS:
        fl = float(np.max(np.abs(lo[key].astype(np.longdouble) - hi[key])))
        res["floor"][key] = fl
        res["bound"][key] = 8.0 * fl + 1e-10 * (1.0 + float(np.max(np.abs(res[key]))))
    return res
