"""NumPy reference of the batched iterated EKF (utils.ekf.run_batch(iterations=...), mhe_iekf_run),
for tests/test_iekf_host.py and tests/test_gpu_iekf.py -- TEST INFRASTRUCTURE ONLY.

The recursion of include/mhe.h, written once, generic in dtype and vectorised over the batch as
tests/ukf_reference.py is (its Cholesky and forward substitution, no LAPACK, so the np.longdouble
run really is an extended-precision run).  Per step, after the EKF's predict (mu-, S-), with
x_0 = mu- and over the step's rows:

    pass i:  (h, H) at x_i,  e = z - h - H (mu- - x_i),  P = H S- H^T + R = L L^T,
             Y = L^-1 H S-,  w = L^-1 e,  x_{i+1} = mu- + Y^T w,  step = max_c |x_{i+1,c} - x_{i,c}|
             stop when  not (step > tol)  or  i + 1 == iterations   (tol = 0: the step is not tested)
    after:   mu = x_{i+1},  S = S- - Y^T Y  with the last pass's Y.

S- = G S G^T + Q is formed on and above the diagonal and mirrored, so S is bitwise symmetric.

The gate is the EKF's marginal rule d2 = e^2 / diag P > gate, taken once, in pass 0 (at the
prediction); the kept rows stay fixed.  nis, loglik and rej are pass 0's over the kept rows.  An
instance that has stopped keeps its iterate while the others of the batch go on.

The plug-ins are restated dtype-generic with their Jacobians (bug-compatible with oracle/ekf.py:
the vehicle's Jacobian is taken at the predicted state, the bias row of multi_pseudorange_and_bias
has a zero Jacobian row); tests/test_iekf_host.py holds the iterations = 1 run against
oracle/ekf.py.

Per case and per output, floor = max |float64 run - longdouble run| and
    bound = 8 * floor + 1e-10 * (1 + max |ref|)
(tests/ukf_reference.py's form).  For the device's pass counts and masks to be compared exactly
the reference records, and reference() asserts: every pass of every step has
|step / tol - 1| >= STEP_MARGIN, n_iter and the masks are equal in both precisions, every valid
row has |d2 / gate - 1| >= MARGIN.

Inputs: tests/ekf_ragged.py's builders, B = 70, with a COLD prior -- gnss cases: mean
(x_f[:3], x_f[3], 0) + N(0, COLD_SIGMA^2), x_f the fixture's last state (the point the
pseudoranges were simulated at; its drift is not followed by them and is set to 0), S0 =
diag(COLD_SIGMA^2); car: px and py of the prior moved by N(0, 2000^2) and that variance added to
S0.  The gated cases are tests/ukf_gate_reference.py's input sets (consistent prior, 8 % of the
rows shifted by +400 m).
"""
import functools

import numpy as np

import ekf_ragged as er
import ukf_gate_reference as ug
import ukf_reference as ur
from ukf_reference import cholesky, forward

LOG_2PI = ur.LOG_2PI
B = 70
CASES = ("gnss", "corr", "bias", "car")
KIND = ur.KIND
OUTPUTS = ("mu", "S", "nis", "loglik")
COLD_SIGMA = np.array([1e5, 1e5, 1e5, 1e3, 0.1])
CAR_SIGMA = 2000.0
COLD_SEED = {"gnss": 31, "corr": 32, "bias": 33, "car": 34}
TOL = {"gnss": 1e-4, "corr": 1e-4, "bias": 1e-4, "car": 1e-6}
# the cap on the passes; the bias case's is below what its slowest steps need (its bias row has a
# zero Jacobian row, so the iteration there is no Newton iteration and converges linearly): some of
# its steps end at the cap still moving by more than tol
CAP = {"gnss": 8, "corr": 8, "bias": 6, "car": 8}
STEP_MARGIN = 1e-3
GATES, MARGIN = ug.GATES, ug.MARGIN
GATED = ("gnss", "car")


# ---------------------------------------------------------------- inputs
@functools.lru_cache(maxsize=None)
def inputs(name):
    """The cold-prior input set of a case.  Treat as read-only."""
    if name == "gnss":
        inp = er.gnss_inputs(B, T=12)
    elif name == "corr":
        inp = er.gnss_inputs(B, T=12, corr=(1.0, 0.5))
    elif name == "bias":
        inp = er.bias_inputs()
    elif name == "car":
        inp = er.autocar_inputs()
    else:
        raise KeyError(name)
    rng = np.random.default_rng(COLD_SEED[name])
    out = dict(inp)
    if name == "car":
        out["mu0"], out["S0"] = inp["mu0"].copy(), inp["S0"].copy()
        out["mu0"][:, :2] += CAR_SIGMA * rng.normal(size=(B, 2))
        out["S0"][:, 0, 0] += CAR_SIGMA ** 2
        out["S0"][:, 1, 1] += CAR_SIGMA ** 2
    else:
        xf = inp["fx"]["mu"][-1].copy()
        xf[4] = 0.0
        out["mu0"] = xf + rng.normal(size=(B, 5)) * COLD_SIGMA
        out["S0"] = np.tile(np.diag(COLD_SIGMA ** 2), (B, 1, 1))
    return out


def gated_inputs(name):
    """tests/ukf_gate_reference.py's input set of `gnss` or `car`."""
    return ug.inputs(name)


# ---------------------------------------------------------------- plug-ins with Jacobians, any dtype
def dyn_jac(kind, x, u, inp, dtype):
    """(x+ (B,n), G (B,n,n)) of the dynamics at x (B,n), u (B,m)."""
    dt = dtype(inp["dparams"]["dt"])
    Bn, n = x.shape
    xp = ur.dyn_value(kind, x[:, None, :], u, inp, dtype)[:, 0, :]
    G = np.zeros((Bn, n, n), dtype=dtype)
    G[:, np.arange(n), np.arange(n)] = 1
    if kind["dyn"] == "gnss_pos_and_bias":
        G[:, 3, 4] = dt
        return xp, G
    C = {k: dtype(v) for k, v in inp["dparams"]["car_params"].items()}
    psi, vx, vy, r = xp[:, 2], xp[:, 3], xp[:, 4], xp[:, 5]          # the Jacobian sees the updated state
    M, Iz, DF, DR = C["M"], C["I_Z"], C["D_F"], C["D_R"]
    dFf = (C["C_AF"] * (vy + DF * r) / (vx * vx), -C["C_AF"] / vx, -C["C_AF"] * DF / vx)
    dFr = (C["C_AR"] * (vy - DR * r) / (vx * vx), -C["C_AR"] / vx, C["C_AR"] * DR / vx)
    sp, cp, su, cu = np.sin(psi), np.cos(psi), np.sin(u[:, 1]), np.cos(u[:, 1])
    G[:, 0, 2] += dt * (-vx * sp - vy * cp)
    G[:, 0, 3] += dt * cp
    G[:, 0, 4] += -dt * sp
    G[:, 1, 2] += dt * (vx * cp - vy * sp)
    G[:, 1, 3] += dt * sp
    G[:, 1, 4] += dt * cp
    G[:, 2, 5] += dt
    G[:, 3, 3] += -(dt / M) * (su * dFf[0])
    G[:, 3, 4] += dt * (r - (su * dFf[1]) / M)
    G[:, 3, 5] += dt * (vy - (su * dFf[2]) / M)
    G[:, 4, 3] += dt * ((cu * dFf[0] + dFr[0]) / M - r)
    G[:, 4, 4] += (dt / M) * (cu * dFf[1] + dFr[1])
    G[:, 4, 5] += dt * ((cu * dFf[2] + dFr[2]) / M - vx)
    for j in range(3):
        G[:, 5, 3 + j] += (dt / Iz) * (DF * cu * dFf[j] - DR * dFr[j])
    G[:, 6, 7] += dt
    return xp, G


def meas_jac(kind, x, sat, nz):
    """(h (B,P), H (B,P,n)) of the measurement rows at x (B,n) for satellites sat (B,P,3) and row
    counts nz (B); rows at or beyond nz hold values that the caller masks."""
    pos, clk = ((0, 1, 8), 6) if kind["meas"] == "vehicle_sensors_model" else ((0, 1, 2), 3)
    Bn, n = x.shape
    P = sat.shape[1]
    l = [sat[:, :, a] - x[:, None, c] for a, c in enumerate(pos)]
    r = np.sqrt(l[0] * l[0] + l[1] * l[1] + l[2] * l[2])
    h = r + x[:, None, clk]
    H = np.zeros((Bn, P, n), dtype=x.dtype)
    for a, c in enumerate(pos):
        H[:, :, c] = -l[a] / r
    H[:, :, clk] = 1
    if kind["meas"] == "multi_pseudorange_and_bias":      # the last row: h = x[3], a zero Jacobian row
        last = np.arange(P)[None, :] == (nz - 1)[:, None]
        h = np.where(last, x[:, None, 3], h)
        H = np.where(last[:, :, None], 0, H)
    return h, H


# ---------------------------------------------------------------- the filter
def run(inp, kind, iterations, tol, gate=np.inf, dtype=np.float64, pmax=None):
    """The iterated filter on every instance of `inp`.  Returns a dict: mu (B,T,n), S (B,T,n,n),
    nis, loglik (B,T), n_iter (B,T) int32, rej (B,T) int32 bit masks, nkept (B,T), status (B),
    mp (B,T,n) and SP (B,T,n,n) (the predictions), step_last (B,T) (the last pass's step), and the
    margins: step_margin = min |step / tol - 1| over every pass made (inf for tol = 0),
    gate_margin = min |d2 / gate - 1| over the valid rows (inf for gate = inf), margin = the
    smallest Cholesky pivot / diagonal entry of P met."""
    f = lambda a: np.asarray(a, dtype=dtype)                      # noqa: E731
    mu, S = f(inp["mu0"]).copy(), f(inp["S0"]).copy()
    U, Z, sat, Q, Rall, nzall = f(inp["U"]), f(inp["Z"]), f(inp["sat"]), f(inp["Q"]), f(inp["R"]), inp["nz"]
    Bn, T = nzall.shape
    n, P = mu.shape[1], Z.shape[2]
    pmax = P if pmax is None else pmax
    tol, gate = dtype(tol), dtype(gate)
    Q = np.triu(Q) + np.triu(Q, 1).T                             # only the upper triangle is read
    bit = np.uint64(1) << np.arange(P, dtype=np.uint64)
    out = {"mu": np.zeros((Bn, T, n), dtype), "S": np.zeros((Bn, T, n, n), dtype), "nis": np.zeros((Bn, T), dtype),
           "loglik": np.zeros((Bn, T), dtype), "n_iter": np.zeros((Bn, T), np.int32),
           "rej": np.zeros((Bn, T), np.uint32), "nkept": np.zeros((Bn, T), int), "mp": np.zeros((Bn, T, n), dtype),
           "SP": np.zeros((Bn, T, n, n), dtype), "step_last": np.zeros((Bn, T), dtype), "step_margin": np.inf,
           "gate_margin": np.inf, "margin": np.inf}
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
            x, Yl = mp.copy(), np.zeros((Bn, P, n), dtype)
            R = Rall[:, k] if Rall.ndim == 4 else np.broadcast_to(Rall[k], (Bn, P, P))
            for i in range(iterations):
                if not going.any():
                    break
                h, H = meas_jac(kind, x, sat[:, k], rows)
                e = Z[:, k] - h
                for c in range(n):
                    e = e - H[:, :, c] * (mp[:, c] - x[:, c])[:, None]
                T1 = H @ SP
                Pm = T1 @ np.swapaxes(H, 1, 2) + R
                if i == 0:
                    den = np.einsum("bii->bi", Pm)
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
                for r in range(P):                                 # the rows in increasing order
                    dmu = dmu + Y[:, r, :] * w[:, r, None]
                xn = mp + dmu
                step = np.max(np.abs(xn - x), axis=1)              # NaN if any component is
                if i == 0:
                    nis = (w * w).sum(axis=1)
                    logdet = np.where(keep, np.log(np.where(keep, np.einsum("bii->bi", L), 1)), 0).sum(axis=1)
                    out["nis"][:, k] = np.where(go, nis, 0)
                    out["loglik"][:, k] = np.where(go, -(nis + 2 * logdet + keep.sum(axis=1) * dtype(LOG_2PI)) / 2, 0)
                if tol > 0:
                    dist = np.where(going, np.abs(step / tol - 1).astype(np.float64), np.inf)
                    out["step_margin"] = min(out["step_margin"], float(np.fmin.reduce(dist, axis=None)))
                x = np.where(going[:, None], xn, x)
                Yl = np.where(going[:, None, None], Y, Yl)
                out["n_iter"][:, k] += going
                out["step_last"][:, k] = np.where(going, step, out["step_last"][:, k])
                going = going & ((step > tol) if tol > 0 else True)    # tol = 0: the step is not tested
            dS = np.zeros_like(SP)
            for r in range(P):
                dS = dS + Yl[:, r, :, None] * Yl[:, r, None, :]
            mu = np.where(go[:, None], x, mp)
            S = np.where(go[:, None, None], SP - dS, SP)
            out["mu"][:, k], out["S"][:, k] = mu, S
    out["status"] = status
    out["rej"] = out["rej"].view(np.int32)
    return out


@functools.lru_cache(maxsize=None)
def reference(name, iterations=None, tol=None, gate=None):
    """Both runs of a case, computed once and shared (read-only): the cold-prior inputs, or with a
    gate tests/ukf_gate_reference.py's.  ref = the longdouble run rounded to float64, floor and
    bound per output, the float64 run under "f64", and n_iter / rej / nkept / status, asserted equal
    in the two precisions, with the margins (the smaller of the two runs')."""
    ur.require_extended()
    inp = inputs(name) if gate is None else gated_inputs(name)
    iterations = CAP[name] if iterations is None else iterations
    tol = TOL[name] if tol is None else tol
    g = np.inf if gate is None else gate
    lo = run(inp, KIND[name], iterations, tol, g, np.float64)
    hi = run(inp, KIND[name], iterations, tol, g, np.longdouble)
    for key in ("n_iter", "rej", "status", "nkept"):
        np.testing.assert_array_equal(lo[key], hi[key], err_msg=f"{name}: {key} differs between the precisions")
    res = {"f64": lo, "floor": {}, "bound": {}, "iterations": iterations, "tol": tol}
    for key in ("n_iter", "rej", "status", "nkept"):
        res[key] = hi[key]
    for key in ("step_margin", "gate_margin", "margin"):
        res[key] = min(lo[key], hi[key])
    assert res["step_margin"] >= STEP_MARGIN, (name, res["step_margin"])
    assert res["gate_margin"] >= MARGIN, (name, res["gate_margin"])
    for key in OUTPUTS + ("mp", "SP", "step_last"):
        res[key] = hi[key].astype(np.float64)
        res[key].setflags(write=False)
    for key in OUTPUTS:
        fl = float(np.max(np.abs(lo[key].astype(np.longdouble) - hi[key])))
        res["floor"][key] = fl
        res["bound"][key] = 8.0 * fl + 1e-10 * (1.0 + float(np.max(np.abs(res[key]))))
    return res
