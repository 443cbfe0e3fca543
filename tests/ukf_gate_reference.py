"""Innovation-gated unscented filter in NumPy -- TEST INFRASTRUCTURE ONLY.

The reference of tests/test_ukf_gate_host.py and tests/test_gpu_ukf_gate.py: the recursion of
tests/ukf_reference.py (its helpers, dtype-generic, no LAPACK) with one added step.  After Pzz
(R included) and Pxz are formed from the redrawn sigma points,

    den = diag Pzz,  d2 = e^2 / den,  rej = act & (den > 0) & (d2 > gate)

and the step goes on with act & ~rej: the Cholesky sweep over the kept rows in their order (a row
that is not active is an identity row of the factor and a zero row of Y and w), nis and loglik
over the kept rows, predict-only when none is kept.  The measurement model sees the original row
count, so the bias row of multi_pseudorange_and_bias keeps its place.  The Cholesky of S- is
taken whenever the step has rows, kept or not, as the device takes it.

Also here: the tests' inputs (tests/ukf_reference.py's four cases with
tests/ekf_gate_reference.py's consistent prior and +400 m on a seeded 8 % of the valid rows),
their references in float64 and np.longdouble, computed once per process, and the host-side
compaction that removes the screened rows from an input set.
"""
import functools

import numpy as np

import ekf_gate_reference as eg
import ukf_reference as ur
from ukf_reference import cholesky, dyn_value, forward, meas_value, sigma_points, weights, wsum

GATES = eg.GATES           # 10.83: chi-square(1) 0.999 quantile; 0.5: a threshold inside the clean rows' bulk
MARGIN = eg.MARGIN         # every valid row: |d2 / gate - 1| >= MARGIN, so the masks are compared exactly
CASES, KIND, PARAMS, OUTPUTS = ur.CASES, ur.KIND, ur.PARAMS, ur.OUTPUTS


def run(inp, kind, gate, params=PARAMS[0], dtype=np.float64, pmax=None):
    """ukf_reference.run with the screen.  Returns its dict (mu, S, nis, loglik, status,
    fail_step, margin, min_vx) plus rej (B,T) int32 bit masks, nrej and nkept (B,T) counts and
    gate_margin = min |d2 / gate - 1| over the valid rows of live filters (inf for gate = inf)."""
    f = lambda a: np.asarray(a, dtype=dtype)                      # noqa: E731
    mu, S = f(inp["mu0"]).copy(), f(inp["S0"]).copy()
    U, Z, sat, Q, Rall, nzall = f(inp["U"]), f(inp["Z"]), f(inp["sat"]), f(inp["Q"]), f(inp["R"]), inp["nz"]
    Bn, T = nzall.shape
    n, P = mu.shape[1], Z.shape[2]
    pmax = P if pmax is None else pmax
    gate = dtype(gate)
    c, wm, wc = weights(*params, n, dtype)
    Q = np.triu(Q) + np.triu(Q, 1).T                             # only the upper triangle is read
    out = {"mu": np.zeros((Bn, T, n), dtype), "S": np.zeros((Bn, T, n, n), dtype), "nis": np.zeros((Bn, T), dtype),
           "loglik": np.zeros((Bn, T), dtype), "fail_step": np.full(Bn, -1), "margin": np.inf, "min_vx": np.inf,
           "rej": np.zeros((Bn, T), dtype=np.uint32), "nrej": np.zeros((Bn, T), dtype=int),
           "nkept": np.zeros((Bn, T), dtype=int), "gate_margin": np.inf}
    dead = np.zeros(Bn, dtype=bool)
    status = np.zeros(Bn, dtype=np.int32)
    alln = np.ones((Bn, n), dtype=bool)
    bit = np.uint64(1) << np.arange(P, dtype=np.uint64)
    live = lambda m: float(np.min(m[~dead], initial=np.inf))      # noqa: E731

    def factor(M):
        nonlocal dead
        L, ok, margin = cholesky(M, alln)
        out["margin"] = min(out["margin"], live(margin))
        dead = dead | ~ok
        return L

    with np.errstate(all="ignore"):
        for k in range(T):
            X = sigma_points(mu, factor(S), c)
            out["min_vx"] = min(out["min_vx"], live(X[:, :, 3].min(axis=1).astype(np.float64)))
            Y = dyn_value(kind, X, U[:, k], inp, dtype)
            mp = wsum(wm, Y)
            D = Y - mp[:, None, :]
            SP = wsum(wc, D[:, :, :, None] * D[:, :, None, :]) + Q[None]
            nz = nzall[:, k].astype(np.int64)
            status[(nz > pmax) & (status == 0)] = 2
            rows = np.where((nz > 0) & (nz <= pmax), nz, 0)
            act = np.arange(P)[None, :] < rows[:, None]            # (B, P)
            mu, S = mp, SP
            if act.any():
                has = rows > 0
                Lp = factor(np.where(has[:, None, None], SP, np.eye(n, dtype=dtype)[None]))
                X = sigma_points(mp, Lp, c)
                out["min_vx"] = min(out["min_vx"],
                                    live(np.where(has, X[:, :, 3].min(axis=1).astype(np.float64), np.inf)))
                Zs = np.where(act[:, None, :], meas_value(kind, X, sat[:, k], rows) - Z[:, k][:, None, :], 0)
                e = -wsum(wm, Zs)
                Dz = np.where(act[:, None, :], Zs + e[:, None, :], 0)
                R = Rall[:, k] if Rall.ndim == 4 else np.broadcast_to(Rall[k], (Bn, P, P))
                R = np.triu(R) + np.swapaxes(np.triu(R, 1), 1, 2)
                Pzz = wsum(wc, Dz[:, :, :, None] * Dz[:, :, None, :]) + R
                Pxz = wsum(wc, (X - mp[:, None, :])[:, :, :, None] * Dz[:, :, None, :])        # (B, n, P)
                # ---- the screen: marginal, at the prediction
                den = np.einsum("bii->bi", Pzz)
                d2 = e * e / den
                rej = act & (den > 0) & (d2 > gate)
                if np.isfinite(gate):
                    dist = np.where(act & ~dead[:, None], np.abs(d2 / gate - 1).astype(np.float64), np.inf)
                    out["gate_margin"] = min(out["gate_margin"], float(np.fmin.reduce(dist, axis=None)))
                out["rej"][:, k] = (rej * bit).sum(axis=1).astype(np.uint32)
                out["nrej"][:, k], out["nkept"][:, k] = rej.sum(axis=1), (act & ~rej).sum(axis=1)
                act = act & ~rej
                go, rows = act.any(axis=1), act.sum(axis=1)
                Lz, ok, margin = cholesky(Pzz, act)
                out["margin"] = min(out["margin"], live(np.where(go, margin, np.inf)))
                dead = dead | (go & ~ok)
                Yw = forward(Lz, np.concatenate([np.swapaxes(Pxz, 1, 2), e[:, :, None]], axis=2))
                Yw = np.where(act[:, :, None], Yw, 0)
                Ym, w = Yw[:, :, :n], Yw[:, :, n]
                dmu, dS = np.zeros_like(mp), np.zeros_like(SP)
                for i in range(P):                                  # sums over the rows in increasing order
                    dmu = dmu + Ym[:, i, :] * w[:, i, None]
                    dS = dS + Ym[:, i, :, None] * Ym[:, i, None, :]
                mu = np.where(go[:, None], mp + dmu, mp)
                S = np.where(go[:, None, None], SP - dS, SP)
                nis = (w * w).sum(axis=1)
                logdet = np.where(act, np.log(np.where(act, np.einsum("bii->bi", Lz), 1)), 0).sum(axis=1)
                out["nis"][:, k] = np.where(go, nis, 0)
                out["loglik"][:, k] = np.where(go, -(nis + 2 * logdet + rows * dtype(ur.LOG_2PI)) / 2, 0)
            new = dead & (out["fail_step"] < 0)
            out["fail_step"][new] = k
            mu[dead], S[dead] = np.nan, np.nan
            out["nis"][dead, k], out["loglik"][dead, k] = np.nan, np.nan
            out["mu"][:, k], out["S"][:, k] = mu, S
    status[dead] = 1
    out["status"] = status
    out["rej"] = out["rej"].view(np.int32)
    return out


# ---------------------------------------------------------------- the tests' inputs

@functools.lru_cache(maxsize=None)
def inputs(name):
    """ukf_reference's case with outliers planted (out["planted"]); the gnss cases get the prior
    that is consistent with its covariance first.  Treat as read-only."""
    inp = ur.inputs(name)
    return eg.plant(inp if name == "car" else eg.consistent_prior(inp))


def compact(inp, rej):
    """`inp` with the rows of the bit masks rej (B,T) removed and the kept rows moved up in their
    order: Z, sat, the kept sub-block of R (made per instance) and nz = the kept count."""
    Bn, T = inp["nz"].shape
    P = inp["Z"].shape[2]
    out = dict(inp, Z=np.zeros_like(inp["Z"]), sat=np.zeros_like(inp["sat"]), nz=np.zeros_like(inp["nz"]),
               R=np.zeros((Bn, T, P, P)))
    word = rej.view(np.uint32)
    for b in range(Bn):
        for k in range(T):
            ns = int(inp["nz"][b, k])
            keep = [i for i in range(ns) if not (int(word[b, k]) >> i) & 1]
            m = len(keep)
            R = inp["R"][b, k] if inp["R"].ndim == 4 else inp["R"][k]
            out["Z"][b, k, :m], out["sat"][b, k, :m] = inp["Z"][b, k, keep], inp["sat"][b, k, keep]
            out["R"][b, k, :m, :m] = R[np.ix_(keep, keep)]
            out["nz"][b, k] = m
    return out


@functools.lru_cache(maxsize=None)
def reference(name, gate, params=PARAMS[0]):
    """Both gated runs of a case, computed once and shared (read-only): ref = the longdouble run
    rounded to float64, with floor and bound per output in ukf_reference's form taken from these
    two runs, the float64 run under "f64", and rej / nrej / nkept / gate_margin (the smaller of
    the two runs').  The two runs' masks and statuses are asserted equal."""
    ur.require_extended()
    inp, kind = inputs(name), KIND[name]
    lo, hi = run(inp, kind, gate, params, np.float64), run(inp, kind, gate, params, np.longdouble)
    np.testing.assert_array_equal(lo["rej"], hi["rej"])
    np.testing.assert_array_equal(lo["status"], hi["status"])
    res = {"f64": lo, "status": hi["status"], "margin": min(lo["margin"], hi["margin"]),
           "min_vx": min(lo["min_vx"], hi["min_vx"]), "gate_margin": min(lo["gate_margin"], hi["gate_margin"]),
           "rej": hi["rej"], "nrej": hi["nrej"], "nkept": hi["nkept"], "fail_step": hi["fail_step"],
           "floor": {}, "bound": {}}
    for key in OUTPUTS:
        res[key] = hi[key].astype(np.float64)
        res[key].setflags(write=False)
        fl = float(np.max(np.abs(lo[key].astype(np.longdouble) - hi[key])))
        res["floor"][key] = fl
        res["bound"][key] = 8.0 * fl + 1e-10 * (1.0 + float(np.max(np.abs(res[key]))))
    return res
