"""NumPy reference of the batched unscented Kalman filter (utils.ukf, mhe_ukf_run), for
tests/test_ukf_host.py and tests/test_gpu_ukf.py.

The recursion of include/mhe.h is written once, generic in dtype, and vectorised over the
batch (every instance runs the same arithmetic on its own rows; rows beyond an instance's nz
are padded with an identity block and zeros, which changes no value).  Its Cholesky and its
forward substitution are written here in that dtype -- no LAPACK -- so the np.longdouble run
really is an extended-precision run.  The plug-in values are restated dtype-generic as well
(oracle/ekf.py casts to float64); tests/test_ukf_host.py checks them against oracle/ekf.py.

Per case and per output, `floor` is the largest absolute difference between the float64 and
the longdouble run over all instances and steps, and
    bound = 8 * floor + 1e-10 * (1 + max |ref|)
is what the device is held to (DESIGN 5d's form: the 8 covers a different but fixed summation
order and FMA contraction, which change the rounding error by a small factor, not its order).
"""
import functools

import numpy as np

import ekf_ragged as er

LOG_2PI = 1.8378770664093454836
PARAMS = ((1.0, 0.0, 0.0), (1.0, 2.0, 1.0))      # (alpha, beta, kappa); the second has lambda = 1, wc_0 != wm_0
CASES = ("gnss", "corr", "bias", "car")
KIND = {"gnss": dict(dyn="gnss_pos_and_bias", meas="multi_pseudorange"),
        "corr": dict(dyn="gnss_pos_and_bias", meas="multi_pseudorange"),
        "bias": dict(dyn="gnss_pos_and_bias", meas="multi_pseudorange_and_bias"),
        "car": dict(dyn="discrete_vehicle_dynamics", meas="vehicle_sensors_model")}
OUTPUTS = ("mu", "S", "nis", "loglik")
B = 70


def require_extended():
    """The floor needs a longdouble that is wider than float64; without one the tests fail."""
    eps = float(np.finfo(np.longdouble).eps)
    assert eps < 1e-18, (f"np.longdouble has eps = {eps:.3e} on this platform (not below 1e-18): the "
                         "float64-vs-extended floor of the UKF reference cannot be formed")


@functools.lru_cache(maxsize=None)
def inputs(name):
    """The seeded builders of tests/ekf_ragged.py the issue names, B = 70."""
    if name == "gnss":
        return er.gnss_inputs(B, T=12)
    if name == "corr":
        return er.gnss_inputs(B, T=12, corr=(1.0, 0.3))
    if name == "bias":
        return er.bias_inputs()
    if name == "car":
        return er.autocar_inputs()
    raise KeyError(name)


# ---------------------------------------------------------------- plug-in values, any dtype
def dyn_value(kind, X, u, inp, dtype):
    """f(X, u) for sigma points X (B, J, n) and controls u (B, m)."""
    dt = dtype(inp["dparams"]["dt"])
    Y = X.copy()
    if kind["dyn"] == "gnss_pos_and_bias":
        for c in range(3):
            Y[..., c] = X[..., c] + dt * u[:, None, c]
        Y[..., 3] = X[..., 3] + dt * X[..., 4]
        return Y
    C = {k: dtype(v) for k, v in inp["dparams"]["car_params"].items()}
    psi, vx, vy, r = X[..., 2], X[..., 3], X[..., 4], X[..., 5]
    Fx, de = u[:, None, 0], u[:, None, 1]
    Fr = -C["C_AR"] * ((vy - C["D_R"] * r) / vx)
    Ff = -C["C_AF"] * ((vy + C["D_F"] * r) / vx - de)
    sp, cp, su, cu = np.sin(psi), np.cos(psi), np.sin(de), np.cos(de)
    Y[..., 0] = X[..., 0] + dt * (vx * cp - vy * sp)
    Y[..., 1] = X[..., 1] + dt * (vx * sp + vy * cp)
    Y[..., 2] = psi + dt * r
    Y[..., 3] = vx + dt * ((-Ff * su + Fx) / C["M"] + r * vy)
    Y[..., 4] = vy + dt * ((Ff * cu + Fr) / C["M"] - r * vx)
    Y[..., 5] = r + dt * ((C["D_F"] * Ff * cu - C["D_R"] * Fr) / C["I_Z"])
    Y[..., 6] = X[..., 6] + dt * X[..., 7]
    return Y


def meas_value(kind, X, sat, nz):
    """h(X) for sigma points X (B, J, n), satellites sat (B, P, 3) and row counts nz (B):
    (B, J, P); rows at or beyond nz hold values that the caller masks."""
    pos, clk = ((0, 1, 8), 6) if kind["meas"] == "vehicle_sensors_model" else ((0, 1, 2), 3)
    d2 = 0
    for a, c in enumerate(pos):
        d = X[:, :, None, c] - sat[:, None, :, a]
        d2 = d2 + d * d
    h = np.sqrt(d2) + X[:, :, None, clk]
    if kind["meas"] == "multi_pseudorange_and_bias":      # the last row is the bias itself
        last = np.arange(sat.shape[1])[None, None, :] == (nz - 1)[:, None, None]
        h = np.where(last, X[:, :, None, 3], h)
    return h


# ---------------------------------------------------------------- linear algebra, any dtype
def cholesky(A, act):
    """Right-looking Cholesky of A (B, N, N), instance b on its leading act[b].sum() rows (the
    rest is taken as identity).  Returns (L, ok (B), margin (B)): ok is False where an active
    pivot was not positive and finite, margin the smallest pivot / diagonal entry."""
    A = A.copy()
    Bn, N = A.shape[0], A.shape[1]
    both = act[:, :, None] & act[:, None, :]
    A = np.where(both, A, np.eye(N, dtype=A.dtype)[None])
    diag0 = np.einsum("bii->bi", A).copy()
    L = np.zeros_like(A)
    ok = np.ones(Bn, dtype=bool)
    margin = np.full(Bn, np.inf)
    with np.errstate(all="ignore"):
        for c in range(N):
            piv = A[:, c, c]
            good = (piv > 0) & np.isfinite(piv)
            ok &= good | ~act[:, c]
            ratio = np.where(good, (piv / diag0[:, c]).astype(np.float64), -np.inf)
            margin = np.minimum(margin, np.where(act[:, c], ratio, np.inf))
            d = np.sqrt(np.where(good, piv, np.nan))
            col = A[:, :, c] / d[:, None]
            col[:, :c] = 0
            col[:, c] = d
            L[:, :, c] = col
            A = A - col[:, :, None] * col[:, None, :]
    return L, ok, margin


def forward(L, M):
    """L^-1 M for lower-triangular L (B, N, N) and M (B, N, K), column by column."""
    M = M.copy()
    N = L.shape[1]
    Y = np.zeros_like(M)
    with np.errstate(all="ignore"):
        for c in range(N):
            Y[:, c] = M[:, c] / L[:, c, c, None]
            M[:, c + 1:] = M[:, c + 1:] - L[:, c + 1:, c, None] * Y[:, None, c]
    return Y


def weights(alpha, beta, kappa, n, dtype):
    alpha, beta, kappa, nn = dtype(alpha), dtype(beta), dtype(kappa), dtype(n)
    lam = alpha * alpha * (nn + kappa) - nn
    wm = np.full(2 * n + 1, 1 / (2 * (nn + lam)), dtype=dtype)
    wc = wm.copy()
    wm[0] = lam / (nn + lam)
    wc[0] = wm[0] + 1 - alpha * alpha + beta
    return np.sqrt(nn + lam), wm, wc


def sigma_points(mu, L, c):
    """(B, 2n+1, n): mu, mu + c L[:, j], mu - c L[:, j]."""
    cols = c * np.swapaxes(L, 1, 2)
    return np.concatenate([mu[:, None, :], mu[:, None, :] + cols, mu[:, None, :] - cols], axis=1)


def wsum(w, V):
    """sum_j w_j V[:, j], j in increasing order."""
    acc = w[0] * V[:, 0]
    for j in range(1, V.shape[1]):
        acc = acc + w[j] * V[:, j]
    return acc


def run(inp, kind, params=PARAMS[0], dtype=np.float64, pmax=None):
    """The filter of include/mhe.h on every instance of `inp`.  Returns a dict: mu (B,T,n),
    S (B,T,n,n), nis, loglik (B,T), status (B), fail_step (B; -1: none), margin (the smallest
    Cholesky pivot / diagonal entry met), and min_vx (the smallest x[3] of any sigma point)."""
    f = lambda a: np.asarray(a, dtype=dtype)                      # noqa: E731
    mu, S = f(inp["mu0"]).copy(), f(inp["S0"]).copy()
    U, Z, sat, Q, Rall, nzall = f(inp["U"]), f(inp["Z"]), f(inp["sat"]), f(inp["Q"]), f(inp["R"]), inp["nz"]
    Bn, T = nzall.shape
    n, P = mu.shape[1], Z.shape[2]
    pmax = P if pmax is None else pmax
    c, wm, wc = weights(*params, n, dtype)
    Q = np.triu(Q) + np.triu(Q, 1).T                             # only the upper triangle is read
    out = {"mu": np.zeros((Bn, T, n), dtype), "S": np.zeros((Bn, T, n, n), dtype), "nis": np.zeros((Bn, T), dtype),
           "loglik": np.zeros((Bn, T), dtype), "fail_step": np.full(Bn, -1), "margin": np.inf, "min_vx": np.inf}
    dead = np.zeros(Bn, dtype=bool)
    status = np.zeros(Bn, dtype=np.int32)
    alln = np.ones((Bn, n), dtype=bool)
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
                go = rows > 0
                Lp = factor(np.where(go[:, None, None], SP, np.eye(n, dtype=dtype)[None]))
                X = sigma_points(mp, Lp, c)
                out["min_vx"] = min(out["min_vx"],
                                    live(np.where(go, X[:, :, 3].min(axis=1).astype(np.float64), np.inf)))
                Zs = np.where(act[:, None, :], meas_value(kind, X, sat[:, k], rows) - Z[:, k][:, None, :], 0)
                e = -wsum(wm, Zs)
                Dz = np.where(act[:, None, :], Zs + e[:, None, :], 0)
                R = Rall[:, k] if Rall.ndim == 4 else np.broadcast_to(Rall[k], (Bn, P, P))
                R = np.triu(R) + np.swapaxes(np.triu(R, 1), 1, 2)
                Pzz = wsum(wc, Dz[:, :, :, None] * Dz[:, :, None, :]) + R
                Pxz = wsum(wc, (X - mp[:, None, :])[:, :, :, None] * Dz[:, :, None, :])        # (B, n, P)
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
                out["loglik"][:, k] = np.where(go, -(nis + 2 * logdet + rows * dtype(LOG_2PI)) / 2, 0)
            new = dead & (out["fail_step"] < 0)
            out["fail_step"][new] = k
            mu[dead], S[dead] = np.nan, np.nan
            out["nis"][dead, k], out["loglik"][dead, k] = np.nan, np.nan
            out["mu"][:, k], out["S"][:, k] = mu, S
    status[dead] = 1
    out["status"] = status
    return out


@functools.lru_cache(maxsize=None)
def reference(name, params=PARAMS[0]):
    """Both runs of a case, computed once and shared: ref (the longdouble run rounded to
    float64) with floor and bound per output, and the float64 run under "f64"."""
    require_extended()
    inp, kind = inputs(name), KIND[name]
    lo, hi = run(inp, kind, params, np.float64), run(inp, kind, params, np.longdouble)
    res = {"f64": lo, "status": hi["status"], "margin": min(lo["margin"], hi["margin"]),
           "min_vx": min(lo["min_vx"], hi["min_vx"]), "floor": {}, "bound": {}}
    assert (lo["status"] == hi["status"]).all()
    for key in OUTPUTS:
        res[key] = hi[key].astype(np.float64)
        res[key].setflags(write=False)
        fl = float(np.max(np.abs(lo[key].astype(np.longdouble) - hi[key])))
        res["floor"][key] = fl
        res["bound"][key] = 8.0 * fl + 1e-10 * (1.0 + float(np.max(np.abs(res[key]))))
    return res
