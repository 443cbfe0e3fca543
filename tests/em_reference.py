"""NumPy reference of the EKF noise identification -- TEST INFRASTRUCTURE ONLY.

The reference of tests/test_em_host.py and tests/test_gpu_em.py: the RTS smoother with the
lag-one covariances (utils.ekf.smooth_batch(lag_one=True), mhe_ekf_smooth_args), the EM
sufficient statistics (utils.ekf.em_stats, mhe_ekf_em_stats) and the fitting loop
(utils.ekf.fit_noise), written once, generic in dtype and vectorised over the batch.  Full
matrices throughout -- C_k = Ss_k @ G_{k-1}.T and W_k as written below -- so nothing of the
kernels' triangle, column and row-of-C schemes is shared.  No LAPACK: the Cholesky factor and
the triangular solves are the loops below, so the np.longdouble run really is an
extended-precision run.  The plug-ins are restated here in the working dtype (oracle/ekf.py's
are float64 only); tests/test_em_host.py pins them to the oracle's.

Notation of tests/rts_reference.py: filtered history (mu_k, S_k), k = 0..T-1, k = -1 the prior.
    (x-, F) = f(mu_{k-1}, u_k);  S- = F S_{k-1} F^T + Q;  G_{k-1} = S_{k-1} F^T (S-)^-1
    mus_{k-1} = mu_{k-1} + G_{k-1} (mus_k - x-);  Ss_{k-1} = S_{k-1} + G_{k-1} (Ss_k - S-) G_{k-1}^T
    C_k = Ss_k G_{k-1}^T                                       (C_0 needs the prior: NaN without)
Statistics, with (f, F) at mus_{k-1} and (h, H) at mus_k:
    W_k = d d^T + Ss_k - C_k F^T - F C_k^T + F Ss_{k-1} F^T,  d = mus_k - f;   Qsum = sum_k W_k
    r2[k, i] = (z_i - h_i)^2 + H_i Ss_k H_i^T  for the counted rows, 0 elsewhere

Bound per case and output (the convention of tests/urts_reference.py):
    floor = max |float64 run - longdouble run|,   bound = 8 floor + 1e-10 (1 + max |ref|).
"""
import os

import numpy as np

import ekf_ragged as er

GNSS = dict(name="gnss", n=5, m=3, pos=(0, 1, 2), bias=3, extra=0)
BIAS = dict(GNSS, name="bias", extra=1)
CAR = dict(name="car", n=9, m=2, pos=(0, 1, 8), bias=6, extra=0)

FIT_FIXTURE = os.path.join(er.GOLDEN, "em_fit_gnss.npz")
FIT_ROUNDS = 12


def require_extended():
    assert np.finfo(np.longdouble).eps < 1e-18, "np.longdouble is not an extended format here"


# ---------------------------------------------------------------- plug-ins, any dtype, batched

def dynamics(kind, x, u, dparams, dtype):
    """(f (B,n), F (B,n,n)) of the dynamics plug-in at x (B,n), u (B,m)."""
    dt = dtype(dparams["dt"])
    Bn, n = x.shape
    F = np.zeros((Bn, n, n), dtype=dtype)
    F[:, np.arange(n), np.arange(n)] = 1
    if kind["n"] == 5:
        f = x.copy()
        f[:, :3] = x[:, :3] + dt * u
        f[:, 3] = x[:, 3] + dt * x[:, 4]
        F[:, 3, 4] = dt
        return f, F
    C = {k: dtype(v) for k, v in dparams["car_params"].items()}
    vx, vy, r, psi = x[:, 3], x[:, 4], x[:, 5], x[:, 2]
    Fr = -C["C_AR"] * ((vy - C["D_R"] * r) / vx)
    Ff = -C["C_AF"] * ((vy + C["D_F"] * r) / vx - u[:, 1])
    su, cu = np.sin(u[:, 1]), np.cos(u[:, 1])
    xd = np.zeros_like(x)
    xd[:, 0] = vx * np.cos(psi) - vy * np.sin(psi)
    xd[:, 1] = vx * np.sin(psi) + vy * np.cos(psi)
    xd[:, 2] = r
    xd[:, 3] = (-Ff * su + u[:, 0]) / C["M"] + r * vy
    xd[:, 4] = (Ff * cu + Fr) / C["M"] - r * vx
    xd[:, 5] = (C["D_F"] * Ff * cu - C["D_R"] * Fr) / C["I_Z"]
    xd[:, 6] = x[:, 7]
    f = x + dt * xd
    vx, vy, r, psi = f[:, 3], f[:, 4], f[:, 5], f[:, 2]          # the plug-in's Jacobian sees the updated state
    M, Iz, DF, DR = C["M"], C["I_Z"], C["D_F"], C["D_R"]
    dFf = np.stack([C["C_AF"] * (vy + DF * r) / vx ** 2, -C["C_AF"] / vx, -C["C_AF"] * DF / vx + 0 * vx], 1)
    dFr = np.stack([C["C_AR"] * (vy - DR * r) / vx ** 2, -C["C_AR"] / vx, C["C_AR"] * DR / vx + 0 * vx], 1)
    F[:, 0, 2] += dt * (-vx * np.sin(psi) - vy * np.cos(psi))
    F[:, 0, 3] += dt * np.cos(psi)
    F[:, 0, 4] += -dt * np.sin(psi)
    F[:, 1, 2] += dt * (vx * np.cos(psi) - vy * np.sin(psi))
    F[:, 1, 3] += dt * np.sin(psi)
    F[:, 1, 4] += dt * np.cos(psi)
    F[:, 2, 5] += dt
    F[:, 3, 3] += -(dt / M) * su * dFf[:, 0]
    F[:, 3, 4] += dt * (r - su * dFf[:, 1] / M)
    F[:, 3, 5] += dt * (vy - su * dFf[:, 2] / M)
    F[:, 4, 3] += dt * ((cu * dFf[:, 0] + dFr[:, 0]) / M - r)
    F[:, 4, 4] += (dt / M) * (cu * dFf[:, 1] + dFr[:, 1])
    F[:, 4, 5] += dt * ((cu * dFf[:, 2] + dFr[:, 2]) / M - vx)
    F[:, 5, 3:6] += (dt / Iz) * (DF * cu[:, None] * dFf - DR * dFr)
    F[:, 6, 7] += dt
    return f, F


def measurement(kind, x, sat, nz, dtype):
    """(h (B,pmax), H (B,pmax,n), valid (B,pmax)) of the measurement plug-in at x (B,n) with
    sat (B,pmax,3) and nz (B) rows; rows i >= nz are zero.  The bias variant's last row is
    h = x[3] with the plug-in's all-zero Jacobian row."""
    Bn, pmax = sat.shape[:2]
    i = np.arange(pmax)[None, :]
    valid = i < nz[:, None]
    p = x[:, list(kind["pos"])]
    d = p[:, None, :] - sat
    rng = np.sqrt((d ** 2).sum(-1))
    h = rng + x[:, None, kind["bias"]]
    H = np.zeros((Bn, pmax, x.shape[1]), dtype=dtype)
    with np.errstate(all="ignore"):
        H[:, :, list(kind["pos"])] = d / rng[:, :, None]
    H[:, :, kind["bias"]] = 1
    if kind["extra"]:
        last = valid & (i == nz[:, None] - 1)
        h = np.where(last, x[:, None, 3], h)
        H[last] = 0
    h = np.where(valid, h, 0)
    H[~valid] = 0
    return h, H, valid


# ---------------------------------------------------------------- linear algebra without LAPACK

def cholesky(A):
    """Lower factor of A (B,N,N), column by column; NaN where a pivot is not positive."""
    N = A.shape[1]
    L = np.zeros_like(A)
    with np.errstate(all="ignore"):
        for j in range(N):
            piv = A[:, j, j] - (L[:, j, :j] ** 2).sum(-1)
            L[:, j, j] = np.sqrt(np.where(piv > 0, piv, np.nan))
            for i in range(j + 1, N):
                L[:, i, j] = (A[:, i, j] - (L[:, i, :j] * L[:, j, :j]).sum(-1)) / L[:, j, j]
    return L


def solve_spd(A, Y):
    """A^-1 Y for symmetric positive definite A (B,N,N) and Y (B,N,K)."""
    L = cholesky(A)
    N = A.shape[1]
    W = np.zeros_like(Y)
    with np.errstate(all="ignore"):
        for r in range(N):
            W[:, r] = (Y[:, r] - (L[:, r, :r, None] * W[:, :r]).sum(1)) / L[:, r, r, None]
        X = np.zeros_like(Y)
        for r in range(N - 1, -1, -1):
            X[:, r] = (W[:, r] - (L[:, r + 1:, r, None] * X[:, r + 1:]).sum(1)) / L[:, r, r, None]
    return X, L


def T_(A):
    return np.swapaxes(A, -1, -2)


# ---------------------------------------------------------------- forward filter (for the fit)

def forward(kind, mu0, S0, U, Z, nz, sat, Q, R, dparams, dtype=np.float64, keep_H=False):
    """The EKF of oracle/ekf.py with the batch correction solved by Cholesky; rows i >= nz are
    taken out by a zero Jacobian row, zero innovation and a unit diagonal of P.  R (T,p,p) or
    (B,T,p,p).  Returns (mu (B,T,n), S (B,T,n,n), loglik (B,T)) and with keep_H the per-step
    (H, R) the corrections used."""
    f = lambda a: np.asarray(a, dtype=dtype)          # noqa: E731
    mu, S, U, Z, sat, Q, R = f(mu0).copy(), f(S0).copy(), f(U), f(Z), f(sat), f(Q), f(R)
    Bn, T, pmax = Z.shape
    mus, Ss, ll, Hs = [], [], [], []
    log2pi = np.log(2 * np.arccos(dtype(-1)))
    for k in range(T):
        xp, F = dynamics(kind, mu, U[:, k], dparams, dtype)
        SP = F @ S @ T_(F) + Q
        nk = np.where(nz[:, k] <= pmax, nz[:, k], 0)
        h, H, valid = measurement(kind, xp, sat[:, k], nk, dtype)
        Rk = np.broadcast_to(R[k] if R.ndim == 3 else R[:, k], (Bn, pmax, pmax)).copy()
        vv = valid[:, :, None] & valid[:, None, :]
        Rk = np.where(vv, Rk, 0)
        Rk[:, np.arange(pmax), np.arange(pmax)] += np.where(valid, 0, 1)
        e = np.where(valid, Z[:, k] - h, 0)
        P = H @ SP @ T_(H) + Rk
        X, L = solve_spd(P, np.concatenate([H @ SP, e[:, :, None]], 2))     # P^-1 [H S- | e]
        mu = xp + (T_(H @ SP) @ X[:, :, -1:])[:, :, 0]
        S = SP - T_(H @ SP) @ X[:, :, :-1]
        nis = (e * X[:, :, -1]).sum(-1)
        logdet = 2 * np.log(L[:, np.arange(pmax), np.arange(pmax)]).sum(-1)
        ll.append(np.where(nk > 0, -(nis + logdet + nk * log2pi) / 2, 0))
        mus.append(mu)
        Ss.append(S)
        Hs.append((H, Rk))
    out = (np.stack(mus, 1), np.stack(Ss, 1), np.stack(ll, 1))
    return out + (Hs,) if keep_H else out


# ---------------------------------------------------------------- smoother with lag-one

def smooth(kind, mu_hist, S_hist, U, Q, dparams, mu0=None, S0=None, dtype=np.float64):
    """dict mu_s (B,T,n), S_s, C (B,T,n,n) and with a prior mu0_s, S0_s.  Only the upper triangle
    of the history's S is read (mirrored), as the kernel does."""
    f = lambda a: np.asarray(a, dtype=dtype)          # noqa: E731
    mh, Sh, U, Q = f(mu_hist), f(S_hist), f(U), f(Q)
    Sh = np.triu(Sh) + T_(np.triu(Sh, 1))
    Bn, T, n = mh.shape
    ms, Ss, C = mh.copy(), Sh.copy(), np.full_like(Sh, np.nan)
    out = {}
    prior = mu0 is not None
    for k in range(T - 1, -1 if prior else 0, -1):           # C_k and the smoothed step k-1
        mu, S = (f(mu0), f(S0)) if k == 0 else (mh[:, k - 1], Sh[:, k - 1])
        xp, F = dynamics(kind, mu, U[:, k], dparams, dtype)
        SP = F @ S @ T_(F) + Q
        G = T_(solve_spd(SP, F @ S)[0])                      # S F^T (S-)^-1
        C[:, k] = Ss[:, k] @ T_(G)
        m_new = mu + (G @ (ms[:, k] - xp)[:, :, None])[:, :, 0]
        S_new = S + G @ (Ss[:, k] - SP) @ T_(G)
        if k == 0:
            out["mu0_s"], out["S0_s"] = m_new, S_new
        else:
            ms[:, k - 1], Ss[:, k - 1] = m_new, S_new
    out.update(mu_s=ms, S_s=Ss, C=C)
    return out


# ---------------------------------------------------------------- sufficient statistics

def stats(kind, mu_s, S_s, C, U, Z, nz, sat, dparams, mu0_s=None, S0_s=None, rejected=None, dtype=np.float64,
          keep_W=False):
    """dict Qsum (B,n,n), q_cnt (B), r2 (B,T,pmax), r_cnt (B), status (B) [and W (B,K,n,n)]."""
    f = lambda a: np.asarray(a, dtype=dtype)          # noqa: E731
    ms, Ss, C, U, Z, sat = f(mu_s), f(S_s), f(C), f(U), f(Z), f(sat)
    Ss = np.triu(Ss) + T_(np.triu(Ss, 1))
    Bn, T, n = ms.shape
    pmax = Z.shape[2]
    Qsum = np.zeros((Bn, n, n), dtype=dtype)
    r2 = np.zeros((Bn, T, pmax), dtype=dtype)
    r_cnt = np.zeros(Bn, dtype=np.int32)
    status = np.zeros(Bn, dtype=np.int32)
    prior = mu0_s is not None
    W = []
    with np.errstate(all="ignore"):
        for k in range(T):
            if k > 0 or prior:
                mp, Sp = (f(mu0_s), f(S0_s)) if k == 0 else (ms[:, k - 1], Ss[:, k - 1])
                if k == 0:
                    Sp = np.triu(Sp) + T_(np.triu(Sp, 1))
                fk, F = dynamics(kind, mp, U[:, k], dparams, dtype)
                d = ms[:, k] - fk
                Wk = d[:, :, None] * d[:, None, :] + Ss[:, k] - C[:, k] @ T_(F) - F @ T_(C[:, k]) + F @ Sp @ T_(F)
                Qsum = Qsum + Wk
                W.append(Wk)
            over = nz[:, k] > pmax
            status[over] = 2
            nk = np.where(over, 0, nz[:, k])
            h, H, valid = measurement(kind, ms[:, k], sat[:, k], nk, dtype)
            if rejected is not None:
                bits = (rejected[:, k].astype(np.int64)[:, None] & 0xFFFFFFFF) >> np.arange(pmax)[None, :] & 1
                valid = valid & (bits == 0)
            e = Z[:, k] - h
            val = e ** 2 + np.einsum("bij,bjk,bik->bi", H, Ss[:, k], H)
            r2[:, k] = np.where(valid, val, 0)
            r_cnt += valid.sum(-1).astype(np.int32)
    Qsum = (Qsum + T_(Qsum)) / 2
    bad = ~(np.isfinite(Qsum).all((1, 2)) & np.isfinite(r2).all((1, 2)))
    Qsum[bad], r2[bad], status[bad] = np.nan, np.nan, 1
    out = dict(Qsum=Qsum, q_cnt=np.full(Bn, T - 1 + int(prior), dtype=np.int32), r2=r2, r_cnt=r_cnt, status=status)
    if keep_W:
        out["W"] = np.stack(W, 1) if W else np.zeros((Bn, 0, n, n), dtype=dtype)
    return out


def bounds(lo, hi, keys):
    """(ref, floor, bound) per output from a float64 and a longdouble run (NaNs must coincide)."""
    ref, floor, bound = {}, {}, {}
    for key in keys:
        a, b = np.asarray(lo[key], dtype=np.longdouble), np.asarray(hi[key], dtype=np.longdouble)
        assert (np.isnan(a) == np.isnan(b)).all(), key
        ref[key] = np.asarray(hi[key]).astype(np.float64)
        ref[key].setflags(write=False)
        fin = ~np.isnan(b)
        floor[key] = float(np.max(np.abs(a - b)[fin], initial=0.0))
        bound[key] = 8.0 * floor[key] + 1e-10 * (1.0 + float(np.max(np.abs(ref[key][fin]), initial=0.0)))
    return ref, floor, bound


def both(fn, keys, *a, **kw):
    """fn in float64 and in np.longdouble; the longdouble run rounded per output, with
    "floor", "bound" and "f64"."""
    require_extended()
    lo, hi = fn(*a, dtype=np.float64, **kw), fn(*a, dtype=np.longdouble, **kw)
    ref, floor, bound = bounds(lo, hi, keys)
    for key in hi:
        if key not in ref:
            ref[key] = hi[key]
    ref.update(floor=floor, bound=bound, f64=lo)
    return ref


def check(what, got, ref, key):
    """Print observed, floor and bound, then assert; NaNs must sit where the reference's do."""
    got = np.asarray(got, dtype=np.float64)
    want = ref[key]
    assert got.shape == want.shape, (what, key, got.shape, want.shape)
    nan = np.isnan(want)
    assert (np.isnan(got) == nan).all(), f"{what} {key}: NaN pattern differs"
    err = float(np.max(np.abs(got - want)[~nan], initial=0.0))
    print(f"{what} {key}: observed {err:.3e}, floor {ref['floor'][key]:.3e}, bound {ref['bound'][key]:.3e}")
    assert err <= ref["bound"][key], (what, key, err, ref["bound"][key])
    return err


# ---------------------------------------------------------------- the fitting loop

def fit(kind, mu0, S0, U, Z, nz, sat, Q, R, dparams, rounds=FIT_ROUNDS, dtype=np.float64):
    """utils.ekf.fit_noise's loop (full Q, one scale on a diagonal R, no gate).  dict Q, R, rho,
    loglik (rounds,)."""
    Q, R = np.asarray(Q, dtype=dtype), np.asarray(R, dtype=dtype)
    rho, ll = dtype(1), []
    for _ in range(rounds):
        mh, Sh, lk = forward(kind, mu0, S0, U, Z, nz, sat, Q, R, dparams, dtype)
        sm = smooth(kind, mh, Sh, U, Q, dparams, mu0, S0, dtype)
        st = stats(kind, sm["mu_s"], sm["S_s"], sm["C"], U, Z, nz, sat, dparams, sm["mu0_s"], sm["S0_s"], dtype=dtype)
        assert not st["status"].any()
        ll.append(lk.sum())
        Q = st["Qsum"].sum(0) / st["q_cnt"].sum()
        Rd = np.diagonal(R, axis1=-2, axis2=-1)
        with np.errstate(all="ignore"):
            ratio = np.where(st["r2"] > 0, st["r2"] / Rd, 0)
        rr = ratio.sum() / st["r_cnt"].sum()
        R, rho = R * rr, rho * rr
    return dict(Q=Q, R=R, rho=np.asarray(rho, dtype=dtype), loglik=np.asarray(ll, dtype=dtype))


FIT_Q_TRUE = np.diag([0.5, 0.5, 0.5, 2.0, 0.01])
FIT_R_TRUE, FIT_R_START, FIT_Q_SCALE = 9.0, 100.0, 50.0
FIT_S0 = np.diag([25.0, 25.0, 25.0, 100.0, 1.0])


def make_fit_recipe(B=8, T=40, pmax=8, seed=5):
    """The synthetic gnss log of the fit test: satellites er.satellites(fx, default_rng(5), 40, 8),
    truth Q = diag(0.5, 0.5, 0.5, 2, 0.01) and r = 9, prior mean at the fixture's last mean with
    S0 = diag(25, 25, 25, 100, 1) and the true initial states drawn from it, U = 0, every step
    with all pmax rows.  tests/golden/em_fit_gnss.npz holds exactly these arrays."""
    fx = er.gnss_fixture()
    rng = np.random.default_rng(seed)
    sat = np.repeat(er.satellites(fx, rng, T, pmax)[None], B, 0)
    mean = fx["mu"][-1].copy()
    x = mean + rng.normal(size=(B, 5)) * np.sqrt(np.diag(FIT_S0))
    U = np.zeros((B, T, 3))
    Z = np.zeros((B, T, pmax))
    nz = np.full((B, T), pmax, dtype=np.int32)
    for k in range(T):
        x, _ = dynamics(GNSS, x, U[:, k], {"dt": 1.0}, np.float64)
        x = x + rng.normal(size=(B, 5)) * np.sqrt(np.diag(FIT_Q_TRUE))
        h, _, _ = measurement(GNSS, x, sat[:, k], nz[:, k], np.float64)
        Z[:, k] = h + np.sqrt(FIT_R_TRUE) * rng.normal(size=(B, pmax))
    return dict(mu0=np.tile(mean, (B, 1)), S0=np.tile(FIT_S0, (B, 1, 1)), U=U, Z=Z, nz=nz, sat=sat)


def fit_inputs():
    """The committed fixture plus the start of the fit: Q = 50 Q_true, R = 100 I."""
    d = dict(np.load(FIT_FIXTURE))
    T, pmax = d["Z"].shape[1:]
    d["Q"] = FIT_Q_SCALE * FIT_Q_TRUE
    d["R"] = np.repeat((FIT_R_START * np.eye(pmax))[None], T, 0)
    d["dparams"] = {"dt": 1.0}
    return d


_FIT = {}


def fit_reference():
    """fit() on the fixture in float64 and longdouble, once per process."""
    if not _FIT:
        d = fit_inputs()
        a = (GNSS, d["mu0"], d["S0"], d["U"], d["Z"], d["nz"], d["sat"], d["Q"], d["R"], d["dparams"])
        _FIT.update(both(lambda dtype: fit(*a, dtype=dtype), ("Q", "rho", "loglik")))
    return _FIT
