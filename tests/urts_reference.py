"""NumPy reference of the unscented RTS smoother (utils.ukf.smooth_batch, mhe_ukf_smooth), for
tests/test_urts_host.py and tests/test_gpu_urts.py.

The backward recursion of include/mhe.h, written once, generic in dtype and vectorised over the
batch, on tests/ukf_reference.py's weights, sigma_points, wsum, dyn_value, cholesky and forward
plus the back substitution below -- no LAPACK, so the np.longdouble run really is an
extended-precision run.  Carrying (mu_s, S_s) of step k+1 (the filtered values at step T-1), for
k = T-2 .. 0 and once more from the prior (mu0, S0) with u_0:

    S_k = L L^T (upper triangle read, mirrored);  X_j the sigma points of (mu_k, L)
    Y_j = f(X_j, u_{k+1});  mu- = sum wm_j Y_j;  S- = sum wc_j (Y_j - mu-)(Y_j - mu-)^T + Q
    C = sum wc_j (X_j - mu_k)(Y_j - mu-)^T;  S- = L- L-^T;  M = S-^-1 C^T
    mu_s[k] = mu_k + M^T (mu_s[k+1] - mu-);  S_s[k] = S_k + M^T (S_s[k+1] - S-) M

Failure (status 1): a pivot of S_k or S- is not positive and finite, or a value written at a
step is not finite; that filter's outputs are NaN from that step down to step 0 and in the
smoothed prior.

`reference(name, params)` runs it in float64 and in np.longdouble on the float64 forward history
ukf_reference.reference(name, params)["f64"] with that case's mu0, S0, U and Q.  Per output,
floor = max |float64 run - longdouble run| and
    bound = 8 * floor + 1e-10 * (1 + max |ref|)
(tests/ukf_reference.py's form: the 8 covers a different but fixed summation order and FMA
contraction).  The bound comes from the reference alone.
"""
import functools

import numpy as np

import ukf_reference as ur

OUTPUTS = ("mu_s", "S_s", "mu0_s", "S0_s")


def backward(L, Y):
    """L^-T Y for lower-triangular L (B, N, N) and Y (B, N, K), row by row from the last."""
    Y = Y.copy()
    N = L.shape[1]
    M = np.zeros_like(Y)
    with np.errstate(all="ignore"):
        for c in range(N - 1, -1, -1):
            M[:, c] = Y[:, c] / L[:, c, c, None]
            Y[:, :c] = Y[:, :c] - L[:, c, :c, None] * M[:, None, c]
    return M


def mirror(S):
    """The matrix the upper triangle of S (B, n, n) stands for."""
    up = np.triu(S)
    return up + np.swapaxes(np.triu(S, 1), -1, -2)


def step(kind, inp, weights, mu, S, u, Q, mu_next, S_next, dtype):
    """One step of the recursion for the whole batch.  Returns (mu_s, S_s, ok (B), margin (B),
    pred): ok is False where a pivot of S_k or S- failed, margin the smallest pivot / diagonal
    entry of the two factorisations, pred the recomputed (mu-, S-)."""
    c, wm, wc = weights
    n = mu.shape[1]
    alln = np.ones((mu.shape[0], n), dtype=bool)
    S = mirror(S)
    L, ok1, m1 = ur.cholesky(S, alln)
    X = ur.sigma_points(mu, L, c)
    Y = ur.dyn_value(kind, X, u, inp, dtype)
    mp = ur.wsum(wm, Y)
    D = Y - mp[:, None, :]
    SP = ur.wsum(wc, D[:, :, :, None] * D[:, :, None, :]) + Q[None]
    C = ur.wsum(wc, (X - mu[:, None, :])[:, :, :, None] * D[:, :, None, :])          # (B, n, n)
    Lp, ok2, m2 = ur.cholesky(SP, alln)
    M = backward(Lp, ur.forward(Lp, np.swapaxes(C, 1, 2)))                            # S-^-1 C^T
    G = np.swapaxes(M, 1, 2)
    dmu, E = np.zeros_like(mu), np.zeros_like(S)
    dS = S_next - SP
    for i in range(n):                                                                # fixed order
        dmu = dmu + G[:, :, i] * (mu_next - mp)[:, None, i]
        E = E + dS[:, :, i, None] * G[:, None, :, i]                                  # E = D G^T
    GE = np.zeros_like(S)
    for i in range(n):
        GE = GE + G[:, :, i, None] * E[:, i, None, :]
    Ss = mirror(S + GE)
    return mu + dmu, Ss, ok1 & ok2, np.minimum(m1, m2), (mp, SP)


def smooth(inp, kind, mu_hist, S_hist, params=ur.PARAMS[0], dtype=np.float64, prior=True):
    """The smoother on every instance.  mu_hist (B,T,n), S_hist (B,T,n,n); U, Q and the prior
    are inp's.  Returns a dict: mu_s, S_s, mu0_s, S0_s (the last two None without a prior),
    status (B), fail_step (B; T: none, -1: the prior's step only), margin (the smallest
    Cholesky pivot / diagonal entry met on a live filter)."""
    f = lambda a: np.asarray(a, dtype=dtype)                      # noqa: E731
    mh, Sh, U, Q = f(mu_hist), f(S_hist), f(inp["U"]), f(inp["Q"])
    Q = mirror(Q[None])[0]
    Bn, T, n = mh.shape
    w = ur.weights(*params, n, dtype)
    ms, Ss = np.zeros_like(mh), np.zeros_like(Sh)
    out = {"fail_step": np.full(Bn, T), "margin": np.inf, "mu0_s": None, "S0_s": None}

    def finite(mu, S):
        return np.isfinite(mu).all(axis=1) & np.isfinite(S).all(axis=(1, 2))

    def put(k, mu, S, dead):
        new = dead & (out["fail_step"] == T)
        out["fail_step"][new] = k
        mu, S = mu.copy(), S.copy()
        mu[dead], S[dead] = np.nan, np.nan
        return mu, S

    with np.errstate(all="ignore"):
        mu, S = mh[:, -1].copy(), mirror(Sh[:, -1])
        dead = ~finite(mu, S)
        mu, S = put(T - 1, mu, S, dead)
        ms[:, -1], Ss[:, -1] = mu, S
        for k in range(T - 2, -2 if prior else -1, -1):
            src = (f(inp["mu0"]), f(inp["S0"])) if k < 0 else (mh[:, k], Sh[:, k])
            mu, S, ok, margin, _ = step(kind, inp, w, src[0], src[1], U[:, k + 1], Q, mu, S, dtype)
            out["margin"] = min(out["margin"], float(np.min(margin[~dead], initial=np.inf)))
            dead = dead | ~ok | ~finite(mu, S)
            mu, S = put(k, mu, S, dead)
            if k < 0:
                out["mu0_s"], out["S0_s"] = mu, S
            else:
                ms[:, k], Ss[:, k] = mu, S
    out.update(mu_s=ms, S_s=Ss, status=dead.astype(np.int32))
    return out


def bounds(lo, hi):
    """(ref, floor, bound) per output from a float64 and a longdouble run."""
    ref, floor, bound = {}, {}, {}
    for key in OUTPUTS:
        ref[key] = hi[key].astype(np.float64)
        ref[key].setflags(write=False)
        floor[key] = float(np.max(np.abs(lo[key].astype(np.longdouble) - hi[key])))
        bound[key] = 8.0 * floor[key] + 1e-10 * (1.0 + float(np.max(np.abs(ref[key]))))
    return ref, floor, bound


def on_history(name, params, mu_hist, S_hist):
    """Both runs of the smoother on a given float64 history of a case: the longdouble run
    rounded to float64 per output, with "floor", "bound", "status", "margin", "f64"."""
    ur.require_extended()
    inp, kind = ur.inputs(name), ur.KIND[name]
    lo = smooth(inp, kind, mu_hist, S_hist, params, np.float64)
    hi = smooth(inp, kind, mu_hist, S_hist, params, np.longdouble)
    res, floor, bound = bounds(lo, hi)
    res.update(floor=floor, bound=bound, status=hi["status"], margin=min(lo["margin"], hi["margin"]), f64=lo)
    return res


@functools.lru_cache(maxsize=None)
def history(name, params=ur.PARAMS[0]):
    """The float64 forward history of a case, (mu (B,T,n), S (B,T,n,n)), read-only."""
    fwd = ur.reference(name, params)["f64"]
    mh, Sh = fwd["mu"].astype(np.float64), fwd["S"].astype(np.float64)
    mh.setflags(write=False)
    Sh.setflags(write=False)
    return mh, Sh


@functools.lru_cache(maxsize=None)
def reference(name, params=ur.PARAMS[0]):
    """Computed once and shared: the smoother on the float64 forward history of the case."""
    return on_history(name, params, *history(name, params))
