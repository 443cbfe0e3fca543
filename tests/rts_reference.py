"""Textbook Rauch-Tung-Striebel smoother in NumPy -- TEST INFRASTRUCTURE ONLY.

The reference of tests/test_ekf_smooth_host.py and tests/test_gpu_ekf_smooth.py: full
matrices and np.linalg.solve on top of oracle/ekf.py's dynamics plug-ins, independent of the
kernel's triangle and column scheme (csrc/mhe_ekf.hip, k_ekf_rts).  Given the filtered
history (mu_k, S_k), k = 0..T-1, of a filter that predicted with x-_{k+1} = f(mu_k, u_{k+1}):

    (x-, G) = f(mu_k, u_{k+1});  S- = G S_k G^T + Q;  C = S_k G^T (S-)^-1
    mu_s[k] = mu_k + C (mu_s[k+1] - x-);  S_s[k] = S_k + C (S_s[k+1] - S-) C^T

from k = T-2 down to 0, with mu_s[T-1], S_s[T-1] the filtered values.  The smoothed prior
is one more step of the recursion from (mu0, S0) with u_0.
"""
import numpy as np


def _step(dyn, mu, S, u, Q, dparams, mu_next, S_next):
    xp, G = dyn(mu, u, params=dparams, jac=True)
    SP = G @ (S @ G.T) + Q
    C = np.linalg.solve(SP, G @ S).T          # S G^T SP^-1 (S and SP symmetric)
    return mu + C @ (mu_next - xp), S + C @ (S_next - SP) @ C.T


def smooth(dyn, mu_hist, S_hist, U, Q, dparams, mu0=None, S0=None):
    """One filter: mu_hist (T,n), S_hist (T,n,n), U (T,m).  Returns (mu_s, S_s), and with a
    prior (mu_s, S_s, mu0_s, S0_s).  The inputs are left unchanged."""
    mu_hist, S_hist = np.asarray(mu_hist, dtype=np.float64), np.asarray(S_hist, dtype=np.float64)
    T = mu_hist.shape[0]
    ms, Ss = mu_hist.copy(), S_hist.copy()
    for k in range(T - 2, -1, -1):
        ms[k], Ss[k] = _step(dyn, mu_hist[k], S_hist[k], U[k + 1], Q, dparams, ms[k + 1], Ss[k + 1])
    if mu0 is None:
        return ms, Ss
    m0, S0s = _step(dyn, np.asarray(mu0, dtype=np.float64), np.asarray(S0, dtype=np.float64), U[0], Q, dparams,
                    ms[0], Ss[0])
    return ms, Ss, m0, S0s


def smooth_batch(dyn, mu_hist, S_hist, U, Q, dparams, mu0=None, S0=None):
    """Every filter of a batch: mu_hist (B,T,n), S_hist (B,T,n,n), U (B,T,m), priors (B,n) /
    (B,n,n).  Returns stacked arrays in the order of `smooth`."""
    B = mu_hist.shape[0]
    out = [smooth(dyn, mu_hist[b], S_hist[b], U[b], Q, dparams, None if mu0 is None else mu0[b],
                  None if S0 is None else S0[b]) for b in range(B)]
    return tuple(np.stack([o[i] for o in out]) for i in range(len(out[0])))
