"""Unscented Kalman filter on the GPU -- the Jacobian-free companion of ``utils.ekf``.

``run_batch`` runs many independent filters over many steps in one launch of
``mhe_ukf_run`` (csrc/mhe_ukf.hip, one wavefront per filter); ``UKF(dyn_func, meas_func,
mu0, S0)`` / ``UKF.update(u, z, Q, R, ...)`` have ``utils.ekf.EKF``'s signature and
semantics, one launch per update.  The filter is the additive-noise UKF with the scaled
unscented transform (include/mhe.h states the recursion): sigma points are redrawn from
the prediction before the correction, the measurement values are centred on z before
they are averaged, and the correction is a Cholesky sweep of Pzz with no explicit inverse.

Only the plug-ins' *values* enter, so neither of the EKF's reference-compatible Jacobian
quirks does: the bias row of ``multi_pseudorange_and_bias`` (h = x[3]) acts here, and
``discrete_vehicle_dynamics`` is its plain Euler step.  Plug-ins resolve and are verified
exactly as for the EKF (``utils.ekf.models`` / ``verify``); there is no CPU path.

Why the defaults are alpha = 1, beta = 0, kappa = 0: they give lambda = 0, that is 2n
equally weighted points and no negative weight.  With the textbook alpha = 1e-3 the
centre weight is about -1e6 and the weighted sums cancel at that magnitude: in float64
the rounding floor of the gnss position rose from 1.6e-6 m to 1.6e-3 m.  alpha, beta and
kappa remain parameters.

``smooth_batch`` is the unscented fixed-interval (RTS) smoother over the history
``run_batch`` returns (``mhe_ukf_smooth``, k_ukf_rts): the backward pass by the same sigma
points and the dynamics' values.  ``utils.ekf.smooth_batch`` over a UKF history is the
EKF-linearised smoother instead, which puts the hand-written Jacobians back in.

``run_batch(gate=...)`` / ``UKF.update(gate=...)`` screen rows on their normalised innovation
d2_i = e_i^2 / Pzz_ii as ``utils.ekf`` does and report the rejection mask (``mhe_ukf_run_gated``,
k_ukf<.., GATE>); without ``gate`` the call is ``mhe_ukf_run``'s and its instances, as before.

Not formed: a filter-per-lane kernel, two filters per wave, joint (chi-square of nz) gating.
"""
import ctypes
import math

import numpy as np

from mhe import _lib

from . import ekf as _ekf

MAXP = _ekf.MAXP


def _real(v):
    return not isinstance(v, (bool, np.bool_)) and isinstance(v, (int, float, np.integer, np.floating))


def sigma_params(alpha, beta, kappa, n):
    """(alpha, beta, kappa) as floats, or ValueError: alpha must be finite and > 0, beta and
    kappa finite, and n + kappa > 0 (so that n + lambda = alpha^2 (n + kappa) > 0)."""
    for name, v in (("alpha", alpha), ("beta", beta), ("kappa", kappa)):
        if not _real(v) or not math.isfinite(float(v)):
            raise ValueError(f"{name} must be a finite number, not {v!r}")
    if not float(alpha) > 0.0:
        raise ValueError(f"alpha must be > 0, not {alpha!r}")
    if not n + float(kappa) > 0.0:
        raise ValueError(f"n + kappa must be > 0 (n = {n}, kappa = {kappa!r})")
    s = float(alpha) * float(alpha) * (n + float(kappa))
    if not (s > 0.0 and math.isfinite(s)):
        raise ValueError(f"alpha^2 (n + kappa) = {s!r} is not a positive finite number")
    return float(alpha), float(beta), float(kappa)


def run_batch(dyn_func, meas_func, mu0, S0, U, Z, nz, Q, R, dt, sat_pos, device=None, stream=None,
              keep_history=True, inputs="batch_outer", dyn_params=None, alpha=1.0, beta=0.0, kappa=0.0,
              innovations=False, **screen):
    """Run B independent unscented filters for T steps in one launch.

    Shapes, layouts (``inputs``) and ``stream`` are ``utils.ekf.run_batch``'s: mu0 (B,n),
    S0 (B,n,n), U (B,T,m), Z (B,T,pmax), nz (B,T) valid rows per step (0 = predict only),
    Q (n,n), R (T,pmax,pmax) or (B,T,pmax,pmax), sat_pos (B,T,pmax,3); only the upper
    triangles of Q and R are read.
    Returns (mu_hist (B,T,n), S_hist (B,T,n,n), mu (B,n), S (B,n,n), status (B)) on the
    device; S_hist and S are bitwise symmetric.  status: 0 ok; 1 a Cholesky pivot of S, S-
    or Pzz was not positive and finite -- that filter's history from that step on and its
    final mu / S are NaN, no other filter is touched; 2 nz > pmax at some step (that step is
    predict-only).
    innovations=True appends (nis (B,T), loglik (B,T)): nis = e^T Pzz^-1 e and
    loglik = -(nis + log det Pzz + nz log 2 pi) / 2, both 0 on a step without a correction.
    alpha, beta, kappa: the scaled unscented transform's parameters (see the module
    docstring for the defaults); a bad value raises ValueError.
    gate (keyword only, default None; the named parameters are the ungated call's, which
    tests/test_ukf_host.py pins): None, or a threshold > 0 on the normalised innovation of each row at the prediction,
    d2_i = e_i^2 / Pzz_ii with e and Pzz (R included) of the redrawn sigma points: a row with
    d2_i > gate is screened out and the correction is the usual one over the rows that remain,
    exactly the ungated filter fed only those rows (none: the step is predict-only).  Rows
    keep their index.  10.83 is the 0.999 quantile of chi-square with one degree of freedom;
    np.inf screens nothing.  With a gate, innovations=True appends (nis (B,T), loglik (B,T),
    rejected (B,T) int32) as ``utils.ekf.run_batch`` does: nis and loglik over the kept rows
    (0 when no row was applied), bit i of rejected set iff row i was screened out.  A bad
    gate raises ValueError.  Without ``gate`` the call, the entry point (mhe_ukf_run) and the
    returned tuple are what they were."""
    gate = screen.pop("gate", None)
    if screen:
        raise TypeError(f"run_batch() got an unexpected keyword argument {next(iter(screen))!r}")
    gated = gate is not None
    gate = _ekf._gate_value(gate)
    (did, n, m), (mid, _, q) = _ekf.models(dyn_func, meas_func)
    alpha, beta, kappa = sigma_params(alpha, beta, kappa, n)
    import torch

    from mhe.streams import launch_stream

    if dyn_params is not None and "dt" in dyn_params:
        dt = dyn_params["dt"]
    _ekf.verify(dyn_func, meas_func, dict(dyn_params or {}, dt=dt))
    dp = _ekf.dyn_par(dyn_func, dyn_params)
    dev = torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())
    with launch_stream(stream, dev) as (s, cur):
        return _run_batch(did, n, m, mid, q, dev, s, cur, mu0, S0, U, Z, nz, Q, R, dt, sat_pos, keep_history,
                          inputs, dp, alpha, beta, kappa, bool(innovations), gate if gated else None)


def _run_batch(did, n, m, mid, q, dev, s, cur, mu0, S0, U, Z, nz, Q, R, dt, sat_pos, keep_history, inputs, dp,
               alpha, beta, kappa, innovations, gate=None):
    """run_batch on torch stream s (staging and allocation ordered on s)."""
    import torch

    from mhe.streams import keep_alive

    def d(a, dt_=torch.float64):
        return torch.as_tensor(np.asarray(a) if not torch.is_tensor(a) else a, dtype=dt_, device=dev).contiguous()

    mu = d(mu0).clone()
    S = d(S0).clone()
    B = mu.shape[0]
    Zt = d(Z)
    bi = inputs == "batch_inner"
    if inputs not in ("batch_outer", "batch_inner"):
        raise ValueError(f"unknown inputs layout {inputs!r}")
    T, pmax = (Zt.shape[0], Zt.shape[1]) if bi else (Zt.shape[1], Zt.shape[2])
    if pmax > MAXP:
        raise ValueError(f"at most {MAXP} measurement rows per step")
    Ut = d(U)
    nzt = d(nz, torch.int32)
    Pt = d(sat_pos)
    Rt = d(R)
    Qt = d(Q)
    shapes = ((T, m, B), (T, B), (T, pmax, q, B), (T, pmax, B)) if bi else \
        ((B, T, m), (B, T), (B, T, pmax, q), (B, T, pmax))
    if mu.shape != (B, n) or S.shape != (B, n, n) or Ut.shape != shapes[0] or nzt.shape != shapes[1] \
            or Pt.shape != shapes[2] or Zt.shape != shapes[3] or Qt.shape != (n, n):
        raise ValueError("run_batch: inconsistent shapes")
    if Rt.dim() == 3:
        r_b, r_s = 0, pmax * pmax
        if Rt.shape != (T, pmax, pmax):
            raise ValueError("R must be (T,pmax,pmax) or (B,T,pmax,pmax)")
    else:
        r_b, r_s = T * pmax * pmax, pmax * pmax
        if Rt.shape != (B, T, pmax, pmax):
            raise ValueError("R must be (T,pmax,pmax) or (B,T,pmax,pmax)")
    # histories and statistics are written batch-innermost (coalesced device stores) and
    # returned as (B, T, ...) views of that storage
    mh_st = torch.empty((T, n, B), dtype=torch.float64, device=dev) if keep_history else None
    Sh_st = torch.empty((T, n, n, B), dtype=torch.float64, device=dev) if keep_history else None
    st = torch.empty(B, dtype=torch.int32, device=dev)
    kinds = (torch.float64, torch.float64) + ((torch.int32,) if gate is not None else ())
    stats = tuple(torch.empty((T, B), dtype=dt_, device=dev) for dt_ in kinds) if innovations else ()
    nis, ll, rej = (stats + (None,))[:3] if innovations else (None, None, None)
    dims = _lib.MheEkfDims(n=n, m=m, pmax=pmax, q=q, dyn_model=did, meas_model=mid, dt=float(dt),
                           hist_batch_inner=1, in_batch_inner=int(bi))
    for i in range(8):
        dims.dyn_par[i] = float(dp[i])
    p = _ekf._ptr
    fields = dict(batch=B, steps=T, mu=mu.data_ptr(), S=S.data_ptr(), U=Ut.data_ptr(), u_bstride=T * m,
                  Z=Zt.data_ptr(), z_bstride=T * pmax, nz=nzt.data_ptr(), nz_bstride=T,
                  PAR=Pt.data_ptr(), par_bstride=T * pmax * q, Q=Qt.data_ptr(), R=Rt.data_ptr(),
                  r_bstride=r_b, r_sstride=r_s, mu_hist=p(mh_st), S_hist=p(Sh_st), status=st.data_ptr(),
                  alpha=alpha, beta=beta, kappa=kappa, nis=p(nis), loglik=p(ll))
    if gate is None:
        args = _lib.MheUkfArgs(**fields)
        rc = _lib.load().mhe_ukf_run(ctypes.byref(dims), ctypes.byref(args), ctypes.c_void_p(s.cuda_stream))
        _lib.check(rc, "mhe_ukf_run")
    else:
        args = _lib.MheUkfGateArgs(gate=gate, rej=p(rej), **fields)
        rc = _lib.load().mhe_ukf_run_gated(ctypes.byref(dims), ctypes.byref(args), ctypes.c_void_p(s.cuda_stream))
        _lib.check(rc, "mhe_ukf_run_gated")
    keep_alive(s, cur, mu, S, Ut, Zt, nzt, Pt, Qt, Rt, mh_st, Sh_st, st, *stats)
    mh = mh_st.permute(2, 0, 1) if keep_history else None
    Sh = Sh_st.permute(3, 0, 1, 2) if keep_history else None
    return (mh, Sh, mu, S, st) + tuple(t.permute(1, 0) for t in stats)


def smooth_batch(dyn_func, mu_hist, S_hist, U, Q, dt, mu0=None, S0=None, dyn_params=None, inputs="batch_outer",
                 alpha=1.0, beta=0.0, kappa=0.0, device=None, stream=None):
    """Unscented fixed-interval (Rauch-Tung-Striebel) smoother over a filtered history, B
    filters in one launch of ``mhe_ukf_smooth`` (one wavefront per filter; include/mhe.h
    states the recursion).  The backward pass redoes the forward's prediction from the
    dynamics' values and the same sigma points: no Jacobian enters.

    Arguments, shapes, layouts and ``stream`` are ``utils.ekf.smooth_batch``'s: mu_hist (B,T,n),
    S_hist (B,T,n,n) as ``run_batch`` returned them (its batch-innermost views go to the kernel
    without a copy), U (B,T,m) -- or (T,m,B) with inputs="batch_inner" -- Q (n,n), dt and
    dyn_params as given to ``run_batch``; mu0 (B,n), S0 (B,n,n) optionally the prior the filter
    started from.  alpha, beta, kappa: the forward run's (a bad value raises ValueError).
    Returns (mu_s (B,T,n), S_s (B,T,n,n), status (B)) and, with a prior, also (mu0_s (B,n),
    S0_s (B,n,n)); S_s is bitwise symmetric.  status 1: a Cholesky pivot of S_k or of the
    predicted covariance was not positive and finite, or the history held a non-finite value;
    that filter is NaN from the failing step down, no other filter is touched.
    Measurements do not enter the backward pass, so the history of a gated run (run_batch's
    ``gate``) smooths as any other."""
    did, n, m = _ekf.dynamics(dyn_func)
    alpha, beta, kappa = sigma_params(alpha, beta, kappa, n)
    if dyn_params is not None and "dt" in dyn_params:
        dt = dyn_params["dt"]
    if inputs not in ("batch_outer", "batch_inner"):
        raise ValueError(f"unknown inputs layout {inputs!r}")
    if (mu0 is None) != (S0 is None):
        raise ValueError("smooth_batch: mu0 and S0 go together")
    bi = inputs == "batch_inner"
    shp = lambda a: tuple(a.shape)   # noqa: E731
    if len(shp(mu_hist)) != 3 or len(shp(S_hist)) != 4:
        raise ValueError("smooth_batch: mu_hist must be (B,T,n) and S_hist (B,T,n,n)")
    B, T = shp(mu_hist)[:2]
    if shp(mu_hist) != (B, T, n) or shp(S_hist) != (B, T, n, n) or shp(Q) != (n, n) \
            or shp(U) != ((T, m, B) if bi else (B, T, m)) \
            or (mu0 is not None and (shp(mu0) != (B, n) or shp(S0) != (B, n, n))):
        raise ValueError("smooth_batch: inconsistent shapes")
    _ekf.verify_dynamics(dyn_func, dict(dyn_params or {}, dt=dt))
    dp = _ekf.dyn_par(dyn_func, dyn_params)
    import torch

    from mhe.streams import keep_alive, launch_stream

    dev = torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())
    with launch_stream(stream, dev) as (s, cur):
        def d(a):
            return torch.as_tensor(np.asarray(a) if not torch.is_tensor(a) else a, dtype=torch.float64, device=dev)

        mh, mh_bi = _ekf._hist_storage(d(mu_hist), (n,))
        Sh, Sh_bi = _ekf._hist_storage(d(S_hist), (n, n))
        if mh_bi != Sh_bi:   # one layout flag covers both histories
            mh, Sh, mh_bi = d(mu_hist).contiguous(), d(S_hist).contiguous(), False
        Ut, Qt = d(U).contiguous(), d(Q).contiguous()
        prior = mu0 is not None
        m0, S0t = (d(mu0).contiguous(), d(S0).contiguous()) if prior else (None, None)
        ms, Ss = torch.empty_like(mh), torch.empty_like(Sh)
        m0s, S0s = (torch.empty_like(m0), torch.empty_like(S0t)) if prior else (None, None)
        st = torch.empty(B, dtype=torch.int32, device=dev)
        dims = _lib.MheEkfDims(n=n, m=m, dyn_model=did, dt=float(dt), hist_batch_inner=int(mh_bi),
                               in_batch_inner=int(bi))
        for i in range(8):
            dims.dyn_par[i] = float(dp[i])
        p = lambda t: None if t is None else t.data_ptr()   # noqa: E731
        args = _lib.MheUkfSmoothArgs(batch=B, steps=T, mu_hist=p(mh), S_hist=p(Sh), U=p(Ut), u_bstride=T * m,
                                     Q=p(Qt), mu0=p(m0), S0=p(S0t), mu_s=p(ms), S_s=p(Ss), mu0_s=p(m0s),
                                     S0_s=p(S0s), status=p(st), alpha=alpha, beta=beta, kappa=kappa)
        rc = _lib.load().mhe_ukf_smooth(ctypes.byref(dims), ctypes.byref(args), ctypes.c_void_p(s.cuda_stream))
        _lib.check(rc, "mhe_ukf_smooth")
        keep_alive(s, cur, mh, Sh, Ut, Qt, m0, S0t, ms, Ss, m0s, S0s, st)
        if mh_bi:
            ms, Ss = ms.permute(2, 0, 1), Ss.permute(3, 0, 1, 2)
        return (ms, Ss, st, m0s, S0s) if prior else (ms, Ss, st)


class UKF(object):
    """``utils.ekf.EKF``'s interface on the unscented filter."""

    def __init__(self, dyn_func, meas_func, mu0, S0, alpha=1.0, beta=0.0, kappa=0.0):
        (_, n, _), _ = _ekf.models(dyn_func, meas_func)  # fail at construction for unregistered plug-ins
        self.alpha, self.beta, self.kappa = sigma_params(alpha, beta, kappa, n)
        self.mu = mu0
        self.S = S0
        self.dynamics = dyn_func
        self.measurement = meas_func

    def update(self, u, z, Q, R, dyn_func_params=None, meas_func=None, meas_func_params=None, gate=None):
        """One predict (+ correct when z is given) step: one launch.  Status 1 raises
        np.linalg.LinAlgError and leaves mu / S as they were.

        gate (run_batch's; np.inf: statistics only): rows of z whose normalised innovation
        exceeds it are left out of the correction, and the object then holds ``nis``,
        ``loglik`` (floats) and ``rejected`` (bool, one per row of z) of this update.
        Without a gate nothing changes."""
        gv = _ekf._gate_value(gate)
        meas = meas_func if meas_func is not None else self.measurement
        (_, n, m), (_, extra, q) = _ekf.models(self.dynamics, meas)
        dt = float((dyn_func_params or {})["dt"])
        mu0 = np.asarray(self.mu, dtype=np.float64).reshape(1, n)
        S0 = np.asarray(self.S, dtype=np.float64).reshape(1, n, n)
        u_ = np.asarray(u, dtype=np.float64).reshape(1, 1, m)
        if z is None:
            pmax, nz = 1, 0
            Z = np.zeros((1, 1, 1))
            P = np.zeros((1, 1, 1, q))
            Rm = np.zeros((1, 1, 1))
        else:
            zz = np.atleast_1d(np.asarray(z, dtype=np.float64))
            nz = pmax = zz.shape[0]
            Z = zz.reshape(1, 1, pmax)
            sp = np.asarray(meas_func_params["sat_pos"], dtype=np.float64).reshape(-1, q)
            if sp.shape[0] + extra != nz:
                raise ValueError("z and meas_func_params['sat_pos'] disagree in size")
            P = np.zeros((1, 1, pmax, q))
            P[0, 0, :sp.shape[0]] = sp
            Rm = np.asarray(R, dtype=np.float64).reshape(1, pmax, pmax)
        kw = {} if gate is None else dict(gate=gv, innovations=True)
        out = run_batch(self.dynamics, meas, mu0, S0, u_, Z, np.full((1, 1), nz, np.int32),
                        np.asarray(Q, dtype=np.float64), Rm, dt, P, keep_history=False,
                        dyn_params=dyn_func_params, alpha=self.alpha, beta=self.beta, kappa=self.kappa, **kw)
        mu, S, st = out[2:5]
        if int(st[0].item()) != 0:
            raise np.linalg.LinAlgError("a covariance of the unscented filter is not positive definite")
        if gate is not None:
            self.nis, self.loglik = float(out[5][0, 0].item()), float(out[6][0, 0].item())
            word = int(out[7][0, 0].item()) & 0xFFFFFFFF
            self.rejected = np.array([bool((word >> i) & 1) for i in range(nz)], dtype=bool)
        self.mu = mu[0].cpu().numpy()
        self.S = S[0].cpu().numpy()
