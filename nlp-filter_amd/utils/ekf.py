"""Extended Kalman filter on the GPU -- drop-in for kingdwd/nlp-filter utils/ekf.py.

``EKF(dyn_func, meas_func, mu0, S0)`` and ``EKF.update(u, z, Q, R,
dyn_func_params, meas_func, meas_func_params)`` keep the reference signatures
and semantics (utils/ekf.py:11-38): ``mu`` / ``S`` are NumPy arrays replaced by
each update; ``z=None`` predicts only.  Each update is one launch of
``mhe_ekf_run`` (csrc/mhe_ekf.hip); ``run_batch`` runs many independent filter
instances over many steps in a single launch (the GPU-shaped entry point), and
``smooth_batch`` is the fixed-interval (RTS) smoother over the history it returns
(``mhe_ekf_smooth``).
Plug-ins are resolved by name (``utils.gnss.EKF_DYN`` / ``EKF_MEAS``: the
utils/gnss.py models and autonomous-car.py's own ``discrete_vehicle_dynamics`` /
``vehicle_sensors_model``); a user's callable is then evaluated at seeded points
against the registered twin (``utils.gnss``, ``utils.vehicle``) and refused on any
difference.  An unregistered or mismatching plug-in raises ``UnsupportedPlugin`` --
there is no CPU path.

Numerics: the reference forms inv(P) (utils/ekf.py:55); the kernel uses a
Cholesky sweep of P, so results agree to floating-point rounding (tests state
the tolerance).
"""
import ctypes

import numpy as np

from mhe import _lib
from mhe.registry import UnsupportedPlugin

from . import gnss as _gnss
from . import vehicle as _vehicle

MAXP = 32


def _name(fn):
    return fn if isinstance(fn, str) else getattr(fn, "__name__", None)


def models(dyn_func, meas_func):
    dn, mn = _name(dyn_func), _name(meas_func)
    if dn not in _gnss.EKF_DYN:
        raise UnsupportedPlugin(f"EKF dynamics plug-in {dn!r} has no HIP functor; registered: {sorted(_gnss.EKF_DYN)}")
    if mn not in _gnss.EKF_MEAS:
        raise UnsupportedPlugin(f"EKF measurement plug-in {mn!r} has no HIP functor; registered: {sorted(_gnss.EKF_MEAS)}")
    if (dn, mn) not in _gnss.EKF_PAIRS:
        raise UnsupportedPlugin(f"EKF pair ({dn!r}, {mn!r}) is not compiled into libmhe.so; "
                                f"available: {sorted(_gnss.EKF_PAIRS)}")
    return _gnss.EKF_DYN[dn], _gnss.EKF_MEAS[mn]


def dyn_par(dyn_func, params):
    """mhe_ekf_dims.dyn_par for a dynamics plug-in and its dyn_func_params."""
    out = np.zeros(8)
    if _name(dyn_func) == "discrete_vehicle_dynamics":
        C = (params or {}).get("car_params")
        if C is None:
            raise UnsupportedPlugin("discrete_vehicle_dynamics needs dyn_func_params['car_params'] "
                                    "(autonomous-car.py:160)")
        out[:6] = [float(C[k]) for k in _vehicle.CAR_KEYS]
    return out


# ---------------------------------------------------------------- identity checks
_VERIFIED = {}


def _twin(name):
    for mod in (_gnss, _vehicle):
        if hasattr(mod, name):
            return getattr(mod, name)
    raise UnsupportedPlugin(f"EKF plug-in {name!r} has no registered twin to verify against")


def _close(a, b, rtol=1e-12):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return a.shape == b.shape and bool(np.all(np.abs(a - b) <= rtol * (1.0 + np.abs(b))))


def _params_key(p):
    if not p:
        return ()
    return tuple(sorted((k, _params_key(v) if isinstance(v, dict) else float(v)) for k, v in p.items()
                        if isinstance(v, (dict, int, float, np.floating, np.integer))))


def verify(dyn_func, meas_func, dyn_params):
    """Refuse (UnsupportedPlugin) user callables whose values or Jacobians differ from
    the registered twins at 4 seeded points: a same-named plug-in with other math or
    other constants must not silently get the built-in device functor.  Strings and this
    package's own functions pass without evaluation; results are cached per callable
    and parameter values."""
    (_, n, m), _ = models(dyn_func, meas_func)
    _verify_one(dyn_func, "dyn", n, m, dyn_params)
    _verify_one(meas_func, "meas", n, m, dyn_params)


def dynamics(dyn_func):
    """(id, n, m) of a dynamics plug-in by name -- the dynamics half of ``models``."""
    dn = _name(dyn_func)
    if dn not in _gnss.EKF_DYN:
        raise UnsupportedPlugin(f"EKF dynamics plug-in {dn!r} has no HIP functor; registered: {sorted(_gnss.EKF_DYN)}")
    return _gnss.EKF_DYN[dn]


def verify_dynamics(dyn_func, dyn_params):
    """The dynamics half of ``verify`` (the smoother has no measurement model)."""
    _, n, m = dynamics(dyn_func)
    _verify_one(dyn_func, "dyn", n, m, dyn_params)


def _verify_one(fn, kind, n, m, dyn_params):
    if isinstance(fn, str):
        return
    twin = _twin(_name(fn))
    if fn is twin:
        return
    key = (id(fn), kind, _params_key(dyn_params) if kind == "dyn" else ())
    if _VERIFIED.get(key) is fn:
        return
    rng = np.random.default_rng(20262)
    for _ in range(4):
        x = rng.normal(size=n) * 3.0
        if n == 9:
            x[3] = 5.0 + abs(x[3])   # forward speed away from the tyre model's pole at vx = 0
        try:
            if kind == "dyn":
                u = rng.normal(size=m)
                got = fn(x.copy(), u, params=dyn_params, jac=True)
                ref = twin(x.copy(), u, params=dyn_params, jac=True)
            else:
                p = {"sat_pos": rng.normal(size=(4, 3)) * 2.0e4}
                got = fn(x.copy(), params=p, jac=True)
                ref = twin(x.copy(), params=p, jac=True)
        except UnsupportedPlugin:
            raise
        except Exception as e:
            raise UnsupportedPlugin(f"EKF plug-in {_name(fn)!r} could not be evaluated to verify it matches "
                                    f"the device functor: {type(e).__name__}: {e}") from e
        if not (_close(got[0], ref[0]) and _close(got[1], ref[1])):
            raise UnsupportedPlugin(f"EKF plug-in {_name(fn)!r} is not the registered {_name(fn)}: its values "
                                    "or Jacobian differ from the device functor's (same name, different math "
                                    "or constants)")
    _VERIFIED[key] = fn


def _ptr(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


def _gate_value(gate):
    """mhe_ekf_args.gate for run_batch's `gate`: None -> 0.0 (no screening), else a float > 0
    (np.inf allowed); anything else raises ValueError."""
    if gate is None:
        return 0.0
    if isinstance(gate, (bool, np.bool_)) or not isinstance(gate, (int, float, np.integer, np.floating)) \
            or not float(gate) > 0.0:
        raise ValueError(f"gate must be None or a float > 0 (np.inf allowed), not {gate!r}")
    return float(gate)


MAX_ITERATIONS = 64


def _iter_values(iterations, iter_tol, method="auto"):
    """(max_iter, tol) of mhe_iekf_args for run_batch's `iterations` / `iter_tol`; iterations=None
    -> (None, 0.0).  Anything but an int in 1..64 and a number >= 0 raises ValueError, and so
    does method="lane" with iterations (no lane-per-filter form of the iterated filter exists)."""
    if isinstance(iter_tol, (bool, np.bool_)) or not isinstance(iter_tol, (int, float, np.integer, np.floating)) \
            or not float(iter_tol) >= 0.0:
        raise ValueError(f"iter_tol must be a number >= 0, not {iter_tol!r}")
    if iterations is None:
        return None, float(iter_tol)
    if isinstance(iterations, (bool, np.bool_)) or not isinstance(iterations, (int, np.integer)) \
            or not 1 <= int(iterations) <= MAX_ITERATIONS:
        raise ValueError(f"iterations must be None or an int in 1..{MAX_ITERATIONS}, not {iterations!r}")
    if method == "lane":
        raise ValueError('iterations with method="lane": the iterated filter has the wave form only')
    return int(iterations), float(iter_tol)


def _huber_value(huber, iterations):
    """run_batch's `huber`: None, or (delta, DELTA) of mhe_iekf_robust_args -- (float > 0, None)
    for a number (np.inf allowed) or (0.0, the array) for an array of Z's shape (its shape is
    checked with the others').  A NumPy array is checked here for entries > 0; a torch tensor is
    not read.  Anything else, and huber without iterations, raises ValueError."""
    if huber is None:
        return None
    if iterations is None:
        raise ValueError("huber needs iterations: the pseudo-Huber rows are the iterated filter's")
    if isinstance(huber, (bool, np.bool_)):
        raise ValueError(f"huber must be None, a float > 0 or an array of Z's shape, not {huber!r}")
    if isinstance(huber, (int, float, np.integer, np.floating)):
        if not float(huber) > 0.0:
            raise ValueError(f"huber must be > 0 (np.inf allowed), not {huber!r}")
        return float(huber), None
    if isinstance(huber, np.ndarray):
        if huber.ndim != 3 or huber.dtype.kind not in "fiu" or not bool(np.all(huber > 0)):
            raise ValueError("a huber array has Z's shape and entries > 0 (np.inf allowed)")
        return 0.0, huber
    if hasattr(huber, "data_ptr") and hasattr(huber, "dim"):     # a torch tensor: not checked, as nz
        if huber.dim() != 3:
            raise ValueError("a huber array has Z's shape")
        return 0.0, huber
    raise ValueError(f"huber must be None, a float > 0 or an array of Z's shape, not {huber!r}")


def run_batch(dyn_func, meas_func, mu0, S0, U, Z, nz, Q, R, dt, sat_pos, device=None, stream=None,
              keep_history=True, method="auto", inputs="batch_outer", dyn_params=None, gate=None,
              innovations=False, iterations=None, iter_tol=0.0, huber=None):
    """Run B independent filters for T steps in one launch.

    mu0 (B,n), S0 (B,n,n), U (B,T,m), Z (B,T,pmax), nz (B,T) valid rows per step
    (0 = predict only), Q (n,n), R (T,pmax,pmax) or (B,T,pmax,pmax), sat_pos
    (B,T,pmax,3); dt = dyn_func_params["dt"]; dyn_params = the whole dyn_func_params
    (needed for discrete_vehicle_dynamics: "car_params"; its "dt", when given, wins
    over dt).  Inputs may be NumPy or torch.
    Returns (mu_hist (B,T,n), S_hist (B,T,n,n), mu (B,n), S (B,n,n), status (B))
    as torch tensors on the device.  status: 0 ok, 1 innovation covariance not
    positive definite, 2 nz > pmax at some step (that step is predict-only; nz may be
    a device tensor and is not checked on the host).

    method: "lane" (diagonal R: sequential scalar updates, one filter per lane),
    "wave" (any R: one wavefront per filter, augmented Cholesky sweep) or "auto"
    (lane when every R block is diagonal -- one device-side check).

    inputs="batch_inner": U, Z, nz, sat_pos are given batch-innermost instead,
    (T,m,B), (T,pmax,B), (T,B), (T,pmax,3,B) -- the device reads then coalesce.

    gate: None, or a threshold > 0 on the normalised innovation of each row,
    d2_i = (z_i - h_i(mu-))^2 / (H_i S- H_i^T + R_ii), evaluated at the prediction: a row
    with d2_i > gate is screened out and the correction is the usual one on the rows that
    remain (none: the step is predict-only).  The screen is the same for both methods.
    10.83 is the 0.999 quantile of chi-square with one degree of freedom; np.inf screens
    nothing.
    innovations=True appends (nis (B,T), loglik (B,T), rejected (B,T) int32) to the
    returned tuple: over the accepted rows a of a step, nis = e_a^T P_a^-1 e_a and
    loglik = -(nis + log det P_a + |a| log 2 pi) / 2 (both 0 when no row was applied);
    bit i of rejected is set iff row i was screened out.  Like the histories they are
    views of batch-innermost storage.  Without either keyword the call and its result
    are what they were (mhe_ekf_run's instances; otherwise mhe_ekf_run_args').

    iterations: None, or an int in 1..64: the iterated EKF (mhe_iekf_run, one wavefront per
    filter for every R; method="lane" is refused).  A step's correction becomes the
    Gauss-Newton solve of its MAP problem: with x_0 = mu-,
        pass i:  (h, H) at x_i,  e = z - h - H (mu- - x_i),  P = H S- H^T + R,
                 K = S- H^T P^-1,  x_{i+1} = mu- + K e
        stop when  not (max_c |x_{i+1,c} - x_{i,c}| > iter_tol)  or after `iterations` passes
        then     mu = x_{i+1},  S = S- - K H S- with the last pass's H.
    iterations=1 is the EKF step.  iter_tol is an absolute max-norm in the state's own units
    (0: every corrected step makes `iterations` passes).  It must sit above the rounding floor
    of the rows -- about 1e-8 m for pseudoranges of 2e7 m -- or the step stalls there and the
    counts depend on rounding.  gate screens once, at the prediction (pass 0), and the kept rows
    stay fixed; nis, loglik and rejected are pass 0's, the EKF's definition.  n_iter (B,T) int32,
    the passes each step made (0: predict-only), is appended to the returned tuple last, after
    the innovations triple when that is present.  smooth_batch takes an iterated run's history
    as any other.  iterations=None is the call as it was.

    huber: None, a float > 0 (np.inf allowed) or an array of Z's shape in Z's layout: pseudo-Huber
    measurement rows (mhe_iekf_run_robust), the Huber-type Kalman correction by iteratively
    reweighted Gauss-Newton.  It needs `iterations` (ValueError without).  delta is in the
    measurement's own units, as the solver's meas_delta.  In every pass, with r = z - h(x_i):
        t_j = r_j / delta_j,  s_j = sqrt(1 + t_j^2),  R~_jl = R_jl sqrt(s_j) sqrt(s_l),
        P = H S- H^T + R~   and the pass, the stop rule and the final S are as above.
    For a diagonal R this minimises sum_j 2 (delta_j^2 / R_jj) (s_j - 1) + the prior's term: a row
    counts fully while |r_j| << delta_j and like |r_j| beyond it; for any R it is the covariance
    inflation D^-1/2 R D^-1/2 with D = diag(omega), omega_j = 1 / s_j.  np.inf is the plain
    iterated run, bitwise.  A NumPy array is checked on the host for entries > 0; a device tensor
    is not checked, as nz: a zero or NaN entry of a counted row makes that filter's status 1.
    gate goes with it: the screen is taken once, at the prediction, on the UNWEIGHTED
    H_i S- H_i^T + R_ii, so the mask is the plain run's at the same prediction and a screened row
    is out for every pass.  nis and loglik are then pass 0's over the kept rows of the REWEIGHTED
    model (R~ at the prediction in place of R).  weights (B,T,pmax), omega of the last pass per
    row and 0 for every row that was not applied (beyond nz, screened out, predict-only step), is
    appended to the returned tuple last, after n_iter.  huber=None is the call as it was: its
    result and the kernel it launches do not change.

    stream: a torch stream to order the work on (default: the current one); outputs
    belong to it (mhe.streams)."""
    gate = _gate_value(gate)
    iterations, iter_tol = _iter_values(iterations, iter_tol, method)
    huber = _huber_value(huber, iterations)
    if huber is not None and huber[1] is not None and tuple(huber[1].shape) != tuple(np.shape(Z)):
        raise ValueError("a huber array has Z's shape, in Z's layout")
    import torch

    from mhe.streams import launch_stream

    (did, n, m), (mid, _, q) = models(dyn_func, meas_func)
    if dyn_params is not None and "dt" in dyn_params:
        dt = dyn_params["dt"]
    verify(dyn_func, meas_func, dict(dyn_params or {}, dt=dt))
    dp = dyn_par(dyn_func, dyn_params)
    dev = torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())
    with launch_stream(stream, dev) as (s, cur):
        return _run_batch(did, n, m, mid, q, dev, s, cur, mu0, S0, U, Z, nz, Q, R, dt, sat_pos, keep_history,
                          method, inputs, dp, gate, bool(innovations), iterations, iter_tol, huber)


def _run_batch(did, n, m, mid, q, dev, s, cur, mu0, S0, U, Z, nz, Q, R, dt, sat_pos, keep_history, method,
               inputs, dp, gate=0.0, innovations=False, iterations=None, iter_tol=0.0, huber=None):
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
    Dt = d(huber[1]) if huber is not None and huber[1] is not None else None     # laid out and strided as Z
    if Dt is not None and Dt.shape != Zt.shape:
        raise ValueError("a huber array has Z's shape, in Z's layout")
    if Rt.dim() == 3:
        r_b, r_s = 0, pmax * pmax
        if Rt.shape != (T, pmax, pmax):
            raise ValueError("R must be (T,pmax,pmax) or (B,T,pmax,pmax)")
    else:
        r_b, r_s = T * pmax * pmax, pmax * pmax
        if Rt.shape != (B, T, pmax, pmax):
            raise ValueError("R must be (T,pmax,pmax) or (B,T,pmax,pmax)")
    # histories are written batch-innermost (coalesced device stores) and returned as
    # (B, T, ...) views of that storage
    mh_st = torch.empty((T, n, B), dtype=torch.float64, device=dev) if keep_history else None
    Sh_st = torch.empty((T, n, n, B), dtype=torch.float64, device=dev) if keep_history else None
    st = torch.empty(B, dtype=torch.int32, device=dev)
    if iterations is not None:
        if method not in ("auto", "wave"):
            raise ValueError(f"unknown method {method!r}")
        r_diag = False            # mhe_iekf_run ignores it: one wavefront per filter for every R
    elif method == "auto":
        offd = Rt - torch.diag_embed(torch.diagonal(Rt, dim1=-2, dim2=-1))
        r_diag = Rt.numel() == 0 or not bool((offd != 0).any().item())
    elif method in ("lane", "wave"):
        r_diag = method == "lane"
    else:
        raise ValueError(f"unknown method {method!r}")
    dims = _lib.MheEkfDims(n=n, m=m, pmax=pmax, q=q, dyn_model=did, meas_model=mid, dt=float(dt),
                           r_diag=int(r_diag), hist_batch_inner=1, in_batch_inner=int(bi))
    for i in range(8):
        dims.dyn_par[i] = float(dp[i])
    lib = _lib.load()
    if iterations is not None:
        stats = tuple(torch.empty((T, B), dtype=dt_, device=dev)
                      for dt_ in (torch.float64, torch.float64, torch.int32)) if innovations else ()
        nis, ll, rej = stats if innovations else (None, None, None)
        stats += (torch.empty((T, B), dtype=torch.int32, device=dev),)      # n_iter, last
        kw = dict(batch=B, steps=T, mu=mu.data_ptr(), S=S.data_ptr(), U=Ut.data_ptr(), u_bstride=T * m,
                  Z=Zt.data_ptr(), z_bstride=T * pmax, nz=nzt.data_ptr(), nz_bstride=T,
                  PAR=Pt.data_ptr(), par_bstride=T * pmax * q, Q=Qt.data_ptr(), R=Rt.data_ptr(),
                  r_bstride=r_b, r_sstride=r_s, mu_hist=_ptr(mh_st), S_hist=_ptr(Sh_st),
                  status=st.data_ptr(), gate=gate, nis=_ptr(nis), loglik=_ptr(ll), rej=_ptr(rej),
                  tol=iter_tol, n_iter=stats[-1].data_ptr(), max_iter=iterations)
        if huber is None:
            args = _lib.MheIekfArgs(**kw)
            rc = lib.mhe_iekf_run(ctypes.byref(dims), ctypes.byref(args), ctypes.c_void_p(s.cuda_stream))
            _lib.check(rc, "mhe_iekf_run")
        else:
            w_st = torch.empty((T, pmax, B), dtype=torch.float64, device=dev)   # every entry is written
            args = _lib.MheIekfRobustArgs(delta=huber[0], DELTA=_ptr(Dt), weights=w_st.data_ptr(), **kw)
            rc = lib.mhe_iekf_run_robust(ctypes.byref(dims), ctypes.byref(args), ctypes.c_void_p(s.cuda_stream))
            _lib.check(rc, "mhe_iekf_run_robust")
    elif gate == 0.0 and not innovations:
        rc = lib.mhe_ekf_run(ctypes.byref(dims), B, T, _ptr(mu), _ptr(S), _ptr(Ut), T * m, _ptr(Zt), T * pmax,
                             _ptr(nzt), T, _ptr(Pt), T * pmax * q, _ptr(Qt), _ptr(Rt), r_b, r_s, _ptr(mh_st),
                             _ptr(Sh_st), _ptr(st), ctypes.c_void_p(s.cuda_stream))
        _lib.check(rc, "mhe_ekf_run")
        stats = ()
    else:
        # per-step statistics: batch-innermost (T, B) storage as the histories (hist_batch_inner)
        stats = tuple(torch.empty((T, B), dtype=dt_, device=dev)
                      for dt_ in (torch.float64, torch.float64, torch.int32)) if innovations else ()
        nis, ll, rej = stats if innovations else (None, None, None)
        args = _lib.MheEkfArgs(batch=B, steps=T, mu=mu.data_ptr(), S=S.data_ptr(), U=Ut.data_ptr(), u_bstride=T * m,
                               Z=Zt.data_ptr(), z_bstride=T * pmax, nz=nzt.data_ptr(), nz_bstride=T,
                               PAR=Pt.data_ptr(), par_bstride=T * pmax * q, Q=Qt.data_ptr(), R=Rt.data_ptr(),
                               r_bstride=r_b, r_sstride=r_s, mu_hist=_ptr(mh_st), S_hist=_ptr(Sh_st),
                               status=st.data_ptr(), gate=gate, nis=_ptr(nis), loglik=_ptr(ll), rej=_ptr(rej))
        rc = lib.mhe_ekf_run_args(ctypes.byref(dims), ctypes.byref(args), ctypes.c_void_p(s.cuda_stream))
        _lib.check(rc, "mhe_ekf_run_args")
    robust = () if huber is None else (w_st,)
    keep_alive(s, cur, mu, S, Ut, Zt, nzt, Pt, Qt, Rt, mh_st, Sh_st, st, Dt, *stats, *robust)
    mh = mh_st.permute(2, 0, 1) if keep_history else None
    Sh = Sh_st.permute(3, 0, 1, 2) if keep_history else None
    return (mh, Sh, mu, S, st) + tuple(t.permute(1, 0) for t in stats) + tuple(t.permute(2, 0, 1) for t in robust)


def _hist_storage(t, w):
    """The storage a (B, T, *w) history tensor hands to the kernel and whether it is
    batch-innermost: run_batch's views (permuted (T, *w, B) storage) pass as they are, no
    copy; every other layout is made contiguous batch-outermost."""
    if t.dim() == 2 + len(w) and t.shape[0] > 0:
        perm = tuple(range(1, t.dim())) + (0,)
        if not t.is_contiguous() and t.permute(*perm).is_contiguous():
            return t.permute(*perm), True
    return t.contiguous(), False


def _flag(name, v):
    """A keyword that is True or False and nothing else (ValueError otherwise)."""
    if not isinstance(v, (bool, np.bool_)):
        raise ValueError(f"{name} must be True or False, not {v!r}")
    return bool(v)


def smooth_batch(dyn_func, mu_hist, S_hist, U, Q, dt, mu0=None, S0=None, dyn_params=None, inputs="batch_outer",
                 device=None, stream=None, lag_one=False):
    """Fixed-interval (Rauch-Tung-Striebel) smoother over a filtered history, B filters
    in one launch of ``mhe_ekf_smooth`` (one filter per lane).

    mu_hist (B,T,n), S_hist (B,T,n,n): what run_batch returned (its batch-innermost views
    go to the kernel without a copy; other layouts are copied to contiguous batch-outermost);
    U (B,T,m) -- or (T,m,B) with inputs="batch_inner" -- and Q (n,n), dt, dyn_params: as
    given to run_batch.  mu0 (B,n), S0 (B,n,n): optionally the prior the filter started
    from; the smoothed prior is then returned too.  Measurements do not enter the backward
    pass, so the history of a gated run (run_batch's ``gate``) smooths as any other, and so
    does that of an iterated run (run_batch's ``iterations``).
    Returns (mu_s (B,T,n), S_s (B,T,n,n), status (B)) and, with a prior, also
    (mu0_s (B,n), S0_s (B,n,n)).  status 1: a predicted covariance had no Cholesky factor or
    the history held a non-finite value; that filter is NaN from the failing step down.

    lag_one=True (``mhe_ekf_smooth_args``) appends C (B,T,n,n) last to the returned tuple, the
    lag-one smoothed covariances C[:, k] = Cov(x_k, x_{k-1} | all data) = S_s[k] G_{k-1}^T with
    G_{k-1} the smoother gain of step k-1: all n x n entries, not symmetric, a view of
    batch-innermost storage when the histories were.  C[:, 0] pairs step 0 with the prior: it is
    formed when mu0 / S0 are given and NaN otherwise.  A filter with status 1 has C NaN from the
    step above the failing one down.  Everything else returned is bitwise what it is without the
    keyword, and lag_one=False is the call as it was.

    stream: as run_batch (mhe.streams)."""
    lag_one = _flag("lag_one", lag_one)
    import torch

    from mhe.streams import keep_alive, launch_stream

    did, n, m = dynamics(dyn_func)
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
    verify_dynamics(dyn_func, dict(dyn_params or {}, dt=dt))
    dp = dyn_par(dyn_func, dyn_params)
    dev = torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())
    with launch_stream(stream, dev) as (s, cur):
        def d(a):
            return torch.as_tensor(np.asarray(a) if not torch.is_tensor(a) else a, dtype=torch.float64, device=dev)

        mh, mh_bi = _hist_storage(d(mu_hist), (n,))
        Sh, Sh_bi = _hist_storage(d(S_hist), (n, n))
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
        lib = _lib.load()
        Ct = torch.empty_like(Sh) if lag_one else None
        if lag_one:
            args = _lib.MheEkfLagArgs(batch=B, steps=T, mu_hist=mh.data_ptr(), S_hist=Sh.data_ptr(), U=Ut.data_ptr(),
                                      u_bstride=T * m, Q=Qt.data_ptr(), mu0=_ptr(m0), S0=_ptr(S0t),
                                      mu_s=ms.data_ptr(), S_s=Ss.data_ptr(), mu0_s=_ptr(m0s), S0_s=_ptr(S0s),
                                      status=st.data_ptr(), C=Ct.data_ptr())
            rc = lib.mhe_ekf_smooth_args(ctypes.byref(dims), ctypes.byref(args), ctypes.c_void_p(s.cuda_stream))
            _lib.check(rc, "mhe_ekf_smooth_args")
        else:
            rc = lib.mhe_ekf_smooth(ctypes.byref(dims), B, T, _ptr(mh), _ptr(Sh), _ptr(Ut), T * m, _ptr(Qt), _ptr(m0),
                                    _ptr(S0t), _ptr(ms), _ptr(Ss), _ptr(m0s), _ptr(S0s), _ptr(st),
                                    ctypes.c_void_p(s.cuda_stream))
            _lib.check(rc, "mhe_ekf_smooth")
        keep_alive(s, cur, mh, Sh, Ut, Qt, m0, S0t, ms, Ss, m0s, S0s, st, Ct)
        if mh_bi:
            ms, Ss = ms.permute(2, 0, 1), Ss.permute(3, 0, 1, 2)
            Ct = Ct.permute(3, 0, 1, 2) if lag_one else None
        out = (ms, Ss, st, m0s, S0s) if prior else (ms, Ss, st)
        return out + (Ct,) if lag_one else out


def em_stats(dyn_func, meas_func, mu_s, S_s, C, U, Z, nz, dt, sat_pos, mu0_s=None, S0_s=None, rejected=None,
             dyn_params=None, inputs="batch_outer", device=None, stream=None):
    """EM sufficient statistics of the noise model from a smoothed history, B filters in one
    launch of ``mhe_ekf_em_stats`` (one filter per lane).

    mu_s (B,T,n), S_s (B,T,n,n), C (B,T,n,n): what smooth_batch(..., lag_one=True) returned (its
    batch-innermost views go to the kernel without a copy); mu0_s (B,n), S0_s (B,n,n):
    optionally the smoothed prior, and step 0 then counts in the dynamics' sum.  U, Z, nz,
    sat_pos, dt, dyn_params, inputs: as given to run_batch.  rejected (B,T) int32: optionally
    the mask a gated run_batch returned; bit i set leaves row i of that step out.
    Per filter, with (f, F) the dynamics and its Jacobian at the smoothed mean of step k-1 and
    (h, H) the measurement model at that of step k:
        W_k = d d^T + S_s[k] - C_k F^T - F C_k^T + F S_s[k-1] F^T,   d = mu_s[k] - f
        Qsum = sum of W_k over k = 1..T-1 (and 0 with the smoothed prior),  q_cnt their number
        r2[k, i] = (z_i - h_i)^2 + H_i S_s[k] H_i^T for every counted row (i < nz_k <= pmax, not
        rejected), 0 for every other row;  r_cnt the number of counted rows.
    Returns (Qsum (B,n,n) bitwise symmetric, q_cnt (B) int32, r2 (B,T,pmax), r_cnt (B) int32,
    status (B) int32) on the device.  status 1: a non-finite value was met, that filter's Qsum
    and r2 are NaN; 2: nz > pmax at some step (that step's rows are skipped).  The M-step is
    the caller's: Q = sum_b Qsum / sum_b q_cnt, and r2 pooled as the application needs (per
    satellite, per elevation, one scale: fit_noise does the last).

    stream: as run_batch (mhe.streams)."""
    (did, n, m), (mid, _, q) = models(dyn_func, meas_func)
    if dyn_params is not None and "dt" in dyn_params:
        dt = dyn_params["dt"]
    if inputs not in ("batch_outer", "batch_inner"):
        raise ValueError(f"unknown inputs layout {inputs!r}")
    if (mu0_s is None) != (S0_s is None):
        raise ValueError("em_stats: mu0_s and S0_s go together")
    bi = inputs == "batch_inner"
    shp = lambda a: tuple(np.shape(a)) if not hasattr(a, "shape") else tuple(a.shape)   # noqa: E731
    if len(shp(mu_s)) != 3 or len(shp(Z)) != 3:
        raise ValueError("em_stats: mu_s must be (B,T,n) and Z (B,T,pmax) or (T,pmax,B)")
    B, T = shp(mu_s)[:2]
    pmax = shp(Z)[1] if bi else shp(Z)[2]
    if not 1 <= pmax <= MAXP:
        raise ValueError(f"between 1 and {MAXP} measurement rows per step")
    want = ((T, m, B), (T, pmax, B), (T, B), (T, pmax, q, B)) if bi else \
        ((B, T, m), (B, T, pmax), (B, T), (B, T, pmax, q))
    if shp(mu_s) != (B, T, n) or shp(S_s) != (B, T, n, n) or shp(C) != (B, T, n, n) \
            or (shp(U), shp(Z), shp(nz), shp(sat_pos)) != want \
            or (mu0_s is not None and (shp(mu0_s) != (B, n) or shp(S0_s) != (B, n, n))) \
            or (rejected is not None and shp(rejected) != (B, T)):
        raise ValueError("em_stats: inconsistent shapes")
    verify(dyn_func, meas_func, dict(dyn_params or {}, dt=dt))
    dp = dyn_par(dyn_func, dyn_params)
    import torch

    from mhe.streams import keep_alive, launch_stream

    dev = torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())
    with launch_stream(stream, dev) as (s, cur):
        def d(a, dt_=torch.float64):
            return torch.as_tensor(np.asarray(a) if not torch.is_tensor(a) else a, dtype=dt_, device=dev)

        ms, ms_bi = _hist_storage(d(mu_s), (n,))
        Ss, Ss_bi = _hist_storage(d(S_s), (n, n))
        Ct, C_bi = _hist_storage(d(C), (n, n))
        hbi = ms_bi and Ss_bi and C_bi          # one layout flag covers the three histories, the mask and r2
        if not hbi:
            ms, Ss, Ct = d(mu_s).contiguous(), d(S_s).contiguous(), d(C).contiguous()
        rj = None
        if rejected is not None:
            rj = d(rejected, torch.int32)
            rj = rj.permute(1, 0).contiguous() if hbi else rj.contiguous()
        Ut, Zt, nzt, Pt = d(U).contiguous(), d(Z).contiguous(), d(nz, torch.int32).contiguous(), \
            d(sat_pos).contiguous()
        prior = mu0_s is not None
        m0, S0t = (d(mu0_s).contiguous(), d(S0_s).contiguous()) if prior else (None, None)
        Qsum = torch.empty((B, n, n), dtype=torch.float64, device=dev)
        r2 = torch.empty((T, pmax, B) if hbi else (B, T, pmax), dtype=torch.float64, device=dev)
        q_cnt, r_cnt, st = (torch.empty(B, dtype=torch.int32, device=dev) for _ in range(3))
        dims = _lib.MheEkfDims(n=n, m=m, pmax=pmax, q=q, dyn_model=did, meas_model=mid, dt=float(dt),
                               hist_batch_inner=int(hbi), in_batch_inner=int(bi))
        for i in range(8):
            dims.dyn_par[i] = float(dp[i])
        args = _lib.MheEmArgs(batch=B, steps=T, mu_s=ms.data_ptr(), S_s=Ss.data_ptr(), C=Ct.data_ptr(),
                              mu0_s=_ptr(m0), S0_s=_ptr(S0t), U=Ut.data_ptr(), u_bstride=T * m, Z=Zt.data_ptr(),
                              z_bstride=T * pmax, nz=nzt.data_ptr(), nz_bstride=T, PAR=Pt.data_ptr(),
                              par_bstride=T * pmax * q, rej=_ptr(rj), Qsum=Qsum.data_ptr(), q_cnt=q_cnt.data_ptr(),
                              r2=r2.data_ptr(), r_cnt=r_cnt.data_ptr(), status=st.data_ptr())
        rc = _lib.load().mhe_ekf_em_stats(ctypes.byref(dims), ctypes.byref(args), ctypes.c_void_p(s.cuda_stream))
        _lib.check(rc, "mhe_ekf_em_stats")
        keep_alive(s, cur, ms, Ss, Ct, rj, Ut, Zt, nzt, Pt, m0, S0t, Qsum, r2, q_cnt, r_cnt, st)
        return Qsum, q_cnt, (r2.permute(2, 0, 1) if hbi else r2), r_cnt, st


Q_STRUCTURES = ("full", "diag")
MAX_ROUNDS = 1000


def _fit_values(rounds, fit_Q, fit_R, q_structure):
    """fit_noise's keywords, validated as _gate_value / _iter_values validate theirs."""
    if isinstance(rounds, (bool, np.bool_)) or not isinstance(rounds, (int, np.integer)) \
            or not 1 <= int(rounds) <= MAX_ROUNDS:
        raise ValueError(f"rounds must be an int in 1..{MAX_ROUNDS}, not {rounds!r}")
    if q_structure not in Q_STRUCTURES:
        raise ValueError(f"q_structure must be one of {Q_STRUCTURES}, not {q_structure!r}")
    return int(rounds), _flag("fit_Q", fit_Q), _flag("fit_R", fit_R), q_structure


def fit_noise(dyn_func, meas_func, mu0, S0, U, Z, nz, Q, R, dt, sat_pos, rounds=10, fit_Q=True, fit_R=True,
              q_structure="full", gate=None, dyn_params=None, inputs="batch_outer", device=None, stream=None):
    """EM identification of the EKF's noise model (Shumway-Stoffer; Sarkka, Bayesian Filtering
    and Smoothing, ch. 12, the extended-RTS form) over a batch of logs that share Q and R.

    mu0 .. sat_pos, gate, dyn_params, inputs: as run_batch's; Q (n,n) and R ((T,pmax,pmax) or
    (B,T,pmax,pmax)) are the starting guess.  Each of `rounds` rounds runs
    run_batch(innovations=True, gate=gate), smooth_batch with the prior and lag_one=True,
    em_stats (with the run's rejection mask when gated) and then the M-step as torch
    reductions on the device, pooled over the filters whose three statuses are all 0:
        Q <- sum_b Qsum_b / sum_b q_cnt_b                      (q_structure="diag": its diagonal only)
        rho_round = sum r2[b,k,i] / R[k,i,i] / sum_b r_cnt_b;   R <- rho_round R
    so R keeps its given shape and structure and is fitted by ONE common scale (fit_R needs a
    diagonal R: ValueError otherwise); Q is one matrix shared by the batch.  The linearisations
    are the filter's and the smoother's own (the EKF's prediction and the smoothed means), so
    this is the extended-RTS approximation of EM: the likelihood usually rises at every round
    but is not guaranteed to -- read `loglik`.  No history leaves the device.
    Returns a dict of device tensors and ints: Q (n,n), R (as given), rho (the cumulative scale
    on the given R), loglik (rounds,) the summed log-likelihood (over the used filters) of the
    parameters that ENTERED each round, n_used (the filters pooled in the last round),
    n_iter = rounds."""
    gate_v = _gate_value(gate)
    rounds, fit_Q, fit_R, q_structure = _fit_values(rounds, fit_Q, fit_R, q_structure)
    (_, n, m), (_, _, q) = models(dyn_func, meas_func)
    if inputs not in ("batch_outer", "batch_inner"):
        raise ValueError(f"unknown inputs layout {inputs!r}")
    bi = inputs == "batch_inner"
    shp = lambda a: tuple(np.shape(a)) if not hasattr(a, "shape") else tuple(a.shape)   # noqa: E731
    if len(shp(mu0)) != 2 or len(shp(Z)) != 3:
        raise ValueError("fit_noise: mu0 must be (B,n) and Z (B,T,pmax) or (T,pmax,B)")
    B = shp(mu0)[0]
    T, pmax = shp(Z)[:2] if bi else shp(Z)[1:]
    if not 1 <= pmax <= MAXP:
        raise ValueError(f"between 1 and {MAXP} measurement rows per step")
    want = ((T, m, B), (T, pmax, B), (T, B), (T, pmax, q, B)) if bi else \
        ((B, T, m), (B, T, pmax), (B, T), (B, T, pmax, q))
    if shp(mu0) != (B, n) or shp(S0) != (B, n, n) or shp(Q) != (n, n) \
            or (shp(U), shp(Z), shp(nz), shp(sat_pos)) != want \
            or shp(R) not in ((T, pmax, pmax), (B, T, pmax, pmax)):
        raise ValueError("fit_noise: inconsistent shapes")
    if dyn_params is not None and "dt" in dyn_params:
        dt = dyn_params["dt"]
    verify(dyn_func, meas_func, dict(dyn_params or {}, dt=dt))
    import torch

    dev = torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())
    Qt = torch.as_tensor(np.asarray(Q) if not torch.is_tensor(Q) else Q, dtype=torch.float64, device=dev).clone()
    Rt = torch.as_tensor(np.asarray(R) if not torch.is_tensor(R) else R, dtype=torch.float64, device=dev).clone()
    offd = Rt - torch.diag_embed(torch.diagonal(Rt, dim1=-2, dim2=-1))     # method="auto"'s check, made once
    r_diag = Rt.numel() == 0 or not bool((offd != 0).any().item())
    if fit_R and not r_diag:
        raise ValueError("fit_R needs a diagonal R (one common scale on the given R is fitted)")
    method = "lane" if r_diag else "wave"
    on_dev = [torch.as_tensor(np.asarray(a) if not torch.is_tensor(a) else a, device=dev)
              for a in (mu0, S0, U, Z, nz, sat_pos)]
    mu0, S0, U, Z, nz, sat_pos = on_dev
    rho = torch.ones((), dtype=torch.float64, device=dev)
    loglik = torch.zeros(rounds, dtype=torch.float64, device=dev)
    n_used = torch.zeros((), dtype=torch.int64, device=dev)
    kw = dict(dyn_params=dyn_params, inputs=inputs, device=dev, stream=stream)
    for it in range(rounds):
        mh, Sh, _, _, st_f, _, ll, rej = run_batch(dyn_func, meas_func, mu0, S0, U, Z, nz, Qt, Rt, dt, sat_pos,
                                                   method=method, gate=gate, innovations=True, **kw)
        ms, Ss, st_s, m0s, S0s, C = smooth_batch(dyn_func, mh, Sh, U, Qt, dt, mu0=mu0, S0=S0, lag_one=True, **kw)
        Qsum, q_cnt, r2, r_cnt, st_e = em_stats(dyn_func, meas_func, ms, Ss, C, U, Z, nz, dt, sat_pos, mu0_s=m0s,
                                                S0_s=S0s, rejected=rej if gate_v != 0.0 else None, **kw)
        ok = (st_f == 0) & (st_s == 0) & (st_e == 0)
        zero = torch.zeros((), dtype=torch.float64, device=dev)
        loglik[it] = torch.where(ok, ll.sum(1), zero).sum()
        n_used = ok.sum()
        if fit_Q:
            Qn = torch.where(ok[:, None, None], Qsum, torch.zeros_like(Qsum)).sum(0) / (q_cnt * ok).sum()
            Qt = torch.diag(torch.diagonal(Qn)) if q_structure == "diag" else Qn
        if fit_R:
            Rd = torch.diagonal(Rt, dim1=-2, dim2=-1)                       # (T,pmax) or (B,T,pmax)
            ratio = torch.where(r2 > 0.0, r2 / Rd, torch.zeros_like(r2))    # uncounted rows are exactly 0
            cnt = (r_cnt * ok).sum()
            rr = torch.where(cnt > 0, torch.where(ok, ratio.sum((1, 2)), zero).sum() / cnt, torch.ones_like(rho))
            Rt = Rt * rr
            rho = rho * rr
    return {"Q": Qt, "R": Rt, "rho": rho, "loglik": loglik, "n_used": n_used, "n_iter": rounds}


class EKF(object):
    """utils/ekf.py:4-18 -- notation of Probabilistic Robotics (Thrun et al.)."""

    def __init__(self, dyn_func, meas_func, mu0, S0):
        self.mu = mu0
        self.S = S0
        self.dynamics = dyn_func
        self.measurement = meas_func
        models(dyn_func, meas_func)  # fail at construction for unregistered plug-ins

    def update(self, u, z, Q, R, dyn_func_params=None, meas_func=None, meas_func_params=None, gate=None,
               iterations=None, iter_tol=0.0, huber=None):
        """One predict (+ correct when z is given) step, utils/ekf.py:20-38.

        gate (run_batch's; np.inf: statistics only): rows of z whose normalised innovation
        exceeds it are left out of the correction, and the object then holds ``nis``,
        ``loglik`` (floats) and ``rejected`` (bool, one per row of z) of this update.
        Without a gate nothing changes.

        iterations, iter_tol (run_batch's): the iterated EKF -- the correction is repeated with
        the measurement model relinearised at the iterate, x_{i+1} = mu- + K_i (z - h(x_i) -
        H_i (mu- - x_i)), until the step's max-norm is not above iter_tol (absolute, in the
        state's units; keep it above the rows' rounding floor, about 1e-8 m for pseudoranges)
        or `iterations` passes are made; the object then holds ``n_iter`` (int), the passes
        this update made (0: no correction).

        huber (run_batch's; needs iterations): a float > 0 (np.inf allowed) or one per row of z --
        pseudo-Huber rows; the object then holds ``weights`` (one float per row of z: omega of
        the last pass, 0 for a row that was screened out or not applied).  Without the keyword
        nothing changes and no ``weights`` is set."""
        gv = _gate_value(gate)
        iterations, iter_tol = _iter_values(iterations, iter_tol)
        if huber is not None and not isinstance(huber, (bool, np.bool_, int, float, np.integer, np.floating)):
            huber = np.asarray(huber)
            if huber.dtype.kind not in "fiu" or huber.ndim != 1:
                raise ValueError("huber must be a float > 0 or one float > 0 per row of z")
            huber = huber.astype(np.float64).reshape(1, 1, -1)
        hv = _huber_value(huber, iterations)
        meas = meas_func if meas_func is not None else self.measurement
        (_, n, m), (_, extra, q) = models(self.dynamics, meas)
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
        if iterations is not None:
            kw.update(iterations=iterations, iter_tol=iter_tol)
        if hv is not None:
            if hv[1] is not None and z is None:
                hv = (float(np.min(hv[1])), None)       # no row: nothing to weigh
            elif hv[1] is not None and hv[1].shape != Z.shape:
                raise ValueError("huber and z disagree in size")
            kw.update(huber=hv[0] if hv[1] is None else hv[1])
        out = run_batch(self.dynamics, meas, mu0, S0, u_, Z, np.full((1, 1), nz, np.int32),
                        np.asarray(Q, dtype=np.float64), Rm, dt, P, keep_history=False,
                        dyn_params=dyn_func_params, **kw)
        mu, S, st = out[2:5]
        if int(st[0].item()) != 0:
            raise np.linalg.LinAlgError("innovation covariance is not positive definite")
        if gate is not None:
            self.nis, self.loglik = float(out[5][0, 0].item()), float(out[6][0, 0].item())
            word = int(out[7][0, 0].item()) & 0xFFFFFFFF
            self.rejected = np.array([bool((word >> i) & 1) for i in range(nz)], dtype=bool)
        if iterations is not None:
            self.n_iter = int(out[-2 if hv is not None else -1][0, 0].item())
        if hv is not None:
            self.weights = out[-1][0, 0, :nz].cpu().numpy().astype(np.float64)
        self.mu = mu[0].cpu().numpy()
        self.S = S[0].cpu().numpy()
