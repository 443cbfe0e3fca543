"""GNSS least-squares fixes on the GPU -- drop-in for kingdwd/nlp-filter utils/leastsquares.py.

Same entry points and semantics as the reference:
  ``iterativeLeastSquares(sat_pos, pr, x=<shared>, b=0, maxiter=100)``  (:19-42)
      GN position + clock-bias fix; ``x`` is updated IN PLACE and the default
      argument is one shared array, so consecutive calls warm-start from the
      previous fix exactly as the reference's mutable default does;
  ``iterativeLeastSquaresVel(sat_pos, sat_vel, pr_rate, x)``            (:45-63)
  ``runLeastSquares(t, sat_pos, pr, sat_vel, pr_rate, p_ref_ECEF)``     (:97-141)
      the per-epoch loop, as ONE launch (one lane walks the epochs in order,
      carrying the warm start), same result dict;
  ``run_batch(...)``: many logs at once (one lane per log, or with
      ``warm=False`` one lane per epoch).
  ``iterativeLeastSquares_multiTimeStep(t, sat_pos, pr, x=<shared>, b0=0, alpha=0, maxiter=100)``  (:66-94)
      the stationary receiver with a linearly drifting clock: ONE x, b0 (bias at
      t = 0) and alpha (drift) over all rows of a log; ``x`` is updated IN PLACE
      and its default is one shared array of its own (not iterativeLeastSquares's);
  ``runBatchLeastSquares(t, sat_pos, pr, p_ref_ECEF)``                  (:144-169)
      stacks a log's epochs and calls the above with its shared default; same dict;
  ``run_batch_multi(...)``: that fix for many logs at once (a group of 16 or 64
      lanes per log, ``mhe_ls_multi_run``).
Every solve runs in ``mhe_ls_run`` / ``mhe_ls_multi_run`` (csrc/mhe_ls.hip); without
libmhe.so the calls raise ``MheLibraryError``.  ``buildGeometryMatrix`` is the reference's
host helper (:6-16), kept for API parity.

Numerics: the reference solves pinv(G) drho; the kernel solves the 4x4 normal
equations by Cholesky -- the same least-squares solution for a full-rank G,
equal to rounding (tests state the tolerance).  Epochs with fewer than four
independent satellites report iters = -1 (the reference's pinv would return a
minimum-norm step there); a singular velocity system leaves v and bd NaN and the
position fix's iteration count untouched.

The multi-epoch fix solves the 5x5 normal equations the same way.  A log with fewer
than five rows, with all rows at one time (the 1 and t columns are then parallel) or
with a non-positive pivot reports iters = -1 and its last complete iterate.  Time
origin: with t = 0...39 s, as every reference script has it, cond(G) <= 130, and the
Cholesky and pinv iterations agree to 8e-9 m in x, 7e-9 m in b0 and 3e-9 m/s in
alpha with equal iteration counts (6, in 60 ragged cases of 2 to 40 epochs).  With t
offset by >= 1e3 s cond(G) grows to 1e5...1e12, b0 is the bias extrapolated far
outside the data, and the reference's own iteration misses its 1e-7 stop rule and
runs to maxiter (offset 1e4 s: two of three cases, 1e6 s: all three).  Centring t
inside the solve does not change that (the noise is in b0 itself), so none is done:
iteration counts are reproducible only for a time origin inside or next to the log.
"""
import ctypes

import numpy as np

from mhe import _lib

from . import utils as _gu

_DEFAULT_X = np.zeros(3)  # the reference's shared mutable default (utils/leastsquares.py:19)
_DEFAULT_X_MULTI = np.zeros(3)  # iterativeLeastSquares_multiTimeStep's own one (utils/leastsquares.py:66)


def buildGeometryMatrix(sat_pos, x):
    """Rows -(sat - x)/||sat - x|| (utils/leastsquares.py:6-16)."""
    sat_pos = np.asarray(sat_pos, dtype=np.float64)
    los = sat_pos - np.asarray(x, dtype=np.float64)[None, :]
    return -los / np.linalg.norm(los, axis=1, keepdims=True)


def _ptr(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


def run_batch(sat_pos, pr, nsat, x_init=None, sat_vel=None, pr_rate=None, warm=True, maxiter=100, tol=1e-7,
              device=None, stream=None):
    """Least-squares fixes for C logs of T epochs in one launch.

    sat_pos (C,T,S,3) ECEF, pr (C,T,S), nsat (C,T) valid slots per epoch,
    x_init (C,3) starting position (default zeros); sat_vel / pr_rate (C,T,S[,3])
    add the velocity solve.  NumPy or torch inputs.  Returns a dict of device
    tensors: x (C,T,3), b (C,T), iters (C,T), x_last (C,3) and, with velocities,
    v (C,T,3), bd (C,T).  stream: a torch stream to order the work on (default:
    the current one); outputs belong to it (mhe.streams)."""
    import torch

    from mhe.streams import keep_alive, launch_stream

    lib = _lib.load()
    dev = torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())
    with launch_stream(stream, dev) as (s, cur):
        out, used = _run_batch(lib, dev, s, sat_pos, pr, nsat, x_init, sat_vel, pr_rate, warm, maxiter, tol)
        keep_alive(s, cur, *used)
    return out


def _run_batch(lib, dev, s, sat_pos, pr, nsat, x_init, sat_vel, pr_rate, warm, maxiter, tol):
    import torch

    def d(a, dt=torch.float64):
        return None if a is None else torch.as_tensor(a, dtype=dt, device=dev).contiguous()

    sp, prt, ns = d(sat_pos), d(pr), d(nsat, torch.int32)
    if sp.dim() != 4 or sp.shape[-1] != 3:
        raise ValueError("sat_pos must be (chains, epochs, slots, 3)")
    C, T, S = sp.shape[:3]
    if tuple(prt.shape) != (C, T, S) or tuple(ns.shape) != (C, T):
        raise ValueError("pr must be (chains, epochs, slots) and nsat (chains, epochs)")
    xi = d(np.zeros((C, 3)) if x_init is None else x_init)
    with_vel = sat_vel is not None
    sv, rr = d(sat_vel), d(pr_rate)
    out = {"x": torch.empty((C, T, 3), dtype=torch.float64, device=dev),
           "b": torch.empty((C, T), dtype=torch.float64, device=dev),
           "iters": torch.empty((C, T), dtype=torch.int32, device=dev),
           "x_last": xi.clone()}
    if with_vel:
        out["v"] = torch.empty((C, T, 3), dtype=torch.float64, device=dev)
        out["bd"] = torch.empty((C, T), dtype=torch.float64, device=dev)
    dims = _lib.MheLsDims(slots=S, max_iter=int(maxiter), warm=1 if warm else 0, with_vel=1 if with_vel else 0,
                          tol=float(tol))
    rc = lib.mhe_ls_run(ctypes.byref(dims), C, T, _ptr(sp), _ptr(prt), _ptr(ns), _ptr(sv), _ptr(rr), _ptr(xi),
                        _ptr(out["x"]), _ptr(out["b"]), _ptr(out.get("v")), _ptr(out.get("bd")),
                        _ptr(out["iters"]), _ptr(out["x_last"]) if warm else None, ctypes.c_void_p(s.cuda_stream))
    _lib.check(rc, "mhe_ls_run")
    return out, [sp, prt, ns, sv, rr, xi] + list(out.values())


def _pack(sat_pos_list, values_lists, S=None):
    T = len(sat_pos_list)
    cnt = np.array([np.asarray(s).reshape(-1, 3).shape[0] for s in sat_pos_list], dtype=np.int32)
    S = max(4, int(cnt.max()) if T else 4) if S is None else S
    sp = np.zeros((1, T, S, 3))
    vals = [np.zeros((1, T, S) + np.asarray(v[0]).shape[1:]) if v is not None else None for v in values_lists]
    for k in range(T):
        c = cnt[k]
        sp[0, k, :c] = np.asarray(sat_pos_list[k]).reshape(-1, 3)
        for v, arr in zip(values_lists, vals):
            if v is not None:
                arr[0, k, :c] = np.asarray(v[k])
    return sp, vals, cnt[None]


def iterativeLeastSquares(sat_pos, pr, x=_DEFAULT_X, b=0, maxiter=100):
    """One epoch (utils/leastsquares.py:19-42); updates ``x`` in place, returns (x, b)."""
    sp, (prv,), cnt = _pack([sat_pos], [[pr]])
    if b != 0:  # the kernel starts b at 0 (the only value the reference ever passes)
        raise NotImplementedError("iterativeLeastSquares: non-zero initial bias")
    r = run_batch(sp, prv, cnt, x_init=np.asarray(x, dtype=np.float64)[None], maxiter=maxiter)
    x[:] = r["x"][0, 0].cpu().numpy()
    return x, float(r["b"][0, 0].item())


def iterativeLeastSquaresVel(sat_pos, sat_vel, pr_rate, x):
    """Velocity and bias rate at position x (utils/leastsquares.py:45-63)."""
    sp, (sv, rr), cnt = _pack([sat_pos], [[sat_vel], [pr_rate]])
    prv = np.zeros(sp.shape[:3])
    r = run_batch(sp, prv, cnt, x_init=np.asarray(x, dtype=np.float64)[None], sat_vel=sv, pr_rate=rr, maxiter=0)
    return r["v"][0, 0].cpu().numpy(), float(r["bd"][0, 0].item())


def runLeastSquares(t, sat_pos, pr, sat_vel=None, pr_rate=None, p_ref_ECEF=None):
    """Per-epoch fixes (utils/leastsquares.py:97-141), one launch; same dict."""
    T = np.asarray(t).shape[0]
    with_vel = sat_vel is not None
    sp, vals, cnt = _pack(list(sat_pos), [list(pr), list(sat_vel) if with_vel else None,
                                          list(pr_rate) if with_vel else None])
    r = run_batch(sp, vals[0], cnt, x_init=_DEFAULT_X[None], sat_vel=vals[1], pr_rate=vals[2])
    _DEFAULT_X[:] = r["x_last"][0].cpu().numpy()  # the shared default moves on, as in the reference
    X = r["x"][0].cpu().numpy()
    sol = {"t": t, "p_ref_ECEF": p_ref_ECEF, "bias": r["b"][0].cpu().numpy().copy(), "bias_rate": np.zeros(T)}
    for k in ("x_ECEF", "y_ECEF", "z_ECEF", "xd_ECEF", "yd_ECEF", "zd_ECEF", "x_ENU", "y_ENU", "z_ENU",
              "xd_ENU", "yd_ENU", "zd_ENU", "lat", "lon", "h"):
        sol[k] = np.zeros(T)
    sol["x_ECEF"], sol["y_ECEF"], sol["z_ECEF"] = X[:, 0].copy(), X[:, 1].copy(), X[:, 2].copy()
    for k in range(T):
        lla = _gu.ecef2lla(X[k])
        sol["lat"][k], sol["lon"][k], sol["h"][k] = lla[0], lla[1], lla[2]
        if p_ref_ECEF is not None:
            e = _gu.ecef2enu(X[k], p_ref_ECEF)
            sol["x_ENU"][k], sol["y_ENU"][k], sol["z_ENU"][k] = e[0], e[1], e[2]
    if with_vel:
        V = r["v"][0].cpu().numpy()
        sol["xd_ECEF"], sol["yd_ECEF"], sol["zd_ECEF"] = V[:, 0].copy(), V[:, 1].copy(), V[:, 2].copy()
        sol["bias_rate"] = r["bd"][0].cpu().numpy().copy()
        if p_ref_ECEF is not None:
            for k in range(T):
                e = _gu.ecef2enu(V[k], p_ref_ECEF, rotation_only=True)
                sol["xd_ENU"][k], sol["yd_ENU"][k], sol["zd_ENU"][k] = e[0], e[1], e[2]
    sol["iters"] = r["iters"][0].cpu().numpy()
    return sol


# ---------------------------------------------------------------- multi-epoch fix

def run_batch_multi(sat_pos, pr, t, nrows=None, p_init=None, maxiter=100, tol=1e-7, device=None, stream=None):
    """Stationary-receiver fixes (x, b0, alpha over all rows of a log) for C logs in one launch.

    Flat rows: sat_pos (C,R,3) ECEF, pr (C,R), t (C,R) the time of each row, nrows (C)
    valid rows per log (default R).  Or run_batch's epoch-packed layout: sat_pos
    (C,T,S,3), pr (C,T,S), t (C,T) one time per epoch, nrows (C,T) valid slots per epoch
    (default S); it is compacted to flat rows of capacity T*S on the device (torch
    operations, no host round trip).  p_init (C,5): x, b0, alpha to start from (default
    zeros).  NumPy or torch inputs.  Returns a dict of device tensors: x (C,3), b0 (C),
    alpha (C), iters (C) (-1: flagged, see the module docstring).  The lane-group size is a
    function of the row capacity alone, so a log's result is bitwise the same alone or in
    any batch of that capacity.  stream: as run_batch."""
    import torch

    from mhe.streams import keep_alive, launch_stream

    lib = _lib.load()
    dev = torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())
    with launch_stream(stream, dev) as (s, cur):
        out, used = _run_batch_multi(lib, dev, s, sat_pos, pr, t, nrows, p_init, maxiter, tol)
        keep_alive(s, cur, *used)
    return out


def _compact_epochs(sp, prt, tt, ns):
    """(C,T,S[,3]) with nsat (C,T) -> flat rows (C,T*S[,3]), the valid slots first and in
    order (a stable sort of the validity mask), and the rows per log."""
    import torch

    C, T, S = prt.shape
    valid = (torch.arange(S, device=prt.device)[None, None, :] < ns[..., None]).reshape(C, T * S)
    order = torch.argsort((~valid).to(torch.int8), dim=1, stable=True)
    sp = torch.gather(sp.reshape(C, T * S, 3), 1, order[..., None].expand(C, T * S, 3)).contiguous()
    prt = torch.gather(prt.reshape(C, T * S), 1, order).contiguous()
    tt = torch.gather(tt[..., None].expand(C, T, S).reshape(C, T * S), 1, order).contiguous()
    return sp, prt, tt, valid.sum(1).to(torch.int32)


def _run_batch_multi(lib, dev, s, sat_pos, pr, t, nrows, p_init, maxiter, tol):
    import torch

    def d(a, dt=torch.float64):
        return None if a is None else torch.as_tensor(a, dtype=dt, device=dev).contiguous()

    sp, prt, tt, nr = d(sat_pos), d(pr), d(t), d(nrows, torch.int32)
    if sp.dim() == 4 and sp.shape[-1] == 3:
        C, T, S = sp.shape[:3]
        if tuple(prt.shape) != (C, T, S) or tuple(tt.shape) != (C, T):
            raise ValueError("epoch-packed rows: pr must be (chains, epochs, slots) and t (chains, epochs)")
        nr = torch.full((C, T), S, dtype=torch.int32, device=dev) if nr is None else nr
        if tuple(nr.shape) != (C, T):
            raise ValueError("epoch-packed rows: nrows must be the slots per epoch (chains, epochs)")
        sp, prt, tt, nr = _compact_epochs(sp, prt, tt, nr.clamp(0, S))
    elif sp.dim() != 3 or sp.shape[-1] != 3:
        raise ValueError("sat_pos must be (chains, rows, 3) or (chains, epochs, slots, 3)")
    C, R = sp.shape[:2]
    if tuple(prt.shape) != (C, R) or tuple(tt.shape) != (C, R):
        raise ValueError("pr and t must be (chains, rows)")
    nr = torch.full((C,), R, dtype=torch.int32, device=dev) if nr is None else nr
    if tuple(nr.shape) != (C,):
        raise ValueError("nrows must be (chains,)")
    pi = d(np.zeros((C, 5)) if p_init is None else p_init)
    if tuple(pi.shape) != (C, 5):
        raise ValueError("p_init must be (chains, 5): x, b0, alpha")
    p = torch.empty((C, 5), dtype=torch.float64, device=dev)
    iters = torch.empty((C,), dtype=torch.int32, device=dev)
    dims = _lib.MheLsmDims(max_iter=int(maxiter), tol=float(tol))
    rc = lib.mhe_ls_multi_run(ctypes.byref(dims), C, R, _ptr(sp), _ptr(prt), _ptr(tt), _ptr(nr), _ptr(pi), _ptr(p),
                              _ptr(iters), ctypes.c_void_p(s.cuda_stream))
    _lib.check(rc, "mhe_ls_multi_run")
    out = {"x": p[:, :3], "b0": p[:, 3], "alpha": p[:, 4], "iters": iters}
    return out, [sp, prt, tt, nr, pi, p, iters]


def iterativeLeastSquares_multiTimeStep(t, sat_pos, pr, x=_DEFAULT_X_MULTI, b0=0, alpha=0, maxiter=100):
    """All rows of one log (utils/leastsquares.py:66-94): t, sat_pos, pr are flat, one entry
    per pseudorange.  Updates ``x`` in place, returns (x, b0, alpha)."""
    sp = np.asarray(sat_pos, dtype=np.float64).reshape(1, -1, 3)
    p0 = np.concatenate((np.asarray(x, dtype=np.float64), [float(b0), float(alpha)]))[None]
    r = run_batch_multi(sp, np.asarray(pr, dtype=np.float64).reshape(1, -1),
                        np.asarray(t, dtype=np.float64).reshape(1, -1), p_init=p0, maxiter=maxiter)
    x[:] = r["x"][0].cpu().numpy()
    return x, float(r["b0"][0].item()), float(r["alpha"][0].item())


def runBatchLeastSquares(t, sat_pos, pr, p_ref_ECEF=None):
    """One fix over a whole log (utils/leastsquares.py:144-169): t (T,), sat_pos / pr lists of
    per-epoch arrays.  Same dict; starts from (and moves on) the shared default x."""
    t_rows = np.concatenate([np.full(np.asarray(pr[i]).shape[0], t[i], dtype=np.float64)
                             for i in range(np.asarray(t).shape[0])] + [np.zeros(0)])
    sp_rows = np.concatenate([np.asarray(s_, dtype=np.float64).reshape(-1, 3) for s_ in sat_pos] + [np.zeros((0, 3))])
    pr_rows = np.concatenate([np.asarray(p_, dtype=np.float64).reshape(-1) for p_ in pr] + [np.zeros(0)])
    p_ECEF, b0, alpha = iterativeLeastSquares_multiTimeStep(t_rows, sp_rows, pr_rows)
    p_LLA = _gu.ecef2lla(p_ECEF)
    sol = {"t": t, "p_ref_ECEF": p_ref_ECEF, "b0": b0, "alpha": alpha,
           "x_ECEF": p_ECEF[0], "y_ECEF": p_ECEF[1], "z_ECEF": p_ECEF[2],
           "lat": p_LLA[0], "lon": p_LLA[1], "h": p_LLA[2]}
    if p_ref_ECEF is not None:
        p_ENU = _gu.ecef2enu(p_ECEF, p_ref_ECEF)
        sol["x_ENU"], sol["y_ENU"], sol["z_ENU"] = p_ENU[0], p_ENU[1], p_ENU[2]
    return sol
