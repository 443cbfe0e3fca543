"""Batched Gauss-Newton solver on libmhe.so (device-resident, torch as container).

``BatchSolver`` owns the device constants of one problem structure (N, T,
models, measurement times, weights) and solves many independent trajectories
that share it:  X (B, P, n), U (B|1, P, m), Y (B, M, p), PAR (B|1, M, q),
x0 (B, n).  Everything is fp64 and stays in HBM between calls; the HIP work is
enqueued on the current torch stream (or the one passed in: inputs are staged and
outputs allocated on that stream after it waits for the current one, and every
tensor the launch touches is kept alive for it -- mhe.streams).  The large-system
workspace is cached per stream, so concurrent solves on different streams never
share one.
"""
import collections
import ctypes

import numpy as np
import torch

from . import _lib, registry
from .streams import keep_alive, launch_stream

STATUS_CONVERGED, STATUS_MAX_ITER, STATUS_NOT_SPD, STATUS_NONFINITE, STATUS_BAD_CONSTANTS = 0, 1, 2, 3, 4


def _dev(x, device, shape=None):
    if x is None:
        return None
    if isinstance(x, torch.Tensor):
        t = x.to(device=device, dtype=torch.float64)
    else:
        t = torch.as_tensor(np.asarray(x, dtype=np.float64), device=device)
    t = t.contiguous()
    if shape is not None and tuple(t.shape) != tuple(shape):
        raise ValueError(f"expected shape {shape}, got {tuple(t.shape)}")
    return t


def _ptr(t):
    return None if t is None else ctypes_ptr(t)


def _at(t, lo, per, itemsize=8):
    """Pointer to trajectory ``lo`` of a batch-outermost tensor with ``per`` elements per
    trajectory (per = 0: an input shared by the batch)."""
    if t is None:
        return None
    return ctypes.c_void_p(t.data_ptr() + itemsize * lo * per)


def ctypes_ptr(t):
    import ctypes
    return ctypes.c_void_p(t.data_ptr())


def _handle(s):
    import ctypes
    return ctypes.c_void_p(s.cuda_stream)


# the device inputs BatchSolver.prepare stages (U and PAR with their batch strides, 0 = shared)
Staged = collections.namedtuple("Staged", "X B U ustr Y PAR pstr x0")


class _Point:
    """Everything one operating point stages on the device: the ``Staged`` inputs, the extra
    variables ``Z`` (and where a solve writes them, ``Z_out``) and the per-solve ``Rw``,
    ``meas_delta`` and ``Pw`` with their batch strides.  ``args`` is the one place an
    ``MheSolveArgs`` is filled from them; ``tensors`` is what a launch must keep alive."""

    def __init__(self, solver, staged, Z=None, Z_out=None, Rw=None, meas_delta=None, Pw=None):
        self.solver, self.staged, self.B = solver, staged, staged.B
        self.Z, self.Z_out = Z, Z_out
        self.Rw, self.rstr = solver._rw(Rw, self.B)
        self.md, self.mstr = solver._md(meas_delta, self.B)
        self.Pw, self.wstr = solver._pw(Pw, self.B)

    @property
    def tensors(self):
        g = self.staged
        return g.X, self.Z, self.Z_out, g.U, g.Y, g.PAR, self.Rw, self.md, self.Pw, g.x0

    def args(self, lo, c, ws, nb):
        """``MheSolveArgs`` of the trajectories [lo, lo + c) over the workspace (ws, nb); the
        outputs and iteration limits of a solve are the caller's to add."""
        s, g = self.solver, self.staged
        a = _lib.MheSolveArgs()
        a.batch = c
        a.X0 = _at(g.X, lo, s.P * s.n)
        a.Z0, a.Z_out = _at(self.Z, lo, s.n_extra), _at(self.Z_out, lo, s.n_extra)
        a.U, a.u_bstride = _at(g.U, lo, g.ustr), g.ustr
        a.Y = _at(g.Y, lo, s.M * s.p)
        a.PAR, a.par_bstride = _at(g.PAR, lo, g.pstr), g.pstr
        a.x0 = _at(g.x0, lo, s.n)
        a.Rw, a.rw_bstride = _at(self.Rw, lo, self.rstr), self.rstr
        a.meas_delta, a.md_bstride = _at(self.md, lo, self.mstr), self.mstr
        a.Pw, a.pw_bstride = _at(self.Pw, lo, self.wstr), self.wstr
        a.workspace, a.workspace_bytes = _ptr(ws), nb
        return a


class BatchSolver:
    """Device constants + launch wrappers for one problem structure.

    Parameters (host numpy or torch):
      N, T            collocation order and window length
      dyn, meas       plug-in functions (or names) -- see mhe.registry
      D (P,P), cw (P) differentiation matrix, (T/2) * quadrature weights
      Phi (M,P)       Lagrange basis at the measurement times
      Qw (n,n)        dynamics-cost information (weighted_l2_norm params["Q"])
      Rw (M,p,p)      measurement information (R passed to addResidualCost)
      Pw (n,n)|None   prior information (addInitialCost), None = no prior
      meas_idx        static index parameters of the measurement model
      dyn_cost        "l2" (weighted_l2_norm) or "huber" (pseudo_huber_loss, IRLS; huber_delta)
      bounds          [(state component, lb, ub), ...] enforced by projected Newton (addVarBounds)
      n_extra         extra decision variables z (meas="mixed" rows may reference them)
      eq              (K, 2) equality constraints v[a] - v[b] = r on the node-major state
                      vector (b = -1: v[a] = r), met by every GN step (bordered KKT solve);
                      after each solve ``self.lam`` (B, K) holds their multipliers
                      (L = J + lam^T (C v - r))
      eq_rhs          (K,) the constants r (None: 0, the addEqConstraint rows)
      force_large     take the large-system path even when the register-resident kernel
                      fits (parity tests of the two paths; fixed at construction)
      fused_general   prefer the fused single-launch kernel (k_gn_general) for a mixed-row
                      problem that fits it (L2 dynamics cost, no bounds, n <= 16, padded system
                      <= 208; mhe.h MHE_PATH_FUSED_GENERAL) -- ``self.fused_general`` tells
                      whether it does; otherwise the default path, bitwise.  Exclusive with
                      force_large.  covariance / arrival / assemble / chol_solve and
                      solve(meas_delta=) go through a default-path sibling (``sibling()``):
                      their outputs are exactly the default path's (assemble / chol_solve
                      exchange ITS padded KKT system, ``sibling().kkt_dim`` rows)
      dyn_par         static dynamics parameters (mhe_dims.dyn_par; registry.dyn_params turns a
                      plug-in's params dict into it, e.g. car_params for vehicle_dynamics_and_gnss)
      constants       "build" (default): build the device constants here; "receive": only
                      allocate ``cbuf`` -- a data-parallel rank > 0 receives rank 0's bytes
                      (mhe.dist.broadcast_) and then calls constants_ready()
    With meas="mixed", PAR rows follow include/mhe.h (q = 14) and Rw is (M,) weights.
    """

    WS_CACHE = 2  # large-system workspaces kept alive (one per recently used stream)
    ws_budget = None  # bytes of workspace one launch may use (None: 85 % of the free HBM)

    def __init__(self, N, T, dyn, meas, D, cw, Phi, Qw, Rw, Pw=None, meas_idx=None, device="cuda",
                 dyn_cost="l2", huber_delta=None, bounds=None, n_extra=0, eq=None, force_large=False,
                 dyn_par=None, eq_rhs=None, constants="build", fused_general=False):
        if fused_general and force_large:
            raise ValueError("fused_general and force_large are exclusive (one path preference per solver)")
        self.lib = _lib.load()
        if not torch.cuda.is_available():
            raise _lib.MheLibraryError("no HIP device visible: the estimator has no CPU path")
        self.device = torch.device(device)
        dname, (did, n, m) = registry.dyn_model(dyn)
        mname, (mid, p, q, linear) = registry.meas_model(meas)
        registry.check_pair(dname, mname)
        p = n if p is None else p
        self.N, self.T, self.n, self.m, self.p, self.q = int(N), float(T), n, m, p, q
        self.P = self.N + 1
        Phi = np.asarray(Phi, dtype=np.float64).reshape(-1, self.P)
        self.M = Phi.shape[0]
        self.dyn_name, self.meas_name, self.linear_meas = dname, mname, linear
        dims = _lib.MheDims()
        dims.N, dims.n, dims.m, dims.p, dims.M, dims.q = self.N, n, m, p, self.M, q
        dims.dyn_model, dims.meas_model = did, mid
        dims.has_prior = 0 if Pw is None else 1
        idx = list(meas_idx) if meas_idx is not None else [0, 1, 2, 3]
        for i in range(8):
            dims.meas_idx[i] = idx[i] if i < len(idx) else 0
        dims.T = self.T
        if dyn_cost not in ("l2", "huber"):
            raise ValueError(f"dyn_cost must be 'l2' or 'huber', got {dyn_cost!r}")
        dims.dyn_cost = 1 if dyn_cost == "huber" else 0
        dims.huber_delta = float(huber_delta) if huber_delta is not None else 0.0
        bounds = list(bounds or [])
        if len(bounds) > 8:
            raise ValueError("at most 8 bounded state components")
        dims.n_bounds = len(bounds)
        for i, (c, lo, hi) in enumerate(bounds):
            dims.bound_idx[i] = int(c)
            dims.bound_lb[i] = -np.inf if lo is None else float(lo)
            dims.bound_ub[i] = np.inf if hi is None else float(hi)
        self.dyn_cost, self.huber_delta, self.bounds = dyn_cost, huber_delta, bounds
        self.n_extra = int(n_extra)
        if self.n_extra and mname != "mixed":
            raise ValueError("extra variables enter mixed measurement rows only (meas='mixed')")
        dims.n_extra = self.n_extra
        self._eq = np.zeros(0, dtype=np.int32) if eq is None else np.ascontiguousarray(
            np.asarray(eq, dtype=np.int32).reshape(-1, 2).ravel())
        dims.n_eq = self._eq.size // 2
        self._eq_rhs = np.zeros(dims.n_eq) if eq_rhs is None else np.ascontiguousarray(
            np.asarray(eq_rhs, dtype=np.float64).ravel())
        if self._eq_rhs.size != dims.n_eq:
            raise ValueError("eq_rhs needs one constant per equality row")
        if dims.n_eq:
            import ctypes
            dims.eq_idx = self._eq.ctypes.data_as(ctypes.POINTER(ctypes.c_int32))  # self._eq keeps it alive
            dims.eq_rhs = self._eq_rhs.ctypes.data_as(ctypes.POINTER(ctypes.c_double))
        self.n_eq = dims.n_eq
        self.lam = None
        dims.force_large = (_lib.PATH_FUSED_GENERAL if fused_general else
                            _lib.PATH_LARGE if force_large else _lib.PATH_AUTO)
        if dyn_par is None and dname == "vehicle_dynamics_and_gnss":
            raise ValueError("vehicle_dynamics_and_gnss needs dyn_par (registry.dyn_params(name, params))")
        dp = np.zeros(8) if dyn_par is None else np.asarray(dyn_par, dtype=np.float64).ravel()
        for i in range(8):
            dims.dyn_par[i] = float(dp[i]) if i < dp.size else 0.0
        self.dyn_par = dp
        self.dims = dims
        # the fused single-launch kernel takes these dims (a preference: for every other dims
        # fused_general=True is the default path): a general problem without a workspace
        self.fused_general = bool(fused_general) and self.general and self.lib.mhe_workspace_bytes(dims, 1) == 0
        self._sibling = None
        self._ctor = None
        if self.fused_general:
            # host copies for the default-path sibling (covariance, arrival, assemble,
            # chol_solve, robust rows), built on first use
            host = lambda x: None if x is None else np.array(x.cpu() if isinstance(x, torch.Tensor) else x,  # noqa: E731
                                                             dtype=np.float64)
            self._ctor = dict(N=N, T=T, dyn=dyn, meas=meas, D=host(D), cw=host(cw), Phi=host(Phi), Qw=host(Qw),
                              Rw=host(Rw), Pw=host(Pw), meas_idx=meas_idx, device=device, dyn_cost=dyn_cost,
                              huber_delta=huber_delta, bounds=bounds, n_extra=n_extra, eq=eq, dyn_par=dyn_par,
                              eq_rhs=eq_rhs)
        self._alloc_constants()
        dev = self.device
        self._ws = collections.OrderedDict()  # large-system workspace per stream handle (LRU, <= WS_CACHE)
        self._built = torch.cuda.Event()  # launches on any stream wait for the constants
        if constants == "receive":
            # another process builds the buffer (rank 0 of a data-parallel job); the caller
            # fills self.cbuf (mhe.dist.broadcast_) and then calls constants_ready()
            self._ready = False
            return
        if constants != "build":
            raise ValueError(f"constants must be 'build' or 'receive', got {constants!r}")
        self._ready = True
        src = dict(D=np.asarray(D, np.float64), cw=np.asarray(cw, np.float64), Phi=Phi,
                   Qw=np.asarray(Qw, np.float64), Rw=np.asarray(Rw, np.float64).reshape(self.M, p, p),
                   Pw=None if Pw is None else np.asarray(Pw, np.float64))
        src = {k: _dev(v, dev) for k, v in src.items() if v is not None}
        cur = torch.cuda.current_stream(dev)
        build = lambda: self.lib.mhe_build_constants(  # noqa: E731
            self.dims, _ptr(src["D"]), _ptr(src["cw"]), _ptr(src["Phi"]),
            _ptr(src["Qw"]), _ptr(src["Rw"]), _ptr(src.get("Pw")), _ptr(self.cbuf), _handle(cur))
        rc = build()
        if rc == -4 and self.fused_general:
            # more distinct measurement times than the fused kernel's LDS layout holds: the
            # preference falls back to the default path
            self.dims.force_large = _lib.PATH_AUTO
            self.fused_general, self._ctor = False, None
            self._alloc_constants()
            rc = build()
        _lib.check(rc, "mhe_build_constants")
        # the staging tensors may be freed now: the build reads them on `cur`, where the
        # caching allocator orders their reuse
        self._built.record(cur)

    def _alloc_constants(self):
        self.dp = self.lib.mhe_padded_dim(self.dims)
        if self.dp < 0:
            raise _lib.MheCallError("mhe_padded_dim: unsupported dims (system too large for this build?)")
        nbytes = self.lib.mhe_const_bytes(self.dims)
        if nbytes == 0:
            raise _lib.MheCallError("mhe_const_bytes: invalid dims")
        self.cbuf = torch.empty(nbytes, dtype=torch.uint8, device=self.device)

    def sibling(self):
        """The default-path solver of the same problem, for what the fused kernel does not do
        (covariance, arrival, assemble, chol_solve, solve with meas_delta): built on first use
        from the host arrays this solver keeps; outputs and refusals are the default path's."""
        if not self.fused_general:
            raise _lib.MheCallError("sibling(): not a fused-general solver")
        if self._sibling is None:
            if self._ctor["D"] is None:
                raise _lib.MheCallError("sibling(): this solver received its constants and has no host arrays")
            self._sibling = BatchSolver(**self._ctor)
        return self._sibling

    def constants_ready(self, stream=None):
        """A solver built with constants="receive": self.cbuf now holds the bytes another
        process built for the same dims (enqueued on ``stream``, default the current one);
        later launches on any stream wait for that point.  A buffer built for other dims
        is refused per trajectory by the kernels' layout stamp (MHE_STATUS_BAD_CONSTANTS)."""
        s = torch.cuda.current_stream(self.device) if stream is None else stream
        self._built.record(s)
        self._ready = True

    def _check_ready(self):
        if not self._ready:
            raise _lib.MheCallError("constants not received yet: fill cbuf and call constants_ready()")

    # ------------------------------------------------------------------ inputs
    def _inputs(self, X, U, Y, PAR, x0):
        dev = self.device
        X = _dev(X, dev)
        if X.dim() != 3 or X.shape[1:] != (self.P, self.n):
            raise ValueError(f"X must be (B, {self.P}, {self.n}), got {tuple(X.shape)}")
        B = X.shape[0]
        U_t, ustr = None, 0
        if self.m > 0:
            if U is None:
                raise ValueError("controls U are required for this dynamics model")
            U_t = _dev(U, dev)
            if U_t.dim() == 2:
                U_t = U_t[None]
            if U_t.shape[1:] != (self.P, self.m) or U_t.shape[0] not in (1, B):
                raise ValueError(f"U must be (B|1, {self.P}, {self.m}), got {tuple(U_t.shape)}")
            ustr = 0 if U_t.shape[0] == 1 else self.P * self.m
        Y_t = _dev(Y, dev, (B, self.M, self.p))
        PAR_t, pstr = None, 0
        if self.q > 0:
            PAR_t = _dev(PAR, dev)
            if PAR_t.dim() == 2:
                PAR_t = PAR_t[None]
            if PAR_t.shape[1:] != (self.M, self.q) or PAR_t.shape[0] not in (1, B):
                raise ValueError(f"PAR must be (B|1, {self.M}, {self.q}), got {tuple(PAR_t.shape)}")
            pstr = 0 if PAR_t.shape[0] == 1 else self.M * self.q
        x0_t = None
        if self.dims.has_prior:
            x0_t = _dev(x0, dev, (B, self.n))
        return Staged(X, B, U_t, ustr, Y_t, PAR_t, pstr, x0_t)

    @property
    def large_system(self):
        """True when the problem exceeds the register-resident kernel (C3-C5):
        mhe_gn_solve_ws then needs a device workspace (allocated here, cached)."""
        return self.lib.mhe_workspace_bytes(self.dims, 1) > 0

    def _chunk(self, B, s=None):
        """Trajectories per launch on the large-system path: all B unless their
        workspace exceeds the budget (ws_budget bytes, default 85 % of the free HBM
        plus the workspace this solver holds for stream ``s``, which the launch
        replaces) -- then the batch is streamed in equal chunks through one workspace
        (C5: 2048 trajectories x 0.28 GB).  Workspaces cached for OTHER streams stay
        allocated (a launch there may still be using them), so they are not counted
        as free."""
        per = self.lib.mhe_workspace_bytes(self.dims, 1)
        if per == 0 or B == 0:
            return B
        budget = self.ws_budget
        if budget is None:
            free, _ = torch.cuda.mem_get_info(self.device)
            own = self._ws.get(s.cuda_stream) if s is not None else None
            budget = int(0.85 * (free + (own.numel() if own is not None else 0)))
        k = max(1, min(B, budget // per))
        if k >= B:
            return B
        # k_big_chol runs one workgroup per trajectory: a chunk that is a whole number of
        # CU-fulls leaves no CUs idle in a tail round (C5: 410 -> 256, 0.39 -> 0.46 of peak)
        cus = torch.cuda.get_device_properties(self.device).multi_processor_count
        if k > cus:
            k -= k % cus
        nch = -(-B // k)
        return -(-B // nch)  # equal chunks

    def _workspace(self, B, s):
        """Workspace for B trajectories on stream s (allocated on s: one per stream, so
        concurrent solves on different streams never share or free each other's)."""
        nb = self.lib.mhe_workspace_bytes(self.dims, B)
        if nb == 0:
            return None, 0
        key = s.cuda_stream
        ws = self._ws.pop(key, None)
        if ws is None or ws.numel() < nb:
            ws = None  # release the old one before allocating the larger one
            ws = torch.empty(nb, dtype=torch.uint8, device=self.device)
        self._ws[key] = ws  # most recently used last
        while len(self._ws) > self.WS_CACHE:
            # dropping the reference is safe: a launch on another stream recorded its
            # workspace on that stream (keep_alive), so the allocator reuses it only
            # after that stream's work is done
            self._ws.popitem(last=False)
        return ws, nb

    def _chunks(self, B, s):
        """(chunk, ws, nb, [(lo, c), ...]): the launches that stream B trajectories through one
        workspace on stream s -- the outputs are written in place at each chunk's offset."""
        chunk = max(1, self._chunk(B, s))
        ws, nb = self._workspace(chunk, s)
        return chunk, ws, nb, [(lo, min(chunk, B - lo)) for lo in range(0, B, chunk)]

    def _rw(self, Rw, B):
        """Per-solve measurement weights (mhe_solve_args.Rw): (B|1, M, p, p), or (B|1, M)
        for mixed rows; None = the weights the constants were built with."""
        if Rw is None:
            return None, 0
        if self.linear_meas:
            raise ValueError("per-solve Rw needs a nonlinear measurement model (a linear h folds R into the constants)")
        shape = (self.M,) if self.meas_name == "mixed" else (self.M, self.p, self.p)
        t = _dev(Rw, self.device)
        if t.shape == shape:
            t = t[None]
        if t.shape[1:] != shape or t.shape[0] not in (1, B):
            raise ValueError(f"Rw must be (B|1,) + {shape}, got {tuple(t.shape)}")
        return t, (0 if t.shape[0] == 1 else int(np.prod(shape)))

    def _md(self, meas_delta, B):
        """Pseudo-Huber scales of the measurement rows (mhe_solve_args.meas_delta): (B|1, M)
        or (M,), float64, every value > 0 (+inf = a quadratic row); None = quadratic rows."""
        if meas_delta is None:
            return None, 0
        if self.linear_meas:
            raise ValueError("meas_delta needs a nonlinear measurement model (a linear h folds R into the constants)")
        if self.p != 1:
            raise ValueError("meas_delta needs scalar measurement rows (p = 1)")
        if isinstance(meas_delta, torch.Tensor):
            if meas_delta.dtype != torch.float64:
                raise ValueError(f"meas_delta must be float64, got {meas_delta.dtype}")
        else:
            meas_delta = np.asarray(meas_delta)
            if meas_delta.dtype != np.float64:
                raise ValueError(f"meas_delta must be float64, got {meas_delta.dtype}")
        t = _dev(meas_delta, self.device)
        if t.dim() == 1:
            t = t[None]
        if t.dim() != 2 or t.shape[1] != self.M or t.shape[0] not in (1, B):
            raise ValueError(f"meas_delta must be (B|1, {self.M}) or ({self.M},), got {tuple(t.shape)}")
        if not bool((t > 0).all()):  # NaN fails the comparison too
            raise ValueError("meas_delta must be > 0 (+inf = quadratic row)")
        return t, (0 if t.shape[0] == 1 else self.M)

    def _pw(self, Pw, B):
        """Per-solve prior weight (mhe_solve_args.Pw): (B|1, n, n) or (n, n), float64, every
        block symmetric (checked exactly; the blocks mhe_arrival writes are, NaN blocks of a
        failed trajectory pass and keep that trajectory NaN); needs a prior.  None = the
        weight the constants were built with."""
        if Pw is None:
            return None, 0
        if not self.dims.has_prior:
            raise ValueError("per-solve Pw needs a prior (construct the solver with Pw, e.g. zeros)")
        if isinstance(Pw, torch.Tensor):
            if Pw.dtype != torch.float64:
                raise ValueError(f"Pw must be float64, got {Pw.dtype}")
        else:
            Pw = np.asarray(Pw)
            if Pw.dtype != np.float64:
                raise ValueError(f"Pw must be float64, got {Pw.dtype}")
        n = self.n
        t = _dev(Pw, self.device)
        if t.dim() == 2:
            t = t[None]
        if t.dim() != 3 or t.shape[1:] != (n, n) or t.shape[0] not in (1, B):
            raise ValueError(f"Pw must be (B|1, {n}, {n}) or ({n}, {n}), got {tuple(t.shape)}")
        tt = t.transpose(1, 2)
        if not bool(((t == tt) | ((t != t) & (tt != tt))).all()):
            raise ValueError("Pw must be symmetric (every (n, n) block equal to its transpose)")
        return t, (0 if t.shape[0] == 1 else n * n)

    def _gn(self, s, cur, pt, outs, max_iter, tol, lam=None):
        if pt.B == 0:
            return
        Xo, cost, iters, status = outs
        _, ws, nb, spans = self._chunks(pt.B, s)
        for lo, c in spans:
            a = pt.args(lo, c, ws, nb)
            a.X_out = _at(Xo, lo, self.P * self.n)
            a.cost_out, a.iters_out, a.status_out = _at(cost, lo, 1), _at(iters, lo, 1, 4), _at(status, lo, 1, 4)
            a.max_iter, a.tol = int(max_iter), float(tol)
            a.lambda_out = _at(lam, lo, self.n_eq)
            rc = self.lib.mhe_solve(self.dims, _ptr(self.cbuf), ctypes.byref(a), _handle(s))
            _lib.check(rc, "mhe_solve")
        keep_alive(s, cur, *pt.tensors, Xo, cost, iters, status, ws, lam)

    # ------------------------------------------------------------------ calls
    def solve(self, X0, U, Y, PAR=None, x0=None, max_iter=20, tol=1e-10, stream=None, out=None, Z0=None, Rw=None,
              lam_out=None, meas_delta=None, Pw=None):
        """Gauss-Newton to convergence. Returns (X, cost, iters, status) device tensors,
        and the extra variables Z (B, n_extra) as a fifth element when n_extra > 0.
        ``Pw`` (B|1, n, n) or (n, n), float64, symmetric: the prior (arrival-cost) weight of
        this solve per trajectory, replacing the constants' (every model and solve mode; needs
        a prior) -- ``arrival()`` returns the next window's as a device tensor.
        ``Rw`` (B|1, M, p, p) -- (B|1, M) for mixed rows -- replaces the measurement
        weights of the constants for this solve (nonlinear models; the MHE windows'
        R = 0 slot masks).  ``meas_delta`` (B|1, M) or (M,), float64, > 0: the pseudo-Huber
        scale of every (scalar) measurement row, in the row's units -- the reference's
        pseudo_huber_loss with Q = R_i, solved by IRLS; +inf keeps a row quadratic, ``cost`` is
        the robust objective (nonlinear models with p = 1).  With ``stream`` the work (staging included) is ordered on
        that stream; consume the outputs there or make the consuming stream wait for it.
        ``lam_out`` (B, n_eq) float64 device tensor: receives this solve's constraint
        multipliers (the per-call way; ``self.lam`` is the last solve's on any stream,
        kept for single-stream callers).  A fused-general solver runs k_gn_general; with
        ``meas_delta`` its default-path sibling does."""
        self._check_ready()
        if self.fused_general and meas_delta is not None:
            sib = self.sibling()
            r = sib.solve(X0, U, Y, PAR, x0, max_iter, tol, stream, out, Z0, Rw, lam_out, meas_delta, Pw)
            self.lam = sib.lam
            return r
        with launch_stream(stream, self.device, (self._built,)) as (s, cur):
            staged = self._inputs(X0, U, Y, PAR, x0)
            X, B = staged.X, staged.B
            if out is None:
                Xo = torch.empty_like(X)
                cost = torch.empty(B, dtype=torch.float64, device=self.device)
                iters = torch.empty(B, dtype=torch.int32, device=self.device)
                status = torch.empty(B, dtype=torch.int32, device=self.device)
            else:
                Xo, cost, iters, status = out
            Z = Zo = None
            if self.n_extra:
                Z = _dev(np.zeros((B, self.n_extra)) if Z0 is None else Z0, self.device, (B, self.n_extra))
                Zo = torch.empty_like(Z)
            lam = None
            if self.n_eq:
                if lam_out is not None:
                    if tuple(lam_out.shape) != (B, self.n_eq) or lam_out.dtype != torch.float64:
                        raise ValueError(f"lam_out must be float64 ({B}, {self.n_eq})")
                    lam = lam_out
                    lam.zero_()
                else:
                    lam = torch.zeros((B, self.n_eq), dtype=torch.float64, device=self.device)
            self._gn(s, cur, _Point(self, staged, Z, Zo, Rw, meas_delta, Pw), (Xo, cost, iters, status), max_iter,
                     tol, lam)
            self.lam = lam
        if self.n_extra:
            return Xo, cost, iters, status, Zo
        return Xo, cost, iters, status

    def prepare(self, X0, U, Y, PAR=None, x0=None):
        """Pre-stage device inputs once (bench: inputs resident before timing)."""
        return self._inputs(X0, U, Y, PAR, x0)

    def solve_staged(self, staged, outs, max_iter, tol, stream=None, meas_delta=None, Pw=None):
        self._check_ready()
        with launch_stream(stream, self.device, (self._built,)) as (s, cur):
            staged = staged if isinstance(staged, Staged) else Staged(*staged)
            self._gn(s, cur, _Point(self, staged, meas_delta=meas_delta, Pw=Pw), outs, max_iter, tol)

    def resjac(self, X, U, Y, PAR=None, stream=None):
        """Per-node defects W (B,P,n) and dynamics Jacobians F (B,P,n,n), per-row
        residuals E (B,M,p) and measurement Jacobians Hm (B,M,p,n) at X (mhe_resjac)."""
        self._check_ready()
        with launch_stream(stream, self.device, (self._built,)) as (s, cur):
            X, B, U_t, ustr, Y_t, PAR_t, pstr, _ = self._inputs(X, U, Y, PAR, np.zeros((X.shape[0], self.n))
                                                                if self.dims.has_prior else None)
            f64 = dict(dtype=torch.float64, device=self.device)
            W = torch.empty((B, self.P, self.n), **f64)
            F = torch.empty((B, self.P, self.n, self.n), **f64)
            E = torch.empty((B, self.M, self.p), **f64)
            Hm = torch.empty((B, self.M, self.p, self.n), **f64)
            rc = self.lib.mhe_resjac(self.dims, _ptr(self.cbuf), B, _ptr(X), _ptr(U_t), ustr, _ptr(Y_t), _ptr(PAR_t),
                                     pstr, _ptr(W), _ptr(F), _ptr(E), _ptr(Hm), _handle(s))
            _lib.check(rc, "mhe_resjac")
            keep_alive(s, cur, X, U_t, Y_t, PAR_t, W, F, E, Hm)
        return W, F, E, Hm

    @property
    def kkt_dim(self):
        """Rows of the system assemble() / chol_solve() exchange: dp, plus n_extra + n_eq
        border rows for a bordered (KKT) problem (mhe_kkt_dim)."""
        return self.lib.mhe_kkt_dim(self.dims)

    def assemble(self, X, U, Y, PAR=None, x0=None, stream=None, status_out=False, Z=None, Rw=None, meas_delta=None,
                 Pw=None):
        """GN normal equations at X: H (B,dp,dp), g (B,dp), cost (B) -- dense, node-major
        (row j*n + c; padding nodes last) on both paths.  The large-system path runs the
        solve's own k_big_resid + k_big_assemble over a workspace (mhe_assemble_at) and
        copies H out of their component-major tiles.  A bordered problem (n_extra / n_eq
        > 0) returns the KKT system of kkt_dim rows instead (H_xz, H_zz, the constraint
        rows; g = [g_x; g_z; C v - r]) at (X, Z).  ``Rw`` / ``meas_delta`` / ``Pw`` as for solve():
        the system a solve with them forms at X (mhe_assemble_at; with ``meas_delta`` the IRLS
        weights at X and the robust cost).  ``status_out``: also return the
        per-trajectory status (0, or 4 = constants built for other dims)."""
        self._check_ready()
        if self.fused_general:
            return self.sibling().assemble(X, U, Y, PAR, x0, stream, status_out, Z, Rw, meas_delta, Pw)
        with launch_stream(stream, self.device, (self._built,)) as (s, cur):
            staged = self._inputs(X, U, Y, PAR, x0)
            B = staged.B
            Z_t = None
            if self.n_extra:
                Z_t = _dev(np.zeros((B, self.n_extra)) if Z is None else Z, self.device, (B, self.n_extra))
            dk = self.kkt_dim
            H = torch.empty((B, dk, dk), dtype=torch.float64, device=self.device)
            g = torch.empty((B, dk), dtype=torch.float64, device=self.device)
            cost = torch.empty(B, dtype=torch.float64, device=self.device)
            status = torch.empty(B, dtype=torch.int32, device=self.device)
            # the large-system workspace is streamed in chunks like solve()'s (C5: 0.28 GB per trajectory)
            _, ws, nb, spans = self._chunks(B, s)
            pt = _Point(self, staged, Z_t, None, Rw, meas_delta, Pw)
            for lo, c in spans:
                rc = self.lib.mhe_assemble_at(self.dims, _ptr(self.cbuf), ctypes.byref(pt.args(lo, c, ws, nb)),
                                              _at(H, lo, dk * dk), _at(g, lo, dk), _at(cost, lo, 1),
                                              _at(status, lo, 1, 4), _handle(s))
                _lib.check(rc, "mhe_assemble_at")
            keep_alive(s, cur, *pt.tensors, H, g, cost, status, ws)
        if status_out:
            return H, g, cost, status
        return H, g, cost

    def _query_rows(self, t, Phi):
        """Lagrange basis rows (Tq, P) at the query times ``t``, or the rows ``Phi`` as given."""
        if (t is None) == (Phi is None):
            raise ValueError("give the query times t or the basis rows Phi (one of them)")
        if Phi is None:
            from nlp.collocation import ChebyshevPseudospectralMethod
            Phi = ChebyshevPseudospectralMethod(self.N, 0, self.T).lagrange_matrix(
                np.asarray(t, dtype=np.float64).reshape(-1))
        return np.asarray(Phi.cpu() if isinstance(Phi, torch.Tensor) else Phi, dtype=np.float64).reshape(-1, self.P)

    @property
    def general(self):
        """True for mixed rows, extra variables or equality rows: covariance() and arrival()
        then go through mhe_kkt_cov / mhe_kkt_arrival (the bordered system's inverse)."""
        return self.meas_name == "mixed" or self.n_extra > 0 or self.n_eq > 0

    def _z(self, Z, B):
        """The extra variables (B, n_extra) a general solver's covariance is formed at."""
        if not self.n_extra:
            return None
        if Z is None:
            raise ValueError("this problem has extra variables: pass Z (B, n_extra), the solve's fifth output")
        return _dev(Z, self.device, (B, self.n_extra))

    def arrival(self, X, U, Y, PAR=None, x0=None, t=None, Phi=None, Rw=None, meas_delta=None, Pw=None, stream=None,
                with_cov=False, Z=None):
        """Arrival cost of the window shifted to the query time (mhe_arrival): with the
        covariance block C = S_t H^-1 S_t^T of ``covariance()`` at X (same inputs, the window's
        own ``Pw`` included), x_arr (B, n) = x(t) by the Lagrange row in node order and
        Pw_arr (B, n, n) = inv(C), bitwise symmetric, formed on the device.  Exactly one query:
        ``t`` a scalar (or one-element array) in [0, T], or its basis row ``Phi`` (1, P).
        Returns (x_arr, Pw_arr, status) device tensors -- the next ``solve(x0=x_arr, Pw=Pw_arr)``
        needs no copy -- and C (B, n, n) as a fourth element with ``with_cov`` (bitwise
        ``covariance(..., t=[t])[0][:, 0]``).  status (B,): 0, 2 = not SPD (H or the block), 4 =
        bad constants; the outputs of such a trajectory are NaN, the others unaffected.
        Refusals as ``covariance()``.  A general solver (mixed rows, extra variables: ``Z`` the
        solve's (B, n_extra)) goes through mhe_kkt_arrival; with equality rows the block is
        rank-deficient and the call is refused (MHE_ERR_UNSUPPORTED)."""
        self._check_ready()
        if self.fused_general:
            return self.sibling().arrival(X, U, Y, PAR, x0, t, Phi, Rw, meas_delta, Pw, stream, with_cov, Z)
        Phi = self._query_rows(t, Phi)
        if Phi.shape[0] != 1:
            raise ValueError(f"arrival() takes exactly one query time, got {Phi.shape[0]}")
        with launch_stream(stream, self.device, (self._built,)) as (s, cur):
            staged = self._inputs(X, U, Y, PAR, x0)
            B, n = staged.B, self.n
            pt = _Point(self, staged, self._z(Z, B), None, Rw, meas_delta, Pw)
            phi = _dev(Phi, self.device)
            call, cname = ((self.lib.mhe_kkt_arrival, "mhe_kkt_arrival") if self.general else
                           (self.lib.mhe_arrival, "mhe_arrival"))
            f64 = dict(dtype=torch.float64, device=self.device)
            x_arr = torch.empty((B, n), **f64)
            Pw_arr = torch.empty((B, n, n), **f64)
            cov = torch.empty((B, n, n), **f64) if with_cov else None
            status = torch.empty(B, dtype=torch.int32, device=self.device)
            chunk, ws, nb, spans = self._chunks(B, s)  # streamed in chunks like covariance()
            sb = (self.lib.mhe_kkt_cov_scratch_bytes(self.dims, chunk, 1) if self.general else
                  self.lib.mhe_arrival_scratch_bytes(self.dims, chunk))
            scratch = torch.empty(sb, dtype=torch.uint8, device=self.device) if sb else None
            for lo, c in spans:
                rc = call(self.dims, _ptr(self.cbuf), ctypes.byref(pt.args(lo, c, ws, nb)), _ptr(phi),
                          _at(x_arr, lo, n), _at(Pw_arr, lo, n * n), _at(cov, lo, n * n), _at(status, lo, 1, 4),
                          _ptr(scratch), sb, _handle(s))
                _lib.check(rc, cname)
            keep_alive(s, cur, *pt.tensors, phi, x_arr, Pw_arr, cov, status, ws, scratch)
        if with_cov:
            return x_arr, Pw_arr, status, cov
        return x_arr, Pw_arr, status

    def covariance(self, X, U, Y, PAR=None, x0=None, t=None, Phi=None, Rw=None, stream=None, meas_delta=None,
                   Pw=None, Z=None, with_extra=False):
        """Posterior covariance of the state at query times (mhe_state_cov): with H = J^T W J
        at X (the solve's own assembly: Huber weights, per-solve ``Rw``, the IRLS weights of
        ``meas_delta`` at X) and S_t = phi(t)^T (x)
        I_n, cov[b, q] = S_t H^-1 S_t^T, from the solve's Cholesky factor by a forward sweep
        of the query columns.  Query times ``t`` (Tq,) in [0, T] go through the Lagrange basis
        extractSolution uses; or pass the basis rows ``Phi`` (Tq, P) directly.  Returns
        (cov (B, Tq, n, n), status (B,): 0, 2 = not SPD, 4 = bad constants; cov is NaN where
        status != 0).  The inverse of the half-Hessian: a covariance when the weights are
        inverse covariances.  Bounds are not reflected.  ``Pw``: the per-solve prior weight, as
        for solve(); ``arrival()`` returns the inverse of one query's block without a host round
        trip.  A general solver (mixed rows, extra variables, equality rows) calls mhe_kkt_cov:
        the covariance under the equality rows, the leading block of the bordered system's
        inverse at (X, ``Z``) -- positive semi-definite with equality rows; ``Z`` (B, n_extra) is
        the solve's fifth output.  ``with_extra``: return (cov, covz, status) with covz
        (B, n_extra, n_extra) the extra variables' block (NaN row and column for a variable no
        row depends on; None without extra variables).  A typed solver makes the mhe_state_cov
        call whatever these two arguments are."""
        self._check_ready()
        if self.fused_general:
            return self.sibling().covariance(X, U, Y, PAR, x0, t, Phi, Rw, stream, meas_delta, Pw, Z, with_extra)
        Phi = self._query_rows(t, Phi)
        Tq = Phi.shape[0]
        if Tq == 0:
            raise ValueError("at least one query time")
        with launch_stream(stream, self.device, (self._built,)) as (s, cur):
            staged = self._inputs(X, U, Y, PAR, x0)
            B, n, nz = staged.B, self.n, self.n_extra
            pt = _Point(self, staged, self._z(Z, B) if self.general else None, None, Rw, meas_delta, Pw)
            PhiQ = _dev(Phi, self.device)
            covz = None
            if self.general and with_extra and nz:
                covz = torch.empty((B, nz, nz), dtype=torch.float64, device=self.device)
            cov = torch.empty((B, Tq, n, n), dtype=torch.float64, device=self.device)
            status = torch.empty(B, dtype=torch.int32, device=self.device)
            # the large-system workspace and the query columns' scratch are streamed in
            # chunks like solve()'s
            chunk, ws, nb, spans = self._chunks(B, s)
            sb = (self.lib.mhe_kkt_cov_scratch_bytes if self.general else self.lib.mhe_cov_scratch_bytes)(
                self.dims, chunk, Tq)
            scratch = torch.empty(sb, dtype=torch.uint8, device=self.device) if sb else None
            for lo, c in spans:
                a = ctypes.byref(pt.args(lo, c, ws, nb))
                if self.general:
                    rc = self.lib.mhe_kkt_cov(self.dims, _ptr(self.cbuf), a, _ptr(PhiQ), Tq, _at(cov, lo, Tq * n * n),
                                              _at(covz, lo, nz * nz), _at(status, lo, 1, 4), _ptr(scratch), sb,
                                              _handle(s))
                    _lib.check(rc, "mhe_kkt_cov")
                    continue
                rc = self.lib.mhe_state_cov(self.dims, _ptr(self.cbuf), a, _ptr(PhiQ), Tq, _at(cov, lo, Tq * n * n),
                                            _at(status, lo, 1, 4), _ptr(scratch), sb, _handle(s))
                _lib.check(rc, "mhe_state_cov")
            keep_alive(s, cur, *pt.tensors, PhiQ, cov, covz, status, ws, scratch)
        if with_extra:
            return cov, covz, status
        return cov, status

    def chol_solve(self, H, g, stream=None):
        """delta = -H^{-1} g with the solver's own factorization (H: (B,dp,dp) SPD,
        node-major as ``assemble`` returns it; lower triangle read): the register-tiled
        kernel, or on the large-system path k_big_chol over a workspace (mhe_chol_solve_ws).
        A bordered problem takes the KKT system of kkt_dim rows (``assemble``'s) and
        returns delta = [dx; dz; lambda], solved as every bordered GN step (k_big_border)."""
        self._check_ready()
        if self.fused_general:
            return self.sibling().chol_solve(H, g, stream)
        with launch_stream(stream, self.device, (self._built,)) as (s, cur):
            H = _dev(H, self.device)
            g = _dev(g, self.device)
            B = H.shape[0]
            dk = self.kkt_dim
            if H.shape[1:] != (dk, dk) or g.shape != (B, dk):
                raise ValueError(f"H must be (B,{dk},{dk}) and g (B,{dk})")
            delta = torch.empty((B, dk), dtype=torch.float64, device=self.device)
            status = torch.empty(B, dtype=torch.int32, device=self.device)
            _, ws, nb, spans = self._chunks(B, s)
            for lo, c in spans:
                rc = self.lib.mhe_chol_solve_ws(self.dims, _ptr(self.cbuf), c, _at(H, lo, dk * dk), _at(g, lo, dk),
                                                _at(delta, lo, dk), _at(status, lo, 1, 4), _ptr(ws), nb, _handle(s))
                _lib.check(rc, "mhe_chol_solve_ws")
            keep_alive(s, cur, H, g, delta, status, ws)
        return delta, status


def from_workload(w, device="cuda", **kw):
    """BatchSolver for a mhe.configs.Workload (kw: dyn_cost, huber_delta, bounds)."""
    Phi = w.cpm.lagrange_matrix(w.t_meas)
    kw.setdefault("n_extra", getattr(w, "n_extra", 0))
    if getattr(w, "dyn_par", None) is not None:
        kw.setdefault("dyn_par", w.dyn_par)
    return BatchSolver(w.N, w.T, w.dyn, w.meas, w.cpm.D, (w.T / 2.0) * w.cpm.w, Phi, w.Qw, w.Rw,
                       Pw=w.Pw, meas_idx=w.meas_static.get("idx"), device=device, **kw)
