"""Batches for the stopping-rule tests (tests/test_stopping_host.py, tests/test_gpu_stopping.py)
-- TEST INFRASTRUCTURE (imports oracle/).

Every solver ends a trajectory by the rule of include/mhe.h: status 0 as soon as
max|step| <= tol (1 + max|X|), X after the update, the extra variables included.  The batches
here are built so that the rule's decisions are unambiguous: the guard below is a property of
the inputs, computed on the oracle alone, and a device that is right cannot disagree with any
decision the oracle takes.

Start points.  With X* the oracle's optimum of trajectory b's problem (its iterate at
tol = 1e-12, or after XSTAR_ITERS iterations where it does not get there), trajectory b starts
at X* + s_b (X_init - X*), the extra variables likewise; the blend factors s_b are constants
of the builders.  The trajectories of a batch share the data of trajectory 0 (a per-solve prior
weight and mean are the trajectory's own), so the spread of the iteration counts comes from s_b.

Guard (``Case.guard``).
  band    at every iteration of every trajectory up to its stop, the oracle's ratio
          r = max|step| / (tol (1 + max|X_new|)) lies outside [1/2, 2];
  floor   the oracle's rounding floor of X (tolerance.floor) has 8 floor <= 0.01 tol (1 + max|X|);
  alpha   bounded cases: every accepted step length of the oracle's trace is 1.
Two correct evaluations of one iterate agree within 8 floor + 1e-10 (1 + max|X|), about 1e-4 of
the threshold at tol = 1e-6; the band of 2 leaves three orders of magnitude.

The ratios come from ``trace``: the oracle's iteration restated step for step with the rule as an
argument.  tests/test_stopping_host.py holds it to the oracle under the exact rule (counts and
status exactly, iterates to rounding) and uses wrong rules (an entry, a component or the extra
variables left out of the maxima, max|X| taken before the update) to show that the expected
counts tell them apart.  Bounded cases take their iterates from the oracle at max_iter = k,
tol = 0: with every step length 1 the stationarity step is X_k - X_{k-1} exactly.
"""
import functools

import numpy as np

from mhe import configs
from oracle import gn
from oracle import gn_general as gg

import arrival_reference as ar
import tolerance as tl

TOL = 1e-6          # part 1
MAX_ITER = 40
TOL_ENTRY = 1e-7    # part 2
BAND = 2.0
XSTAR_ITERS = 60
HUBER_DELTA = 0.1    # see S_C2_HUBER
HUBER_MAX_ITER = 400
LB, UB = [-np.inf, 0.5], [1.5, np.inf]                  # the bounds tests/test_gpu_arrival.py runs
BOUNDS = [(1, 0.5, np.inf), (0, -np.inf, 1.5)]          # the same, as BatchSolver takes them


# ---------------------------------------------------------------- the rule, and wrong ones
def rule_exact(step, vnew, vold):
    """(max|step|, max|v|) of include/mhe.h: v = [vec(X); z] after the update."""
    return np.max(np.abs(step)), np.max(np.abs(vnew))


def rule_skipping(mask):
    """The rule with the entries of ``mask`` (flat, over [vec(X); z]) left out of both maxima."""
    keep = ~np.asarray(mask, dtype=bool)
    return lambda step, vnew, vold: (np.max(np.abs(step[keep])), np.max(np.abs(vnew[keep])))


def rule_before_update(step, vnew, vold):
    return np.max(np.abs(step)), np.max(np.abs(vold))


def _step_typed(pb, X, Z, U, Y, PAR, x0):
    """The step of oracle.gn.gauss_newton at X (1, P, n), operation for operation; None: not SPD."""
    H, g, _ = gn.normal_equations(pb, X, U, Y, PAR, x0)
    try:
        L = np.linalg.cholesky(H[0])
    except np.linalg.LinAlgError:
        return None
    return -np.linalg.solve(L.T, np.linalg.solve(L, g[0]))


def _step_general(pb, X, Z, U, Y, PAR, x0):
    """The step of oracle.gn_general.gauss_newton_general at (X, Z), over [vec(X); z]."""
    d, nz = X[0].size, pb.n_extra
    Zb = np.zeros((1, nz)) if Z is None else Z
    H, g, _ = gg.normal_equations_full(pb, X, Zb, U, Y, PAR, x0)
    C = gg.constraint_rows(pb, d, nz)
    cval = C @ np.concatenate([X[0].ravel(), Zb[0]]) - pb.eq_rhs
    try:
        np.linalg.cholesky(H[0][:d, :d])
    except np.linalg.LinAlgError:
        return None
    return gg.kkt_step(H[0], g[0], C, cval)[0]


def _one(A, b):
    """Input of trajectory b as a batch of one (None and shared inputs pass through)."""
    return None if A is None else (A if A.shape[0] == 1 else A[b:b + 1])


class Case:
    """One batch: the inputs of ``BatchSolver.solve`` (numpy) and the per-trajectory oracle.

    kind      "typed" (oracle.gn.gauss_newton), "bounded" (gauss_newton_bounded) or "general"
              (oracle.gn_general.gauss_newton_general)
    w         the mhe.configs.Workload (typed, bounded); pb: the GeneralProblem (general)
    pbkw      oracle.gn.Problem keywords (dyn_cost, delta, lb, ub)
    Pw, x0    per-trajectory prior weight (B, n, n) and mean (B, n), or None
    """

    def __init__(self, name, kind, X0, U, Y, PAR=None, x0=None, Pw=None, Z0=None, w=None, pb=None, pbkw=None,
                 tol=TOL, max_iter=MAX_ITER, min_counts=2):
        self.name, self.kind, self.w, self.pb, self.pbkw = name, kind, w, pb, dict(pbkw or {})
        self.X0, self.U, self.Y, self.PAR, self.x0, self.Pw, self.Z0 = X0, U, Y, PAR, x0, Pw, Z0
        self.tol, self.max_iter, self.min_counts = tol, max_iter, min_counts
        self.B = X0.shape[0]
        for a in (X0, U, Y, PAR, x0, Pw, Z0):
            if a is not None:
                a.setflags(write=False)

    # ------------------------------------------------------------ the oracle, per trajectory
    def problem(self, b):
        if self.kind == "general":
            return self.pb
        w = self.w
        return gn.Problem(w.N, w.T, w.n, w.m, w.dyn, w.meas, w.cpm.D, (w.T / 2) * w.cpm.w,
                          w.cpm.lagrange_matrix(w.t_meas), w.Qw, w.Rw, Pw=w.Pw if self.Pw is None else self.Pw[b],
                          meas_static=w.meas_static, **self.pbkw)

    def _oracle_one(self, b, max_iter, tol, Y, perturb, trace=None):
        """(X, Z, cost, iters, status) of trajectory b as a batch of one."""
        pb, args = self.problem(b), (_one(self.U, b), _one(Y, b), _one(self.PAR, b), _one(self.x0, b))
        if self.kind == "general":
            return gg.gauss_newton_general(pb, self.X0[b:b + 1], _one(self.Z0, b), *args, max_iter=max_iter, tol=tol,
                                           perturb=perturb)
        kw = dict(trace=trace) if self.kind == "bounded" else dict(perturb=perturb)
        X, cost, iters, status = gn.gauss_newton(pb, self.X0[b:b + 1], *args, max_iter=max_iter, tol=tol, **kw)
        return X, None, cost, iters, status

    def oracle(self, max_iter=None, tol=None, Y=None, perturb=None, trace=None):
        """The reference of the batch: (X, Z | None, cost, iters, status), stacked."""
        max_iter = self.max_iter if max_iter is None else max_iter
        tol = self.tol if tol is None else tol
        if self.kind == "typed" and self.Pw is None:  # one problem for the batch: the oracle's own batching
            wide = lambda A: None if A is None else np.broadcast_to(A, (self.B,) + A.shape[1:])  # noqa: E731
            X, cost, iters, status = gn.gauss_newton(self.problem(0), self.X0, wide(self.U), self.Y if Y is None else Y,
                                                     wide(self.PAR), self.x0, max_iter=max_iter, tol=tol,
                                                     perturb=perturb)
            return X, None, cost, iters, status
        out = []
        for b in range(self.B):
            tr = None if trace is None else []
            out.append(self._oracle_one(b, max_iter, tol, self.Y if Y is None else Y, perturb, tr))
            if trace is not None:
                trace.extend((b, it, a) for _, it, a in tr)
        return tuple(None if out[0][k] is None else np.concatenate([o[k] for o in out]) for k in range(5))

    @functools.cached_property
    def ref(self):
        """The oracle at the case's own (max_iter, tol), computed once and never modified."""
        r = self.oracle()
        for a in r:
            if a is not None:
                a.setflags(write=False)
        return r

    @functools.cached_property
    def floors(self):
        """tolerance.floor of (X, cost) and of Z where there is one: (fx, fc, fz | None)."""
        pick = (0, 2, 1) if self.Z0 is not None else (0, 2)
        f = tl.floor(lambda Y, pt: tuple(self.oracle(Y=Y, perturb=pt)[k] for k in pick), self.Y,
                     conditioning=self.kind != "bounded")
        return f[0], f[1], (f[2] if self.Z0 is not None else None)

    # ------------------------------------------------------------ the restated iteration
    def trace(self, rule=rule_exact, max_iter=None, tol=None, only=None):
        """The oracle's iteration with ``rule`` in place of its stopping test (typed and general
        cases): X, Z | None, iters, status, and per trajectory the ratios
        max|step| / (tol (1 + max|v|)) of its iterations.  ``only``: the trajectories to run (the
        others keep their start, 0 iterations and an empty list)."""
        assert self.kind != "bounded"
        max_iter = self.max_iter if max_iter is None else max_iter
        tol = self.tol if tol is None else tol
        X = np.array(self.X0)
        Z = None if self.Z0 is None else np.array(self.Z0)
        iters, status, ratios = np.zeros(self.B, np.int32), np.full(self.B, gn.MAXITER, np.int32), []
        for b in range(self.B):
            pb, args = self.problem(b), (_one(self.U, b), _one(self.Y, b), _one(self.PAR, b), _one(self.x0, b))
            rs = []
            for _ in range(max_iter if only is None or b in only else 0):
                vold = np.concatenate([X[b].ravel(), Z[b] if Z is not None else np.zeros(0)])
                step = (_step_general if self.kind == "general" else _step_typed)(pb, X[b:b + 1],
                                                                                   None if Z is None else Z[b:b + 1], *args)
                if step is None:
                    status[b] = gn.NOT_SPD
                    break
                d = X[b].size
                X[b] = X[b] + step[:d].reshape(X[b].shape)
                if Z is not None:
                    Z[b] = Z[b] + step[d:]
                iters[b] += 1
                vnew = np.concatenate([X[b].ravel(), Z[b] if Z is not None else np.zeros(0)])
                dmax, xmax = rule(step, vnew, vold)
                rs.append(dmax / (tol * (1.0 + xmax)) if tol > 0 else np.inf)
                if dmax <= tol * (1.0 + xmax):
                    status[b] = gn.OK
                    break
            ratios.append(rs)
        return X, Z, iters, status, ratios

    @functools.cached_property
    def ratios(self):
        """Per trajectory, the oracle's ratio at every iteration up to its stop."""
        if self.kind != "bounded":
            return self.trace()[4]
        # bounded: the iterates of the oracle itself, one more step at a time
        it = self.ref[3]
        lo, hi = gn.box(self.problem(0), self.X0.shape[1:])
        out = []
        for b in range(self.B):
            Xk, rs = np.clip(self.X0[b], lo, hi), []
            for k in range(1, int(it[b]) + 1):
                Xn = self._oracle_one(b, k, 0.0, self.Y, None)[0][0]
                rs.append(np.max(np.abs(Xn - Xk)) / (self.tol * (1.0 + np.max(np.abs(Xn)))))
                Xk = Xn
            out.append(rs)
        return out

    @functools.cached_property
    def alphas(self):
        trace = []
        self.oracle(trace=trace)
        return [a for _, _, a in trace]

    def guard(self):
        """Asserts the module docstring's guard and returns the smallest |log2 r| of any ratio
        (1 = on the band's edge) with the floor's share of the threshold."""
        X, Z, _, iters, status = self.ref
        assert status.tolist() == [gn.OK] * self.B, (self.name, status)
        margin = np.inf
        for b, rs in enumerate(self.ratios):
            assert len(rs) == iters[b], (self.name, b, rs, iters[b])
            for k, r in enumerate(rs):
                assert not (1.0 / BAND <= r <= BAND), f"{self.name}: trajectory {b} iteration {k + 1} ratio {r:.3f}"
                assert (r <= 1.0) == (k + 1 == iters[b]), (self.name, b, k, r)
                margin = min(margin, abs(np.log2(r)))
        fx, _, fz = self.floors
        share = 8.0 * fx / (self.tol * (1.0 + np.abs(X).max()))
        if fz is not None:
            share = max(share, 8.0 * fz / (self.tol * (1.0 + max(np.abs(X).max(), np.abs(Z).max()))))
        assert share <= 0.01, f"{self.name}: 8 floor is {share:.2e} of the threshold"
        assert len(set(iters.tolist())) >= self.min_counts, (self.name, iters)
        if self.kind == "bounded":
            assert self.alphas and all(a == 1.0 for a in self.alphas), (self.name, self.alphas)
        return margin, share


# ---------------------------------------------------------------- part 1: blended starts
def _xstar(case0):
    """The optimum of a one-trajectory case started at X_init: tol 1e-12, XSTAR_ITERS at most."""
    X, Z, _, _, _ = case0.oracle(max_iter=max(XSTAR_ITERS, case0.max_iter), tol=1e-12)
    return X[0], (None if Z is None else Z[0])


def _blend(star, init, s):
    return np.stack([star + sb * (init - star) for sb in s])


def _typed(name, w, s, pbkw=None, prior=False, kind="typed", min_counts=2, max_iter=MAX_ITER, tol=TOL):
    """Trajectory 0's data of ``w`` for every blend factor of ``s``; with ``prior`` each trajectory
    has the prior weight and mean of arrival_reference.prior_inputs, and the constants a weight
    that none of them uses (tests/test_gpu_arrival.py)."""
    B = len(s)
    Y = np.repeat(w.Y[:1], B, axis=0)
    Pw = x0 = None
    if prior:
        wB = configs.Workload(**dict(w.__dict__, B=B, X_init=np.repeat(w.X_init[:1], B, axis=0)))
        Pw, x0 = ar.prior_inputs(wB)
        w.Pw = ar.const_prior(w)
    X0 = np.empty((B,) + w.X_init.shape[1:])
    star = None
    for b in range(B):
        if star is None or prior:  # the optimum depends on the trajectory only through its prior
            one = Case(name, kind, w.X_init[:1].copy(), w.U, Y[:1].copy(), w.PAR, _one(x0, b), _one(Pw, b), w=w,
                       pbkw=pbkw, max_iter=max_iter)
            star, _ = _xstar(one)
        X0[b] = star + s[b] * (w.X_init[0] - star)
    return Case(name, kind, X0, w.U, Y, w.PAR, x0, Pw, w=w, pbkw=pbkw, min_counts=min_counts, max_iter=max_iter,
                tol=tol)


def _general(name, pb, X_init, Z_init, U, Y, PAR, x0, s, min_counts=3):
    B = len(s)
    first = lambda A: None if A is None else A[:1].copy()  # noqa: E731
    one = Case(name, "general", first(X_init), first(U), first(Y), first(PAR), first(x0), Z0=first(Z_init), pb=pb)
    xs, zs = _xstar(one)
    rep = lambda A: None if A is None else np.repeat(A[:1], B, axis=0)  # noqa: E731
    return Case(name, "general", _blend(xs, X_init[0], s), first(U), rep(Y), first(PAR), rep(x0),
                Z0=None if Z_init is None else _blend(zs, Z_init[0], s), pb=pb, min_counts=min_counts)


# blend factors: every trajectory of every case meets the guard (tests/test_stopping_host.py)
S_C2 = [2e-6, 2.3e-5, 1.6e-4, 1e-3, 6.4e-3, 4.6e-2, 0.46, 3.2e-6]     # 1, 2, 3, 4, 5, 6, 7, 1 iterations
S_C2_PW = S_C2
# IRLS converges linearly: at the scale of tests/test_gpu_robust.py (0.02) consecutive ratios are
# a factor 0.4 .. 0.75 apart, so no trajectory with two or more iterations clears the band; at
# HUBER_DELTA = 0.1 those with 1 and with 3 iterations do
S_C2_HUBER = [2e-6, 1.08e-4, 1e-6, 1e-4, 3.2e-6, 1.08e-4, 1.47e-6, 1e-4]
S_GNSS = [1e-6, 1e-3, 1.0, 3e-6, 1e-2, 0.1, 1e-4, 3.2e-5]              # 1 or 2 iterations
# projected Newton: nearer the KKT point than s ~ 0.09 the first step of the blend backtracks
# (entries that left their bound by more than the epsilon of the active set are free there),
# and beyond s ~ 0.57 a later one does; in between the counts are 6 and 7
S_C2_BOUNDED = [0.09675, 0.5721, 0.1127, 0.1312, 0.5721, 0.1528, 0.1779, 0.1452]
S_TWO_RX = [1e-5, 1e-3, 1.0, 1e-2, 4.6e-5, 0.46]                        # 1, 2, 3, 2, 1, 3
S_MULTI_RX = [1e-5, 1.5e-3, 0.1, 1.0, 1e-4, 4.6e-2]                     # 1, 2, 3, 4, 1, 3
# the large path's B = 20: trajectories of the eight above, so that the first stream's 16 and the
# second stream's 4 (launch_big_factor splits at batch >= 16) both hold early and late stoppers
LARGE_ORDER = [0, 5, 1, 4, 2, 3, 6, 7, 5, 0, 4, 1, 3, 2, 7, 6, 5, 0, 4, 1]


@functools.lru_cache(maxsize=None)
def blended(name):
    """The part-1 case ``name`` (built once per process)."""
    if name == "c2":
        return _typed(name, configs.make_c2(B=1, N=20), S_C2, min_counts=4)
    if name == "c2_large20":
        return _typed(name, configs.make_c2(B=1, N=20), [S_C2[i] for i in LARGE_ORDER], min_counts=4)
    if name == "c2_pw":
        return _typed(name, configs.make_c2(B=1, N=20), S_C2_PW, prior=True, min_counts=4)
    if name == "c2_huber":
        return _typed(name, configs.make_c2(B=1, N=20), S_C2_HUBER, pbkw=dict(dyn_cost="huber", delta=HUBER_DELTA),
                      max_iter=HUBER_MAX_ITER, min_counts=2)
    if name == "gnss_small":
        return _typed(name, configs.make_gnss_small(B=1), S_GNSS, min_counts=2)
    if name == "c2_bounded":
        return _typed(name, configs.make_c2(B=1, N=20), S_C2_BOUNDED, pbkw=dict(lb=LB, ub=UB), kind="bounded",
                      min_counts=2)
    if name == "two_receiver":
        from general_problems import two_receiver_problem
        pb, X0, U, Y, PAR, x0, _ = two_receiver_problem(N=6, B=1)
        return _general(name, pb, X0, None, U, Y, PAR, x0, S_TWO_RX)
    if name == "multi_receiver":
        from general_problems import multi_receiver_problem
        pb, X0, Z0, U, Y, PAR, _, _ = multi_receiver_problem(B=1)
        return _general(name, pb, X0, Z0, U, Y, PAR, None, S_MULTI_RX)
    raise KeyError(name)


BLENDED = ["c2", "c2_large20", "c2_pw", "c2_huber", "gnss_small", "c2_bounded", "two_receiver", "multi_receiver"]


# ---------------------------------------------------------------- part 2: one displaced entry
ENTRY_SHAPES = {
    # name: (dynamics, P, M) of tests/test_gpu_pairs.make_linear
    "di_P17_M16": ("double_integrator", 17, 16),            # d = 68, padding rows
    "gpb_P41_M33": ("gnss_pos_and_bias", 41, 33),           # d = 205, n = 5
    "si2d_P104_M101": ("single_integrator_2D", 104, 101),   # d = 208, no padding
    "di_P70_M40": ("double_integrator", 70, 40),            # d = 280: the large path by its size
}


def entries_of(P, n):
    """Flat (node-major) entries a reduction can lose: every component of the first and the last
    node, both sides of every wavefront edge below d, the first wrap of a 256-thread loop."""
    d = P * n
    e = set(range(n)) | set(range(d - n, d))
    e |= {i for i in (63, 64, 127, 128, 191, 192, 255, 256) if i < d}
    return sorted(e)


def _linear_workload(name):
    from test_gpu_pairs import make_linear
    return make_linear(*ENTRY_SHAPES[name])


@functools.lru_cache(maxsize=None)
def displaced(name):
    """(case, entries): for each entry e a trajectory started at X* + s e_e (s = 10 tol (1 + max|X*|):
    stops after 2) and one at X* + (s / 40) e_e (stops after 1), then one at X* itself (1).  On a
    linear pair one step from anywhere lands on the optimum, so the step is -s e_e and nothing else."""
    w = _linear_workload(name)
    w.X_init = w.X_init[:1]
    one = Case(name, "typed", w.X_init.copy(), w.U, w.Y[:1].copy(), w.PAR, w=w, tol=TOL_ENTRY)
    star, _ = _xstar(one)
    ent = entries_of(w.P, w.n)
    s = 10.0 * TOL_ENTRY * (1.0 + np.abs(star).max())
    X0 = np.repeat(star[None], 2 * len(ent) + 1, axis=0)
    for k, e in enumerate(ent):
        X0[2 * k].reshape(-1)[e] += s
        X0[2 * k + 1].reshape(-1)[e] += s / 40.0
    return Case(name, "typed", X0, w.U, np.repeat(w.Y[:1], X0.shape[0], axis=0), w.PAR, w=w, tol=TOL_ENTRY), ent


def displaced_counts(ent):
    return [2, 1] * len(ent) + [1]


SCALE_C = 1e3
SCALE_TOL_AFTER = 4.0


@functools.lru_cache(maxsize=None)
def scale_case():
    """double_integrator (d = 68) with SCALE_C added to every measurement of position 0: the
    dynamics do not read the position, so X* moves by SCALE_C in that component alone and
    max|X| lives there.  Trajectory k is displaced at a velocity entry (component 2 or 3 of the
    first, a middle and the last node) by s with ratio 1/4 under the true max|X| -- and above 2
    were component 0 left out of the maximum.  Every trajectory stops after 1 iteration."""
    w = _linear_workload("di_P17_M16")
    w.X_init = w.X_init[:1]
    Y = w.Y[:1].copy()
    Y[:, :, 0] += SCALE_C
    w.Y = Y
    w.X_init = configs._init_from_measurements(w.cpm, w.t_meas, Y)
    one = Case("scale", "typed", w.X_init.copy(), w.U, Y.copy(), w.PAR, w=w, tol=TOL_ENTRY)
    star, _ = _xstar(one)
    s = 0.25 * TOL_ENTRY * (1.0 + np.abs(star).max())
    ent = [(0, 2), (0, 3), (w.P // 2, 2), (w.P - 1, 2), (w.P - 1, 3)]
    X0 = np.repeat(star[None], len(ent), axis=0)
    for k, (j, c) in enumerate(ent):
        X0[k, j, c] += s
    return Case("scale", "typed", X0, w.U, np.repeat(Y, len(ent), axis=0), w.PAR, w=w, tol=TOL_ENTRY,
                min_counts=1), star


@functools.lru_cache(maxsize=None)
def scale_after_update_case():
    """The same problem from X* with position 0 moved back by SCALE_C at every node, solved at
    tol = SCALE_TOL_AFTER: the step is SCALE_C in that component, max|X| is ~SCALE_C after the
    update (ratio 1/4: stop after 1) and a few units before it (ratio > 2: a rule that takes
    max|X| before the update goes on).  At tol << 1 the two maxima differ by less than the
    band, whatever the start: only a tolerance of order 1 separates them."""
    base, star = scale_case()
    X0 = star[None].copy()
    X0[:, :, 0] -= SCALE_C
    return Case("scale_after", "typed", X0, base.U, base.Y[:1].copy(), base.PAR, w=base.w, tol=SCALE_TOL_AFTER,
                min_counts=1)


@functools.lru_cache(maxsize=None)
def extra_variable_case():
    """multi_receiver from (X*, Z* + s e_i) for each extra variable i that a row depends on
    (z[2] enters none), s = 10 tol (1 + max|(X*, Z*)|): the first ratio is about 10 and the X part
    of that step far below the threshold, so a rule that ignores Z stops after 1 iteration."""
    from general_problems import multi_receiver_problem
    pb, X0, Z0, U, Y, PAR, _, _ = multi_receiver_problem(B=1)
    one = Case("extra", "general", X0.copy(), None, Y.copy(), PAR.copy(), Z0=Z0.copy(), pb=pb)
    xs, zs = _xstar(one)
    s = 10.0 * TOL * (1.0 + max(np.abs(xs).max(), np.abs(zs).max()))
    Zs = np.repeat(zs[None], 2, axis=0)
    Zs[0, 0] += s
    Zs[1, 1] += s
    return Case("extra", "general", np.repeat(xs[None], 2, axis=0), None, np.repeat(Y, 2, axis=0), PAR.copy(),
                Z0=Zs, pb=pb, min_counts=1)


@functools.lru_cache(maxsize=None)
def at_optimum():
    """c2 started at X* with max_iter = 1: the rule is evaluated on the last permitted iteration
    too, so the status is 0 (converged), not 1."""
    return _typed("c2_at_optimum", configs.make_c2(B=1, N=20), [0.0, 0.0], max_iter=1, min_counts=1)
