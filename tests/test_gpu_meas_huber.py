"""Pseudo-Huber measurement rows (mhe_solve_args.meas_delta, ABI v9) on the GPU vs the
reference tests/meas_huber_reference.py (IRLS on the oracle's normal equations).

Inputs: configs.make_gnss_small (pseudorange rows, |y| ~ 2.2e7 m) at B = 4 in two shapes --
N = 10 (d = 55, M = 408: a partial last row pass of meas_phase) and N = 6 with 9 epochs x 6
satellites (M = 54) -- with 8 % of the rows shifted by +400 m (rng seed 7) and delta = 15 m.

Tolerances come from tests/tolerance.py, measured on the reference: floor = the change of
the reference's own result when every y moves by eps |y| and (iterates) when H and g move
by eps of every entry.  The IRLS weight lambda = R / sqrt(1 + e^2 / delta^2) inherits the
rounding of e = y - h (eps |y| ~ 5e-9 m moves lambda by up to ~2e-10 relative at |e| ~ delta),
so H is compared against its measured floor too, not against 1e-12 alone:
  H       <= 8 floor_H + 1e-12 max|H|  (register path, as tests/test_gpu_parity.py), and
             diagonal-scaled <= 8 floor + 1e-12 (large path, as tests/test_gpu_big_parity.py)
  g       <= 8 floor_g + 1e-12 max|g|  (register) / entrywise 8 big_oracle.g_rounding_floor
             of the reweighted problem + 1e-12 max|g| (large)
  cost    <= 8 floor_c + 1e-12 max|cost| (assembly), 1e-10 max|cost| (iterates)
  X       <= tolerance.bound(floor_X, X)  after the same number of iterations; with the
             stopping rule (tol 1e-10, iteration counts within 1) rel = 1e-8 as
             tests/test_gpu_parity.py::test_gn_converges_to_oracle_optimum
  status exact; iteration counts exact at tol 0.
Every check prints the observed figure beside its bound.
"""
import numpy as np
import pytest

torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu

from mhe import configs, solver  # noqa: E402
from oracle import gn  # noqa: E402
from oracle import gn_general as gg  # noqa: E402

import cov_reference as cr  # noqa: E402
import meas_huber_reference as mh  # noqa: E402
import tolerance as tl  # noqa: E402
from big_oracle import g_rounding_floor  # noqa: E402

SHAPES = {"n10": dict(B=4, N=10), "n6": dict(B=4, N=6, epochs=9, n_sat=6)}
PATHS = [False, True]  # force_large


def _np(ts):
    return [t.cpu().numpy() for t in ts]


class Case:
    """One shape: the workload with outliers, the oracle problem, and the reference results
    (computed once per module, with their floors)."""

    def __init__(self, name):
        w = configs.make_gnss_small(**SHAPES[name])
        self.w, self.name = w, name
        self.pb = gn.Problem(w.N, w.T, w.n, w.m, w.dyn, w.meas, w.cpm.D, (w.T / 2) * w.cpm.w,
                             w.cpm.lagrange_matrix(w.t_meas), w.Qw, w.Rw, Pw=w.Pw, meas_static=w.meas_static)
        self.U = np.broadcast_to(w.U, (w.B,) + w.U.shape[1:])
        self.PAR = np.broadcast_to(w.PAR, (w.B,) + w.PAR.shape[1:])
        self.Y, self.out = mh.with_outliers(w.Y)
        self.delta = np.full(w.M, mh.DELTA)
        self._ref, self._solvers = {}, {}

    def solver(self, force_large=False, **kw):
        key = (force_large, repr(sorted(kw.items())))
        if key not in self._solvers:
            s = solver.from_workload(self.w, force_large=force_large, **kw)
            assert s.large_system == force_large
            self._solvers[key] = s
        return self._solvers[key]

    def run(self, Y, max_iter, tol, perturb=None):
        return mh.gauss_newton(self.pb, self.w.X_init, self.U, Y, self.PAR, self.delta, max_iter=max_iter, tol=tol,
                               perturb=perturb)

    def ref(self, max_iter, tol):
        """(X, cost, iters, status, floor_X, floor_cost) of the reference IRLS."""
        key = (max_iter, tol)
        if key not in self._ref:
            X, c, it, st = self.run(self.Y, max_iter, tol)
            fx, fc = tl.floor(lambda Y, pt: self.run(Y, max_iter, tol, pt)[:2], self.Y)
            for a in (X, c, it, st):
                a.setflags(write=False)
            self._ref[key] = (X, c, it, st, fx, fc)
        return self._ref[key]

    def solve(self, s, max_iter, tol, **kw):
        w = self.w
        kw.setdefault("meas_delta", self.delta)
        return _np(s.solve(w.X_init, w.U, self.Y, w.PAR, max_iter=max_iter, tol=tol, **kw))


_cases = {}


def case(name):
    if name not in _cases:
        _cases[name] = Case(name)
    return _cases[name]


def _check_solve(label, c, got, max_iter, tol):
    X, cost, iters, status = got
    Xr, cr_, ir, sr, fx, fc = c.ref(max_iter, tol)
    assert status.tolist() == sr.tolist(), (status, sr)
    if tol == 0.0:
        assert iters.tolist() == ir.tolist() == [max_iter] * c.w.B
    else:
        assert sr.tolist() == [gn.OK] * c.w.B and np.all(np.abs(iters - ir) <= 1), (iters, ir)
    tl.check(f"{label} X", np.abs(X - Xr).max(), tl.bound(fx, Xr, rel=tl.REL if tol == 0.0 else 1e-8), " m")
    tl.check(f"{label} cost", np.abs(cost - cr_).max(), tl.FLOOR_MULT * fc + 1e-10 * np.abs(cr_).max())


# ---------------------------------------------------------------- 1. assembly parity at X_init
@pytest.mark.parametrize("force_large", PATHS)
@pytest.mark.parametrize("name", sorted(SHAPES))
def test_assembly_matches_reference(name, force_large):
    c = case(name)
    w, s = c.w, c.solver(force_large)
    H, g, cost, status = _np(s.assemble(w.X_init, w.U, c.Y, w.PAR, meas_delta=c.delta, status_out=True))
    assert status.tolist() == [0] * w.B
    run = lambda Y: mh.normal_equations(c.pb, w.X_init, c.U, Y, c.PAR, c.delta)  # noqa: E731
    Hr, gr, cr_ = run(c.Y)
    d = c.pb.d
    dg = np.sqrt(np.abs(np.einsum("bii->bi", Hr)))
    scale = dg[:, :, None] * dg[:, None, :]
    fH, fg, fc, fHs = tl.floor(lambda Y, pt: (lambda r: r + (r[0] / scale,))(run(Y)), c.Y, conditioning=False)
    label = f"{name} {'large' if force_large else 'register'}"
    if force_large:
        tl.check(f"{label} H (diagonal-scaled)", (np.abs(H[:, :d, :d] - Hr) / scale).max(), tl.FLOOR_MULT * fHs + 1e-12)
        gb = (tl.FLOOR_MULT * g_rounding_floor(mh.reweighted(c.pb, w.X_init, c.U, c.Y, c.PAR, c.delta), w.X_init, c.Y,
                                               c.PAR, c.U) + 1e-12 * np.abs(gr).max())
        tl.check(f"{label} g (entrywise / bound)", (np.abs(g[:, :d] - gr) / gb).max(), 1.0)
        assert np.array_equal(H, np.swapaxes(H, 1, 2))  # both triangles from the same tile element
    else:
        tl.check(f"{label} H", np.abs(H[:, :d, :d] - Hr).max(), tl.FLOOR_MULT * fH + 1e-12 * np.abs(Hr).max())
        tl.check(f"{label} g", np.abs(g[:, :d] - gr).max(), tl.FLOOR_MULT * fg + 1e-12 * np.abs(gr).max())
    tl.check(f"{label} cost", np.abs(cost - cr_).max(), tl.FLOOR_MULT * fc + 1e-12 * np.abs(cr_).max())
    # the robust system is not the quadratic one: far outside either bound
    Hq, gq, cq = _np(s.assemble(w.X_init, w.U, c.Y, w.PAR))
    assert np.abs(gq[:, :d] - gr).max() > 1e3 * (tl.FLOOR_MULT * fg + 1e-12 * np.abs(gr).max())
    assert np.all(cq > cost)


# ---------------------------------------------------------------- 2. iterates and convergence
@pytest.mark.parametrize("max_iter,tol", [(5, 0.0), (40, 1e-10)])
@pytest.mark.parametrize("force_large", PATHS)
@pytest.mark.parametrize("name", sorted(SHAPES))
def test_iterates_match_reference(name, force_large, max_iter, tol):
    c = case(name)
    if tol > 0.0:  # precondition: the reference itself converges every trajectory
        _, _, ir, sr, _, _ = c.ref(max_iter, tol)
        assert sr.tolist() == [gn.OK] * c.w.B and ir.max() < max_iter, (ir, sr)
    got = c.solve(c.solver(force_large), max_iter, tol)
    _check_solve(f"{name} {'large' if force_large else 'register'} ({max_iter}, {tol:g})", c, got, max_iter, tol)


# ---------------------------------------------------------------- 3. outlier rejection
@pytest.mark.parametrize("force_large", PATHS)
def test_outliers_are_rejected(force_large):
    c = case("n10")
    w = c.w
    Xr = c.ref(40, 1e-10)[0]
    Xq, _, _, sq = gn.gauss_newton(c.pb, w.X_init, c.U, c.Y, c.PAR, max_iter=40, tol=1e-10)
    er, eq = mh.position_error(w, Xr), mh.position_error(w, Xq)
    print(f"reference position error [m]: robust {er}, quadratic {eq}")
    assert sq.tolist() == [gn.OK] * w.B and np.all(er <= eq / 3.0)  # precondition, on the reference alone
    got = c.solve(c.solver(force_large), 40, 1e-10)
    _check_solve(f"outliers {'large' if force_large else 'register'}", c, got, 40, 1e-10)
    eg = mh.position_error(w, got[0])
    print(f"device position error [m]: {eg}")
    assert np.all(eg <= eq / 3.0 + tl.bound(c.ref(40, 1e-10)[4], Xr, rel=1e-8))


# ---------------------------------------------------------------- 4. identities
def _outputs(c, s, **kw):
    """Solve, assembly and covariance outputs of one argument set."""
    w = c.w
    out = c.solve(s, 5, 0.0, **kw)
    X = out[0]
    out += _np(s.assemble(w.X_init, w.U, c.Y, w.PAR, **kw))
    out += _np(s.covariance(X, w.U, c.Y, w.PAR, t=np.array([0.0, 0.4 * w.T]), **kw))
    return out


@pytest.mark.parametrize("force_large", PATHS)
def test_infinite_delta_is_bitwise_the_quadratic_call(force_large):
    c = case("n10")
    s = c.solver(force_large)
    a = _outputs(c, s, meas_delta=None)
    b = _outputs(c, s, meas_delta=np.full(c.w.M, np.inf))
    for x, y in zip(a, b):
        assert np.array_equal(x, y)
    # per row: +inf on the outlier-free rows only changes nothing on them (same result as
    # a large finite scale there, far from the all-quadratic one)
    mixed = np.where(c.out[0, :, 0], mh.DELTA, np.inf)
    m = c.solve(s, 5, 0.0, meas_delta=mixed)
    assert np.all(np.isfinite(m[0])) and not np.array_equal(m[0], a[0])


@pytest.mark.parametrize("force_large", PATHS)
def test_shared_and_per_trajectory_delta_agree_bitwise(force_large):
    c = case("n10")
    s = c.solver(force_large)
    a = _outputs(c, s, meas_delta=c.delta)
    b = _outputs(c, s, meas_delta=np.broadcast_to(c.delta, (c.w.B, c.w.M)).copy())
    for x, y in zip(a, b):
        assert np.array_equal(x, y)
    # the pre-staged form (bench-style callers) takes the same keyword
    w = c.w
    staged = s.prepare(w.X_init, w.U, c.Y, w.PAR)
    outs = (torch.empty_like(staged[0]), torch.empty(w.B, dtype=torch.float64, device=s.device),
            torch.empty(w.B, dtype=torch.int32, device=s.device), torch.empty(w.B, dtype=torch.int32, device=s.device))
    s.solve_staged(staged, outs, 5, 0.0, meas_delta=torch.as_tensor(c.delta, device=s.device))
    for x, y in zip(a[:4], _np(outs)):
        assert np.array_equal(x, y)


@pytest.mark.parametrize("force_large", PATHS)
def test_zero_weight_masks_a_robust_row(force_large):
    """R = 0 with a finite delta: the row stays masked -- finite outputs whatever y holds
    there, equal to the problem without those rows."""
    c = case("n6")
    w = c.w
    drop = np.zeros(w.M, dtype=bool)
    drop[[1, 7, 20, 21, 40, 53]] = True
    Rw = w.Rw.copy()
    Rw[drop] = 0.0
    Y = c.Y.copy()
    Y[:, drop] = 1e300  # e^2 would overflow if the row were evaluated
    s = c.solver(force_large)
    Xm, cm, im, sm = _np(s.solve(w.X_init, w.U, Y, w.PAR, max_iter=5, tol=0.0, Rw=Rw, meas_delta=c.delta))
    assert np.all(np.isfinite(Xm)) and np.all(np.isfinite(cm)) and sm.tolist() == [1] * w.B
    keep = ~drop
    pbk = gn.Problem(w.N, w.T, w.n, w.m, w.dyn, w.meas, w.cpm.D, (w.T / 2) * w.cpm.w,
                     w.cpm.lagrange_matrix(w.t_meas[keep]), w.Qw, w.Rw[keep], meas_static=w.meas_static)
    run = lambda Yk, pt=None: mh.gauss_newton(pbk, w.X_init, c.U, Yk, c.PAR[:, keep], c.delta[keep],  # noqa: E731
                                              max_iter=5, tol=0.0, perturb=pt)[:2]
    Xr, cr_ = run(c.Y[:, keep])
    fx, fc = tl.floor(run, c.Y[:, keep])
    tl.check("masked rows X", np.abs(Xm - Xr).max(), tl.bound(fx, Xr), " m")
    tl.check("masked rows cost", np.abs(cm - cr_).max(), tl.FLOOR_MULT * fc + 1e-10 * np.abs(cr_).max())
    # and the same rows dropped on the device
    sk = solver.BatchSolver(w.N, w.T, w.dyn, w.meas, w.cpm.D, (w.T / 2.0) * w.cpm.w, w.cpm.lagrange_matrix(w.t_meas[keep]),
                            w.Qw, w.Rw[keep], meas_idx=w.meas_static["idx"], force_large=force_large)
    Xk, ck, _, _ = _np(sk.solve(w.X_init, w.U, c.Y[:, keep], w.PAR[:, keep], max_iter=5, tol=0.0, meas_delta=c.delta[keep]))
    tl.check("masked vs dropped rows X", np.abs(Xm - Xk).max(), tl.bound(fx, Xr), " m")


def test_chunked_large_path_is_bitwise_the_unchunked():
    """ws_budget of two trajectories' workspace: B = 4 runs as 2 chunks, and meas_delta
    (different per trajectory) must be offset per chunk like Rw."""
    c = case("n10")
    w = c.w
    delta = c.delta[None, :] * (1.0 + 0.25 * np.arange(w.B))[:, None]
    Rw = np.broadcast_to(w.Rw, (w.B,) + w.Rw.shape) * (1.0 + 0.1 * np.arange(w.B))[:, None, None, None]
    s = c.solver(True)
    kw = dict(meas_delta=delta, Rw=Rw)
    a = _outputs(c, s, **kw)
    s2 = solver.from_workload(w, force_large=True)
    s2.ws_budget = 2 * s2.lib.mhe_workspace_bytes(s2.dims, 1)
    assert s2._chunk(w.B) == 2
    b = _outputs(c, s2, **kw)
    for x, y in zip(a, b):
        assert np.array_equal(x, y)
    # the scales do differ by trajectory: trajectory 3 alone with its own row gives its result
    one = _np(s.solve(w.X_init[3:], w.U, c.Y[3:], w.PAR, max_iter=5, tol=0.0, meas_delta=delta[3:], Rw=Rw[3:]))
    assert np.array_equal(one[0][0], a[0][3])


# ---------------------------------------------------------------- 5. the two paths agree
@pytest.mark.parametrize("name", sorted(SHAPES))
def test_register_and_large_paths_agree(name):
    c = case(name)
    a = c.solve(c.solver(False), 6, 0.0)
    b = c.solve(c.solver(True), 6, 0.0)
    err = np.abs(a[0] - b[0]).max()
    print(f"{name}: register vs large after 6 iterations: max |dX| {err:.3e}")
    assert err <= 1e-10 * (1 + np.abs(a[0]).max())
    assert np.allclose(a[1], b[1], rtol=1e-10)


# ---------------------------------------------------------------- 6. mixed rows
@pytest.mark.parametrize("name,max_iter,tol", [("n10", 5, 0.0), ("n6", 5, 0.0), ("n6", 40, 1e-10)])
def test_mixed_pseudorange_rows_match_reference(name, max_iter, tol):
    """The same problem written as MHE_ROW_PSEUDORANGE rows (large path), against the
    mixed-row form of the reference (oracle.gn_general)."""
    c = case(name)
    w = c.w
    PAR = np.array([[configs.pr_row([0, 1, 2, 3], sat) for sat in w.PAR[0]]])
    Rw = w.Rw[:, 0, 0]
    Phi = w.cpm.lagrange_matrix(w.t_meas)
    pb = gg.GeneralProblem(w.N, w.T, w.n, w.m, w.dyn, "mixed", w.cpm.D, (w.T / 2) * w.cpm.w, Phi, w.Qw, Rw)
    s = solver.BatchSolver(w.N, w.T, w.dyn, "mixed", w.cpm.D, (w.T / 2.0) * w.cpm.w, Phi, w.Qw, Rw)
    assert s.large_system
    X, cost, iters, status = _np(s.solve(w.X_init, w.U, c.Y, PAR, max_iter=max_iter, tol=tol, meas_delta=c.delta))
    run = lambda Y, pt=None: mh.general_gauss_newton(pb, w.X_init, c.U, Y, PAR, c.delta, max_iter=max_iter,  # noqa: E731
                                                     tol=tol, perturb=pt)
    Xr, cr_, ir, sr = run(c.Y)
    fx, fc = tl.floor(lambda Y, pt: run(Y, pt)[:2], c.Y)
    assert status.tolist() == sr.tolist()
    assert np.all(np.abs(iters - ir) <= (0 if tol == 0.0 else 1))
    tl.check(f"mixed {name} X", np.abs(X - Xr).max(), tl.bound(fx, Xr, rel=tl.REL if tol == 0.0 else 1e-8), " m")
    tl.check(f"mixed {name} cost", np.abs(cost - cr_).max(), tl.FLOOR_MULT * fc + 1e-10 * np.abs(cr_).max())
    # the two reference forms agree with each other (typed rows vs mixed rows)
    Xt = c.ref(max_iter, tol)[0]
    assert np.abs(Xr - Xt).max() <= tl.bound(fx, Xr, rel=tl.REL if tol == 0.0 else 1e-8)


# ---------------------------------------------------------------- 7. bounded
# Lower bound on x[4], the clock drift (the free robust solution has drifts 0.53, 0.42, -0.003
# and 0.13 m/s: the bound binds on trajectories 2 and 3).  The projected Newton method decides
# active / free by the sign of g at the entries on their bound; with the bound at 0.2 the
# REFERENCE's own decision at iteration 3 sits at 0.02 of g's rounding level (rounding decides:
# two correct evaluations then differ by 1e-5 m at a fixed iteration count and meet again at
# the KKT point), at 0.3 every decision of the first 6 iterations is 8e10 rounding levels
# clear.  The test asserts that margin on the reference (a precondition, like test 3's).
DRIFT_LB = 0.3


def _kkt_residual(c, X, lo, hi):
    """max |X - P(X - 2 g)| per trajectory, g the reference's IRLS half-gradient at X."""
    _, g, _ = mh.normal_equations(c.pb, X, c.U, c.Y, c.PAR, c.delta)
    grad = 2.0 * g.reshape(X.shape)
    return np.abs(X - np.clip(X - grad, lo, hi)).reshape(X.shape[0], -1).max(axis=1)


def test_bounded_robust_solve_reaches_a_kkt_point():
    c = case("n10")
    w = c.w
    bounds = [(4, DRIFT_LB, np.inf)]
    lo = np.broadcast_to(np.array([-np.inf] * 4 + [DRIFT_LB]), w.X_init.shape)
    hi = np.full(w.X_init.shape, np.inf)
    pbb = gn.Problem(w.N, w.T, w.n, w.m, w.dyn, w.meas, w.cpm.D, (w.T / 2) * w.cpm.w, w.cpm.lagrange_matrix(w.t_meas),
                     w.Qw, w.Rw, meas_static=w.meas_static, lb=[-np.inf] * 4 + [DRIFT_LB])
    m_g, m_x = mh.active_set_margins(pbb, w.X_init, c.U, c.Y, c.PAR, c.delta,
                                     lambda q, X: g_rounding_floor(q, X, c.Y, c.PAR, c.U), 6)
    print(f"reference active-set margins over 6 iterations: |g| / floor >= {m_g:.3g}, distance from the eps band >= {m_x:.3g} m")
    assert m_g >= 1e3 and m_x >= 1e-7  # precondition: no decision of the reference is made by rounding
    sr_, sb = c.solver(False, bounds=bounds), c.solver(True, bounds=bounds)
    a, b = c.solve(sr_, 6, 0.0), c.solve(sb, 6, 0.0)
    err = np.abs(a[0] - b[0]).max()
    print(f"bounded: register vs large after 6 iterations: max |dX| {err:.3e}")
    assert a[2].tolist() == b[2].tolist() == [6] * w.B
    assert err <= 1e-10 * (1 + np.abs(a[0]).max()) and np.allclose(a[1], b[1], rtol=1e-10)
    r0 = _kkt_residual(c, np.clip(w.X_init, lo, hi), lo, hi)
    for label, s in (("register", sr_), ("large", sb)):
        X, cost, iters, status = c.solve(s, 60, 1e-10)
        assert status.tolist() == [gn.OK] * w.B, (status, iters)
        assert (X[:, :, 4] >= DRIFT_LB).all() and (X[:, :, 4] == DRIFT_LB).any(), "the bound should be active"
        r = _kkt_residual(c, X, lo, hi)
        print(f"bounded {label}: iters {iters}, projected-gradient residual {r} (start {r0})")
        assert np.all(r <= 1e-9 * r0)
        assert np.allclose(cost, mh.cost(c.pb, X, c.U, c.Y, c.PAR, c.delta), rtol=1e-10)


# ---------------------------------------------------------------- 8. covariance
@pytest.mark.parametrize("force_large", PATHS)
def test_covariance_uses_the_irls_weights(force_large):
    c = case("n10")
    w = c.w
    X = c.ref(40, 1e-10)[0]
    t = cr.query_times(w.cpm, w.T)
    C, bound = cr.cov_reference(mh.reweighted(c.pb, X, c.U, c.Y, c.PAR, c.delta), w.cpm, t, X, c.U, c.Y, c.PAR)
    s = c.solver(force_large)
    cov, status = _np(s.covariance(X, w.U, c.Y, w.PAR, t=t, meas_delta=c.delta))
    assert status.tolist() == [0] * w.B
    cr.check_blocks(f"cov robust {'large' if force_large else 'register'}", cov, C, bound)
    Cq, _ = _np(s.covariance(X, w.U, c.Y, w.PAR, t=t))
    assert np.abs(Cq - C).max() > 100 * bound  # not the quadratic problem's


# ---------------------------------------------------------------- 9. facade
def test_facade_pseudo_huber_rows():
    """addResidualCost(pseudorange, ..., cost_function=pseudo_huber_loss) per satellite, as
    gnss_stationary.py:121-128 adds its rows."""
    import nlp.cost_functions as cost_functions
    import nlp.dynamics as dynamics
    import nlp.measurements as measurements
    import nlp.nlp as nlp
    c = case("n6")
    w = c.w
    problem = nlp.fixedTimeOptimalEstimationNLP(w.N, w.T, 5, 3)
    X = problem.addVariables(w.N + 1, 5, name="x")
    for k, x in enumerate(X):
        problem.initialGuess(x, w.X_init[0, k])
    _, W = problem.addDynamics(dynamics.gnss_pos_and_bias, X, np.array([0.0, w.T]), np.zeros((3, 2)))
    problem.addDynamicsCost(cost_functions.weighted_l2_norm, W, {"Q": w.Qw})
    for i, t in enumerate(w.t_meas):
        problem.addResidualCost(measurements.pseudorange, X, np.array([[t]]), np.array([[c.Y[0, i, 0]]]),
                                np.array([[w.Rw[i, 0, 0]]]), {"sat_pos": w.PAR[0, i]},
                                cost_function=cost_functions.pseudo_huber_loss, cost_params={"delta": mh.DELTA})
    problem.max_iter, problem.tol = 40, 1e-10
    problem.build()
    problem.solve()
    one = slice(0, 1)
    run = lambda Y, pt=None: mh.gauss_newton(c.pb, w.X_init[one], c.U[one], Y, c.PAR[one], c.delta, max_iter=40,  # noqa: E731
                                             tol=1e-10, perturb=pt)
    Xr, cr_, ir, sr = run(c.Y[one])
    fx, fc = tl.floor(lambda Y, pt: run(Y, pt)[:2], c.Y[one])
    Xs = np.stack([problem.extractVariableValue("x", k) for k in range(w.N + 1)])
    assert sr[0] == gn.OK and problem.solver["success"] and abs(problem.solver["iter_count"] - ir[0]) <= 1
    tl.check("facade X", np.abs(Xs - Xr[0]).max(), tl.bound(fx, Xr, rel=1e-8), " m")
    tl.check("facade objective", abs(problem.solver["objective"] - cr_[0]), tl.FLOOR_MULT * fc + 1e-10 * abs(cr_[0]))
    t = np.array([0.0, 0.37 * w.T, w.T])
    C, bound = cr.cov_reference(mh.reweighted(c.pb, Xs[None], c.U[one], c.Y[one], c.PAR[one], c.delta), w.cpm, t,
                                Xs[None], c.U[one], c.Y[one], c.PAR[one])
    cov = problem.extractCovariance("x", t)
    tl.check("facade covariance", np.abs(cov - C[0]).max(), bound)
