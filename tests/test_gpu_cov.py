"""Posterior covariance of the state estimate at query times (mhe_state_cov,
BatchSolver.covariance, NLP.extractCovariance) vs the CPU oracle.

Reference and tolerance: tests/cov_reference.py -- C_ref = S inv(H) S^T with H from
oracle.gn.normal_equations at the point and S = phi(t) (x) I from the collocation's
lagrange_matrix;  bound = FLOOR_MULT * floor_H + 1e-12 max|C_ref|, floor_H the change of
C_ref when every entry of H moves by eps of its magnitude.  Every comparison prints the
observed error beside its bound.  Query times: 0, 0.37 T, T (the endpoint nodes, where phi
is a unit row) and one interior node time.

One deviation from a literal two-path comparison at the C3 shape: make_c3(N=40) has 2412
measurement rows, whose per-row blocks do not fit the register-resident kernel's LDS, so
that shape takes the large-system path with or without force_large.  It is compared
against the oracle there; the register path and the large path are compared with each
other on make_gnss_small, which fits both.
"""
import numpy as np
import pytest

torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu

import nlp.cost_functions as cost_functions  # noqa: E402
import nlp.dynamics as dynamics  # noqa: E402
import nlp.measurements as measurements  # noqa: E402
import nlp.nlp as nlp  # noqa: E402
from mhe import configs, solver  # noqa: E402
from oracle import gn  # noqa: E402

import cov_reference as cr  # noqa: E402
import tolerance as tl  # noqa: E402


def _problem(w, Rw=None, **kw):
    return gn.Problem(w.N, w.T, w.n, w.m, w.dyn, w.meas, w.cpm.D, (w.T / 2) * w.cpm.w,
                      w.cpm.lagrange_matrix(w.t_meas), w.Qw, w.Rw if Rw is None else Rw, Pw=w.Pw,
                      meas_static=w.meas_static, **kw)


def _U(w):
    return np.broadcast_to(w.U, (w.B,) + w.U.shape[1:])


def _PAR(w):
    return None if w.PAR is None else np.broadcast_to(w.PAR, (w.B,) + w.PAR.shape[1:])


class Case:
    """A workload, the oracle's Gauss-Newton iterate X of it (the point), the query times
    and the reference covariance with its bound -- computed once per module."""

    def __init__(self, w, Rw=None, max_iter=20, **kw):
        self.w, self.Rw = w, Rw
        self.pb = _problem(w, Rw, **kw)
        self.X, _, _, st = gn.gauss_newton(self.pb, w.X_init, _U(w), w.Y, _PAR(w), w.x0, max_iter=max_iter, tol=1e-9)
        assert np.all(st != gn.NOT_SPD) and np.all(np.isfinite(self.X))
        self.t = cr.query_times(w.cpm, w.T)
        self.C, self.bound = cr.cov_reference(self.pb, w.cpm, self.t, self.X, _U(w), w.Y, _PAR(w), w.x0)
        assert np.linalg.eigvalsh(self.C).min() > 0.0

    def device(self, s, t=None, **kw):
        w = self.w
        dev_rw = None if self.Rw is None else self.Rw
        cov, status = s.covariance(self.X, w.U, w.Y, w.PAR, w.x0, t=self.t if t is None else t, Rw=dev_rw, **kw)
        torch.cuda.synchronize()
        return cov.cpu().numpy(), status.cpu().numpy()


REGISTER = {
    "c1": lambda: configs.make_c1(),
    "c2_n20": lambda: configs.make_c2(B=3, N=20),
    "c2_n100": lambda: configs.make_c2(B=3, N=100),  # dp = 208: every slot, the largest panel
    "gnss_small": lambda: configs.make_gnss_small(B=3),  # n = 5: three queries per panel, one spare column
}
_cache = {}


def _case(name):
    if name not in _cache:
        _cache[name] = Case(REGISTER[name]())
    return _cache[name]


# ---------------------------------------------------------------- 1. register path vs the oracle
@pytest.mark.parametrize("name", sorted(REGISTER))
def test_register_path_matches_oracle(name):
    c = _case(name)
    s = solver.from_workload(c.w)
    assert not s.large_system
    C, status = c.device(s)
    assert C.shape == (c.w.B, 4, c.w.n, c.w.n)
    assert np.all(status == 0), status
    cr.check_blocks(f"cov {name}", C, c.C, c.bound)


# ---------------------------------------------------------------- 2. more than one panel
def test_blocks_do_not_depend_on_the_other_queries():
    c = _case("c2_n20")
    s = solver.from_workload(c.w)
    t9 = np.linspace(0.05, 0.95, 9) * c.w.T  # 18 columns: two panels, the second partly filled
    C9, status = c.device(s, t=t9)
    assert np.all(status == 0) and C9.shape[1] == 9
    for q in range(9):
        C1, _ = c.device(s, t=t9[q:q + 1])
        assert np.array_equal(C9[:, q], C1[:, 0]), q
    Cr, bound = cr.cov_reference(c.pb, c.w.cpm, t9, c.X, _U(c.w), c.w.Y)
    tl.check("cov 9 queries", float(np.abs(C9 - Cr).max()), bound)


# ---------------------------------------------------------------- 3. per-solve Rw
def test_per_solve_rw_masks_rows():
    w = configs.make_gnss_small(B=3)
    mask = np.random.default_rng(3).random((w.B, w.M)) < 0.25
    Rw = np.broadcast_to(w.Rw, (w.B,) + w.Rw.shape).copy()
    Rw[mask] = 0.0
    assert Rw.shape == (w.B, w.M, 1, 1) and 0.15 < mask.mean() < 0.35
    c = Case(w, Rw=Rw)
    s = solver.from_workload(w)
    C, status = c.device(s)
    assert np.all(status == 0)
    cr.check_blocks("cov masked rows", C, c.C, c.bound)
    # the mask matters: the unmasked problem's covariance is smaller by far more than the bound
    C0, _ = s.covariance(c.X, w.U, w.Y, w.PAR, t=c.t)
    assert np.abs(C0.cpu().numpy() - C).max() > 100 * c.bound


# ---------------------------------------------------------------- 4. Huber IRLS weights
def test_huber_weights_enter():
    w = configs.make_c2(B=3, N=20)
    c = Case(w, dyn_cost="huber", delta=0.02)
    s = solver.from_workload(w, dyn_cost="huber", huber_delta=0.02)
    C, status = c.device(s)
    assert np.all(status == 0)
    cr.check_blocks("cov huber", C, c.C, c.bound)
    assert np.abs(C - _case("c2_n20").C).max() > 100 * c.bound  # not the L2 problem's


# ---------------------------------------------------------------- 5. bounds are not reflected
def test_bounds_are_ignored():
    c = _case("c2_n20")
    free = solver.from_workload(c.w)
    boxed = solver.from_workload(c.w, bounds=[(0, -1.0, 1.0)])
    Cf, _ = c.device(free)
    Cb, status = c.device(boxed)
    assert np.all(status == 0)
    tl.check("cov bounded solver", float(np.abs(Cb - c.C).max()), c.bound)
    assert np.array_equal(Cb, Cf)


# ---------------------------------------------------------------- 6. large-system path
def test_large_path_c3_n40_matches_oracle():
    w = configs.make_c3(B=2, N=40)
    c = Case(w, max_iter=8)
    s = solver.from_workload(w, force_large=True)
    assert s.large_system
    C, status = c.device(s)
    assert np.all(status == 0)
    cr.check_blocks("cov c3 N=40 large", C, c.C, c.bound)


def test_large_path_matches_register_path():
    c = _case("gnss_small")
    Cr, _ = c.device(solver.from_workload(c.w))
    big = solver.from_workload(c.w, force_large=True)
    assert big.large_system
    Cl, status = c.device(big)
    assert np.all(status == 0)
    cr.check_blocks("cov gnss_small large", Cl, c.C, c.bound)
    tl.check("cov gnss_small register", float(np.abs(Cr - c.C).max()), c.bound)


def test_large_path_c3_n200_matches_oracle():
    """The tightest case: observed 6.6e-9 against 7.4e-9 on the MI355X.  With the solve's own
    pivots (v_rsq_f64 and one Newton step: 4e-15 of relative error, measured) it was 7.8e-9;
    the covariance stage factors with a second Newton step on the pivots."""
    w = configs.make_c3(B=2, N=200)  # d = 1005: the split / envelope plan
    c = Case(w, max_iter=4)
    s = solver.from_workload(w)
    assert s.large_system
    C, status = c.device(s)
    assert np.all(status == 0)
    cr.check_blocks("cov c3 N=200", C, c.C, c.bound)


def test_large_path_chunked_equals_unchunked():
    w = configs.make_c3(B=3, N=40)
    s = solver.from_workload(w, force_large=True)
    t = cr.query_times(w.cpm, w.T)
    ref, st0 = s.covariance(w.X_init, w.U, w.Y, w.PAR, t=t)
    s.ws_budget = 2 * s.lib.mhe_workspace_bytes(s.dims, 1)
    try:
        assert s._chunk(3, None) == 2  # two launches: 2 + 1 trajectories
        out, st1 = s.covariance(w.X_init, w.U, w.Y, w.PAR, t=t)
        torch.cuda.synchronize()
    finally:
        s.ws_budget = None
    assert np.all(st0.cpu().numpy() == 0) and np.all(st1.cpu().numpy() == 0)
    assert np.array_equal(out.cpu().numpy(), ref.cpu().numpy())


# ---------------------------------------------------------------- 7. the device's own H
def test_consistent_with_the_assembled_system():
    c = _case("c2_n100")
    w = c.w
    s = solver.from_workload(w)
    H, _, _ = s.assemble(c.X, w.U, w.Y)
    C, _ = c.device(s)
    d = w.P * w.n
    Ch = cr.cov_from_H(H.cpu().numpy()[:, :d, :d], w.cpm.lagrange_matrix(c.t), w.n)
    tl.check("cov vs inv(assembled H)", float(np.abs(C - Ch).max()), c.bound)


# ---------------------------------------------------------------- 8. streams
@pytest.mark.parametrize("force_large", [False, True])
def test_side_stream_matches_current_stream(force_large):
    w = configs.make_c2(B=6, N=40)
    s = solver.from_workload(w, force_large=force_large)
    t = cr.query_times(w.cpm, w.T)
    ref, st = s.covariance(w.X_init, w.U, w.Y, t=t)
    ref, st = ref.cpu().numpy(), st.cpu().numpy()
    assert np.all(st == 0)
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    halves = (slice(0, 3), slice(3, 6))
    outs = [s.covariance(w.X_init[sl], w.U, w.Y[sl], t=t, stream=stq)  # no sync in between
            for stq, sl in zip((s1, s2, s1), halves + (slice(0, 6),))]
    torch.cuda.synchronize()
    for (cov, status), sl in zip(outs, halves + (slice(0, 6),)):
        assert np.array_equal(cov.cpu().numpy(), ref[sl])
        assert np.array_equal(status.cpu().numpy(), st[sl])
    assert len(s._ws) <= solver.BatchSolver.WS_CACHE


# ---------------------------------------------------------------- 9. facade: the arrival cost, updated
def test_moving_horizon_with_updated_arrival_cost():
    """The window loop of tests/test_gpu_mhe_window.py (van der Pol, N = 8), 4 windows, with
    the arrival cost updated: after each solve P = extractCovariance("x", [DT])[0], and the
    next window's prior is N(extractSolution("x", [DT]), P) -- weight inv(P).  The oracle
    runs the same loop with cov_reference."""
    N, T, n, m = 8, 2.0, 2, 1
    DT, windows = 0.5, 4
    rng = np.random.default_rng(21)
    t_all = np.linspace(0.0, DT * windows + T, 81)
    x_true = configs._rk4(configs.vdp_rhs, np.array([[0.2, 1.0]]), t_all)[0]
    y_all = x_true + rng.normal(size=x_true.shape) * np.array([0.1, 0.14])
    R = np.linalg.inv(np.diag([0.01, 0.02]))
    Q = np.diag([1e-3, 1e-3])
    problem = nlp.fixedTimeOptimalEstimationNLP(N, T, n, m)
    X = problem.addVariables(N + 1, n, name="x")
    U, W = problem.addDynamics(dynamics.van_der_pol, X, None, None)
    problem.addDynamicsCost(cost_functions.weighted_l2_norm, W, {"Q": np.linalg.inv(Q)})
    Pw_par = problem.addParameter(1, n * n)[0]  # the arrival-cost weight, re-set every window
    X0 = problem.addInitialCost(cost_functions.weighted_l2_norm, X[0], {"Q": Pw_par})
    t_meas = np.linspace(0.0, T, 9)
    Y = problem.addResidualCost(measurements.full_state, X, t_meas, np.zeros((n, t_meas.shape[0])), R)
    cpm = problem.CPM
    with pytest.raises(nlp.UnsupportedFeature):
        problem.extractCovariance("x", [DT])  # before any solve
    problem.initializeEstimate(X, t_all[:20], y_all[:20].T)
    xhat_g = xhat_r = y_all[0]
    P_g = P_r = np.diag([0.1, 0.1])
    sym_inv = lambda P: 0.5 * (np.linalg.inv(P) + np.linalg.inv(P).T)  # noqa: E731
    for step in range(windows):
        t0 = step * DT
        problem.setControl(U, np.array([0.0, T]), np.zeros((m, 2)))
        problem.setParameter(X0, xhat_g)
        problem.setParameter(Pw_par, sym_inv(P_g))
        y_w = np.stack([np.interp(t0 + t_meas, t_all, y_all[:, c]) for c in range(n)])
        problem.setMeasurement(Y, t_meas, y_w)
        X_init = np.stack([x.value if (step > 0) else x.init for x in X])[None]
        problem.solve(warmstart=True)
        Xg = np.stack([problem.extractVariableValue("x", k) for k in range(N + 1)])
        pb = gn.Problem(N, T, n, m, "van_der_pol", "full_state", cpm.D, (T / 2) * cpm.w,
                        cpm.lagrange_matrix(t_meas), np.linalg.inv(Q), np.broadcast_to(R, (9, n, n)),
                        Pw=sym_inv(P_r))
        args = (np.zeros((1, N + 1, m)), y_w.T[None], None, xhat_r[None])
        X_r, _, _, sr = gn.gauss_newton(pb, X_init, *args, max_iter=problem.max_iter, tol=problem.tol)
        assert problem.solver["success"] and sr[0] == gn.OK
        tl.check(f"window {step} X", float(np.abs(Xg - X_r[0]).max()), 1e-8 * (1 + float(np.abs(X_r).max())))
        Cr, bound = cr.cov_reference(pb, cpm, [DT], X_r, *args)
        P_g = problem.extractCovariance("x", [DT])[0]
        P_r = Cr[0, 0]
        assert P_g.shape == (n, n) and np.array_equal(P_g, P_g.T)
        tl.check(f"window {step} cov", float(np.abs(P_g - P_r).max()), bound)
        assert np.linalg.eigvalsh(P_g).min() > 0.0
        xhat_g = problem.extractSolution("x", [DT])[0]
        xhat_r = cpm.evaluateSolution(DT, list(X_r[0]))
    with pytest.raises(nlp.UnsupportedFeature):
        problem.extractCovariance("w", [DT])  # not the state trajectory
