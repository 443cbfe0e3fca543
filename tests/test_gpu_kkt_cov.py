"""Covariance and arrival cost of mixed-row and bordered problems on the GPU (mhe_kkt_cov,
mhe_kkt_arrival, BatchSolver.covariance / arrival of a general solver, NLP.extractCovariance /
extractVariableCovariance) vs the dense KKT inverse (tests/kkt_cov_reference.py).

Points: the oracle's converged Gauss-Newton iterate of tests/general_problems.py's problems,
B = 2; query times [0, 0.37 T, T, 0.2 T].  Tolerance: kkt_cov_reference's bound
(FLOOR_MULT x the reference's change when H moves by eps, + 1e-12 max|ref|); every comparison
prints the observed error beside it.  Shapes:
  two_receiver N = 6    dp = 160, K = 7 (one border panel), 40 query columns (three panels)
  two_receiver N = 20   Pp = 32 (two tiles per component), dp = 320, K = 21 (two border panels)
  multi_receiver N = 7  n = 8, nz = 3 with z[2] in no row (held)
"""
import ctypes

import numpy as np
import pytest

torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu

import nlp.cost_functions as cost_functions  # noqa: E402
import nlp.constraints as constraints  # noqa: E402
import nlp.dynamics as dynamics  # noqa: E402
import nlp.measurements as measurements  # noqa: E402
import nlp.nlp as nlp  # noqa: E402
from mhe import _lib, configs, solver  # noqa: E402
from mhe.solver import _at, _handle, _ptr  # noqa: E402
from oracle import collocation as oc  # noqa: E402
from oracle import gn_general as gg  # noqa: E402

import arrival_reference as ar  # noqa: E402
import cov_reference as cr  # noqa: E402
import kkt_cov_reference as kr  # noqa: E402
import tolerance as tl  # noqa: E402
from general_problems import multi_receiver_problem, two_receiver_problem  # noqa: E402


def _solver(pb):
    return solver.BatchSolver(pb.N, pb.T, pb.dyn, "mixed", pb.D, pb.c, pb.Phi, pb.Qw, pb.Rw, Pw=pb.Pw,
                              n_extra=pb.n_extra, eq=pb.eq if pb.eq.size else None)


class Case:
    """A problem, the oracle's converged iterate (X, Z), the query rows and the reference
    blocks with their bounds -- computed once per module and never modified."""

    def __init__(self, kind, **kw):
        if kind == "multi":
            self.pb, X0, Z0, self.U, self.Y, self.PAR, _, _ = multi_receiver_problem(**kw)
            self.x0 = None
        else:
            self.pb, X0, self.U, self.Y, self.PAR, self.x0, _ = two_receiver_problem(**kw)
            Z0 = None
        pb = self.pb
        self.X, self.Z, _, _, st = gg.gauss_newton_general(pb, X0, Z0, self.U, self.Y, self.PAR, self.x0, max_iter=30)
        assert np.all(st == 0)
        if not pb.n_extra:
            self.Z = None
        self.Phi = kr.query_rows(pb.N, pb.T)
        self.cov, self.covz, self.bx, self.bz = kr.kkt_cov_reference(pb, self.Phi, self.X, self.Z, self.U, self.Y,
                                                                     self.PAR, self.x0)
        self._s = None

    @property
    def s(self):
        if self._s is None:
            self._s = _solver(self.pb)
            assert self._s.large_system and self._s.general
        return self._s

    def device(self, sl=slice(None), Phi=None, X=None, with_extra=False, **kw):
        one = lambda a: None if a is None else a[sl]  # noqa: E731
        out = self.s.covariance(self.X[sl] if X is None else X, one(self.U), self.Y[sl], self.PAR[sl], one(self.x0),
                                Phi=self.Phi if Phi is None else Phi, Z=one(self.Z), with_extra=with_extra, **kw)
        torch.cuda.synchronize()
        return [None if t is None else t.cpu().numpy() for t in out]


CASES = {
    "two_rx": lambda: Case("two_rx", N=6),
    "two_rx_noeq": lambda: Case("two_rx", N=6, with_eq=False),
    "two_rx_n20": lambda: Case("two_rx", N=20),
    "two_rx_n20_noeq": lambda: Case("two_rx", N=20, with_eq=False),
    "multi": lambda: Case("multi", N=7),
}
_cache = {}


def _case(name):
    if name not in _cache:
        _cache[name] = CASES[name]()
    return _cache[name]


def _check_x_blocks(name, C, c, definite):
    assert C.shape == c.cov.shape
    tl.check(f"{name} cov", float(np.abs(C - c.cov).max()), c.bx)
    assert np.array_equal(C, np.swapaxes(C, -1, -2)), f"{name}: blocks not bitwise symmetric"
    emin = float(np.linalg.eigvalsh(C).min())
    print(f"{name}: smallest eigenvalue {emin:.3e} (bound {c.bx:.3e})")
    assert emin > 0.0 if definite else emin >= -c.bx, name


# ---------------------------------------------------------------- 1, 2. equality rows and mixed rows
@pytest.mark.parametrize("name", ["two_rx", "two_rx_n20"])
def test_two_receiver_with_and_without_equality_rows(name):
    c, c0 = _case(name), _case(name + "_noeq")
    s = c.s
    K = s.n_eq
    assert (s.dp, K) == ((160, 7) if name == "two_rx" else (320, 21))
    C, status = c.device()
    assert status.tolist() == [0, 0]
    _check_x_blocks(name, C, c, definite=False)
    # zA = zB at every node: x_2 - x_7 is known exactly at every t
    var = C[:, :, 2, 2] + C[:, :, 7, 7] - 2.0 * C[:, :, 2, 7]
    tl.check(f"{name} var(x2 - x7)", float(np.abs(var).max()), 4.0 * c.bx)
    # K = 0, mixed rows: positive definite blocks
    C0, status0 = c0.device()
    assert status0.tolist() == [0, 0] and c0.s.n_eq == 0
    _check_x_blocks(name + " without rows", C0, c0, definite=True)
    # the rows matter: ignoring C cannot pass
    diff = float(np.abs(C - C0).max())
    print(f"{name}: constrained vs unconstrained {diff:.3e}")
    assert diff > c.bx + c0.bx and diff > 100 * max(c.bx, c0.bx)
    assert float(np.abs(C0 - c.cov).max()) > c.bx and float(np.abs(C - c0.cov).max()) > c0.bx


# ---------------------------------------------------------------- 3. extra variables
def test_extra_variables_block_and_held_component():
    c = _case("multi")
    C, Cz, status = c.device(with_extra=True)
    assert status.tolist() == [0, 0] and c.s.n_extra == 3
    _check_x_blocks("multi", C, c, definite=True)
    assert Cz.shape == (2, 3, 3)
    assert np.all(np.isnan(Cz[:, 2, :])) and np.all(np.isnan(Cz[:, :, 2]))  # z[2] enters no row: nothing known
    zz, zr = Cz[:, :2, :2], c.covz[:, :2, :2]
    assert np.all(np.isfinite(zz))
    tl.check("multi covz", float(np.abs(zz - zr).max()), c.bz)
    assert np.array_equal(zz, np.swapaxes(zz, -1, -2))
    assert np.linalg.eigvalsh(zz).min() > 0.0  # a covariance: the sign of the Schur block
    # covz_out = NULL: the same x blocks
    C1, status1 = c.device()
    assert np.array_equal(C1, C) and status1.tolist() == [0, 0]


# ---------------------------------------------------------------- 4. typed pairs are forwarded
def _raw_cov(s, fn, X, w, Phi, extra=()):
    """mhe_state_cov or mhe_kkt_cov (``extra``: its covz_out) on a typed solver, one launch."""
    X, B, U_t, ustr, Y_t, PAR_t, pstr, x0_t = s._inputs(X, w.U, w.Y, w.PAR, w.x0)
    PhiQ = torch.as_tensor(Phi, device=s.device).contiguous()
    Tq, n = Phi.shape[0], s.n
    cov = torch.full((B, Tq, n, n), 7.0, dtype=torch.float64, device=s.device)
    status = torch.full((B,), -9, dtype=torch.int32, device=s.device)
    cur = torch.cuda.current_stream(s.device)
    ws, nb = s._workspace(B, cur)
    sb = s.lib.mhe_kkt_cov_scratch_bytes(s.dims, B, Tq)
    assert sb == s.lib.mhe_cov_scratch_bytes(s.dims, B, Tq)
    scratch = torch.empty(sb, dtype=torch.uint8, device=s.device) if sb else None
    a = _lib.MheSolveArgs()
    a.batch = B
    a.X0, a.U, a.u_bstride, a.Y = _ptr(X), _ptr(U_t), ustr, _ptr(Y_t)
    a.PAR, a.par_bstride, a.x0 = _ptr(PAR_t), pstr, _ptr(x0_t)
    a.workspace, a.workspace_bytes = _ptr(ws), nb
    rc = fn(s.dims, _ptr(s.cbuf), ctypes.byref(a), _ptr(PhiQ), Tq, _ptr(cov), *extra, _ptr(status), _ptr(scratch), sb,
            _handle(cur))
    assert rc == 0, rc
    torch.cuda.synchronize()
    return cov.cpu().numpy(), status.cpu().numpy()


@pytest.mark.parametrize("name,force_large", [("c2_n20", False), ("c2_n20", True), ("gnss_small", False),
                                              ("gnss_small", True)])
def test_typed_pairs_equal_state_cov_bitwise(name, force_large):
    w = configs.make_c2(B=3, N=20) if name == "c2_n20" else configs.make_gnss_small(B=3)
    s = solver.from_workload(w, force_large=force_large)
    assert s.large_system == force_large and not s.general
    Phi = w.cpm.lagrange_matrix(cr.query_times(w.cpm, w.T))
    A, sa = _raw_cov(s, s.lib.mhe_state_cov, w.X_init, w, Phi)
    Bk, sb = _raw_cov(s, s.lib.mhe_kkt_cov, w.X_init, w, Phi, extra=(None,))
    assert sa.tolist() == sb.tolist() == [0] * 3
    assert np.all(np.isfinite(A)) and np.array_equal(A, Bk)


# ---------------------------------------------------------------- 5. independence
def test_trajectories_and_queries_are_independent():
    c = _case("two_rx")
    C, _ = c.device()
    for b in range(2):
        Cb, st = c.device(sl=slice(b, b + 1))
        assert st.tolist() == [0] and np.array_equal(Cb[0], C[b]), b
    for q in range(4):
        Cq, _ = c.device(Phi=c.Phi[q:q + 1])
        assert np.array_equal(Cq[:, 0], C[:, q]), q
    m = _case("multi")
    Cm, Czm, _ = m.device(with_extra=True)
    C1, Cz1, _ = m.device(sl=slice(1, 2), with_extra=True)
    assert np.array_equal(C1[0], Cm[1]) and np.array_equal(Cz1[0], Czm[1], equal_nan=True)


@pytest.mark.parametrize("name", ["two_rx", "multi"])
def test_nan_trajectory_fails_alone(name):
    c = _case(name)
    good = c.device(with_extra=True)
    X = c.X.copy()
    X[0, 3, 1] = np.nan
    C, Cz, status = c.device(X=X, with_extra=True)
    assert status[0] != 0 and status[1] == 0, status
    assert np.all(np.isnan(C[0])) and np.array_equal(C[1], good[0][1])
    if Cz is not None:
        assert np.all(np.isnan(Cz[0])) and np.array_equal(Cz[1], good[1][1], equal_nan=True)


def test_chunked_and_side_stream_equal_the_plain_call():
    c = _case("two_rx")
    s = c.s
    idx = [0, 1, 0]  # three trajectories
    args = (c.X[idx], c.U[idx], c.Y[idx], c.PAR[idx], c.x0[idx])
    ref, st0 = s.covariance(*args, Phi=c.Phi)
    ref, st0 = ref.cpu().numpy(), st0.cpu().numpy()
    assert st0.tolist() == [0, 0, 0] and np.array_equal(ref[0], ref[2])
    s.ws_budget = 2 * s.lib.mhe_workspace_bytes(s.dims, 1)
    try:
        assert s._chunk(3, None) == 2  # two launches: 2 + 1 trajectories
        out, st1 = s.covariance(*args, Phi=c.Phi)
        torch.cuda.synchronize()
    finally:
        s.ws_budget = None
    assert st1.cpu().numpy().tolist() == [0, 0, 0] and np.array_equal(out.cpu().numpy(), ref)
    side = torch.cuda.Stream()
    out2, st2 = s.covariance(*args, Phi=c.Phi, stream=side)
    torch.cuda.synchronize()
    assert st2.cpu().numpy().tolist() == [0, 0, 0] and np.array_equal(out2.cpu().numpy(), ref)


# ---------------------------------------------------------------- 6. arrival cost
def test_arrival_cost_of_a_mixed_row_problem():
    c = _case("two_rx_noeq")
    pb, s = c.pb, c.s
    t = 0.25 * pb.T
    phi = oc.interp_matrix(pb.N, pb.T, np.array([t]))
    x_arr, Pw_arr, status, cov = s.arrival(c.X, c.U, c.Y, c.PAR, c.x0, Phi=phi, with_cov=True)
    torch.cuda.synchronize()
    x_arr, Pw_arr, status, cov = (v.cpu().numpy() for v in (x_arr, Pw_arr, status, cov))
    assert status.tolist() == [0, 0]
    # the reference block and its inverse, arrival_reference's bound rule
    Cr, _, bx, _ = kr.kkt_cov_reference(pb, phi, c.X, None, c.U, c.Y, c.PAR, c.x0)
    d = pb.P * pb.n
    H, _, _ = gg.normal_equations_full(pb, c.X, None, c.U, c.Y, c.PAR, c.x0)
    Cp = cr.cov_from_H(gg.gn.perturb_rel(H, tl.SEED_H)[:, :d, :d], phi, pb.n)[:, 0]
    tl.check("arrival cov", float(np.abs(cov - Cr[:, 0]).max()), bx)
    C1, _ = c.device(Phi=phi)
    assert np.array_equal(cov, C1[:, 0])  # bitwise the covariance call's block
    for b in range(2):
        A, Ap = ar.sym_inv(Cr[b, 0]), ar.sym_inv(Cp[b])
        bound = tl.FLOOR_MULT * float(np.abs(Ap - A).max()) + 1e-12 * float(np.abs(A).max())
        tl.check(f"Pw_arr[{b}]", float(np.abs(Pw_arr[b] - A).max()), bound)
        assert np.array_equal(Pw_arr[b], Pw_arr[b].T) and np.linalg.eigvalsh(Pw_arr[b]).min() > 0.0
    xb = 4.0 * tl.EPS * np.einsum("j,bjc->bc", np.abs(phi[0]), np.abs(c.X))
    xr = np.einsum("j,bjc->bc", phi[0], c.X)
    tl.check("x_arr (err / bound)", float((np.abs(x_arr - xr) / xb).max()), 1.0)
    # equality rows: refused, the block has no inverse
    ce = _case("two_rx")
    with pytest.raises(_lib.MheCallError, match="UNSUPPORTED"):
        ce.s.arrival(ce.X, ce.U, ce.Y, ce.PAR, ce.x0, Phi=phi)


def test_arrival_with_extra_variables():
    c = _case("multi")
    phi = oc.interp_matrix(c.pb.N, c.pb.T, np.array([0.25 * c.pb.T]))
    x_arr, Pw_arr, status = c.s.arrival(c.X, None, c.Y, c.PAR, None, Phi=phi, Z=c.Z)
    torch.cuda.synchronize()
    Cr, _, _, _ = kr.kkt_cov_reference(c.pb, phi, c.X, c.Z, None, c.Y, c.PAR, None)
    Hp = gg.gn.perturb_rel(gg.normal_equations_full(c.pb, c.X, c.Z, None, c.Y, c.PAR, None)[0], tl.SEED_H)
    Cmat = gg.constraint_rows(c.pb, c.pb.P * c.pb.n, 3)
    assert status.cpu().numpy().tolist() == [0, 0]
    Pw_arr = Pw_arr.cpu().numpy()
    for b in range(2):
        A = ar.sym_inv(Cr[b, 0])
        Cpb = kr._blocks(Hp[b:b + 1], Cmat, phi, c.pb.n, c.pb.P * c.pb.n)[0][0, 0]
        bound = tl.FLOOR_MULT * float(np.abs(ar.sym_inv(Cpb) - A).max()) + 1e-12 * float(np.abs(A).max())
        tl.check(f"multi Pw_arr[{b}]", float(np.abs(Pw_arr[b] - A).max()), bound)
        assert np.array_equal(Pw_arr[b], Pw_arr[b].T) and np.linalg.eigvalsh(Pw_arr[b]).min() > 0.0


# ---------------------------------------------------------------- 7. facade
def _two_rx_rows(N=6, T=5.0, M_range=11):
    """The measurement times of two_receiver_problem in its (time-sorted) row order."""
    t_rng, t_gnss = np.linspace(0, T, M_range), np.linspace(0, T, 6)
    times = list(t_rng) + list(t_rng) + [t for t in t_gnss for _ in range(16)]
    return np.sort(np.array(times), kind="stable")


def _facade_two_rx(with_eq):
    """two_receiver_problem(N=6, B=1) through nlp.nlp, call by call as
    general_problems.two_rx_mhe_facade builds the script's problem."""
    pb, X0, U, Y, PAR, x0, _ = two_receiver_problem(N=6, B=1, with_eq=with_eq)
    N, T, n = pb.N, pb.T, pb.n
    times = _two_rx_rows()
    assert np.array_equal(oc.interp_matrix(N, T, times), pb.Phi)
    code = PAR[0, :, 0].astype(int)
    problem = nlp.fixedTimeOptimalEstimationNLP(N, T, n, 6)
    X = problem.addVariables(N + 1, n, name='x')
    Uh, W = problem.addDynamics(dynamics.gnss_two_receiver, X, None, None)
    problem.addDynamicsCost(cost_functions.weighted_l2_norm, W, {"Q": pb.Qw})
    problem.addInitialCost(cost_functions.weighted_l2_norm, X[0], {"Q": pb.Pw}, x0=x0[0])
    r3, hd = code == gg.ROW_R3, code == gg.ROW_HEAD
    problem.addResidualCost(measurements.multi_receiver_range_3d, X, times[r3], Y[0, r3, 0][None], np.array([10.0]),
                            {"idxA": [0, 1, 2], "idxB": [5, 6, 7]})
    if with_eq:
        for i in range(N + 1):
            problem.addEqConstraint(constraints.equality_constaint, [X[i][2], X[i][7]])
    problem.addResidualCost(measurements.multi_receiver_heading_2d, X, times[hd], Y[0, hd, 0][None], np.array([1.0]),
                            {"idxA": [0, 1], "idxB": [5, 6]})
    for i in np.nonzero(code == gg.ROW_PR)[0]:
        base = int(PAR[0, i, 1])
        problem.addResidualCost(measurements.pseudorange, X, times[i:i + 1], Y[0, i:i + 1, 0][None],
                                np.array([pb.Rw[i]]), {"sat_pos": PAR[0, i, 8:11].copy(),
                                                       "idx": [base, base + 1, base + 2, base + 3]})
    for k in range(N + 1):
        problem.setParameter(Uh[k], U[0, k])
        problem.initialGuess(X[k], X0[0, k])
    return problem


def _facade_reference(problem, Phi):
    """The dense reference at the facade's own solution, from the rows the facade encoded."""
    eng = problem.batch_solver()
    last = problem._last_solve
    t, rows, Rw, Yv, _ = problem._mixed_rows({id(v): off for v, off in problem._extra})
    eq, eq_rhs = problem._eq_pairs()
    pb = gg.GeneralProblem(problem.N, problem.T, problem.n, problem.m, eng.dyn_name, "mixed", problem.CPM.D,
                           (problem.T / 2.0) * problem.CPM.w, problem.CPM.lagrange_matrix(t), problem._dyn_cost, Rw,
                           Pw=None if problem._prior is None else np.asarray(problem._prior[0]),
                           n_extra=eng.n_extra, eq=eq, eq_rhs=eq_rhs)
    X = np.stack([x.value for x in problem._X])[None]
    Z = None if not eng.n_extra else last["Z"].cpu().numpy()
    return pb, kr.kkt_cov_reference(pb, Phi, X, Z, last["U"], Yv.reshape(1, -1, 1), rows[None], last["x0"])


def test_facade_two_receiver_window():
    problem = _facade_two_rx(with_eq=True)
    with pytest.raises(nlp.UnsupportedFeature):
        problem.extractCovariance('x', [1.0])  # before any solve
    problem.solve()
    assert problem.solver["success"]
    tq = [1.0, problem.T]  # DT and T
    C = problem.extractCovariance('x', tq)
    _, (Cr, _, bx, _) = _facade_reference(problem, problem.CPM.lagrange_matrix(np.asarray(tq)))
    assert C.shape == (2, 10, 10)
    tl.check("facade two-receiver cov", float(np.abs(C - Cr[0]).max()), bx)
    assert np.array_equal(C, np.swapaxes(C, -1, -2)) and np.linalg.eigvalsh(C).min() >= -bx
    var = C[:, 2, 2] + C[:, 7, 7] - 2.0 * C[:, 2, 7]
    assert np.abs(var).max() <= 4.0 * bx
    with pytest.raises(nlp.UnsupportedFeature, match="rank-deficient"):
        problem.extractArrivalCost('x', 1.0)
    with pytest.raises(nlp.UnsupportedFeature):
        problem.extractCovariance('w', tq)  # not the state trajectory
    with pytest.raises(nlp.UnsupportedFeature):
        problem.extractVariableCovariance('xa')  # no such extra variable
    # without the rows the same window carries its own arrival cost
    free = _facade_two_rx(with_eq=False)
    free.solve()
    xh, Pw = free.extractArrivalCost('x', 1.0)
    C1 = free.extractCovariance('x', [1.0])[0]
    assert np.array_equal(Pw, Pw.T) and np.linalg.eigvalsh(Pw).min() > 0.0
    assert np.abs(Pw @ C1 - np.eye(10)).max() <= 1e-8
    assert np.allclose(xh, free.extractSolution('x', [1.0])[0], rtol=0, atol=1e-9 * np.abs(xh).max())


def test_facade_extra_variable_covariance():
    pb, X0, Z0, _, Y, PAR, _, _ = multi_receiver_problem(N=7, B=1)
    N, T, n = pb.N, pb.T, pb.n
    t_ep = np.linspace(0, T, 7)
    times = np.repeat(t_ep, 13)
    assert np.array_equal(oc.interp_matrix(N, T, times), pb.Phi)
    problem = nlp.fixedTimeOptimalEstimationNLP(N, T, n, 0)
    X = problem.addVariables(N + 1, n, name='x')
    XA = problem.addVariables(1, 3, name='xa')[0]
    _, W = problem.addDynamics(dynamics.multi_receiver, X, None, None)
    problem.addDynamicsCost(cost_functions.weighted_l2_norm, W, {"Q": pb.Qw})
    for i in range(PAR.shape[1]):
        code, ti, yi, Ri = int(PAR[0, i, 0]), times[i:i + 1], Y[0, i:i + 1, 0][None], np.array([pb.Rw[i]])
        if code == gg.ROW_PR:
            problem.addResidualCost(measurements.pseudorange, X, ti, yi, Ri,
                                    {"sat_pos": PAR[0, i, 8:11].copy(), "idx": [0, 1, 2, 3]})
        elif code == gg.ROW_PRR:
            problem.addResidualCost(measurements.pseudorange_rate, X, ti, yi, Ri,
                                    {"sat_pos": PAR[0, i, 8:11].copy(), "sat_vel": PAR[0, i, 11:14].copy()})
        else:
            problem.addResidualCost(measurements.multi_receiver_range_2d, X, ti, yi, Ri, {"y": XA, "idx": [0, 1]})
    for k in range(N + 1):
        problem.initialGuess(X[k], X0[0, k])
    problem.initialGuess(XA, Z0[0])
    with pytest.raises(nlp.UnsupportedFeature):
        problem.extractVariableCovariance('xa')  # before any solve
    problem.solve()
    assert problem.solver["success"]
    Cz = problem.extractVariableCovariance('xa')
    Phi = problem.CPM.lagrange_matrix(np.array([0.5 * T]))
    _, (Cr, Czr, bx, bz) = _facade_reference(problem, Phi)
    assert Cz.shape == (3, 3)
    assert np.all(np.isnan(Cz[2])) and np.all(np.isnan(Cz[:, 2]))
    tl.check("facade covz", float(np.abs(Cz[:2, :2] - Czr[0, :2, :2]).max()), bz)
    assert np.linalg.eigvalsh(Cz[:2, :2]).min() > 0.0
    C = problem.extractCovariance('x', [0.5 * T])
    tl.check("facade multi cov", float(np.abs(C - Cr[0]).max()), bx)
    with pytest.raises(nlp.UnsupportedFeature):
        problem.extractVariableCovariance('x')  # the state trajectory is not an extra variable
