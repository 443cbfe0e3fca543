"""Per-solve prior weight (mhe_solve_args.Pw) and the on-device arrival cost (mhe_arrival)
on the GPU against the per-trajectory oracle of tests/arrival_reference.py.

Every trajectory of a batch carries its own prior weight Pw_b and prior mean x0_b; the
solver's constants hold a weight no trajectory uses (diag(scale)), so a kernel that reads
the constants' weight, or a neighbour's, misses the parity bounds by orders of magnitude.

Tolerances (every comparison prints the observed error beside its bound):
  iterates after the same number of GN steps   tolerance.bound: 8 floor + 1e-10 (1 + max|X|)
  bounded (projected Newton) iterates          1e-9 (1 + max|X|), the bound tests/test_gpu_robust.py
                                               holds this case to; iteration counts exact
  assembled H                                  |dH_ij| <= 1e-12 sqrt(H_ii H_jj) (tests/test_gpu_big_parity.py)
            g, cost                            8 floor + 1e-12 max|.|
  arrival weight                               arrival_reference: 8 floor + 1e-12 max|A_ref| per trajectory
  x(t)                                         4 eps sum_j |phi_j X_j|
  bitwise identities, status, iteration counts exact
"""
import ctypes
import functools

import numpy as np
import pytest

torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu

from mhe import configs, solver  # noqa: E402
from oracle import gn  # noqa: E402

import arrival_reference as ar  # noqa: E402
import cov_reference as cr  # noqa: E402
import tolerance as tl  # noqa: E402

IT = 4
SHAPES = {
    "c2_n20": lambda: configs.make_c2(B=3, N=20),      # dp = 48
    "c2_n100": lambda: configs.make_c2(B=3, N=100),    # dp = 208: every slot, build_slots_n2
    "gnss_small": lambda: configs.make_gnss_small(B=3),  # n = 5: the prior block does not divide 16; nonlinear h
    "c1": lambda: configs.make_c1(),                   # n = 1
    "c3_n40": lambda: configs.make_c3(B=2, N=40),      # large-system path by its 2412 rows
}
REGISTER = ["c2_n20", "c2_n100", "gnss_small", "c1"]


def _np(ts):
    return [t.cpu().numpy() for t in ts]


@functools.lru_cache(maxsize=None)
def _case(name):
    """Workload with a prior added: (w, Pw (B, n, n), x0 (B, n)); the constants' Pw is
    diag(scale), which no trajectory uses."""
    w = SHAPES[name]()
    Pw, x0 = ar.prior_inputs(w)
    w.Pw = ar.const_prior(w)
    return w, Pw, x0


@functools.lru_cache(maxsize=None)
def _solver(name, force_large=False):
    w, _, _ = _case(name)
    s = solver.from_workload(w, force_large=force_large)
    assert s.large_system == (force_large or name == "c3_n40")
    return s


@functools.lru_cache(maxsize=None)
def _ref(name):
    """The oracle's IT-step iterates of the per-trajectory problems and their floors
    (computed once per shape, shared by the tests of both paths; never modified)."""
    w, Pw, x0 = _case(name)
    run = lambda Y, pt=None: ar.solve(w, Pw, x0, IT, 0.0, Y=Y, perturb=pt)  # noqa: E731
    Xr, cr_, ir, sr = run(w.Y)
    fx, fc = tl.floor(lambda Y, pt: run(Y, pt)[:2], w.Y)
    for a in (Xr, cr_, ir, sr):
        a.setflags(write=False)
    return Xr, cr_, ir, sr, fx, fc


SOLVE_CASES = [(n, fl) for n in REGISTER for fl in (False, True)] + [("c3_n40", False)]


@pytest.mark.parametrize("name,force_large", SOLVE_CASES)
def test_solve_with_per_trajectory_prior_weight(name, force_large):
    w, Pw, x0 = _case(name)
    s = _solver(name, force_large)
    X, cost, iters, status = _np(s.solve(w.X_init, w.U, w.Y, w.PAR, x0, max_iter=IT, tol=0.0, Pw=Pw))
    Xr, cr_, ir, sr, fx, fc = _ref(name)
    assert iters.tolist() == ir.tolist() == [IT] * w.B
    assert status.tolist() == sr.tolist() == [1] * w.B
    tl.check(f"{name} large={force_large} X", float(np.abs(X - Xr).max()), tl.bound(fx, Xr))
    tl.check(f"{name} large={force_large} cost", float(np.abs(cost - cr_).max()),
             tl.FLOOR_MULT * fc + 1e-10 * float(np.abs(cr_).max()))
    # the weight matters at this resolution: the constants' weight instead of Pw_b is far outside
    Xc = _np(s.solve(w.X_init, w.U, w.Y, w.PAR, x0, max_iter=IT, tol=0.0))[0]
    print(f"{name}: max |X(Pw_b) - X(constants' Pw)| = {np.abs(X - Xc).max():.3e}")
    assert np.abs(X - Xc).max() > 100.0 * tl.bound(fx, Xr)


@pytest.mark.parametrize("force_large", [False, True])
def test_bounds_with_per_trajectory_prior_weight(force_large):
    """The backtracking bounds case of tests/test_gpu_robust.py (far start 4 X_init, 8
    projected-Newton steps, tol 0) with a prior per trajectory: the Armijo cost along the
    arc carries Pw_b, so the accept / backtrack decisions equal the oracle's only if every
    cost evaluation reads this trajectory's weight."""
    w = configs.make_c2(B=4, N=20)
    Pw, x0 = ar.prior_inputs(w)
    w.Pw = ar.const_prior(w)
    bounds = [(1, 0.5, np.inf), (0, -np.inf, 1.5)]
    X0 = 4.0 * w.X_init
    trace = []
    Xr, cr_, ir, sr = ar.solve(w, Pw, x0, 8, 0.0, X0=X0, trace=trace, lb=[-np.inf, 0.5], ub=[1.5, np.inf])
    halved = sum(a < 1.0 for _, _, a in trace)
    print(f"oracle: {halved} of {len(trace)} steps backtracked")
    assert halved >= 1, "the case should backtrack"
    s = solver.from_workload(w, bounds=bounds, force_large=force_large)
    assert s.large_system == force_large
    X, cost, iters, status = _np(s.solve(X0, w.U, w.Y, None, x0, max_iter=8, tol=0.0, Pw=Pw))
    assert iters.tolist() == ir.tolist() == [8] * w.B and status.tolist() == sr.tolist()
    tl.check(f"bounded large={force_large} X", float(np.abs(X - Xr).max()), 1e-9 * (1 + float(np.abs(Xr).max())))
    tl.check(f"bounded large={force_large} cost", float(np.abs(cost - cr_).max()), 1e-10 * float(np.abs(cr_).max()))
    assert (X[:, :, 1] >= 0.5).all() and (X[:, :, 0] <= 1.5).all()


def test_envelope_sees_the_trajectory_prior_coupling():
    """The split factorization's envelope comes from the component-pair flags of
    k_big_resid.  gnss_pos_and_bias + pseudorange leaves the (position, drift) pairs of H
    zero; a dense Pw_b couples them while the constants' diagonal weight does not, so flags
    formed from the constants' weight would drop non-zero tiles.  Every large-system shape
    runs the split plan (mhe_solve_kernel_name), so the smallest shape whose components span
    more than one tile is taken: N = 16 (Pp = 32: two tiles per component, NT = 10)."""
    w = configs.make_c3(B=2, N=16)
    Pw, x0 = ar.prior_inputs(w)
    w.Pw = ar.const_prior(w)
    assert np.count_nonzero(w.Pw - np.diag(np.diag(w.Pw))) == 0 and np.all(Pw[:, 0, 4] != 0.0)
    s = solver.from_workload(w)
    buf = ctypes.create_string_buffer(256)
    st = torch.cuda.current_stream()
    assert s.lib.mhe_solve_kernel_name(s.dims, w.B, ctypes.c_void_p(st.cuda_stream), buf, 256) == 0
    print(buf.value.decode())
    assert s.large_system and b"split stages" in buf.value and s.dp == 5 * 32
    X, cost, iters, status = _np(s.solve(w.X_init, w.U, w.Y, w.PAR, x0, max_iter=2, tol=0.0, Pw=Pw))
    run = lambda Y, pt=None: ar.solve(w, Pw, x0, 2, 0.0, Y=Y, perturb=pt)  # noqa: E731
    Xr, cr_, ir, sr = run(w.Y)
    fx, _ = tl.floor(lambda Y, pt: run(Y, pt)[:2], w.Y)
    assert iters.tolist() == ir.tolist() == [2] * w.B and status.tolist() == sr.tolist()
    tl.check("envelope X", float(np.abs(X - Xr).max()), tl.bound(fx, Xr))


@pytest.mark.parametrize("name", ["c2_n20", "gnss_small"])
@pytest.mark.parametrize("force_large", [False, True])
def test_bitwise_identities(name, force_large):
    w, Pw, x0 = _case(name)
    s = _solver(name, force_large)
    go = lambda **kw: _np(s.solve(w.X_init, w.U, w.Y, w.PAR, x0, max_iter=IT, tol=0.0, **kw))  # noqa: E731
    base = go()
    # the constants' own weight passed explicitly: the same result, bit for bit
    for P_explicit in (w.Pw[None], np.broadcast_to(w.Pw, (w.B, w.n, w.n)).copy(), w.Pw):
        for a, b in zip(base, go(Pw=P_explicit)):
            assert np.array_equal(a, b)
    # a batch of three equals its trajectories solved alone (strides)
    full = go(Pw=Pw)
    for b in range(w.B):
        one = _np(s.solve(w.X_init[b:b + 1], w.U, w.Y[b:b + 1], w.PAR, x0[b:b + 1], max_iter=IT, tol=0.0,
                          Pw=Pw[b:b + 1]))
        for a, o in zip(full, one):
            assert np.array_equal(a[b:b + 1], o), (name, force_large, b)
    assert not np.array_equal(full[0], base[0])


@pytest.mark.parametrize("name,force_large", [("c2_n20", False), ("c2_n20", True), ("gnss_small", False),
                                              ("gnss_small", True), ("c1", False)])
def test_assemble_with_per_trajectory_prior_weight(name, force_large):
    w, Pw, x0 = _case(name)
    s = _solver(name, force_large)
    n, d = w.n, w.P * w.n
    H, g, cost = _np(s.assemble(w.X_init, w.U, w.Y, w.PAR, x0, Pw=Pw))
    run = lambda Y: ar.normal_equations(w, Pw, x0, w.X_init, Y)  # noqa: E731
    Hr, gr, cr_ = run(w.Y)
    _, fg, fc = tl.floor(lambda Y, pt: run(Y), w.Y, conditioning=False)
    dg = np.sqrt(np.abs(np.einsum("bii->bi", Hr)))
    tl.check(f"{name} large={force_large} H (diagonal-scaled)",
             float((np.abs(H[:, :d, :d] - Hr) / (dg[:, :, None] * dg[:, None, :])).max()), 1e-12)
    if force_large:  # both triangles from the same tile element (the register path forms each on its own)
        assert np.array_equal(H, np.swapaxes(H, 1, 2))
    tl.check(f"{name} large={force_large} g", float(np.abs(g[:, :d] - gr).max()),
             tl.FLOOR_MULT * fg + 1e-12 * float(np.abs(gr).max()))
    tl.check(f"{name} large={force_large} cost", float(np.abs(cost - cr_).max()),
             tl.FLOOR_MULT * fc + 1e-12 * float(np.abs(cr_).max()))
    # against the system without a per-solve weight: the node-0 block, the first n gradient
    # entries and the cost, nothing else
    H0, g0, c0 = _np(s.assemble(w.X_init, w.U, w.Y, w.PAR, x0))
    dH, dg_ = H != H0, g != g0
    assert dH[:, :n, :n].any() and not dH[:, n:, :].any() and not dH[:, :, n:].any()
    assert dg_[:, :n].any() and not dg_[:, n:].any() and np.all(cost != c0)


ARRIVAL_CASES = [(n, False) for n in REGISTER] + [("gnss_small", True), ("c3_n40", False)]


@pytest.mark.parametrize("name,force_large", ARRIVAL_CASES)
@pytest.mark.parametrize("where", ["quarter", "end"])
def test_arrival_matches_reference(name, force_large, where):
    """At the oracle's IT-step iterate: t = 0.25 T, and t = T (a node: phi is a unit row)."""
    w, Pw, x0 = _case(name)
    s = _solver(name, force_large)
    X = np.array(_ref(name)[0])
    t = 0.25 * w.T if where == "quarter" else w.T
    x_arr, A, status, cov = _np(s.arrival(X, w.U, w.Y, w.PAR, x0, t=t, Pw=Pw, with_cov=True))
    xr, Ar, Cr, bound = ar.arrival(w, Pw, x0, X, t)
    assert status.tolist() == [0] * w.B
    print(f"{name} t={t}: cond(C) {[float(np.linalg.cond(c)) for c in Cr]}")
    for b in range(w.B):
        tl.check(f"{name} large={force_large} t={t} Pw_arr[{b}]", float(np.abs(A[b] - Ar[b]).max()), float(bound[b]))
        assert np.array_equal(A[b], A[b].T) and np.linalg.eigvalsh(A[b]).min() > 0.0
    xb = ar.x_bound(w, X, t)
    tl.check(f"{name} x_arr (err / bound)", float((np.abs(x_arr - xr) / np.maximum(xb, 1e-300)).max()), 1.0)
    cov2, st2 = _np(s.covariance(X, w.U, w.Y, w.PAR, x0, t=[t], Pw=Pw))
    assert st2.tolist() == [0] * w.B and np.array_equal(cov, cov2[:, 0])
    # without with_cov the block is inverted in place: the same weight, bit for bit
    x2, A2, st3 = _np(s.arrival(X, w.U, w.Y, w.PAR, x0, t=t, Pw=Pw))
    assert np.array_equal(A2, A) and np.array_equal(x2, x_arr) and st3.tolist() == [0] * w.B


@pytest.mark.parametrize("force_large", [False, True])
def test_arrival_isolates_a_bad_trajectory(force_large):
    """A NaN in one trajectory's X (data, not a fault): its status is non-zero and its outputs
    NaN; the other two are bitwise the healthy run."""
    w, Pw, x0 = _case("c2_n20")
    s = _solver("c2_n20", force_large)
    X = np.array(_ref("c2_n20")[0])
    t = 0.25 * w.T
    good = _np(s.arrival(X, w.U, w.Y, w.PAR, x0, t=t, Pw=Pw, with_cov=True))
    Xb = X.copy()
    Xb[1, 3, 0] = np.nan
    x_arr, A, status, cov = _np(s.arrival(Xb, w.U, w.Y, w.PAR, x0, t=t, Pw=Pw, with_cov=True))
    assert status[1] != 0 and status[0] == 0 and status[2] == 0
    assert np.isnan(x_arr[1]).all() and np.isnan(A[1]).all() and np.isnan(cov[1]).all()
    for b in (0, 2):
        for a, g_ in zip((x_arr, A, cov), (good[0], good[1], good[3])):
            assert np.array_equal(a[b], g_[b])


def test_arrival_execution_variants():
    """A side stream, and a chunked large-system call (B = 3 as 2 + 1 under ws_budget), both
    equal the plain call bitwise."""
    w, Pw, x0 = _case("gnss_small")
    X = np.array(_ref("gnss_small")[0])
    t = 0.25 * w.T
    for force_large in (False, True):
        s = _solver("gnss_small", force_large)
        plain = _np(s.arrival(X, w.U, w.Y, w.PAR, x0, t=t, Pw=Pw, with_cov=True))
        side = torch.cuda.Stream()
        out = s.arrival(X, w.U, w.Y, w.PAR, x0, t=t, Pw=Pw, with_cov=True, stream=side)
        side.synchronize()
        for a, b in zip(plain, _np(out)):
            assert np.array_equal(a, b)
    s = solver.from_workload(w, force_large=True)
    s.ws_budget = 2 * s.lib.mhe_workspace_bytes(s.dims, 1)
    assert s._chunk(w.B) == 2
    for a, b in zip(plain, _np(s.arrival(X, w.U, w.Y, w.PAR, x0, t=t, Pw=Pw, with_cov=True))):
        assert np.array_equal(a, b)
    full = _np(_solver("gnss_small", True).solve(w.X_init, w.U, w.Y, w.PAR, x0, max_iter=2, tol=0.0, Pw=Pw))
    for a, b in zip(full, _np(s.solve(w.X_init, w.U, w.Y, w.PAR, x0, max_iter=2, tol=0.0, Pw=Pw))):
        assert np.array_equal(a, b)  # the per-trajectory offsets of Pw under chunking


# ------------------------------------------------------------------ the moving-horizon loop
def _vdp_windows(B, windows, N=8, T=2.0, DT=0.5):
    t_all = np.linspace(0.0, DT * windows + T, 81)
    x_true = configs._rk4(configs.vdp_rhs, np.array([[0.2, 1.0]]), t_all)[0]
    y_all = np.stack([x_true + np.random.default_rng(21 + b).normal(size=x_true.shape) * np.array([0.1, 0.14])
                      for b in range(B)])  # the trajectories' noise seeds differ
    t_meas = np.linspace(0.0, T, 9)
    Yw = np.stack([np.stack([np.stack([np.interp(k * DT + t_meas, t_all, y_all[b, :, c]) for c in range(2)], axis=1)
                             for b in range(B)]) for k in range(windows)])  # (windows, B, M, n)
    return t_all, y_all, t_meas, Yw


def test_device_loop_solve_arrival_solve():
    """solve(x0, Pw) -> arrival(t = DT) -> next solve for B = 4 windows side by side: the prior
    mean and weight are the device tensors arrival() returned, one BatchSolver (built with a
    zero prior weight) throughout.  The oracle runs the same loop per trajectory."""
    from nlp.collocation import ChebyshevPseudospectralMethod
    N, T, DT, B, windows, n, m = 8, 2.0, 0.5, 4, 4, 2, 1
    t_all, y_all, t_meas, Yw = _vdp_windows(B, windows, N, T, DT)
    cpm = ChebyshevPseudospectralMethod(N, 0, T)
    R = np.linalg.inv(np.diag([0.01, 0.02]))
    w = configs.Workload(N=N, T=T, n=n, m=m, B=B, dyn="van_der_pol", meas="full_state", meas_static={}, cpm=cpm,
                         t_meas=t_meas, Qw=np.linalg.inv(np.diag([1e-3, 1e-3])), Rw=np.broadcast_to(R, (9, n, n)).copy(),
                         Pw=np.zeros((n, n)), U=np.zeros((1, N + 1, m)), PAR=None, Y=Yw[0],
                         X_init=configs._init_from_measurements(cpm, t_meas, Yw[0]))
    s = solver.from_workload(w)
    Xg = torch.as_tensor(w.X_init, device=s.device)
    xg = torch.as_tensor(y_all[:, 0].copy(), device=s.device)
    Pg = torch.as_tensor(np.broadcast_to(np.diag([10.0, 10.0]), (B, n, n)).copy(), device=s.device)
    Xr, xr, Pr = w.X_init, y_all[:, 0].copy(), np.broadcast_to(np.diag([10.0, 10.0]), (B, n, n)).copy()
    for k in range(windows):
        Xg, cost, iters, status = s.solve(Xg, w.U, Yw[k], None, xg, max_iter=20, tol=1e-10, Pw=Pg)
        xg_next, Pg_next, st = s.arrival(Xg, w.U, Yw[k], None, xg, t=DT, Pw=Pg)
        assert xg_next.device == Xg.device and Pg_next.is_cuda and Pg_next.dtype == torch.float64
        Xr, _, _, sr = ar.solve(w, Pr, xr, 20, 1e-10, X0=Xr, Y=Yw[k])
        xr_next, Pr_next, _, bound = ar.arrival(w, Pr, xr, Xr, DT, Y=Yw[k])
        assert status.cpu().tolist() == sr.tolist() == [0] * B and st.cpu().tolist() == [0] * B
        tl.check(f"window {k} X", float(np.abs(Xg.cpu().numpy() - Xr).max()), 1e-8 * (1 + float(np.abs(Xr).max())))
        A = Pg_next.cpu().numpy()
        for b in range(B):
            tl.check(f"window {k} Pw_arr[{b}]", float(np.abs(A[b] - Pr_next[b]).max()), float(bound[b]))
        assert np.array_equal(A, np.swapaxes(A, 1, 2))
        xg, Pg, xr, Pr = xg_next, Pg_next, xr_next, Pr_next
    # the trajectories differ (their own data, their own arrival cost)
    assert np.abs(A[0] - A[1]).max() > 1e-6 * np.abs(A).max()


def test_facade_moving_horizon_with_arrival_cost():
    """The loop of tests/test_gpu_cov.py::test_moving_horizon_with_updated_arrival_cost with
    extractArrivalCost("x", DT) feeding setParameter: same bounds, and ONE engine build."""
    import nlp.cost_functions as cost_functions
    import nlp.dynamics as dynamics
    import nlp.measurements as measurements
    import nlp.nlp as nlp
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
    Pw_par = problem.addParameter(1, n * n)[0]
    X0 = problem.addInitialCost(cost_functions.weighted_l2_norm, X[0], {"Q": Pw_par})
    t_meas = np.linspace(0.0, T, 9)
    Y = problem.addResidualCost(measurements.full_state, X, t_meas, np.zeros((n, t_meas.shape[0])), R)
    cpm = problem.CPM
    with pytest.raises(nlp.UnsupportedFeature):
        problem.extractArrivalCost("x", DT)  # before any solve
    problem.initializeEstimate(X, t_all[:20], y_all[:20].T)
    xhat_g = xhat_r = y_all[0]
    Pw_g = Pw_r = np.diag([10.0, 10.0])
    for step in range(windows):
        t0 = step * DT
        problem.setControl(U, np.array([0.0, T]), np.zeros((m, 2)))
        problem.setParameter(X0, xhat_g)
        problem.setParameter(Pw_par, Pw_g)
        y_w = np.stack([np.interp(t0 + t_meas, t_all, y_all[:, c]) for c in range(n)])
        problem.setMeasurement(Y, t_meas, y_w)
        X_init = np.stack([x.value if (step > 0) else x.init for x in X])[None]
        problem.solve(warmstart=True)
        Xg = np.stack([problem.extractVariableValue("x", k) for k in range(N + 1)])
        pb = gn.Problem(N, T, n, m, "van_der_pol", "full_state", cpm.D, (T / 2) * cpm.w,
                        cpm.lagrange_matrix(t_meas), np.linalg.inv(Q), np.broadcast_to(R, (9, n, n)), Pw=Pw_r)
        args = (np.zeros((1, N + 1, m)), y_w.T[None], None, xhat_r[None])
        X_r, _, _, sr = gn.gauss_newton(pb, X_init, *args, max_iter=problem.max_iter, tol=problem.tol)
        assert problem.solver["success"] and sr[0] == gn.OK
        tl.check(f"window {step} X", float(np.abs(Xg - X_r[0]).max()), 1e-8 * (1 + float(np.abs(X_r).max())))
        Cr, cbound = cr.cov_reference(pb, cpm, [DT], X_r, *args)
        P_g = problem.extractCovariance("x", [DT])[0]
        tl.check(f"window {step} cov", float(np.abs(P_g - Cr[0, 0]).max()), cbound)
        xhat_g, Pw_g = problem.extractArrivalCost("x", DT)
        H, _, _ = gn.normal_equations(pb, X_r, *args)
        Phi = cpm.lagrange_matrix(np.array([DT]))
        Pw_r = ar.sym_inv(cr.cov_from_H(H, Phi, n)[0, 0])
        floor = float(np.abs(ar.sym_inv(cr.cov_from_H(gn.perturb_rel(H, tl.SEED_H), Phi, n)[0, 0]) - Pw_r).max())
        tl.check(f"window {step} Pw", float(np.abs(Pw_g - Pw_r).max()),
                 tl.FLOOR_MULT * floor + 1e-12 * float(np.abs(Pw_r).max()))
        assert Pw_g.shape == (n, n) and np.array_equal(Pw_g, Pw_g.T) and np.linalg.eigvalsh(Pw_g).min() > 0.0
        xb = 4 * tl.EPS * (np.abs(Phi[0])[:, None] * np.abs(Xg)).sum(axis=0)
        tl.check(f"window {step} xhat (err / bound)",
                 float((np.abs(xhat_g - cpm.evaluateSolution(DT, list(Xg))) / xb).max()), 1.0)
        xhat_r = cpm.evaluateSolution(DT, list(X_r[0]))
    assert problem.engine_builds == 1
    with pytest.raises(nlp.UnsupportedFeature):
        problem.extractArrivalCost("w", DT)  # not the state trajectory
