"""The fused single-launch kernel of small general problems (k_gn_general,
BatchSolver(fused_general=True)) against the dense-KKT oracle (oracle/gn_general.py) and the
large-system path on the same inputs.

Bounds are those tests/test_gpu_general.py applies to the large path on the same problems
(tests/tolerance.py): with floor = the oracle's own change under eps-level perturbations of y
and of (H, g),
  fixed iteration counts (tol 0)   |X - X_oracle| <= 8 floor + 1e-10 (1 + max|X|), iters exact
  converged (tol 1e-10)            |X - X_oracle| <= 8 floor + 1e-8 (1 + max|X|), iters within 1
  cost                             8 floor_cost + 1e-10 max|cost|
  multipliers                      the oracle's KKT solve at the iterate the last step started
                                   from (kkt_step), 8 floor + 1e-10 (1 + max|lambda|) -- 1e-8 for
                                   the converged run, as X
  equality rows                    |v[a] - v[b]| <= 1e-9 (1 + max|X|) after every step
  status exact; a held extra variable bit-identical to its start value.
The large path is held to the same bounds, and the two paths to each other within them.
Every comparison prints the observed error beside its bound.
"""
import ctypes

import numpy as np
import pytest

torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu

from mhe import _lib, configs, solver  # noqa: E402
from oracle import gn  # noqa: E402
from oracle import gn_general as gg  # noqa: E402

import arrival_reference as ar  # noqa: E402
import tolerance as tl  # noqa: E402
from general_problems import multi_receiver_problem, row, two_receiver_problem  # noqa: E402

CONV = dict(max_iter=40, tol=1e-10)


def _solver(pb, **kw):
    kw.setdefault("fused_general", True)
    return solver.BatchSolver(pb.N, pb.T, pb.dyn, "mixed", pb.D, pb.c, pb.Phi, pb.Qw, pb.Rw, Pw=pb.Pw,
                              n_extra=pb.n_extra, eq=pb.eq if pb.eq.size else None, **kw)


def _np(out):
    torch.cuda.synchronize()
    return [t.cpu().numpy() for t in out]


def _kernel_name(s, B=4):
    buf = ctypes.create_string_buffer(256)
    assert s.lib.mhe_solve_kernel_name(s.dims, B, None, buf, 256) == 0
    return buf.value.decode()


def _fused(pb, **kw):
    s = _solver(pb, **kw)
    assert s.fused_general and not s.large_system and _kernel_name(s).startswith("k_gn_general")
    return s


def _oracle_lambda(pb, X0, U, Y, PAR, x0, steps, perturb=None):
    """Multipliers of the bordered step number ``steps[b]`` (>= 1) of trajectory b: the oracle's
    iterate after steps[b] - 1 steps, then its KKT solve there."""
    B, P, n = X0.shape
    C = gg.constraint_rows(pb, P * n, 0)
    lam = np.zeros((B, pb.eq.shape[0]))
    for b in range(B):
        sl = slice(b, b + 1)
        Xk = gg.gauss_newton_general(pb, X0[sl], None, U[sl], Y[sl], PAR[sl], x0[sl], max_iter=int(steps[b]) - 1,
                                     tol=0.0, perturb=perturb)[0]
        H, g, _ = gg.normal_equations_full(pb, Xk, None, U[sl], Y[sl], PAR[sl], x0[sl])
        if perturb is not None:
            H, g = gn.perturb_rel(H, perturb), gn.perturb_rel(g, perturb + 1)
        lam[b] = gg.kkt_step(H[0], g[0], C, C @ Xk[0].ravel() - pb.eq_rhs)[1]
    return lam


# ---------------------------------------------------------------- two receivers
SHAPES = {
    "N6": dict(N=6),                        # K = 7, dp = 80: no padding rows
    "N6_noeq": dict(N=6, with_eq=False),    # K = 0: mixed rows alone
    "N10": dict(N=10),                      # dp = 112: two padding rows
    "N16": dict(N=16),                      # K = 17: two border panels, NT = 11
}
_problems = {}


def _two_rx(name):
    if name not in _problems:
        _problems[name] = two_receiver_problem(B=2, **SHAPES[name])
    return _problems[name]


# one step from X0 pins H (not just the fixed point); three steps on the first shape
RUNS = [("N6", 1), ("N6", 3), ("N6", "conv")] + [(name, it) for name in list(SHAPES)[1:] for it in (1, "conv")]


@pytest.mark.parametrize("name,iters", RUNS)
def test_two_receiver_matches_kkt_oracle_and_large_path(name, iters):
    pb, X0, U, Y, PAR, x0, _ = _two_rx(name)
    kw = CONV if iters == "conv" else dict(max_iter=iters, tol=0.0)
    rel = 1e-8 if iters == "conv" else tl.REL
    B, nc = X0.shape[0], pb.eq.shape[0]
    sf, sl = _fused(pb), _solver(pb, fused_general=False)
    assert sl.large_system
    lamf = torch.zeros((B, nc), dtype=torch.float64, device="cuda") if nc else None
    Xf, cf, itf, stf = _np(sf.solve(X0, U, Y, PAR, x0, lam_out=lamf, **kw))
    Xl, cl, itl, stl = _np(sl.solve(X0, U, Y, PAR, x0, **kw))
    run = lambda Yv, pt=None: gg.gauss_newton_general(pb, X0, None, U, Yv, PAR, x0, perturb=pt, **kw)  # noqa: E731
    Xr, _, cr, ir, sr = run(Y)
    fx, fc = tl.floor(lambda Yv, pt: (lambda r: (r[0], r[2]))(run(Yv, pt)), Y)
    bx, bc = tl.bound(fx, Xr, rel=rel), tl.FLOOR_MULT * fc + 1e-10 * np.abs(cr).max()
    assert stf.tolist() == sr.tolist() and stl.tolist() == sr.tolist()
    if iters == "conv":
        assert sr.tolist() == [0] * B
        assert np.all(np.abs(itf - ir) <= 1), (itf, ir)
    else:
        assert itf.tolist() == ir.tolist() == [iters] * B
    tl.check(f"{name}/{iters} X fused vs oracle", np.abs(Xf - Xr).max(), bx, " m")
    tl.check(f"{name}/{iters} X large vs oracle", np.abs(Xl - Xr).max(), bx, " m")
    tl.check(f"{name}/{iters} X fused vs large", np.abs(Xf - Xl).max(), bx, " m")
    tl.check(f"{name}/{iters} cost fused vs oracle", np.abs(cf - cr).max(), bc)
    tl.check(f"{name}/{iters} cost fused vs large", np.abs(cf - cl).max(), bc)
    if nc:
        assert np.abs(Xf[:, :, 2] - Xf[:, :, 7]).max() <= 1e-9 * (1 + np.abs(Xf).max())
        lam = lamf.cpu().numpy()
        lr = _oracle_lambda(pb, X0, U, Y, PAR, x0, itf)
        fl, = tl.floor(lambda Yv, pt: (_oracle_lambda(pb, X0, U, Yv, PAR, x0, itf, pt),), Y)
        bl = tl.bound(fl, lr, rel=rel)
        tl.check(f"{name}/{iters} lambda fused vs oracle", np.abs(lam - lr).max(), bl)
        if np.array_equal(itf, itl):  # the same step's multipliers
            tl.check(f"{name}/{iters} lambda fused vs large", np.abs(lam - sl.lam.cpu().numpy()).max(), bl)


# ---------------------------------------------------------------- extra variables
def test_extra_variables_and_held_component():
    pb, X0, Z0, U, Y, PAR, xt, zt = multi_receiver_problem(B=3)
    s = _fused(pb)
    X, cost, iters, st, Z = _np(s.solve(X0, None, Y, PAR, Z0=Z0, **CONV))
    run = lambda Yv, pt=None: gg.gauss_newton_general(pb, X0, Z0, None, Yv, PAR, None, perturb=pt, **CONV)  # noqa: E731
    Xr, Zr, cr, ir, sr = run(Y)
    fx, fz, fc = tl.floor(lambda Yv, pt: (lambda r: (r[0], r[1], r[2]))(run(Yv, pt)), Y)
    assert st.tolist() == sr.tolist() == [0] * 3
    assert np.all(np.abs(iters - ir) <= 1)
    tl.check("multi X", np.abs(X - Xr).max(), tl.bound(fx, Xr, rel=1e-8), " m")
    tl.check("multi Z", np.abs(Z - Zr).max(), tl.bound(fz, Zr, rel=1e-8), " m")
    tl.check("multi cost", np.abs(cost - cr).max(), tl.FLOOR_MULT * fc + 1e-10 * np.abs(cr).max())
    assert np.array_equal(Z[:, 2], np.full(3, 7.0))  # no row depends on it: held exactly
    # one step from (X0, Z0) pins the border (H_xz, H_zz), not just the fixed point
    X1, _, it1, _, Z1 = _np(s.solve(X0, None, Y, PAR, Z0=Z0, max_iter=1, tol=0.0))
    run1 = lambda Yv, pt=None: gg.gauss_newton_general(pb, X0, Z0, None, Yv, PAR, None, max_iter=1, tol=0.0, perturb=pt)[:2]  # noqa: E731
    X1r, Z1r = run1(Y)
    f1x, f1z = tl.floor(run1, Y)
    assert it1.tolist() == [1] * 3
    tl.check("multi one step X", np.abs(X1 - X1r).max(), tl.bound(f1x, X1r), " m")
    tl.check("multi one step Z", np.abs(Z1 - Z1r).max(), tl.bound(f1z, Z1r), " m")


def test_per_solve_rw_masks_an_epoch():
    pb, X0, Z0, U, Y, PAR, _, _ = multi_receiver_problem(B=2)
    Rw = np.tile(pb.Rw, (2, 1))
    Rw[:, 13 * 3:13 * 4] = 0.0          # the 13 rows of epoch 3, every trajectory
    Rw[1, 13 * 5] = 0.0                 # and one more row of trajectory 1 alone
    pbm = gg.GeneralProblem(pb.N, pb.T, pb.n, 0, pb.dyn, "mixed", pb.D, pb.c, pb.Phi, pb.Qw, Rw, n_extra=3)
    s = _fused(pb)
    kw = dict(max_iter=3, tol=0.0)
    X, cost, iters, st, Z = _np(s.solve(X0, None, Y, PAR, Z0=Z0, Rw=Rw, **kw))
    run = lambda Yv, pt=None: gg.gauss_newton_general(pbm, X0, Z0, None, Yv, PAR, None, perturb=pt, **kw)  # noqa: E731
    Xr, Zr, cr, ir, sr = run(Y)
    fx, fz, fc = tl.floor(lambda Yv, pt: (lambda r: (r[0], r[1], r[2]))(run(Yv, pt)), Y)
    assert st.tolist() == sr.tolist() and iters.tolist() == ir.tolist()
    tl.check("masked X", np.abs(X - Xr).max(), tl.bound(fx, Xr), " m")
    tl.check("masked Z", np.abs(Z - Zr).max(), tl.bound(fz, Zr), " m")
    tl.check("masked cost", np.abs(cost - cr).max(), tl.FLOOR_MULT * fc + 1e-10 * np.abs(cr).max())
    X0m = _np(s.solve(X0, None, Y, PAR, Z0=Z0, **kw))[0]
    assert not np.array_equal(X, X0m)   # the mask is honoured


def test_per_solve_prior_weight():
    """One prior block per trajectory (inputs of arrival_reference.prior_inputs) on van der Pol
    with its full_state rows written as mixed COMPONENT rows (n = 2, NT = 2, K = 0)."""
    w = configs.make_c2(B=3, N=12)
    Phi = w.cpm.lagrange_matrix(w.t_meas)
    n = w.n
    rows = np.array([row(gg.ROW_COMP, [a]) for i in range(Phi.shape[0]) for a in range(n)])
    Phi2 = np.repeat(Phi, n, axis=0)
    Rw = np.array([w.Rw[i][a, a] for i in range(Phi.shape[0]) for a in range(n)])
    Pw, x0 = ar.prior_inputs(w)
    D, c = w.cpm.D, (w.T / 2.0) * w.cpm.w
    s = solver.BatchSolver(w.N, w.T, w.dyn, "mixed", D, c, Phi2, w.Qw, Rw, Pw=ar.const_prior(w), fused_general=True)
    assert s.fused_general
    U = np.ascontiguousarray(np.broadcast_to(w.U, (w.B,) + w.U.shape[1:]))
    Y = w.Y.reshape(w.B, -1, 1)
    PAR = np.tile(rows[None], (w.B, 1, 1))
    kw = dict(max_iter=6, tol=0.0)  # (GN converges linearly on this short window: a fixed count)
    X, cost, iters, st = _np(s.solve(w.X_init, U, Y, PAR, x0, Pw=Pw, **kw))

    def run(Yv, pt=None):
        out = [gg.gauss_newton_general(gg.GeneralProblem(w.N, w.T, n, w.m, w.dyn, "mixed", D, c, Phi2, w.Qw, Rw,
                                                         Pw=Pw[b]),
                                       w.X_init[b:b + 1], None, U[b:b + 1], Yv[b:b + 1], PAR[b:b + 1], x0[b:b + 1],
                                       perturb=pt, **kw) for b in range(w.B)]
        return np.concatenate([o[0] for o in out]), np.concatenate([o[2] for o in out]), \
            np.concatenate([o[3] for o in out]), np.concatenate([o[4] for o in out])

    Xr, cr, ir, sr = run(Y)
    fx, fc = tl.floor(lambda Yv, pt: run(Yv, pt)[:2], Y)
    assert st.tolist() == sr.tolist() and iters.tolist() == ir.tolist() == [6] * w.B
    tl.check("Pw X", np.abs(X - Xr).max(), tl.bound(fx, Xr))
    tl.check("Pw cost", np.abs(cost - cr).max(), tl.FLOOR_MULT * fc + 1e-10 * np.abs(cr).max())
    Xc = _np(s.solve(w.X_init, U, Y, PAR, x0, **kw))[0]
    assert not np.array_equal(X, Xc)    # the per-solve blocks are used, not the constants'


# ---------------------------------------------------------------- invariance
def test_result_does_not_depend_on_batch_rerun_or_occupancy():
    pb, X0, U, Y, PAR, x0, _ = two_receiver_problem(B=3, seed=7)
    s = _fused(pb)
    kw = dict(max_iter=8, tol=1e-10)
    lam3 = torch.zeros((3, 7), dtype=torch.float64, device="cuda")
    ref = _np(s.solve(X0, U, Y, PAR, x0, lam_out=lam3, **kw))
    one = lambda a: a[1:2]  # noqa: E731
    lam1 = torch.zeros((1, 7), dtype=torch.float64, device="cuda")
    alone = _np(s.solve(one(X0), one(U), one(Y), one(PAR), one(x0), lam_out=lam1, **kw))
    for a, r in zip(alone, ref):
        assert np.array_equal(a, r[1:2])        # alone = inside a batch of 3, bitwise
    assert np.array_equal(lam1.cpu().numpy(), lam3.cpu().numpy()[1:2])
    # more workgroups than the device runs at once: copies of the three trajectories
    B = torch.cuda.get_device_properties(0).multi_processor_count + 8
    idx = np.arange(B) % 3
    big = [np.ascontiguousarray(a[idx]) for a in (X0, U, Y, PAR, x0)]
    r1 = _np(s.solve(*big, **kw))
    r2 = _np(s.solve(*big, **kw))
    for a, b2, r in zip(r1, r2, ref):
        assert np.array_equal(a, b2)            # rerun
        assert np.array_equal(a, r[idx])        # every copy equals the small batch's


def test_nan_trajectory_fails_alone():
    pb, X0, U, Y, PAR, x0, _ = two_receiver_problem(B=3, seed=7)
    s = _fused(pb)
    kw = dict(max_iter=8, tol=1e-10)
    ref = _np(s.solve(X0, U, Y, PAR, x0, **kw))
    Xn = X0.copy()
    Xn[1, 2, 3] = np.nan
    out = _np(s.solve(Xn, U, Y, PAR, x0, **kw))
    assert out[3][1] in (solver.STATUS_NOT_SPD, solver.STATUS_NONFINITE)
    for a, r in zip(out, ref):
        assert np.array_equal(a[[0, 2]], r[[0, 2]])


def test_rank_deficient_system_is_not_spd():
    """Zero dynamics and prior weights and, for trajectory 1, zero row weights: its H has rank 0
    (no fault is provoked: a non-positive pivot is a status).  It reports NOT_SPD at its first
    step and keeps X0."""
    pb, X0, U, Y, PAR, x0, _ = two_receiver_problem(B=2, seed=7)
    s = _fused(pb)
    ref = _np(s.solve(X0, U, Y, PAR, x0, max_iter=4, tol=0.0))
    Rw = np.tile(pb.Rw, (2, 1))
    Rw[1] = 0.0
    sz = solver.BatchSolver(pb.N, pb.T, pb.dyn, "mixed", pb.D, pb.c, pb.Phi, np.zeros_like(pb.Qw), pb.Rw,
                            Pw=np.zeros_like(pb.Pw), eq=pb.eq, fused_general=True)
    out = _np(sz.solve(X0, U, Y, PAR, x0, Rw=Rw, max_iter=4, tol=0.0))
    assert out[3][1] == solver.STATUS_NOT_SPD and out[2][1] == 0
    assert np.array_equal(out[0][1], X0[1])     # the iterate the failing step started from
    assert ref[3].tolist() == [1, 1]


def test_side_stream_equals_plain_call():
    pb, X0, U, Y, PAR, x0, _ = two_receiver_problem(B=3, seed=7)
    s = _fused(pb)
    ref = _np(s.solve(X0, U, Y, PAR, x0, max_iter=5, tol=0.0))
    side = torch.cuda.Stream()
    out = s.solve(X0, U, Y, PAR, x0, max_iter=5, tol=0.0, stream=side)
    side.synchronize()
    for a, r in zip(_np(out), ref):
        assert np.array_equal(a, r)


# ---------------------------------------------------------------- sibling routing, fallback
def test_covariance_and_arrival_go_through_the_default_path():
    pb, X0, U, Y, PAR, x0, _ = two_receiver_problem(B=2, with_eq=False)
    sf, sd = _fused(pb), _solver(pb, fused_general=False)
    X = _np(sf.solve(X0, U, Y, PAR, x0, **CONV))[0]
    t = [1.0, pb.T]
    for a, r in zip(_np(sf.covariance(X, U, Y, PAR, x0, t=t)), _np(sd.covariance(X, U, Y, PAR, x0, t=t))):
        assert np.array_equal(a, r)
    for a, r in zip(_np(sf.arrival(X, U, Y, PAR, x0, t=1.0)), _np(sd.arrival(X, U, Y, PAR, x0, t=1.0))):
        assert np.array_equal(a, r)
    assert sf.sibling().large_system and not sf.large_system
    # with equality rows: the covariance under them, and the default path's refusal of arrival()
    pb, X0, U, Y, PAR, x0, _ = _two_rx("N6")
    sf, sd = _fused(pb), _solver(pb, fused_general=False)
    for a, r in zip(_np(sf.covariance(X0, U, Y, PAR, x0, t=t)), _np(sd.covariance(X0, U, Y, PAR, x0, t=t))):
        assert np.array_equal(a, r)
    with pytest.raises(_lib.MheCallError, match="UNSUPPORTED"):
        sf.arrival(X0, U, Y, PAR, x0, t=1.0)


def test_assemble_chol_solve_and_robust_rows_go_through_the_default_path():
    pb, X0, U, Y, PAR, x0, _ = _two_rx("N6")
    sf, sd = _fused(pb), _solver(pb, fused_general=False)
    assert sf.kkt_dim == 80 + 7 and sd.kkt_dim == 160 + 7
    Hf, gf, cf = _np(sf.assemble(X0, U, Y, PAR, x0))
    Hd, gd, cd = _np(sd.assemble(X0, U, Y, PAR, x0))
    assert np.array_equal(Hf, Hd) and np.array_equal(gf, gd) and np.array_equal(cf, cd)
    for a, r in zip(_np(sf.chol_solve(Hf, gf)), _np(sd.chol_solve(Hd, gd))):
        assert np.array_equal(a, r)
    md = np.full(pb.M, 5.0)
    for a, r in zip(_np(sf.solve(X0, U, Y, PAR, x0, max_iter=3, tol=0.0, meas_delta=md)),
                    _np(sd.solve(X0, U, Y, PAR, x0, max_iter=3, tol=0.0, meas_delta=md))):
        assert np.array_equal(a, r)
    assert np.array_equal(sf.lam.cpu().numpy(), sd.lam.cpu().numpy())


def test_fallback_dims_run_the_default_path_bitwise():
    """C5s at N = 40 (P n = 328 > 208): the preference is ignored."""
    w = configs.make_c5_small(B=3, N=40)
    sa, sb = solver.from_workload(w, fused_general=True), solver.from_workload(w)
    assert not sa.fused_general and sa.large_system
    assert _kernel_name(sa) == _kernel_name(sb) and _kernel_name(sa).startswith("large-system path")
    ra = _np(sa.solve(w.X_init, None, w.Y, w.PAR, max_iter=3, tol=0.0, Z0=w.Z_init))
    rb = _np(sb.solve(w.X_init, None, w.Y, w.PAR, max_iter=3, tol=0.0, Z0=w.Z_init))
    for a, b2 in zip(ra, rb):
        assert np.array_equal(a, b2)


def test_more_epochs_than_the_lds_layout_holds_fall_back():
    """The dims are fused-general, but Phi has 1200 distinct rows and the kernel's LDS layout
    holds fewer epochs (a function of dims; n = 2, N = 12: below 1000): mhe_build_constants
    refuses the fused layout and the solver takes the default path, bitwise."""
    w = configs.make_c2(B=2, N=12)
    t = np.linspace(0.0, w.T, 1200)
    Phi = w.cpm.lagrange_matrix(t)
    rows = np.array([row(gg.ROW_COMP, [i % 2]) for i in range(len(t))])
    Rw = np.full(len(t), 0.5)
    Y = np.random.default_rng(3).normal(size=(w.B, len(t), 1))
    mk = lambda fused: solver.BatchSolver(w.N, w.T, w.dyn, "mixed", w.cpm.D, (w.T / 2.0) * w.cpm.w, Phi, w.Qw, Rw,  # noqa: E731
                                          fused_general=fused)
    sa, sb = mk(True), mk(False)
    assert not sa.fused_general and sa.large_system and sa.dp == sb.dp
    U = np.ascontiguousarray(np.broadcast_to(w.U, (w.B,) + w.U.shape[1:]))
    for a, b2 in zip(_np(sa.solve(w.X_init, U, Y, rows[None], max_iter=3, tol=0.0)),
                     _np(sb.solve(w.X_init, U, Y, rows[None], max_iter=3, tol=0.0))):
        assert np.array_equal(a, b2)


# ---------------------------------------------------------------- facade
def test_facade_two_receiver_windows(golden, monkeypatch):
    """gnss-multi-receiver.py's moving horizon (general_problems.two_rx_mhe_facade) with
    problem.fused_general = True, two windows, window by window against the oracle -- the
    bound of tests/test_multi_receiver.py (1e-6 (1 + max|x|): the pseudorange rows lose ~5
    digits to cancellation).  One engine build serves both windows."""
    from general_problems import two_rx_mhe_facade, two_rx_mhe_oracle
    from nlp import nlp as nlpmod
    from test_multi_receiver import _synthetic
    from utils import utils as gu
    made = []
    init = nlpmod.fixedTimeOptimalEstimationNLP.__init__

    def init_fused(self, *a, **kw):
        init(self, *a, **kw)
        self.fused_general = True
        made.append(self)

    monkeypatch.setattr(nlpmod.fixedTimeOptimalEstimationNLP, "__init__", init_fused)
    dA, dB, lsA, lsB, p_ref, ov = _synthetic(golden)
    XT, XD, st = two_rx_mhe_facade(dA, dB, lsA, lsB, p_ref, 2, overrides=ov)
    RT, RD, rst = two_rx_mhe_oracle(dA, dB, lsA, lsB, p_ref, 2, lambda s: gu.ecef2enu(s, p_ref), overrides=ov)
    problem, = made
    assert problem.engine_builds == 1
    eng = problem.batch_solver()
    assert eng.fused_general and eng.dp == 112 and _kernel_name(eng, 1).startswith("k_gn_general")
    assert all(s == "Solve_Succeeded" for s in st) and (rst == 0).all()
    scale = 1 + np.abs(RT).max()
    for k in range(2):
        tl.check(f"window {k} x(T)", np.abs(XT[k] - RT[k]).max(), 1e-6 * scale, " m")
        tl.check(f"window {k} x(DT)", np.abs(XD[k] - RD[k]).max(), 1e-6 * scale, " m")
    assert np.abs(XT[:, 2] - XT[:, 7]).max() <= 1e-9 * scale
