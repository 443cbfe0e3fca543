"""The trimmed instruction stream of k_gn against the CPU oracle (tests/tolerance.py bounds,
as tests/test_gpu_parity.py): padding row groups that leave the mat-vec phases at once, the
cost-only pass after the last step, and the factorization's slot loops at the block counts
where a wave's active slot range is empty, a single slot, or starts at slot 0.

Shapes are van der Pol / full_state problems built like configs.make_c2 with the node and
measurement counts (P, M) chosen at the edges of the 16-row groups of a wave.
"""
import functools

import numpy as np
import pytest

torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu

from mhe import configs, solver  # noqa: E402
from nlp.collocation import ChebyshevPseudospectralMethod  # noqa: E402
from oracle import gn  # noqa: E402

import tolerance as tl  # noqa: E402

PW = np.linalg.inv(np.diag([0.1, 0.2]))


def make_vdp(P, M, B=4, seed=11, prior=False):
    """configs.make_c2 with P nodes and M measurement times (same scales and noise)."""
    T, N = 10.0, P - 1
    rng = np.random.default_rng(seed)
    x0 = np.array([0.0, 1.0])[None, :] + rng.normal(size=(B, 2)) * 0.1
    t = np.linspace(0, T, M)
    xt = configs._rk4(configs.vdp_rhs, x0, t)
    R = np.diag([0.01, 0.02])
    Y = xt + rng.normal(size=(B, M, 2)) * np.sqrt(np.diag(R))[None, None, :]
    cpm = ChebyshevPseudospectralMethod(N, 0, T)
    Q = np.diag([1e-4, 1e-4])
    return configs.Workload(name=f"vdp_P{P}_M{M}", N=N, T=T, n=2, m=1, p=2, M=M, B=B,
                            dyn="van_der_pol", meas="full_state", meas_static={},
                            t_meas=t, Y=Y, U=np.zeros((1, N + 1, 1)), PAR=None, Qw=np.linalg.inv(Q),
                            Rw=np.broadcast_to(np.linalg.inv(R), (M, 2, 2)).copy(),
                            Pw=PW if prior else None,
                            x0=x0 + rng.normal(size=(B, 2)) * 0.05 if prior else None,
                            X_init=configs._init_from_measurements(cpm, t, Y), X_true=xt, cpm=cpm)


def _problem(w):
    return gn.Problem(w.N, w.T, w.n, w.m, w.dyn, w.meas, w.cpm.D, (w.T / 2) * w.cpm.w,
                      w.cpm.lagrange_matrix(w.t_meas), w.Qw, w.Rw, Pw=w.Pw, meas_static=w.meas_static)


def _U(w):
    return np.broadcast_to(w.U, (w.B,) + w.U.shape[1:])


@functools.lru_cache(maxsize=None)
def _case(P, M, B=4, prior=False):
    w = make_vdp(P, M, B=B, prior=prior)
    return w, solver.from_workload(w), _problem(w)


def _np(r):
    return [t.cpu().numpy() for t in r]


# (P, M): rows ending on a group boundary; one row into the next group; M > P and P > M (the
# node phase skips on max(P, M), the gradient phase on P alone); the largest d = 208; C2's
# own shape; M > 128: the un-fused node_phase + meas_phase fallback
SHAPES = [(16, 16), (17, 16), (16, 33), (33, 17), (104, 101), (101, 101), (17, 130)]


@pytest.mark.parametrize("P,M", SHAPES, ids=[f"P{p}_M{m}" for p, m in SHAPES])
def test_padding_row_groups_match_oracle(P, M):
    w, s, pb = _case(P, M)
    it = 3
    X, cost, iters, status = _np(s.solve(w.X_init, w.U, w.Y, max_iter=it, tol=0.0))
    run = lambda Y, pt=None: gn.gauss_newton(pb, w.X_init, _U(w), Y, max_iter=it, tol=0.0, perturb=pt)  # noqa: E731
    Xr, cr, ir, sr = run(w.Y)
    fx, fc = tl.floor(lambda Y, pt: run(Y, pt)[:2], w.Y)
    assert iters.tolist() == ir.tolist() == [it] * w.B
    assert status.tolist() == sr.tolist() == [1] * w.B
    tl.check("X", np.abs(X - Xr).max(), tl.bound(fx, Xr))
    tl.check("cost", np.abs(cost - cr).max(), tl.FLOOR_MULT * fc + 1e-10 * np.abs(cr).max())


def _check_cost_at(w, pb, X, cost):
    """The returned cost is the oracle's cost at the returned X (prior term included), to the
    bound of the assembled cost in tests/test_gpu_parity.py."""
    run = lambda Y, pt=None: (gn.residuals(pb, X, _U(w), Y, x0=w.x0)[3],)  # noqa: E731
    cr = run(w.Y)[0]
    (fc,) = tl.floor(run, w.Y, conditioning=False)
    bnd = tl.FLOOR_MULT * fc + 1e-12 * np.abs(cr).max()
    tl.check("cost", np.abs(cost - cr).max(), bnd)
    return bnd


@pytest.mark.parametrize("prior", [False, True], ids=["no_prior", "prior"])
@pytest.mark.parametrize("max_iter", [0, 1])
@pytest.mark.parametrize("P,M", [(33, 17), (17, 130)], ids=["fused_rows", "rows_over_128"])
def test_cost_only_final_pass(P, M, max_iter, prior):
    w, s, pb = _case(P, M, prior=prior)
    X, cost, iters, status = _np(s.solve(w.X_init, w.U, w.Y, x0=w.x0, max_iter=max_iter, tol=0.0))
    assert iters.tolist() == [max_iter] * w.B and status.tolist() == [1] * w.B
    if max_iter == 0:
        assert np.array_equal(X, w.X_init)
    else:
        Xr = gn.gauss_newton(pb, w.X_init, _U(w), w.Y, x0=w.x0, max_iter=1, tol=0.0)[0]
        fx = tl.floor(lambda Y, pt: (gn.gauss_newton(pb, w.X_init, _U(w), Y, x0=w.x0, max_iter=1, tol=0.0,
                                                     perturb=pt)[0],), w.Y)[0]
        tl.check("X", np.abs(X - Xr).max(), tl.bound(fx, Xr))
    bnd = _check_cost_at(w, pb, X, cost)
    if prior:  # the prior term is far above the bound: a pass that dropped it would have failed
        r0 = X[:, 0] - w.x0
        assert np.all(np.einsum("ba,ac,bc->b", r0, PW, r0) > 100.0 * bnd)


@pytest.mark.parametrize("prior", [False, True], ids=["no_prior", "prior"])
def test_cost_at_converged_exit(prior):
    w, s, pb = _case(17, 16, prior=prior)
    X, cost, iters, status = _np(s.solve(w.X_init, w.U, w.Y, x0=w.x0, max_iter=50, tol=1e-9))
    Xr, cr, ir, sr = gn.gauss_newton(pb, w.X_init, _U(w), w.Y, x0=w.x0, max_iter=50, tol=1e-9)
    assert status.tolist() == sr.tolist() == [0] * w.B
    assert np.all(np.abs(iters - ir) <= 1) and np.all(iters < 50)
    _check_cost_at(w, pb, X, cost)


@pytest.mark.parametrize("P,NT", [(16, 2), (17, 3), (104, 13)], ids=["NT2", "NT3", "NT13"])
def test_slot_loop_entry_chol_solve(P, NT):
    """MODE_LINSOLVE through mhe_chol_solve: at NT = 2 seven of the eight waves own no slot,
    at NT = 3 three own a single one, at NT = 13 every wave starts at slot 0."""
    w, s, pb = _case(P, 16 if P < 104 else 101)
    dp = s.dp
    assert dp == 16 * NT
    rng = np.random.default_rng(7)
    B = 5
    A = rng.normal(size=(B, dp, dp))
    H = A @ np.swapaxes(A, 1, 2) + dp * np.eye(dp)[None]
    g = rng.normal(size=(B, dp))
    delta, status = s.chol_solve(H, g)
    ref = -np.linalg.solve(H, g[..., None])[..., 0]
    assert np.all(status.cpu().numpy() == 0)
    assert np.abs(delta.cpu().numpy() - ref).max() <= 1e-10 * np.abs(ref).max()


def test_slot_loop_entry_not_spd_at_two_blocks():
    w, s, pb = _case(16, 16)
    dp = s.dp
    assert dp == 32
    rng = np.random.default_rng(8)
    A = rng.normal(size=(dp, dp))
    spd = A @ A.T + dp * np.eye(dp)
    H = np.stack([spd, spd, spd, np.eye(dp)])
    H[1, dp - 3, dp - 3] = -1.0                 # indefinite: the pivot fails in the second block
    H[2, :16, :16] -= 100.0 * dp * np.eye(16)   # negative definite leading block
    H[3, 20, 20] = np.nan                       # non-finite pivot
    delta, status = s.chol_solve(H, np.ones((4, dp)))
    assert status.cpu().numpy().tolist() == [0, 2, 2, 2]
    ref = -np.linalg.solve(spd, np.ones(dp))
    assert np.abs(delta.cpu().numpy()[0] - ref).max() <= 1e-10 * np.abs(ref).max()


def test_bitwise_deterministic_two_workgroups_per_cu():
    """(104, 101) at B = 2 CUs + 8 runs the two-workgroups-per-CU instance with every wave's
    rows in play: two runs agree bit for bit, and its first four trajectories with the same
    four solved on their own (the small-batch instance, which the oracle checks above)."""
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    _, s, _ = _case(104, 101)
    w = make_vdp(104, 101, B=2 * cus + 8)
    r1 = _np(s.solve(w.X_init, w.U, w.Y, max_iter=3, tol=0.0))
    r2 = _np(s.solve(w.X_init, w.U, w.Y, max_iter=3, tol=0.0))
    for a, b in zip(r1, r2):
        assert np.array_equal(a, b)
    small = _np(s.solve(w.X_init[:4], w.U, w.Y[:4], max_iter=3, tol=0.0))
    for a, b in zip(small, r1):
        assert np.array_equal(a, b[:4])
