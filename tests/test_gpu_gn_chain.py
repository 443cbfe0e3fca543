"""The factorization of k_gn's two-workgroups-per-CU instance with the panel-aware slot map
(make_chain_map in csrc/mhe_core.h: tile ownership with wave 0 as the panel wave of every block
step, the diagonal blocks beyond k+1 dealt to the other waves), against the CPU oracle with the
bounds of tests/tolerance.py (as tests/test_gpu_gn_trim.py).

Shapes are van der Pol / full_state problems built like configs.make_c2, at the block counts
NT = ceil(2 P / 16) where the map's tables can go wrong:

  NT  1  (P = 8)    no off-diagonal tile
  NT  2  (P = 16)   one tile
  NT  3  (P = 17)   first trailing tile
  NT  9  (P = 72)   first size at which a row has as many tiles as there are waves (the light
                    wave is forced to take one)
  NT 13  (P = 101, C2's shape; P = 104, d = 208: no padding): ten slots in use, two diagonal
                    blocks per step for some waves

Four trajectories are checked per case.  A batch of at most one trajectory per CU runs the
small-batch instance (factor_forward_sb, which this map does not touch), so the four are solved
inside a batch of CUs + 8 -- copies of the same four -- which runs the instance under test;
every copy must also equal its source bit for bit.

Two kernels take the map.  A solve that passes no per-solve prior weight runs the instance
without it, whether or not the constants hold a prior (the no_prior / constants_prior cases).
A solve that passes Pw = (B, n, n) runs the instance that reads it, in which the diagonal
blocks stay with their cyclic owners (wave 0 keeps blocks 0 and 8 beside its panels): the
per_solve_prior_weight cases, each trajectory with its own weight and prior mean against the
per-trajectory oracle of tests/arrival_reference.py, at NT = 9 and 13.
"""
import functools

import numpy as np
import pytest

torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu

from mhe import configs, solver  # noqa: E402
from nlp.collocation import ChebyshevPseudospectralMethod  # noqa: E402
from oracle import gn  # noqa: E402

import arrival_reference as ar  # noqa: E402
import tolerance as tl  # noqa: E402

PW = np.linalg.inv(np.diag([0.1, 0.2]))
B = 4
ITERS = 3


def make_vdp(P, M, seed=11, prior=False):
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


@functools.lru_cache(maxsize=None)
def _case(P, prior):
    w = make_vdp(P, min(P, 101), prior=prior)
    pb = gn.Problem(w.N, w.T, w.n, w.m, w.dyn, w.meas, w.cpm.D, (w.T / 2) * w.cpm.w,
                    w.cpm.lagrange_matrix(w.t_meas), w.Qw, w.Rw, Pw=w.Pw, meas_static=w.meas_static)
    return w, solver.from_workload(w), pb


# P -> NT
SHAPES = {8: 1, 16: 2, 17: 3, 72: 9, 101: 13, 104: 13}


@pytest.mark.parametrize("prior", [False, True], ids=["no_prior", "constants_prior"])
@pytest.mark.parametrize("P", sorted(SHAPES), ids=[f"NT{SHAPES[p]}_P{p}" for p in sorted(SHAPES)])
def test_chain_factorization_matches_oracle(P, prior):
    w, s, pb = _case(P, prior)
    assert s.dp == 16 * SHAPES[P]
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    rep = np.arange(cus + 8) % B  # more than one trajectory per CU: not the small-batch instance
    x0 = None if w.x0 is None else w.x0[rep]
    X, cost, iters, status = [t.cpu().numpy() for t in
                              s.solve(w.X_init[rep], w.U, w.Y[rep], x0=x0, max_iter=ITERS, tol=0.0)]
    for a in (X, cost, iters, status):
        assert np.array_equal(a, a[:B][rep])
    U = np.broadcast_to(w.U, (B,) + w.U.shape[1:])
    run = lambda Y, pt=None: gn.gauss_newton(pb, w.X_init, U, Y, x0=w.x0, max_iter=ITERS, tol=0.0, perturb=pt)  # noqa: E731
    Xr, cr, ir, sr = run(w.Y)
    fx, fc = tl.floor(lambda Y, pt: run(Y, pt)[:2], w.Y)
    assert iters[:B].tolist() == ir.tolist() == [ITERS] * B
    assert status[:B].tolist() == sr.tolist() == [1] * B
    tl.check("X", np.abs(X[:B] - Xr).max(), tl.bound(fx, Xr))
    tl.check("cost", np.abs(cost[:B] - cr).max(), tl.FLOOR_MULT * fc + 1e-10 * np.abs(cr).max())


@functools.lru_cache(maxsize=None)
def _pw_case(P):
    """The shape with a prior weight and mean of its own per trajectory; the constants hold
    diag(scale), which no trajectory uses (as tests/test_gpu_arrival.py)."""
    w = make_vdp(P, min(P, 101))
    Pw, x0 = ar.prior_inputs(w)
    w.Pw = ar.const_prior(w)
    return w, Pw, x0, solver.from_workload(w)


@pytest.mark.parametrize("P", [72, 101, 104], ids=[f"NT{SHAPES[p]}_P{p}" for p in (72, 101, 104)])
def test_chain_factorization_per_solve_prior_weight(P):
    w, Pw, x0, s = _pw_case(P)
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    rep = np.arange(cus + 8) % B
    X, cost, iters, status = [t.cpu().numpy() for t in
                              s.solve(w.X_init[rep], w.U, w.Y[rep], x0=x0[rep], max_iter=ITERS, tol=0.0, Pw=Pw[rep])]
    for a in (X, cost, iters, status):
        assert np.array_equal(a, a[:B][rep])
    run = lambda Y, pt=None: ar.solve(w, Pw, x0, ITERS, 0.0, Y=Y, perturb=pt)  # noqa: E731
    Xr, cr, ir, sr = run(w.Y)
    fx, fc = tl.floor(lambda Y, pt: run(Y, pt)[:2], w.Y)
    assert iters[:B].tolist() == ir.tolist() == [ITERS] * B
    assert status[:B].tolist() == sr.tolist() == [1] * B
    tl.check("X", np.abs(X[:B] - Xr).max(), tl.bound(fx, Xr))
    tl.check("cost", np.abs(cost[:B] - cr).max(), tl.FLOOR_MULT * fc + 1e-10 * np.abs(cr).max())
    # the weight is read: the same solve without it lands elsewhere
    base = s.solve(w.X_init[:B], w.U, w.Y[:B], x0=x0, max_iter=ITERS, tol=0.0)[0].cpu().numpy()
    assert not np.array_equal(base, X[:B])
