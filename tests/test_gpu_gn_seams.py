"""The start of an iteration in k_gn's two-workgroups-per-CU instances (CHAIN, csrc/mhe_core.h):
diagonal tile 0 is built and factored by ONE wave during the gradient phase (first_panel: the
wave whose rows are all padding, else wave 0), build_tiles leaves that tile alone and the
factorization enters at k = 0; a wave whose slot range is empty in a step skips the T / U slot
loops, and backward's slot loop likewise.  No floating-point operation changes, so the checks are those of
tests/test_gpu_gn_chain.py -- the CPU oracle within the bounds of tests/tolerance.py, iters and
status exact -- on van der Pol / full_state problems built by its make_vdp:

  P = 8    (NT 1)   every wave but wave 0 is padding: wave 7 runs the first panel, and the
                    factorization's step loop has nothing left to do
  P = 16, 17 (NT 2, 3)  first T step, first trailing tile
  P = 72   (NT 9)   waves 5..7 are padding; the highest, wave 7, is chosen
  P = 101, 104 (NT 13), M = 101: C2's shape, and the shape without a padding column
  P = 64, M = 120   no wave is padding (M > 112): wave 0 runs the first panel
  P = 72, 101 with a per-solve prior weight Pw = (B, n, n): the instance whose tile 0 takes
                    Pw_b - Pw_const

each without and with a prior in the constants.  Four trajectories, 3 iterations, tol 0, solved
inside a batch of CUs + 8 copies (a batch of at most one trajectory per CU runs the small-batch
instance); every copy must equal its source bit for bit.

A check that needs no earlier build: the small-batch instance (factor_forward_sb) shares none of
this code and performs the same operations in the same order, so the four trajectories solved
alone must equal the four solved inside the large batch bit for bit (the invariant of
test_small_batch_instance_matches_full_occupancy_instance in tests/test_gpu_parity.py), here at
P = 8, 72 and 101 and with one trajectory whose X_init holds a NaN: its first pivot is bad, the
flag is raised by the first-panel wave, and its status, iters and untouched X must be the
small-batch instance's, its neighbours' results unchanged.  At P = 72 and 101 the NaN spreads
to the later diagonal blocks and the panels of the step loop raise the flag as well; at P = 8
(NT 1) the step loop runs no panel and the first-panel wave's flag write is the only source of
the status.
"""
import functools

import numpy as np
import pytest

torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu

from mhe import solver  # noqa: E402
from oracle import gn  # noqa: E402

import arrival_reference as ar  # noqa: E402
import tolerance as tl  # noqa: E402
from test_gpu_gn_chain import B, ITERS, make_vdp  # noqa: E402

# (P, M) -> NT
SHAPES = {(8, 8): 1, (16, 16): 2, (17, 17): 3, (72, 72): 9, (101, 101): 13, (104, 101): 13, (64, 120): 8}
IDS = [f"NT{SHAPES[k]}_P{k[0]}_M{k[1]}" for k in sorted(SHAPES)]


@functools.lru_cache(maxsize=None)
def _case(P, M, prior):
    w = make_vdp(P, M, prior=prior)
    pb = gn.Problem(w.N, w.T, w.n, w.m, w.dyn, w.meas, w.cpm.D, (w.T / 2) * w.cpm.w,
                    w.cpm.lagrange_matrix(w.t_meas), w.Qw, w.Rw, Pw=w.Pw, meas_static=w.meas_static)
    return w, solver.from_workload(w), pb


def _rep():
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    return np.arange(cus + 8) % B  # more than one trajectory per CU: not the small-batch instance


def _check(X, cost, iters, status, ref, floor):
    Xr, cr, ir, sr = ref
    fx, fc = floor
    assert iters[:B].tolist() == ir.tolist() == [ITERS] * B
    assert status[:B].tolist() == sr.tolist() == [1] * B
    tl.check("X", np.abs(X[:B] - Xr).max(), tl.bound(fx, Xr))
    tl.check("cost", np.abs(cost[:B] - cr).max(), tl.FLOOR_MULT * fc + 1e-10 * np.abs(cr).max())


@pytest.mark.parametrize("prior", [False, True], ids=["no_prior", "constants_prior"])
@pytest.mark.parametrize("PM", sorted(SHAPES), ids=IDS)
def test_seams_match_oracle(PM, prior):
    w, s, pb = _case(*PM, prior)
    assert s.dp == 16 * SHAPES[PM]
    rep = _rep()
    x0 = None if w.x0 is None else w.x0[rep]
    X, cost, iters, status = [t.cpu().numpy() for t in
                              s.solve(w.X_init[rep], w.U, w.Y[rep], x0=x0, max_iter=ITERS, tol=0.0)]
    for a in (X, cost, iters, status):
        assert np.array_equal(a, a[:B][rep])
    U = np.broadcast_to(w.U, (B,) + w.U.shape[1:])
    run = lambda Y, pt=None: gn.gauss_newton(pb, w.X_init, U, Y, x0=w.x0, max_iter=ITERS, tol=0.0, perturb=pt)  # noqa: E731
    _check(X, cost, iters, status, run(w.Y), tl.floor(lambda Y, pt: run(Y, pt)[:2], w.Y))


@functools.lru_cache(maxsize=None)
def _pw_case(P):
    """A prior weight and mean of its own per trajectory; the constants hold diag(scale), which
    no trajectory uses (as tests/test_gpu_arrival.py)."""
    w = make_vdp(P, min(P, 101))
    Pw, x0 = ar.prior_inputs(w)
    w.Pw = ar.const_prior(w)
    return w, Pw, x0, solver.from_workload(w)


@pytest.mark.parametrize("P", [72, 101], ids=["NT9_P72", "NT13_P101"])
def test_seams_per_solve_prior_weight(P):
    w, Pw, x0, s = _pw_case(P)
    rep = _rep()
    X, cost, iters, status = [t.cpu().numpy() for t in
                              s.solve(w.X_init[rep], w.U, w.Y[rep], x0=x0[rep], max_iter=ITERS, tol=0.0, Pw=Pw[rep])]
    for a in (X, cost, iters, status):
        assert np.array_equal(a, a[:B][rep])
    run = lambda Y, pt=None: ar.solve(w, Pw, x0, ITERS, 0.0, Y=Y, perturb=pt)  # noqa: E731
    _check(X, cost, iters, status, run(w.Y), tl.floor(lambda Y, pt: run(Y, pt)[:2], w.Y))
    # the weight is read: the same solve without it lands elsewhere
    base = s.solve(w.X_init[:B], w.U, w.Y[:B], x0=x0, max_iter=ITERS, tol=0.0)[0].cpu().numpy()
    assert not np.array_equal(base, X[:B])


def _solve(s, w, Xi, rep, **kw):
    x0 = None if w.x0 is None else w.x0[rep]
    return [t.cpu().numpy() for t in s.solve(Xi[rep], w.U, w.Y[rep], x0=x0, max_iter=ITERS, tol=0.0, **kw)]


@pytest.mark.parametrize("prior", [False, True], ids=["no_prior", "constants_prior"])
@pytest.mark.parametrize("P", [8, 72, 101], ids=["NT1_P8", "NT9_P72", "NT13_P101"])
def test_seams_equal_small_batch_instance(P, prior):
    w, s, _ = _case(P, min(P, 101), prior)
    rep = _rep()
    alone = _solve(s, w, w.X_init, np.arange(B))
    large = _solve(s, w, w.X_init, rep)
    for a, l in zip(alone, large):
        assert np.array_equal(l, a[rep])
    # one trajectory starts from a NaN: a bad first pivot, found by the first-panel wave
    Xn = w.X_init.copy()
    Xn[1, 3, 0] = np.nan
    alone_n = _solve(s, w, Xn, np.arange(B))
    large_n = _solve(s, w, Xn, rep)
    assert alone_n[3][1] != 1 and alone_n[2][1] == 0  # not converged, no step taken
    assert np.array_equal(alone_n[0][1], Xn[1], equal_nan=True)  # X untouched
    for a, l in zip(alone_n, large_n):
        assert np.array_equal(l, a[rep], equal_nan=True)
    keep = rep != 1
    for l, ln in zip(large, large_n):
        assert np.array_equal(l[keep], ln[keep])
