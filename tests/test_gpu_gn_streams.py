"""The constant tables of k_gn's node / measurement and gradient phases as 16-byte streams
(csrc/mhe_core.h: const_layout's NMS and GRS, written by k_copy_consts and read by the
instances of state dimension 2 and 4, mv_stream).  Every lane multiplies the operands it always did, in the same
order, so the checks are those of tests/test_gpu_gn_seams.py -- the CPU oracle within the bounds
of tests/tolerance.py, iters and status exact, every copy in the batch bit-equal to its source
-- at the smallest shapes (van der Pol / full_state, tests/test_gpu_gn_chain.py's make_vdp) at
which a stream or a tile table can go wrong:

  P = M = 8         two terms per part: one pair of the gradient stream, no trip loop
  P = M = 9         part 0 has three terms: the odd tail of a pair, in both streams
  P = M = 16, 17    second wave; NT = 2, 3: the first off-diagonal Cc slot
  P = M = 72        NT = 9, padding waves
  P = M = 101       C2: 26 / 25 terms per part, padding in the last tile column
  P = 104, M = 101  no padding column
  P = 64, M = 120   M > P: the D and Phi halves of the gradient run different lengths
  P = 101, M = 50   M < P
  P = 64, M = 130   M > 128: the multi-pass branch on D^T / Phi^T beside the new layout (the
                    node / measurement stream is absent, the gradient stream is not)
  P = M = 101 with a per-solve prior weight: the instance whose first_panel reads Cc

each without and with a prior in the constants; four trajectories, 3 iterations, tol 0, inside a
batch of CUs + 8 copies.  Then one pair with n != 2 (the streams under the generic build_tiles),
one bounded solve (k_gn_bounded runs both phases), one solve through a constants buffer
byte-copied from another solver of the same dims (the streams travel with the broadcast), and a
buffer of other dims, which is refused.
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
SHAPES = {(8, 8): 1, (9, 9): 2, (16, 16): 2, (17, 17): 3, (72, 72): 9, (101, 101): 13, (104, 101): 13,
          (64, 120): 8, (101, 50): 13, (64, 130): 8}
IDS = [f"NT{SHAPES[k]}_P{k[0]}_M{k[1]}" for k in sorted(SHAPES)]


def _rep():
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    return np.arange(cus + 8) % B  # more than one trajectory per CU: not the small-batch instance


@functools.lru_cache(maxsize=None)
def _case(P, M, prior, bounded=False):
    """Workload, solver and the oracle's result with its floors, computed once."""
    w = make_vdp(P, M, prior=prior)
    kw = dict(lb=[-np.inf, 0.5], ub=[1.5, np.inf]) if bounded else {}
    pb = gn.Problem(w.N, w.T, w.n, w.m, w.dyn, w.meas, w.cpm.D, (w.T / 2) * w.cpm.w,
                    w.cpm.lagrange_matrix(w.t_meas), w.Qw, w.Rw, Pw=w.Pw, meas_static=w.meas_static, **kw)
    U = np.broadcast_to(w.U, (B,) + w.U.shape[1:])
    run = lambda Y, pt=None: gn.gauss_newton(pb, w.X_init, U, Y, x0=w.x0, max_iter=ITERS, tol=0.0, perturb=pt)  # noqa: E731
    ref, floor = run(w.Y), tl.floor(lambda Y, pt: run(Y, pt)[:2], w.Y)
    s = solver.from_workload(w, bounds=[(1, 0.5, np.inf), (0, -np.inf, 1.5)] if bounded else None)
    return w, s, ref, floor


def _solve(s, w, rep, **kw):
    x0 = None if w.x0 is None else w.x0[rep]
    out = [t.cpu().numpy() for t in s.solve(w.X_init[rep], w.U, w.Y[rep], x0=x0, max_iter=ITERS, tol=0.0, **kw)]
    for a in out:
        assert np.array_equal(a, a[:B][rep])
    return out


def _check(X, cost, iters, status, ref, floor):
    Xr, cr, ir, sr = ref
    fx, fc = floor
    assert iters[:B].tolist() == ir.tolist() == [ITERS] * B
    assert status[:B].tolist() == sr.tolist() == [1] * B
    tl.check("X", np.abs(X[:B] - Xr).max(), tl.bound(fx, Xr))
    tl.check("cost", np.abs(cost[:B] - cr).max(), tl.FLOOR_MULT * fc + 1e-10 * np.abs(cr).max())


@pytest.mark.parametrize("prior", [False, True], ids=["no_prior", "constants_prior"])
@pytest.mark.parametrize("PM", sorted(SHAPES), ids=IDS)
def test_streams_match_oracle(PM, prior):
    w, s, ref, floor = _case(*PM, prior)
    assert s.dp == 16 * SHAPES[PM]
    _check(*_solve(s, w, _rep()), ref, floor)


def test_streams_per_solve_prior_weight():
    """The instance without DOFF; first_panel's read of Cc and the compact blocks."""
    w = make_vdp(101, 101)
    Pw, x0 = ar.prior_inputs(w)
    w.Pw = ar.const_prior(w)
    s = solver.from_workload(w)
    rep = _rep()
    out = [t.cpu().numpy() for t in
           s.solve(w.X_init[rep], w.U, w.Y[rep], x0=x0[rep], max_iter=ITERS, tol=0.0, Pw=Pw[rep])]
    for a in out:
        assert np.array_equal(a, a[:B][rep])
    run = lambda Y, pt=None: ar.solve(w, Pw, x0, ITERS, 0.0, Y=Y, perturb=pt)  # noqa: E731
    _check(*out, run(w.Y), tl.floor(lambda Y, pt: run(Y, pt)[:2], w.Y))


def test_streams_under_generic_tile_build():
    """n = 4 (double integrator, P = 17: a second wave, parts of 5 and 4 terms): the mat-vec
    streams with the tile build that reads Cc and the full alpha D tables."""
    from test_gpu_pairs import case
    c = case("di_P17_M16")
    w, s = c.w, c.solver()
    rep = _rep()
    X, cost, iters, status = [t.cpu().numpy() for t in
                              s.solve(w.X_init[rep], w.U, w.Y[rep], w.PAR, max_iter=ITERS, tol=0.0)]
    for a in (X, cost, iters, status):
        assert np.array_equal(a, a[:B][rep])
    Xr, cr, ir, sr, fx, fc = c.ref(ITERS)
    _check(X, cost, iters, status, (Xr, cr, ir, sr), (fx, fc))


def test_streams_bounded_solve():
    """k_gn_bounded: both mat-vec phases (the node / measurement one again per line-search
    trial) and the tile build with the active-set masking."""
    w, s, ref, floor = _case(21, 21, False, True)
    X, cost, iters, status = _solve(s, w, _rep())
    assert (X[:, :, 1] >= 0.5).all() and (X[:, :, 0] <= 1.5).all()
    _check(X, cost, iters, status, ref, floor)


def test_streams_travel_with_the_constants_bytes():
    """A solver that received another's constants bytes (mhe.dist.broadcast_ on a rank > 0)
    solves like the one that built them; bytes of other dims are refused by the stamp."""
    w, src, ref, floor = _case(101, 101, True)
    dst = solver.from_workload(w, constants="receive")
    assert dst.cbuf.numel() == src.cbuf.numel()
    dst.cbuf.copy_(src.cbuf)
    dst.constants_ready()
    rep = _rep()
    a, b = _solve(src, w, rep), _solve(dst, w, rep)
    for x, y in zip(a, b):
        assert np.array_equal(x, y)
    _check(*b, ref, floor)

    other = _case(104, 101, True)[1]
    bad = solver.from_workload(w, constants="receive")
    k = min(bad.cbuf.numel(), other.cbuf.numel())
    bad.cbuf.zero_()
    bad.cbuf[:k].copy_(other.cbuf[:k])
    bad.constants_ready()
    X, cost, iters, status = [t.cpu().numpy() for t in
                              bad.solve(w.X_init, w.U, w.Y, x0=w.x0, max_iter=ITERS, tol=0.0)]
    assert status.tolist() == [solver.STATUS_BAD_CONSTANTS] * B and iters.tolist() == [0] * B
    assert np.array_equal(X, w.X_init) and np.isnan(cost).all()
