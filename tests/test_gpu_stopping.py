"""The stopping rule of include/mhe.h on every Gauss-Newton solve path, exactly: status 0 as soon
as max|step| <= tol (1 + max|X|), X after the update, extra variables included.

The batches come from tests/stopping_cases.py; tests/test_stopping_host.py shows on the oracle
alone that every decision in them is a factor 2 away from the threshold while two correct
evaluations differ by 1e-4 of it, so ``iters`` and ``status`` are compared with ==, never within 1.

Per batch (``_check_batch``):
  iters, status          equal to the oracle's for every trajectory
  frozen after the stop  for each count k in the batch, the same batch solved with max_iter = k,
                         tol = 0 gives the trajectories that stopped at k the same X (and Z) bit
                         for bit: the rule fired after the update of iteration k and nothing
                         touched the trajectory while its neighbours went on
  X, cost                8 floor + 1e-8 (1 + max|X|), 8 floor + 1e-10 max|cost| (tests/tolerance.py),
                         the bounds of the converged tests on the same paths
  no state across calls  the reversed batch on the same solver object gives the reversed result
  chunks (large path)    under a workspace budget of two trajectories the result is bitwise the
                         unchunked one, iters and status included
Every comparison prints the observed error beside its bound.
"""
import ctypes

import numpy as np
import pytest

torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu

from mhe import solver  # noqa: E402

import stopping_cases as sc  # noqa: E402
import tolerance as tl  # noqa: E402

REGISTER, TILED, LARGE, FUSED = "register", "tiled", "large", "fused"


def _np(out):
    return [t.cpu().numpy() for t in out]


def _kernel_name(s, batch):
    buf = ctypes.create_string_buffer(256)
    st = torch.cuda.current_stream()
    assert s.lib.mhe_solve_kernel_name(s.dims, batch, ctypes.c_void_p(st.cuda_stream), buf, 256) == 0
    return buf.value.decode()


def _cus():
    return torch.cuda.get_device_properties(0).multi_processor_count


def _build(c, path):
    """The device solver of a case on one path, its path asserted."""
    if c.kind == "general":
        pb = c.pb
        s = solver.BatchSolver(pb.N, pb.T, pb.dyn, "mixed", pb.D, pb.c, pb.Phi, pb.Qw, pb.Rw, Pw=pb.Pw,
                               n_extra=pb.n_extra, eq=pb.eq if pb.eq.size else None, fused_general=path == FUSED)
        assert s.fused_general == (path == FUSED) and s.large_system == (path == LARGE)
        return s
    kw = {}
    if c.pbkw.get("dyn_cost") == "huber":
        kw.update(dyn_cost="huber", huber_delta=c.pbkw["delta"])
    if c.kind == "bounded":
        kw.update(bounds=sc.BOUNDS)
    s = solver.from_workload(c.w, force_large=path == LARGE, **kw)
    assert s.large_system == (path == LARGE)
    return s


_solvers = {}


def _solver(c, path):
    key = (c.name, LARGE if path == LARGE else FUSED if path == FUSED else REGISTER)
    if key not in _solvers:
        _solvers[key] = _build(c, path)
    return _solvers[key]


def _solve(s, c, idx, max_iter, tol):
    """(X, cost, iters, status, Z | None) of the trajectories ``idx`` of the case, as numpy."""
    pick = lambda A: None if A is None else A[idx]  # noqa: E731
    copy = lambda A: None if A is None else np.array(A)  # noqa: E731  (the case's arrays are read-only)
    out = _np(s.solve(c.X0[idx], copy(c.U), c.Y[idx], copy(c.PAR), pick(c.x0), max_iter=max_iter, tol=tol, Z0=pick(c.Z0),
                      Pw=pick(c.Pw)))
    return out + [None] if len(out) == 4 else out


def _same(a, b, what):
    for x, y, name in zip(a, b, ("X", "cost", "iters", "status", "Z")):
        if x is not None:
            assert np.array_equal(x, y), f"{what}: {name} differs"


def _check_kernel(c, s, path, batch):
    name = _kernel_name(s, batch)
    print(name)
    if path == LARGE:
        assert name.startswith("large-system path")
        assert ("k_big_linesearch" if c.kind == "bounded" else "k_big_update") in name
    elif path == FUSED:
        assert name.startswith("k_gn_general")
    else:
        assert name.startswith("mhe::k_gn_bounded<" if c.kind == "bounded" else "mhe::k_gn<")
        huber = c.pbkw.get("dyn_cost") == "huber"
        assert ("HUBER=1" in name) == huber
        if c.name == "gnss_small":
            return                                         # either instance: 408 rows decide its LDS layout
        if path == REGISTER and c.kind == "typed" and not huber:
            assert "SB=true" in name                       # the small-batch instance
        else:
            assert "two workgroups per CU" in name and "SB=true" not in name


def _check_batch(c, path):
    s = _solver(c, path)
    B = c.B
    idx = np.arange(B) if path != TILED else np.arange(_cus() + 8) % B
    _check_kernel(c, s, path, idx.size)
    Xr, Zr, cr, ir, sr = c.ref
    out = _solve(s, c, idx, c.max_iter, c.tol)
    X, cost, iters, status, Z = out
    print(f"{c.name} {path}: iterations {iters[:B].tolist()} (oracle {ir.tolist()})")
    _same(out, [None if a is None else a[:B][idx] for a in out], "every copy bitwise its source")
    assert iters[:B].tolist() == ir.tolist()
    assert status[:B].tolist() == sr.tolist() == [0] * B
    # frozen from the update of its last iteration on
    for k in sorted(set(ir.tolist())):
        Xk, _, itk, stk, Zk = _solve(s, c, idx, k, 0.0)
        assert itk.tolist() == [k] * idx.size and stk.tolist() == [1] * idx.size
        at = iters == k
        assert np.array_equal(X[at], Xk[at]), f"{c.name} {path}: X of the trajectories that stopped at {k}"
        if Z is not None:
            assert np.array_equal(Z[at], Zk[at]), f"{c.name} {path}: Z of the trajectories that stopped at {k}"
    fx, fc, fz = c.floors
    tl.check(f"{c.name} {path} X", float(np.abs(X[:B] - Xr).max()), tl.bound(fx, Xr, rel=1e-8))
    if Z is not None:
        tl.check(f"{c.name} {path} Z", float(np.abs(Z[:B] - Zr).max()), tl.bound(fz, Zr, rel=1e-8))
    tl.check(f"{c.name} {path} cost", float(np.abs(cost[:B] - cr).max()),
             tl.FLOOR_MULT * fc + 1e-10 * float(np.abs(cr).max()))
    # no state / iters word survives a call
    rev = _solve(s, c, idx[::-1], c.max_iter, c.tol)
    _same([None if a is None else a[::-1] for a in rev], out, "reversed batch")
    if path == LARGE:
        s.ws_budget = 2 * s.lib.mhe_workspace_bytes(s.dims, 1)
        try:
            assert s._chunk(B) == 2
            _same(_solve(s, c, idx, c.max_iter, c.tol), out, "chunked under a budget of two workspaces")
        finally:
            s.ws_budget = None


# ---------------------------------------------------------------- 1. batches that stop at different iterations
BLENDED_RUNS = [
    ("c2", REGISTER),               # k_gn small-batch instance
    ("c2", TILED),                  # k_gn full-occupancy instance, B = CUs + 8
    ("c2_pw", REGISTER),            # the PW instances: a prior weight per trajectory
    ("c2_pw", TILED),
    ("c2_huber", REGISTER),         # Huber instance (IRLS)
    ("gnss_small", REGISTER),       # n = 5, nonlinear rows
    ("c2_large20", LARGE),          # k_big_update; 16 + 4 over the split factorization's two streams
    ("c2_bounded", REGISTER),       # k_gn_bounded
    ("c2_bounded", LARGE),          # k_big_linesearch
    ("two_receiver", LARGE),        # k_big_border (equality rows)
    ("two_receiver", FUSED),        # k_gn_general
    ("multi_receiver", LARGE),      # k_big_update's nz branch
    ("multi_receiver", FUSED),
]


@pytest.mark.parametrize("name,path", BLENDED_RUNS)
def test_batch_stops_where_the_oracle_stops(name, path):
    c = sc.blended(name)
    if name == "c2_large20":
        assert c.B == 20   # launch_big_factor splits at batch >= 16: halves of 16 and 4
    if name == "two_receiver":
        assert c.pb.eq.shape[0] == 7
    if name == "multi_receiver":
        assert c.pb.n_extra == 3
    _check_batch(c, path)


# ---------------------------------------------------------------- 2. the reduction sees every entry
def _counts(c, path):
    s = _solver(c, path)
    idx = np.arange(c.B) if path != TILED else np.arange(_cus() + 8) % c.B
    if c.kind == "typed":
        _check_kernel(c, s, path, idx.size)
    _, _, iters, status, _ = _solve(s, c, idx, c.max_iter, c.tol)
    assert np.array_equal(iters, iters[:c.B][idx]) and status.tolist() == [0] * idx.size
    return iters[:c.B].tolist()


ENTRY_RUNS = [(n, p) for n in ("di_P17_M16", "gpb_P41_M33", "si2d_P104_M101") for p in (REGISTER, TILED, LARGE)]


@pytest.mark.parametrize("name,path", ENTRY_RUNS)
def test_a_step_in_one_entry_decides_the_count(name, path):
    """Started s = 10 tol (1 + max|X*|) off X* in entry e alone a trajectory stops after 2
    iterations, s / 40 off after 1: a reduction that does not see e stops the first after 1."""
    c, ent = sc.displaced(name)
    expect = sc.displaced_counts(ent)
    assert c.ref[3].tolist() == expect
    got = _counts(c, path)
    wrong = [(ent[k // 2], got[k]) for k in range(len(got) - 1) if got[k] != expect[k]]
    assert not wrong, f"{name} {path}: (entry, count) {wrong}"
    assert got == expect


def test_a_step_in_one_entry_decides_the_count_strided_loop():
    """d = 280 > 256: the large path by its size, and k_big_update's 256-thread loop wraps."""
    c, ent = sc.displaced("di_P70_M40")
    assert {255, 256, 276, 277, 278, 279} <= set(ent) and c.X0[0].size == 280
    expect = sc.displaced_counts(ent)
    assert c.ref[3].tolist() == expect
    s = solver.from_workload(c.w)  # no force_large
    assert s.large_system and _kernel_name(s, c.B).startswith("large-system path")
    _, _, iters, status, _ = _solve(s, c, np.arange(c.B), c.max_iter, c.tol)
    assert status.tolist() == [0] * c.B
    wrong = [(ent[k // 2], int(iters[k])) for k in range(c.B - 1) if iters[k] != expect[k]]
    assert not wrong, f"(entry, count) {wrong}"
    assert iters.tolist() == expect


@pytest.mark.parametrize("path", [REGISTER, TILED, LARGE])
def test_max_x_covers_the_large_component(path):
    """max|X| ~ 1e3 lives in position 0 alone; the step is in a velocity entry with ratio 1/4
    (above 2 were that component left out of the maximum): every count is 1."""
    c, _ = sc.scale_case()
    assert c.ref[3].tolist() == [1] * c.B
    assert _counts(c, path) == [1] * c.B


@pytest.mark.parametrize("path", [REGISTER, TILED, LARGE])
def test_max_x_is_taken_after_the_update(path):
    """tol = 4: a step of 1e3 into the large component has ratio 1/4 with max|X| after the update
    and far above 2 with max|X| before it."""
    c = sc.scale_after_update_case()
    assert c.tol == sc.SCALE_TOL_AFTER and c.ref[3].tolist() == [1]
    assert _counts(c, path) == [1]


@pytest.mark.parametrize("path", [LARGE, FUSED])
def test_a_step_in_an_extra_variable_decides_the_count(path):
    """Started at (X*, Z* + s e_i): the X part of the first step is far below the threshold, so a
    rule that ignores Z stops after 1 iteration; the oracle (and the rule) after 2."""
    c = sc.extra_variable_case()
    assert c.ref[3].tolist() == [2, 2]
    assert _counts(c, path) == [2, 2]


# ---------------------------------------------------------------- 3. edges of tol
@pytest.mark.parametrize("path", [REGISTER, LARGE])
def test_edges_of_tol(path):
    c = sc.blended("c2")
    s = _solver(c, path)
    idx = np.arange(c.B)
    # tol = inf: the rule fires after the first update
    X, _, iters, status, _ = _solve(s, c, idx, c.max_iter, np.inf)
    X1 = _solve(s, c, idx, 1, 0.0)[0]
    assert iters.tolist() == [1] * c.B and status.tolist() == [0] * c.B and np.array_equal(X, X1)
    # tol < 0 never fires: as tol = 0
    neg, zero = _solve(s, c, idx, 5, -1.0), _solve(s, c, idx, 5, 0.0)
    assert neg[2].tolist() == [5] * c.B and neg[3].tolist() == [1] * c.B and np.array_equal(neg[0], zero[0])
    # the rule is evaluated on the last permitted iteration too
    a = sc.at_optimum()
    assert a.ref[3].tolist() == [1, 1] and a.ref[4].tolist() == [0, 0]
    _, _, iters, status, _ = _solve(s, a, np.arange(a.B), 1, a.tol)
    assert iters.tolist() == [1, 1] and status.tolist() == [0, 0]
