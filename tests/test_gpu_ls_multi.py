"""Multi-epoch stationary-receiver least squares on the device (csrc/mhe_ls.hip: k_ls_multi).

One x, b0, alpha over all rows of a log; a group of 16 or 64 lanes owns a log, chosen from
the row capacity alone.  Inputs and references come from tests/ls_multi_reference.py (their
preconditions are asserted without a device in tests/test_ls_multi_host.py): two batches of
37 ragged logs cut from receiver A of tests/golden/least_squares.npz, one at a row capacity
of 480 (40 epochs x 12 slots: the 16-lane instance) and one at the smallest capacity the
library sends to the 64-lane instance, with
spans of 2, 3, 6 and 40 epochs side by side, 10 to ~250 rows, and cold and warm starts
alternating.  Every log is compared.

Reference: the NumPy restatement of the reference's pinv iteration, pinned to the reference's
own results.  Tolerances are those of tests/test_leastsquares.py: x and b0 1e-6 m, alpha
1e-6 m/s, lat / lon 1e-10 deg; iteration counts equal.  h is a length computed from the ECEF
fix (whose fp64 spacing is 9e-10 m), so it is held to the 1e-6 m of the positions.
"""
import os

import numpy as np
import pytest

import ls_multi_reference as lm
from mhe import _lib
from test_leastsquares import LL_TOL, V_TOL, X_TOL

pytestmark = pytest.mark.gpu
BOTH = pytest.mark.parametrize("which", [0, 1])


def _run(d, p0, nrows=None, t=None, rows=slice(None), **kw):
    import utils.leastsquares as uls
    r = uls.run_batch_multi(d["sp"][rows], d["pr"][rows], (d["t"] if t is None else t)[rows],
                            nrows=(d["nrows"] if nrows is None else nrows)[rows], p_init=p0[rows], **kw)
    p = np.concatenate((r["x"].cpu().numpy(), r["b0"].cpu().numpy()[:, None], r["alpha"].cpu().numpy()[:, None]), 1)
    return p, r["iters"].cpu().numpy()


def _assert_fixes(what, got, ref, rows=slice(None)):
    (p, it), (pr, itr) = got, ref
    ex, ev = np.abs(p[rows, :4] - pr[rows, :4]).max(), np.abs(p[rows, 4] - pr[rows, 4]).max()
    print(f"{what}: x, b0 {ex:.2e} m (bound {X_TOL:.0e}); alpha {ev:.2e} m/s (bound {V_TOL:.0e})")
    np.testing.assert_array_equal(it[rows], itr[rows])
    assert ex <= X_TOL and ev <= V_TOL, (what, ex, ev)


def test_both_instances_are_reached():
    lib = _lib.load()
    assert {lib.mhe_ls_multi_group(int(c)) for c in lm.CAPS} == {16, 64}
    assert [lm.batch(w)["sp"].shape[1] for w in (0, 1)] == list(lm.CAPS)


@BOTH
def test_ragged_logs(which):
    d = lm.batch(which)
    assert _lib.load().mhe_ls_multi_group(d["cap"]) == (16, 64)[which]
    _assert_fixes(f"ragged logs, capacity {d['cap']}", _run(d, d["p0"]), d["ref"])


@BOTH
def test_iteration_cap(which):
    d = lm.batch(which)
    got = _run(d, d["p0"], maxiter=2)
    assert (got[1] == 2).all()
    _assert_fixes("two steps from the start", got, d["ref2"])


@BOTH
def test_initial_bias_and_drift(which):
    d = lm.batch(which)
    _assert_fixes("non-zero b0 and alpha to start from", _run(d, d["p0_bias"]), d["ref_bias"])


@BOTH
def test_flagged_logs_beside_healthy_ones(which):
    d = lm.batch(which)
    clean = _run(d, d["p0_bias"])
    nrows, t = lm.planted(d)
    p, it = _run(d, d["p0_bias"], nrows=nrows, t=t)
    bad = list(lm.PLANT_FEW + lm.PLANT_ONE_T + lm.PLANT_EMPTY)
    assert (it[bad] == -1).all()
    np.testing.assert_array_equal(p[bad], d["p0_bias"][bad])
    others = np.setdiff1d(np.arange(lm.C), bad)
    assert (it[others] > 0).all()
    np.testing.assert_array_equal(p[others], clean[0][others])
    np.testing.assert_array_equal(it[others], clean[1][others])


@BOTH
def test_batch_invariance(which):
    d = lm.batch(which)
    p, it = _run(d, d["p0"])
    p1, it1 = _run(d, d["p0"], rows=slice(5, 6))          # log 5 alone, same row capacity
    np.testing.assert_array_equal(p1[0], p[5])
    assert it1[0] == it[5]
    p2, it2 = _run(d, d["p0"])
    np.testing.assert_array_equal(p2, p)
    np.testing.assert_array_equal(it2, it)


def test_short_logs_held_in_registers():
    """Row capacities of at most 64 take the instance that reads a log once and holds its rows
    in registers: the same operations in the same order, so bitwise the results of the same
    logs in a capacity of 80 (rows read again in every iteration), flagged logs included."""
    d = lm.batch(0)
    nrows, t = lm.planted(d)
    for nr, tt, p0, ref, nflag in ((d["nrows"], d["t"], d["p0"], d["ref"], 0), (nrows, t, d["p0_bias"], d["ref_bias"], 6)):
        sel = np.flatnonzero(nr <= 64)
        assert sel.size >= 20 and nr[sel].max() > 32 and 10 in nr[sel]       # 1 to 3 rows per lane
        got = {}
        for cap in (64, 80):
            cut = {"sp": d["sp"][sel, :cap], "pr": d["pr"][sel, :cap], "t": tt[sel, :cap], "nrows": nr[sel]}
            got[cap] = _run(cut, p0[sel])
        np.testing.assert_array_equal(got[64][0], got[80][0])
        np.testing.assert_array_equal(got[64][1], got[80][1])
        assert (got[64][1] < 0).sum() == nflag
        _assert_fixes("short logs held in registers", got[64], (ref[0][sel], ref[1][sel]),
                      rows=np.flatnonzero(got[64][1] >= 0))


def test_epoch_packed_input():
    """(C,T,S) arrays with nsat and per-epoch t against the flat rows compacted by NumPy, at the
    packed layout's row capacity T * S."""
    import utils.leastsquares as uls
    d = lm.batch(0)
    T, S = d["nsat"].shape[1], lm.S
    assert T * S == d["cap"]
    r = uls.run_batch_multi(d["sp4"], d["pr3"], d["t2"], nrows=d["nsat"], p_init=d["p0"])
    p, it = _run(d, d["p0"])
    got = np.concatenate((r["x"].cpu().numpy(), r["b0"].cpu().numpy()[:, None], r["alpha"].cpu().numpy()[:, None]), 1)
    np.testing.assert_array_equal(got, p)
    np.testing.assert_array_equal(r["iters"].cpu().numpy(), it)


def _lists(tag, T):
    fx = lm.fixture()
    cnt = fx[f"{tag}_count"]
    return (np.asarray(fx[f"{tag}_t"], dtype=np.float64)[:T], [fx[f"{tag}_sat_pos"][k, :cnt[k]] for k in range(T)],
            [fx[f"{tag}_pr"][k, :cnt[k]] for k in range(T)])


def test_drop_in_functions_against_the_reference():
    """runBatchLeastSquares and iterativeLeastSquares_multiTimeStep against the reference's own
    results (tests/golden/ls_multi.npz), in the generator's order: every call starts from the
    previous one's fix through the shared default x."""
    import utils.leastsquares as uls
    gold = dict(np.load(os.path.join(lm.GOLDEN, "ls_multi.npz")))
    p_ref = lm.fixture()["p_ref"]
    single = uls._DEFAULT_X.copy()
    uls._DEFAULT_X_MULTI[:] = 0.0
    for name, tag, T in (("A40", "A", 40), ("B40", "B", 40), ("A6", "A", 6), ("B6", "B", 6)):
        t, sp, pr = _lists(tag, T)
        sol = uls.runBatchLeastSquares(t, sp, pr, p_ref)
        assert set(sol) == {"t", "p_ref_ECEF", "b0", "alpha", "x_ECEF", "y_ECEF", "z_ECEF", "lat", "lon", "h",
                            "x_ENU", "y_ENU", "z_ENU"}
        assert sol["t"] is t and sol["p_ref_ECEF"] is p_ref
        for k in ("x_ECEF", "y_ECEF", "z_ECEF", "x_ENU", "y_ENU", "z_ENU", "b0", "h"):
            assert abs(sol[k] - gold[f"{name}_{k}"]) <= X_TOL, (name, k)
        assert abs(sol["alpha"] - gold[f"{name}_alpha"]) <= V_TOL, name
        for k in ("lat", "lon"):
            assert abs(sol[k] - gold[f"{name}_{k}"]) <= LL_TOL, (name, k)
    sol = uls.runBatchLeastSquares(*_lists("A", 6))
    assert "x_ENU" not in sol and sol["p_ref_ECEF"] is None and len(sol) == 10
    # two default-argument calls in a row: the second starts from the first one's fix
    uls._DEFAULT_X_MULTI[:] = 0.0
    for i, (tag, T) in enumerate((("A", 6), ("B", 3))):
        x, b0, alpha = uls.iterativeLeastSquares_multiTimeStep(*lm.stack_log(*_lists(tag, T)))
        assert x is uls._DEFAULT_X_MULTI
        g = gold[f"pair{i}_p"]
        assert np.abs(x - g[:3]).max() <= X_TOL and abs(b0 - g[3]) <= X_TOL and abs(alpha - g[4]) <= V_TOL, i
    # an array of the caller's is updated in place; b0 and alpha are starting values
    tr, spr, prr = lm.stack_log(*_lists("A", 6))
    own = np.array([1.0, 2.0, 3.0])
    xr, b0, alpha = uls.iterativeLeastSquares_multiTimeStep(tr, spr, prr, own, b0=25.0, alpha=-1.5, maxiter=3)
    xo, bo, ao, _ = lm.iterate(tr, spr, prr, np.array([1.0, 2.0, 3.0]), 25.0, -1.5, maxiter=3)
    assert xr is own and np.abs(own - xo).max() <= X_TOL and abs(b0 - bo) <= X_TOL and abs(alpha - ao) <= V_TOL
    # iterativeLeastSquares's own shared default is another array, untouched by all this
    assert uls._DEFAULT_X is not uls._DEFAULT_X_MULTI
    np.testing.assert_array_equal(uls._DEFAULT_X, single)
