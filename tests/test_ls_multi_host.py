"""Multi-epoch stationary-receiver least squares (mhe_ls_multi_run): everything that needs no device.

  * tests/ls_multi_reference.py (the NumPy restatement of utils/leastsquares.py:66-94) is
    pinned to the reference's own results, tests/golden/ls_multi.npz, to 1e-9 m;
  * the C entry point's argument checks, which precede the launch;
  * the preconditions of tests/test_gpu_ls_multi.py, asserted on its exact inputs: every
    unflagged log has >= 5 rows and >= 2 distinct times, and the kernel's formulation (5x5
    normal equations by Cholesky, in NumPy) takes the same iteration count as the pinv
    restatement in EVERY log and agrees with it within the tolerances of
    tests/test_leastsquares.py (positions and biases 1e-6 m, drift 1e-6 m/s).
"""
import ctypes
import os

import numpy as np
import pytest

import ls_multi_reference as lm
from mhe import _lib
from test_leastsquares import V_TOL, X_TOL


@pytest.fixture(scope="module")
def gold():
    return dict(np.load(os.path.join(lm.GOLDEN, "ls_multi.npz")))


def _log(tag, T):
    fx = lm.fixture()
    cnt = fx[f"{tag}_count"]
    return lm.stack_log(np.asarray(fx[f"{tag}_t"], dtype=np.float64)[:T],
                        [fx[f"{tag}_sat_pos"][k, :cnt[k]] for k in range(T)],
                        [fx[f"{tag}_pr"][k, :cnt[k]] for k in range(T)])


def test_restatement_reproduces_reference_runs(gold):
    """The generator's calls in its order, through one shared x as the reference's default."""
    x = np.zeros(3)
    for name, tag, T in (("A40", "A", 40), ("B40", "B", 40), ("A6", "A", 6), ("B6", "B", 6)):
        p, b0, alpha, it = lm.iterate(*_log(tag, T), x)
        assert p is x and 1 < it < 100
        ref = np.array([gold[f"{name}_{k}"] for k in ("x_ECEF", "y_ECEF", "z_ECEF", "b0", "alpha")])
        np.testing.assert_allclose(np.concatenate((p, [b0, alpha])), ref, rtol=0, atol=1e-9)
    x[:] = 0.0
    for i, (tag, T) in enumerate((("A", 6), ("B", 3))):
        p, b0, alpha, _ = lm.iterate(*_log(tag, T), x)
        np.testing.assert_allclose(np.concatenate((p, [b0, alpha])), gold[f"pair{i}_p"], rtol=0, atol=1e-9)


def test_ls_multi_abi_host_checks():
    lib = _lib.load()
    d = _lib.MheLsmDims(max_iter=100, tol=1e-7)
    assert d.struct_size == ctypes.sizeof(_lib.MheLsmDims) == 16
    nul = [None] * 8
    run = lib.mhe_ls_multi_run
    assert run(ctypes.byref(d), 0, 326, *nul) == 0            # no logs: MHE_OK, nothing is touched
    assert run(ctypes.byref(d), 3, 326, *nul) == -5           # MHE_ERR_NULL
    buf = (ctypes.c_double * 16)()
    ptr = ctypes.cast(buf, ctypes.c_void_p)
    for missing in range(7):                                  # any one required pointer missing
        args = [ptr] * 7
        args[missing] = None
        assert run(ctypes.byref(d), 1, 2, *args, None) == -5, missing
    assert run(ctypes.byref(d), -1, 326, *nul) == -1          # MHE_ERR_DIMS
    assert run(ctypes.byref(d), 3, -1, *nul) == -1
    for field, bad in (("max_iter", -1), ("tol", -1e-7), ("tol", float("nan"))):
        e = _lib.MheLsmDims(max_iter=100, tol=1e-7)
        setattr(e, field, bad)
        assert run(ctypes.byref(e), 3, 326, *nul) == -1, field
    for size in (0, 8, 12, 24):                               # zeroed / truncated / foreign struct
        e = _lib.MheLsmDims(max_iter=100, tol=1e-7)
        e.struct_size = size
        assert run(ctypes.byref(e), 3, 326, *nul) == -1
        assert run(ctypes.byref(e), 0, 326, *nul) == -1
    assert run(None, 3, 326, *nul) == -5


def test_group_rule_depends_on_row_capacity_alone():
    """CAPS[1] is the smallest capacity the rule sends to 64 lanes per log; MHE_OPT_LSM_GROUP
    (measurements only) overrides the rule and is refused for other values."""
    lib = _lib.load()
    g = lib.mhe_ls_multi_group
    assert g(lm.CAPS[0]) == 16 and g(lm.CAPS[1] - 1) == 16 and g(lm.CAPS[1]) == 64
    assert g(0) == 16 and g(-1) == -1
    assert [g(r) for r in range(0, 5000, 7)] == sorted(g(r) for r in range(0, 5000, 7))
    assert lib.mhe_set_option(_lib.OPT_LSM_GROUP, 64) == 0
    try:
        assert g(10) == 64
        assert lib.mhe_set_option(_lib.OPT_LSM_GROUP, 32) == -1 and g(10) == 64
    finally:
        assert lib.mhe_set_option(_lib.OPT_LSM_GROUP, 0) == 64
    assert g(10) == 16


@pytest.mark.parametrize("which", [0, 1])
def test_ls_multi_builders_meet_their_preconditions(which):
    d = lm.batch(which)
    cap, G = lm.CAPS[which], (16, 64)[which]
    fx = lm.fixture()
    n = d["nrows"]
    assert n.max() <= cap and n.min() == n[0] == 10 and 10 < G            # fewer rows than lanes
    assert (n % G != 0).sum() >= lm.C - 5 and n.max() > 3 * G             # ragged tails, several passes
    assert 200 <= n.max() <= 300                                           # 40 epochs: four passes of 64 and more
    live = d["nsat"] > 0
    assert (d["nsat"][live] >= 5).all() and (d["nsat"] <= fx[f"{lm.TAG}_count"][None]).all()
    for c in range(lm.C):
        span = lm.SPANS[c % 4]
        ep = np.flatnonzero(live[c])
        assert ep[0] == 0 and ep[-1] == span - 1                           # the span is what it says
        t = lm.rows(d, c)[0]
        assert n[c] >= 5 and np.unique(t).size >= 2
    assert any((~live[c, :lm.SPANS[c % 4]]).any() for c in range(lm.C))    # some epochs dropped entirely
    # the flat rows are the packed layout's valid slots in order
    keep = np.arange(lm.S)[None, None, :] < d["nsat"][..., None]
    for c in (0, 5, 35):
        np.testing.assert_array_equal(d["pr"][c, :n[c]], d["pr3"][c][keep[c]])
        np.testing.assert_array_equal(d["sp"][c, :n[c]], d["sp4"][c][keep[c]])
    # starts alternate and do different amounts of work
    far = np.linalg.norm(d["p0"][:, :3] - lm.fix_A(), axis=1)
    assert (far[1::2] <= 10.0).all() and (far[0::2] > 1e6).all()
    it = d["ref"][1]
    assert it[0::2].min() > it[1::2].max() and it[1::2].min() >= 2 and it.max() < 20
    assert (d["ref2"][1] == 2).all() and (it[0::2] > 2).all()
    assert (np.abs(d["p0_bias"][:, 3:]) > 0).all()
    # planted logs: each kind in the same 4-log wave as a healthy log; one-t logs keep >= 5 rows
    few, one, empty = lm.PLANT_FEW, lm.PLANT_ONE_T, lm.PLANT_EMPTY
    nr, t = lm.planted(d)
    for a, b, c in zip(few, one, empty):
        assert a // 4 == b // 4 == c // 4 and (a // 4) * 4 not in few + one + empty
        assert nr[a] == 4 and nr[c] == 0 and nr[b] >= 5 and np.unique(t[b, :nr[b]]).size == 1
    others = np.setdiff1d(np.arange(lm.C), few + one + empty)
    np.testing.assert_array_equal(nr[others], n[others])
    np.testing.assert_array_equal(t[others], d["t"][others])
    # the two formulations agree at these inputs, in every log: iteration counts, x / b0 / alpha
    for key, p0, mi in (("ref", d["p0"], 100), ("ref2", d["p0"], 2), ("ref_bias", d["p0_bias"], 100)):
        p, it = lm.solve_all(d, lm.normal_equations, p0, maxiter=mi)
        np.testing.assert_array_equal(it, d[key][1])
        ex, ev = np.abs(p[:, :4] - d[key][0][:, :4]).max(), np.abs(p[:, 4] - d[key][0][:, 4]).max()
        print(f"cap {cap} {key}: normal equations vs pinv x, b0 {ex:.2e} m (bound {X_TOL:.0e}); "
              f"alpha {ev:.2e} m/s (bound {V_TOL:.0e})")
        assert ex <= X_TOL and ev <= V_TOL
