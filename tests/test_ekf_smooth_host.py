"""RTS smoother over the EKF history (mhe_ekf_smooth, utils.ekf.smooth_batch): everything
that needs no device.

  * the symbol is exported, declared in include/mhe.h and bound in mhe._lib; the ABI version
    did not move (nothing that existed changed);
  * the C entry point's refusals, which all precede the launch (NULL device pointers);
  * properties of tests/rts_reference.py, the reference of tests/test_gpu_ekf_smooth.py, on
    that file's inputs (tests/ekf_ragged.py);
  * utils.ekf.smooth_batch refuses inconsistent shapes and unregistered or mismatching
    plug-ins before it loads the library.
"""
import ctypes
import os
import re

import numpy as np
import pytest

import ekf_ragged as er
import rts_reference as rts
from mhe import _lib
from mhe.registry import UnsupportedPlugin
from oracle import ekf as oekf
import utils.ekf as ekf
import utils.gnss as gnss

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OK, E_DIMS, E_MODEL, E_NULL = 0, -1, -2, -5
CAR = [1.0e5, 1.2e5, 1500.0, 1.2, 1.4, 2500.0]


def _dims(model="gnss", **kw):
    d = _lib.MheEkfDims(n=5, m=3, dyn_model=1, dt=1.0) if model == "gnss" else \
        _lib.MheEkfDims(n=9, m=2, dyn_model=2, dt=0.1)
    if model == "car":
        for i, v in enumerate(CAR):
            d.dyn_par[i] = v
    for k, v in kw.items():
        setattr(d, k, v)
    return d


# mu_hist, S_hist, U, u_bstride, Q, mu0, S0, mu_s, S_s, mu0_s, S0_s, status, stream
NUL = [None, None, None, 0, None, None, None, None, None, None, None, None, None]


def test_symbol_is_exported_declared_and_bound():
    lib = ctypes.CDLL(_lib.LIB_PATH)
    assert hasattr(lib, "mhe_ekf_smooth")
    hdr = open(os.path.join(ROOT, "include", "mhe.h")).read()
    assert re.search(r"\bint mhe_ekf_smooth\(const mhe_ekf_dims\* dims, int32_t batch, int32_t steps,", hdr)
    assert "#define MHE_ABI_VERSION 11" in hdr
    res, args = _lib.SIGNATURES["mhe_ekf_smooth"]
    assert res is ctypes.c_int and len(args) == 16
    assert args[0] is ctypes.POINTER(_lib.MheEkfDims) and args[6] is ctypes.c_int64
    assert _lib.load().mhe_ekf_smooth.argtypes == args


def test_smooth_refusals_precede_the_launch():
    run = _lib.load().mhe_ekf_smooth
    buf = (ctypes.c_double * 16)()
    p = ctypes.cast(buf, ctypes.c_void_p)      # a host address: never dereferenced, nothing is launched
    assert run(None, 4, 5, *NUL) == E_NULL
    for model in ("gnss", "car"):
        d = _dims(model)
        assert d.struct_size == ctypes.sizeof(_lib.MheEkfDims)
        assert run(ctypes.byref(d), 4, 5, *NUL) == E_NULL                      # every required pointer missing
        req = {"mu_hist": 0, "S_hist": 1, "U": 2, "Q": 4, "mu_s": 7, "S_s": 8}
        for name, i in req.items():                                          # any one of them missing
            a = list(NUL)
            for j in req.values():
                a[j] = p
            a[i] = None
            assert run(ctypes.byref(d), 4, 5, *a) == E_NULL, name
        for outs, priors in (((9,), ()), ((10,), ()), ((9, 10), (5,)), ((9, 10), (6,)), ((9,), (6,))):
            a = list(NUL)                                                    # a smoothed prior without the prior
            for j in tuple(req.values()) + outs + priors:
                a[j] = p
            assert run(ctypes.byref(d), 4, 5, *a) == E_NULL, (outs, priors)
        assert run(ctypes.byref(d), -1, 5, *NUL) == E_DIMS
        assert run(ctypes.byref(d), 4, -1, *NUL) == E_DIMS
        assert run(ctypes.byref(d), 0, 5, *NUL) == OK                          # empty: nothing is read
        assert run(ctypes.byref(d), 4, 0, *NUL) == OK
        for size in (0, d.struct_size - 4, d.struct_size + 8):
            e = _dims(model, struct_size=size)
            assert run(ctypes.byref(e), 4, 5, *NUL) == E_DIMS
            assert run(ctypes.byref(e), 0, 5, *NUL) == E_DIMS
        # fields the smoother does not read may hold anything
        e = _dims(model, pmax=999, q=-7, meas_model=55, r_diag=3)
        assert run(ctypes.byref(e), 0, 5, *NUL) == OK and run(ctypes.byref(e), 4, 5, *NUL) == E_NULL
    for bad in (dict(dyn_model=0), dict(dyn_model=3), dict(n=9), dict(m=2), dict(n=4, m=3)):
        assert run(ctypes.byref(_dims("gnss", **bad)), 4, 5, *NUL) == E_MODEL, bad
    for bad in (dict(n=5), dict(m=3), dict(dyn_model=7)):
        assert run(ctypes.byref(_dims("car", **bad)), 4, 5, *NUL) == E_MODEL, bad
    for i in (2, 5):                                                         # the vehicle's M / I_Z unset
        d = _dims("car")
        d.dyn_par[i] = 0.0
        assert run(ctypes.byref(d), 4, 5, *NUL) == E_DIMS


# ---------------------------------------------------------------- the reference itself

@pytest.fixture(scope="module")
def gnss_case():
    inp = er.gnss_inputs(6)
    inp["hist"] = er.oracle_run(inp)[:2]
    return inp


@pytest.fixture(scope="module")
def car_case():
    inp = er.autocar_inputs(3)
    inp["hist"] = er.oracle_run(inp, dyn=oekf.discrete_vehicle_dynamics, meas=oekf.vehicle_sensors_model)[:2]
    return inp


def _cases(gnss_case, car_case):
    return ((gnss_case, oekf.gnss_pos_and_bias), (car_case, oekf.discrete_vehicle_dynamics))


def test_reference_fixed_points(gnss_case, car_case):
    for inp, dyn in _cases(gnss_case, car_case):
        mh, Sh = inp["hist"]
        keep = mh.copy(), Sh.copy()
        ms, Ss = rts.smooth_batch(dyn, mh, Sh, inp["U"], inp["Q"], inp["dparams"])
        np.testing.assert_array_equal(mh, keep[0])                 # inputs untouched
        np.testing.assert_array_equal(Sh, keep[1])
        np.testing.assert_array_equal(ms[:, -1], mh[:, -1])        # the last step is the filtered one
        np.testing.assert_array_equal(Ss[:, -1], Sh[:, -1])
        assert np.abs(ms[:, :-1] - mh[:, :-1]).max() > 0           # and the pass does something
        m1, S1 = rts.smooth_batch(dyn, mh[:, :1], Sh[:, :1], inp["U"][:, :1], inp["Q"], inp["dparams"])
        np.testing.assert_array_equal(m1, mh[:, :1])               # T = 1 returns the input
        np.testing.assert_array_equal(S1, Sh[:, :1])
        # a prior adds one step and leaves the rest as it was
        p = rts.smooth_batch(dyn, mh, Sh, inp["U"], inp["Q"], inp["dparams"], inp["mu0"], inp["S0"])
        assert len(p) == 4 and p[2].shape == inp["mu0"].shape and p[3].shape == inp["S0"].shape
        np.testing.assert_array_equal(p[0], ms)
        np.testing.assert_array_equal(p[1], Ss)


def test_reference_smoothing_never_adds_uncertainty(gnss_case, car_case):
    for inp, dyn in _cases(gnss_case, car_case):
        mh, Sh = inp["hist"]
        _, Ss, _, S0s = rts.smooth_batch(dyn, mh, Sh, inp["U"], inp["Q"], inp["dparams"], inp["mu0"], inp["S0"])
        for S, Sm in ((Sh, Ss), (inp["S0"], S0s)):
            dS = S - Sm
            lo = np.linalg.eigvalsh(0.5 * (dS + np.swapaxes(dS, -1, -2))).min(-1)
            scale = np.abs(S).reshape(S.shape[:-2] + (-1,)).max(-1)
            print(f"min eig(S - Ss) / max|S| = {(lo / scale).min():.2e}")
            assert (lo >= -1e-9 * scale).all()
            assert (np.linalg.eigvalsh(0.5 * (Sm + np.swapaxes(Sm, -1, -2))) > 0).all()   # Ss stays positive definite


def test_reference_leaves_a_predict_only_run_unchanged(gnss_case, car_case):
    for inp, dyn, meas in ((gnss_case, oekf.gnss_pos_and_bias, oekf.multi_pseudorange),
                           (car_case, oekf.discrete_vehicle_dynamics, oekf.vehicle_sensors_model)):
        free = dict(inp, nz=np.zeros_like(inp["nz"]))
        mh, Sh, _ = er.oracle_run(free, dyn=dyn, meas=meas)
        ms, Ss = rts.smooth_batch(dyn, mh, Sh, inp["U"], inp["Q"], inp["dparams"])
        emu = np.abs(ms - mh).max(-1) / (1.0 + np.abs(mh).max(-1))
        eS = np.abs(Ss - Sh).reshape(Sh.shape[:2] + (-1,)).max(-1) / np.abs(Sh).reshape(Sh.shape[:2] + (-1,)).max(-1)
        print(f"predict-only: mu {emu.max():.2e}, S {eS.max():.2e}")
        assert emu.max() <= 1e-9 and eS.max() <= 1e-9


def test_reference_smoothed_fixture_positions_scatter_less():
    fx = er.gnss_fixture()
    T = fx["mu"].shape[0]
    ms, Ss = rts.smooth(oekf.gnss_pos_and_bias, fx["mu"], fx["S"], np.zeros((T, 3)), fx["Q"],
                        {"dt": float(fx["dt"])})
    f_std, s_std = fx["mu"][:, :3].std(0), ms[:, :3].std(0)
    print(f"position std per axis: filtered {f_std}, smoothed {s_std}; "
          f"tr S at step 0: {np.trace(fx['S'][0]):.2f} -> {np.trace(Ss[0]):.2f}")
    assert (s_std < f_std).all()
    assert np.trace(Ss[0]) < np.trace(fx["S"][0])


# ---------------------------------------------------------------- the host wrapper

def test_smooth_batch_refuses_before_loading_the_library(monkeypatch, gnss_case):
    def no_load(*a, **k):
        raise AssertionError("the library was loaded")
    monkeypatch.setattr(_lib, "load", no_load)
    inp = gnss_case
    mh, Sh = inp["hist"]
    U, Q = inp["U"], inp["Q"]
    good = (gnss.gnss_pos_and_bias, mh, Sh, U, Q, 1.0)
    for i, bad in ((1, mh[:, :, :4]), (1, mh[0]), (2, Sh[:, :, :, :4]), (2, Sh[:, :-1]), (3, U[:, :-1]), (3, U[:-1]),
                   (3, np.moveaxis(U, 0, -1)), (4, Q[:4, :4])):
        a = list(good)
        a[i] = bad
        with pytest.raises(ValueError):
            ekf.smooth_batch(*a)
    with pytest.raises(ValueError):
        ekf.smooth_batch(*good, inputs="batch_inner")              # U is batch-outermost
    with pytest.raises(ValueError):
        ekf.smooth_batch(*good, inputs="sideways")
    with pytest.raises(ValueError):
        ekf.smooth_batch(*good, mu0=inp["mu0"])                    # a prior is mu0 and S0
    with pytest.raises(ValueError):
        ekf.smooth_batch(*good, mu0=inp["mu0"][:-1], S0=inp["S0"])
    with pytest.raises(ValueError):
        ekf.smooth_batch("discrete_vehicle_dynamics", mh, Sh, U, Q, 1.0)   # n = 9 plug-in, n = 5 history

    def my_dyn(x, u, params=None, jac=False):
        return x, np.eye(5)
    with pytest.raises(UnsupportedPlugin):
        ekf.smooth_batch(my_dyn, mh, Sh, U, Q, 1.0)                # unregistered

    def gnss_pos_and_bias(x, u, params=None, jac=False):          # registered name, other math
        xn, J = oekf.gnss_pos_and_bias(x, u, params=params, jac=True)
        return xn + 1e-3, J
    with pytest.raises(UnsupportedPlugin):
        ekf.smooth_batch(gnss_pos_and_bias, mh, Sh, U, Q, 1.0)
    with pytest.raises(UnsupportedPlugin):
        ekf.smooth_batch("discrete_vehicle_dynamics", np.zeros((2, 3, 9)), np.zeros((2, 3, 9, 9)),
                         np.zeros((2, 3, 2)), np.eye(9), 0.1)       # car_params missing


def test_verify_keeps_its_behaviour_for_existing_callers():
    def gnss_pos_and_bias(x, u, params=None, jac=False):
        xn, J = oekf.gnss_pos_and_bias(x, u, params=params, jac=True)
        return xn, 2.0 * J
    with pytest.raises(UnsupportedPlugin):
        ekf.verify(gnss_pos_and_bias, gnss.multi_pseudorange, {"dt": 1.0})
    ekf.verify(gnss.gnss_pos_and_bias, gnss.multi_pseudorange, {"dt": 1.0})
    ekf.verify("gnss_pos_and_bias", "multi_pseudorange", {"dt": 1.0})
    ekf.verify_dynamics(oekf.gnss_pos_and_bias, {"dt": 0.5})       # the oracle's restatement is the same math
    with pytest.raises(UnsupportedPlugin):
        ekf.verify("gnss_pos_and_bias", "vehicle_sensors_model", {"dt": 1.0})   # not a compiled pair
