"""Batched unscented Kalman filter (mhe_ukf_run, utils.ukf): everything that needs no device.

  * the symbol is exported, declared in include/mhe.h and bound in mhe._lib; the ABI version did
    not move (nothing that existed changed);
  * the C entry point's refusals, which all precede the launch (host addresses, never read);
  * utils.ukf.run_batch and UKF(...) refuse bad alpha / beta / kappa before the library is loaded;
  * the conditions on tests/ukf_reference.py that tests/test_gpu_ukf.py relies on, and the
    correctness of that reference against the EKF oracle.
"""
import ctypes
import os
import re

import numpy as np
import pytest

import ekf_ragged as er
import ukf_reference as ur
from mhe import _lib
from oracle import ekf as oekf
import utils.ukf as ukf

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OK, E_DIMS, E_MODEL, E_NULL = 0, -1, -2, -5
CAR = [1.0e5, 1.2e5, 1500.0, 1.2, 1.4, 2500.0]
REQUIRED = ("mu", "S", "U", "Z", "nz", "PAR", "Q", "R")
INF, NAN = float("inf"), float("nan")


def _dims(model="gnss", **kw):
    d = _lib.MheEkfDims(n=5, m=3, pmax=12, q=3, dyn_model=1, meas_model=1, dt=1.0) if model == "gnss" else \
        _lib.MheEkfDims(n=9, m=2, pmax=8, q=3, dyn_model=2, meas_model=3, dt=0.1)
    if model == "car":
        for i, v in enumerate(CAR):
            d.dyn_par[i] = v
    for k, v in kw.items():
        setattr(d, k, v)
    return d


def _args(p=None, batch=4, steps=5, **kw):
    """mhe_ukf_args with every required pointer set to p (None: all NULL) and the default
    alpha, beta, kappa."""
    a = _lib.MheUkfArgs(batch=batch, steps=steps, alpha=1.0, beta=0.0, kappa=0.0)
    for name in REQUIRED:
        setattr(a, name, p)
    for k, v in kw.items():
        setattr(a, k, v)
    return a


def test_symbol_is_exported_declared_and_bound():
    lib = ctypes.CDLL(_lib.LIB_PATH)
    assert hasattr(lib, "mhe_ukf_run")
    hdr = open(os.path.join(ROOT, "include", "mhe.h")).read()
    assert re.search(r"\bint mhe_ukf_run\(const mhe_ekf_dims\* dims, const mhe_ukf_args\* args, void\* stream\);", hdr)
    assert "#define MHE_ABI_VERSION 11" in hdr
    assert "Batched unscented Kalman filter (added within v11; no existing struct or function changed)" in hdr
    res, args = _lib.SIGNATURES["mhe_ukf_run"]
    assert res is ctypes.c_int and len(args) == 3
    assert args[0] is ctypes.POINTER(_lib.MheEkfDims) and args[1] is ctypes.POINTER(_lib.MheUkfArgs)
    assert _lib.load().mhe_ukf_run.argtypes == args
    # the ctypes mirror declares the header's fields in the header's order
    m = re.search(r"typedef struct mhe_ukf_args \{(.*?)\} mhe_ukf_args;", hdr, re.S)
    body = re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S)
    names = [n for decl in body.split(";") for n in re.findall(r"(\w+)\s*(?:,|$)", decl.strip())]
    assert names == [f[0] for f in _lib.MheUkfArgs._fields_]
    # mhe_ekf_args' fields up to status, then the filter's own
    upto = [f[0] for f in _lib.MheEkfArgs._fields_].index("status") + 1
    assert _lib.MheUkfArgs._fields_[:upto] == _lib.MheEkfArgs._fields_[:upto]
    assert _lib.MheUkfArgs._fields_[upto:] == [("alpha", ctypes.c_double), ("beta", ctypes.c_double),
                                               ("kappa", ctypes.c_double), ("nis", ctypes.c_void_p),
                                               ("loglik", ctypes.c_void_p)]
    assert _lib.MheUkfArgs().struct_size == ctypes.sizeof(_lib.MheUkfArgs)


def test_refusals_precede_the_launch():
    run = _lib.load().mhe_ukf_run
    buf = (ctypes.c_double * 16)()
    p = ctypes.cast(buf, ctypes.c_void_p).value     # a host address: never dereferenced, nothing is launched
    d = _dims()
    assert run(None, ctypes.byref(_args(p)), None) == E_NULL
    assert run(ctypes.byref(d), None, None) == E_NULL                        # NULL struct
    good = _args(p)
    assert good.struct_size == ctypes.sizeof(_lib.MheUkfArgs)
    for size in (0, good.struct_size - 4, good.struct_size + 8, ctypes.sizeof(_lib.MheEkfArgs)):
        for batch in (4, 0):
            assert run(ctypes.byref(d), ctypes.byref(_args(p, batch=batch, struct_size=size)), None) == E_DIMS
    bad_abk = [dict(alpha=v) for v in (0.0, -1.0, -1e-300, NAN, INF, -INF)] + \
              [dict(beta=v) for v in (NAN, INF, -INF)] + [dict(kappa=v) for v in (NAN, INF, -INF)]
    for model in ("gnss", "car"):
        d = _dims(model)
        for bad in bad_abk + [dict(kappa=-float(d.n)), dict(kappa=-1.5 - d.n)]:           # n + kappa <= 0
            for batch in (4, 0):
                assert run(ctypes.byref(d), ctypes.byref(_args(p, batch=batch, **bad)), None) == E_DIMS, bad
        assert run(ctypes.byref(d), ctypes.byref(_args(None, batch=0, kappa=0.5 - d.n)), None) == OK   # n + kappa > 0
        for extra in ({}, {"alpha": 1.0, "beta": 2.0, "kappa": 1.0}, {"nis": p, "loglik": p}):
            assert run(ctypes.byref(d), ctypes.byref(_args(None, **extra)), None) == E_NULL
            for name in REQUIRED:                                            # any one required pointer missing
                assert run(ctypes.byref(d), ctypes.byref(_args(p, **dict(extra, **{name: None}))), None) == E_NULL, name
            assert run(ctypes.byref(d), ctypes.byref(_args(p, batch=-1, **extra)), None) == E_DIMS
            assert run(ctypes.byref(d), ctypes.byref(_args(p, steps=-1, **extra)), None) == E_DIMS
            assert run(ctypes.byref(d), ctypes.byref(_args(None, batch=0, **extra)), None) == OK   # empty: nothing is read
            assert run(ctypes.byref(d), ctypes.byref(_args(None, steps=0, **extra)), None) == OK
            for pmax in (0, 33, 64):
                assert run(ctypes.byref(_dims(model, pmax=pmax)), ctypes.byref(_args(p, **extra)), None) == E_DIMS
            assert run(ctypes.byref(_dims(model, q=2)), ctypes.byref(_args(p, **extra)), None) == E_DIMS
            for size in (0, d.struct_size - 4, d.struct_size + 8):
                assert run(ctypes.byref(_dims(model, struct_size=size)), ctypes.byref(_args(p, **extra)), None) == E_DIMS
    for bad in (dict(dyn_model=0), dict(dyn_model=3), dict(n=9), dict(m=2), dict(meas_model=3), dict(meas_model=0)):
        assert run(ctypes.byref(_dims("gnss", **bad)), ctypes.byref(_args(p)), None) == E_MODEL, bad
    for bad in (dict(n=5), dict(meas_model=1), dict(dyn_model=7)):
        assert run(ctypes.byref(_dims("car", **bad)), ctypes.byref(_args(p)), None) == E_MODEL, bad
    for i in (2, 5):                                                         # the vehicle's M / I_Z unset
        d = _dims("car")
        d.dyn_par[i] = 0.0
        assert run(ctypes.byref(d), ctypes.byref(_args(p)), None) == E_DIMS


BAD_ABK = [dict(alpha=v) for v in (0, 0.0, -1.0, NAN, INF, "1", None, True, [1.0])] + \
          [dict(beta=v) for v in (NAN, INF, -INF, "0", None, False)] + \
          [dict(kappa=v) for v in (NAN, INF, -5.0, -7, "0", None)]


def test_python_refuses_bad_parameters_before_loading_the_library(monkeypatch):
    def no_load(*a, **k):
        raise AssertionError("the library was loaded")
    monkeypatch.setattr(_lib, "load", no_load)
    inp = er.gnss_inputs(2, T=6)
    U, Z, nz, sat = er.device_args(inp)
    for bad in BAD_ABK:
        with pytest.raises(ValueError):
            ukf.run_batch("gnss_pos_and_bias", "multi_pseudorange", inp["mu0"], inp["S0"], U, Z, nz, inp["Q"],
                          inp["R"], 1.0, sat, **bad)
        with pytest.raises(ValueError):
            ukf.UKF("gnss_pos_and_bias", "multi_pseudorange", inp["mu0"][0], inp["S0"][0], **bad)
    with pytest.raises(ValueError):                                          # n + kappa <= 0 for the car's n = 9 only
        ukf.UKF("discrete_vehicle_dynamics", "vehicle_sensors_model", np.zeros(9), np.eye(9), kappa=-9.0)
    f = ukf.UKF("gnss_pos_and_bias", "multi_pseudorange", inp["mu0"][0], inp["S0"][0])
    assert (f.alpha, f.beta, f.kappa) == (1.0, 0.0, 0.0)                     # lambda = 0: no negative weight
    assert ukf.sigma_params(1, 2, np.float64(1.0), 5) == (1.0, 2.0, 1.0)
    assert ukf.sigma_params(1e-3, 2.0, -4.5, 5) == (1e-3, 2.0, -4.5)
    import inspect
    sig = inspect.signature(ukf.run_batch).parameters
    assert [sig[k].default for k in ("alpha", "beta", "kappa")] == [1.0, 0.0, 0.0]
    assert "method" not in sig and "gate" not in sig
    assert "negative weight" in ukf.__doc__ and "1e-3" in ukf.__doc__


# ---------------------------------------------------------------- the reference itself

def test_plugin_values_are_the_oracles():
    """The dtype-generic plug-in values of the reference equal oracle/ekf.py's in float64."""
    rng = np.random.default_rng(5)
    car = ur.inputs("car")
    for _ in range(4):
        x5, u3, sat = rng.normal(size=5) * 10, rng.normal(size=3), rng.normal(size=(6, 3)) * 2e4
        got = ur.dyn_value(ur.KIND["gnss"], x5[None, None], u3[None], {"dparams": {"dt": 0.7}}, np.float64)[0, 0]
        np.testing.assert_array_equal(got, oekf.gnss_pos_and_bias(x5, u3, {"dt": 0.7}))
        np.testing.assert_array_equal(ur.meas_value(ur.KIND["gnss"], x5[None, None], sat[None], np.array([6]))[0, 0],
                                      oekf.multi_pseudorange(x5, {"sat_pos": sat}))
        np.testing.assert_array_equal(ur.meas_value(ur.KIND["bias"], x5[None, None], sat[None], np.array([6]))[0, 0],
                                      oekf.multi_pseudorange_and_bias(x5, {"sat_pos": sat[:5]}))
        x9, u2 = rng.normal(size=9), rng.normal(size=2) * 0.1
        x9[3] = 5.0 + abs(x9[3])
        got = ur.dyn_value(ur.KIND["car"], x9[None, None], u2[None], car, np.float64)[0, 0]
        np.testing.assert_allclose(got, oekf.discrete_vehicle_dynamics(x9, u2, car["dparams"]), rtol=1e-14, atol=0)
        np.testing.assert_array_equal(ur.meas_value(ur.KIND["car"], x9[None, None], sat[None], np.array([6]))[0, 0],
                                      oekf.vehicle_sensors_model(x9, {"sat_pos": sat}))


def test_own_cholesky_and_forward_substitution():
    rng = np.random.default_rng(6)
    M = rng.normal(size=(3, 7, 7))
    A = M @ M.transpose(0, 2, 1) + np.eye(7)
    act = np.arange(7)[None, :] < np.array([7, 4, 1])[:, None]
    L, ok, margin = ur.cholesky(A.astype(np.longdouble), act)
    assert L.dtype == np.longdouble and ok.all() and (margin > 0).all()
    for b, k in enumerate((7, 4, 1)):
        np.testing.assert_allclose(L[b, :k, :k].astype(float), np.linalg.cholesky(A[b, :k, :k]), rtol=1e-12)
        np.testing.assert_array_equal(L[b, k:, k:].astype(float), np.eye(7 - k))
    rhs = rng.normal(size=(3, 7, 2))
    Y = ur.forward(L, rhs.astype(np.longdouble))
    np.testing.assert_allclose(np.einsum("bij,bjk->bik", L, Y).astype(float), rhs, atol=1e-13)
    A[1, 2, 2] = -1.0
    _, ok, margin = ur.cholesky(A, act)
    assert ok.tolist() == [True, False, True] and margin[1] == -np.inf


@pytest.mark.parametrize("params", ur.PARAMS)
@pytest.mark.parametrize("name", ur.CASES)
def test_conditions_the_device_test_relies_on(name, params):
    r = ur.reference(name, params)
    print(f"{name} {params}: floors {r['floor']}, bounds {r['bound']}, smallest pivot / diagonal {r['margin']:.2e}, "
          f"smallest sigma-point x[3] {r['min_vx']:.3f}")
    assert not r["status"].any() and not r["f64"]["status"].any()
    assert (r["f64"]["fail_step"] == -1).all()
    # device and reference cannot disagree about status: no pivot is anywhere near zero
    assert r["margin"] > 1e-6
    if name == "car":
        assert r["min_vx"] > 0.0           # no sigma point crosses the tyre model's pole at vx = 0
    for key in ur.OUTPUTS:
        assert np.isfinite(r[key]).all() and 0.0 < r["floor"][key] < r["bound"][key]
    nz = ur.inputs(name)["nz"]
    assert set(er.EDGE_COUNTS) <= set(nz.ravel().tolist()) or name in ("bias", "car")
    assert (nz == 0).any() and not r["nis"][nz == 0].any() and not r["loglik"][nz == 0].any()
    assert (r["nis"][nz > 0] > 0).all()
    np.testing.assert_array_equal(r["S"], np.swapaxes(r["S"], -1, -2))


def test_weights():
    for (a, b, k), lam, w0m, w0c in (((1.0, 0.0, 0.0), 0.0, 0.0, 0.0), ((1.0, 2.0, 1.0), 1.0, 1 / 6, 1 / 6 + 1 - 1 + 2.0)):
        c, wm, wc = ur.weights(a, b, k, 5, np.float64)
        assert c == np.sqrt(5 + lam) and wm[0] == w0m and wc[0] == w0c
        assert np.all(wm[1:] == 1 / (2 * (5 + lam))) and np.all(wc[1:] == wm[1:]) and abs(wm.sum() - 1) < 1e-15


def test_reference_reproduces_the_ekf_where_the_models_are_linear():
    """gnss: pseudoranges are linear up to curvature far below the floor, so the unscented and
    the extended filter agree within the case's bound."""
    inp, r = ur.inputs("gnss"), ur.reference("gnss")
    mu, S, spd = er.oracle_run(inp)
    assert spd.all()
    dmu, dS = np.abs(r["mu"] - mu).max(), np.abs(r["S"] - S).max()
    print(f"UKF reference against the EKF oracle, gnss: mu {dmu:.2e} (bound {r['bound']['mu']:.2e}), "
          f"S {dS:.2e} (bound {r['bound']['S']:.2e})")
    assert dmu <= r["bound"]["mu"] and dS <= r["bound"]["S"]


def test_the_bias_row_acts():
    """bias: the EKF's bias row has an all-zero Jacobian row and corrects nothing; here it acts,
    and the clock state differs by far more than a metre."""
    inp, r = ur.inputs("bias"), ur.reference("bias")
    mu, _, _ = er.oracle_run(inp, meas=oekf.multi_pseudorange_and_bias, extra=1)
    d = np.abs(r["mu"] - mu)[..., 3].max()
    print(f"UKF reference against the EKF oracle, bias: clock state differs by {d:.1f} m")
    assert d > 1.0
