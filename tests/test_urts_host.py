"""Unscented RTS smoother (mhe_ukf_smooth, utils.ukf.smooth_batch): everything that needs no device.

  * the symbol is exported, declared in include/mhe.h and bound in mhe._lib; the ABI version did
    not move (nothing that existed changed);
  * the C entry point's refusals, which all precede the launch (host addresses, never read);
  * utils.ukf.smooth_batch refuses bad parameters and shapes before the library is loaded;
  * the conditions on tests/urts_reference.py that tests/test_gpu_urts.py relies on, and the
    correctness of that reference: against the textbook smoother where the dynamics are linear,
    far from it on the car, and the covariance properties of a smoother.
"""
import ctypes
import os
import re

import numpy as np
import pytest

import rts_reference as rts
import ukf_reference as ur
import urts_reference as urts
from mhe import _lib
from mhe.registry import UnsupportedPlugin
from oracle import ekf as oekf
import utils.ukf as ukf

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OK, E_DIMS, E_MODEL, E_NULL = 0, -1, -2, -5
CAR = [1.0e5, 1.2e5, 1500.0, 1.2, 1.4, 2500.0]
REQUIRED = ("mu_hist", "S_hist", "U", "Q", "mu_s", "S_s")
INF, NAN = float("inf"), float("nan")
ODYN = {"gnss": oekf.gnss_pos_and_bias, "corr": oekf.gnss_pos_and_bias, "bias": oekf.gnss_pos_and_bias,
        "car": oekf.discrete_vehicle_dynamics}
ALL = [(name, params) for name in ur.CASES for params in ur.PARAMS]


def _dims(model="gnss", **kw):
    d = _lib.MheEkfDims(n=5, m=3, dyn_model=1, dt=1.0) if model == "gnss" else \
        _lib.MheEkfDims(n=9, m=2, dyn_model=2, dt=0.1)
    if model == "car":
        for i, v in enumerate(CAR):
            d.dyn_par[i] = v
    for k, v in kw.items():
        setattr(d, k, v)
    return d


def _args(p=None, batch=4, steps=5, **kw):
    """mhe_ukf_smooth_args with every required pointer set to p (None: all NULL) and the
    default alpha, beta, kappa."""
    a = _lib.MheUkfSmoothArgs(batch=batch, steps=steps, alpha=1.0, beta=0.0, kappa=0.0)
    for name in REQUIRED:
        setattr(a, name, p)
    for k, v in kw.items():
        setattr(a, k, v)
    return a


def test_symbol_is_exported_declared_and_bound():
    lib = ctypes.CDLL(_lib.LIB_PATH)
    assert hasattr(lib, "mhe_ukf_smooth")
    hdr = open(os.path.join(ROOT, "include", "mhe.h")).read()
    assert re.search(r"\bint mhe_ukf_smooth\(const mhe_ekf_dims\* dims, const mhe_ukf_smooth_args\* args, "
                     r"void\* stream\);", hdr)
    assert "#define MHE_ABI_VERSION 11" in hdr
    res, args = _lib.SIGNATURES["mhe_ukf_smooth"]
    assert res is ctypes.c_int and len(args) == 3
    assert args[0] is ctypes.POINTER(_lib.MheEkfDims) and args[1] is ctypes.POINTER(_lib.MheUkfSmoothArgs)
    assert _lib.load().mhe_ukf_smooth.argtypes == args
    # the ctypes mirror declares the header's fields in the header's order, with the header's types
    m = re.search(r"typedef struct mhe_ukf_smooth_args \{(.*?)\} mhe_ukf_smooth_args;", hdr, re.S)
    body = re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S)
    kinds = {"int32_t": ctypes.c_int32, "int64_t": ctypes.c_int64, "double": ctypes.c_double}
    fields = []
    for decl in body.split(";"):
        decl = decl.strip()
        if not decl:
            continue
        base = re.match(r"(?:const\s+)?(\w+)", decl).group(1)
        ptr = "*" in decl
        for name in re.findall(r"(\w+)\s*(?:,|$)", decl):
            fields.append((name, ctypes.c_void_p if ptr else kinds[base]))
    assert fields == list(_lib.MheUkfSmoothArgs._fields_)
    assert [f[0] for f in fields] == ["struct_size", "batch", "steps", "mu_hist", "S_hist", "U", "u_bstride", "Q",
                                      "mu0", "S0", "mu_s", "S_s", "mu0_s", "S0_s", "status", "alpha", "beta", "kappa"]
    # the header's sizeof: 3 x int32 (+ 4 bytes of padding before the first pointer), 11 pointers,
    # one int64 and 3 doubles, all 8-aligned
    assert ctypes.sizeof(_lib.MheUkfSmoothArgs) == 16 + 8 * (11 + 1 + 3)
    assert _lib.MheUkfSmoothArgs().struct_size == ctypes.sizeof(_lib.MheUkfSmoothArgs)
    # nothing that existed moved
    assert ctypes.sizeof(_lib.MheUkfArgs) == 16 + 8 * 22 and len(_lib.SIGNATURES["mhe_ekf_smooth"][1]) == 16


def test_refusals_precede_the_launch():
    run = _lib.load().mhe_ukf_smooth
    buf = (ctypes.c_double * 16)()
    p = ctypes.cast(buf, ctypes.c_void_p).value     # a host address: never dereferenced, nothing is launched
    d = _dims()
    assert run(None, ctypes.byref(_args(p)), None) == E_NULL
    assert run(ctypes.byref(d), None, None) == E_NULL                        # NULL struct
    good = _args(p)
    assert good.struct_size == ctypes.sizeof(_lib.MheUkfSmoothArgs)
    for size in (0, good.struct_size - 4, good.struct_size + 8, ctypes.sizeof(_lib.MheUkfArgs)):
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
        for extra in ({}, {"alpha": 1.0, "beta": 2.0, "kappa": 1.0}, {"status": p}):
            assert run(ctypes.byref(d), ctypes.byref(_args(None, **extra)), None) == E_NULL
            for name in REQUIRED:                                            # any one required pointer missing
                assert run(ctypes.byref(d), ctypes.byref(_args(p, **dict(extra, **{name: None}))), None) == E_NULL, name
            # a smoothed prior without the prior
            for outs, priors in ((("mu0_s",), ()), (("S0_s",), ()), (("mu0_s", "S0_s"), ("mu0",)),
                                 (("mu0_s", "S0_s"), ("S0",)), (("mu0_s",), ("S0",))):
                kw = dict(extra, **{k: p for k in outs + priors})
                assert run(ctypes.byref(d), ctypes.byref(_args(p, **kw)), None) == E_NULL, (outs, priors)
            assert run(ctypes.byref(d), ctypes.byref(_args(p, batch=-1, **extra)), None) == E_DIMS
            assert run(ctypes.byref(d), ctypes.byref(_args(p, steps=-1, **extra)), None) == E_DIMS
            assert run(ctypes.byref(d), ctypes.byref(_args(None, batch=0, **extra)), None) == OK   # empty: nothing is read
            assert run(ctypes.byref(d), ctypes.byref(_args(None, steps=0, **extra)), None) == OK
            for size in (0, d.struct_size - 4, d.struct_size + 8):
                e = _dims(model, struct_size=size)
                assert run(ctypes.byref(e), ctypes.byref(_args(p, **extra)), None) == E_DIMS
                assert run(ctypes.byref(e), ctypes.byref(_args(None, batch=0, **extra)), None) == E_DIMS
        # fields the smoother does not read may hold anything
        e = _dims(model, pmax=999, q=-7, meas_model=55, r_diag=3)
        assert run(ctypes.byref(e), ctypes.byref(_args(None, batch=0)), None) == OK
        assert run(ctypes.byref(e), ctypes.byref(_args(None)), None) == E_NULL
    for bad in (dict(dyn_model=0), dict(dyn_model=3), dict(n=9), dict(m=2), dict(n=4, m=3)):
        assert run(ctypes.byref(_dims("gnss", **bad)), ctypes.byref(_args(p)), None) == E_MODEL, bad
    for bad in (dict(n=5), dict(m=3), dict(dyn_model=7)):
        assert run(ctypes.byref(_dims("car", **bad)), ctypes.byref(_args(p)), None) == E_MODEL, bad
    for i in (2, 5):                                                         # the vehicle's M / I_Z unset
        d = _dims("car")
        d.dyn_par[i] = 0.0
        assert run(ctypes.byref(d), ctypes.byref(_args(p)), None) == E_DIMS
        assert run(ctypes.byref(d), ctypes.byref(_args(None)), None) == E_DIMS


BAD_ABK = [dict(alpha=v) for v in (0, 0.0, -1.0, NAN, INF, "1", None, True, [1.0])] + \
          [dict(beta=v) for v in (NAN, INF, -INF, "0", None, False)] + \
          [dict(kappa=v) for v in (NAN, INF, -5.0, -7, "0", None)]


def test_python_refuses_before_loading_the_library(monkeypatch):
    def no_load(*a, **k):
        raise AssertionError("the library was loaded")
    monkeypatch.setattr(_lib, "load", no_load)
    inp = ur.inputs("gnss")
    mh, Sh = (a[:6] for a in urts.history("gnss"))
    U, Q, mu0, S0 = inp["U"][:6], inp["Q"], inp["mu0"][:6], inp["S0"][:6]
    good = ("gnss_pos_and_bias", mh, Sh, U, Q, 1.0)
    for bad in BAD_ABK:
        with pytest.raises(ValueError):
            ukf.smooth_batch(*good, **bad)
    with pytest.raises(ValueError):                                          # n + kappa <= 0 for the car's n = 9 only
        ukf.smooth_batch("discrete_vehicle_dynamics", np.zeros((2, 3, 9)), np.zeros((2, 3, 9, 9)),
                         np.zeros((2, 3, 2)), np.eye(9), 0.1, kappa=-9.0)
    for i, bad in ((1, mh[:, :, :4]), (1, mh[0]), (2, Sh[:, :, :, :4]), (2, Sh[:, :-1]), (3, U[:, :-1]), (3, U[:-1]),
                   (3, np.moveaxis(U, 0, -1)), (4, Q[:4, :4])):
        a = list(good)
        a[i] = bad
        with pytest.raises(ValueError):
            ukf.smooth_batch(*a)
    with pytest.raises(ValueError):
        ukf.smooth_batch(*good, inputs="batch_inner")              # U is batch-outermost
    with pytest.raises(ValueError):
        ukf.smooth_batch(*good, inputs="sideways")
    with pytest.raises(ValueError):
        ukf.smooth_batch(*good, mu0=mu0)                           # a prior is mu0 and S0
    with pytest.raises(ValueError):
        ukf.smooth_batch(*good, S0=S0)
    with pytest.raises(ValueError):
        ukf.smooth_batch(*good, mu0=mu0[:-1], S0=S0)
    with pytest.raises(ValueError):
        ukf.smooth_batch("discrete_vehicle_dynamics", mh, Sh, U, Q, 1.0)   # n = 9 plug-in, n = 5 history

    # the dynamics plug-in is resolved and verified as utils.ekf.smooth_batch does
    def my_dyn(x, u, params=None, jac=False):
        return x, np.eye(5)
    with pytest.raises(UnsupportedPlugin):
        ukf.smooth_batch(my_dyn, mh, Sh, U, Q, 1.0)                # unregistered

    def gnss_pos_and_bias(x, u, params=None, jac=False):          # registered name, other math
        xn, J = oekf.gnss_pos_and_bias(x, u, params=params, jac=True)
        return xn + 1e-3, J
    with pytest.raises(UnsupportedPlugin):
        ukf.smooth_batch(gnss_pos_and_bias, mh, Sh, U, Q, 1.0)
    with pytest.raises(UnsupportedPlugin):
        ukf.smooth_batch("discrete_vehicle_dynamics", np.zeros((2, 3, 9)), np.zeros((2, 3, 9, 9)),
                         np.zeros((2, 3, 2)), np.eye(9), 0.1)       # car_params missing
    import inspect
    sig = inspect.signature(ukf.smooth_batch).parameters
    assert list(sig) == ["dyn_func", "mu_hist", "S_hist", "U", "Q", "dt", "mu0", "S0", "dyn_params", "inputs", "alpha",
                         "beta", "kappa", "device", "stream"]
    assert [sig[k].default for k in ("alpha", "beta", "kappa", "inputs")] == [1.0, 0.0, 0.0, "batch_outer"]
    assert "unscented RTS pass" not in ukf.__doc__ and "smooth_batch" in ukf.__doc__


# ---------------------------------------------------------------- the reference itself

def test_own_back_substitution():
    rng = np.random.default_rng(8)
    M = rng.normal(size=(3, 7, 7))
    A = M @ M.transpose(0, 2, 1) + np.eye(7)
    L, ok, _ = ur.cholesky(A.astype(np.longdouble), np.ones((3, 7), dtype=bool))
    assert ok.all()
    rhs = rng.normal(size=(3, 7, 4))
    X = urts.backward(L, ur.forward(L, rhs.astype(np.longdouble)))
    assert X.dtype == np.longdouble
    np.testing.assert_allclose(np.einsum("bij,bjk->bik", A, X.astype(float)), rhs, atol=1e-12)
    np.testing.assert_allclose(X.astype(float), np.linalg.solve(A, rhs), atol=1e-12)
    S = rng.normal(size=(2, 4, 4))
    np.testing.assert_array_equal(urts.mirror(S), np.swapaxes(urts.mirror(S), 1, 2))
    np.testing.assert_array_equal(np.triu(urts.mirror(S)), np.triu(S))


@pytest.mark.parametrize("name,params", ALL)
def test_conditions_the_device_test_relies_on(name, params):
    r = urts.reference(name, params)
    print(f"{name} {params}: floors {r['floor']}, bounds {r['bound']}, smallest pivot / diagonal {r['margin']:.3e}")
    assert not r["status"].any() and not r["f64"]["status"].any()          # both dtypes end with status 0
    T = urts.history(name, params)[0].shape[1]
    assert T == (61 if name == "car" else 12) and urts.history(name, params)[0].shape[0] == ur.B == 70
    assert (r["f64"]["fail_step"] == T).all()
    # device and reference cannot disagree about status: no pivot of S_k or S- is anywhere near zero
    assert r["margin"] >= 0.05
    for key in urts.OUTPUTS:
        assert np.isfinite(r[key]).all() and 0.0 < r["floor"][key] < r["bound"][key]
    mh, Sh = urts.history(name, params)
    np.testing.assert_array_equal(r["S_s"], np.swapaxes(r["S_s"], -1, -2))
    np.testing.assert_array_equal(r["S0_s"], np.swapaxes(r["S0_s"], -1, -2))
    np.testing.assert_array_equal(r["mu_s"][:, -1], mh[:, -1])               # the last step is the filtered one
    np.testing.assert_array_equal(r["S_s"][:, -1], Sh[:, -1])
    assert np.abs(r["mu_s"][:, :-1] - mh[:, :-1]).max() > 0                  # and the pass does something
    # without the prior the steps are the same and nothing else is returned
    inp, kind = ur.inputs(name), ur.KIND[name]
    if params == ur.PARAMS[0]:
        o = urts.smooth(inp, kind, mh, Sh, params, prior=False)
        assert o["mu0_s"] is None and o["S0_s"] is None
        np.testing.assert_array_equal(o["mu_s"], r["f64"]["mu_s"])
        np.testing.assert_array_equal(o["S_s"], r["f64"]["S_s"])


def _ekf_smoother(name, params):
    inp = ur.inputs(name)
    mh, Sh = urts.history(name, params)
    return rts.smooth_batch(ODYN[name], mh, Sh, inp["U"], inp["Q"], inp["dparams"], inp["mu0"], inp["S0"])


@pytest.mark.parametrize("params", ur.PARAMS)
@pytest.mark.parametrize("name", ["gnss", "corr"])
def test_linear_dynamics_reproduce_the_textbook_smoother(name, params):
    """gnss_pos_and_bias is linear, so the unscented transform of the prediction is exact and the
    unscented smoother is the RTS smoother with the true Jacobian, within the case's bound."""
    r = urts.reference(name, params)
    for key, want in zip(urts.OUTPUTS, _ekf_smoother(name, params)):
        err = float(np.abs(r[key] - want).max())
        print(f"{name} {params} {key}: against rts_reference {err:.2e} (floor {r['floor'][key]:.2e}, "
              f"bound {r['bound'][key]:.2e})")
        assert err <= r["bound"][key], (key, err, r["bound"][key])


@pytest.mark.parametrize("params", ur.PARAMS)
def test_the_car_differs_from_the_ekf_linearised_smoother(params):
    r = urts.reference("car", params)
    for key, want in zip(urts.OUTPUTS, _ekf_smoother("car", params)):
        d = float(np.abs(r[key] - want).max())
        print(f"car {params} {key}: unscented against EKF-linearised smoother of the same history {d:.3g} "
              f"(bound {r['bound'][key]:.2e}, ratio {d / r['bound'][key]:.2e})")
        assert d > 1000.0 * r["bound"][key], (key, d, r["bound"][key])


@pytest.mark.parametrize("name,params", ALL)
def test_smoothing_never_adds_uncertainty(name, params):
    r = urts.reference(name, params)
    inp = ur.inputs(name)
    _, Sh = urts.history(name, params)
    for S, Sm in ((Sh, r["S_s"]), (inp["S0"], r["S0_s"])):
        dS = S - Sm
        lo = np.linalg.eigvalsh(0.5 * (dS + np.swapaxes(dS, -1, -2))).min(-1)
        scale = np.abs(S).reshape(S.shape[:-2] + (-1,)).max(-1)
        print(f"{name} {params}: min eig(S - Ss) / max|S| = {(lo / scale).min():.2e}")
        assert (lo / scale >= -1e-12).all()
        assert (np.linalg.eigvalsh(Sm) > 0).all()                             # Ss stays positive definite
    tr_f, tr_s = np.trace(Sh[:, 0], axis1=-2, axis2=-1).mean(), np.trace(r["S_s"][:, 0], axis1=-2, axis2=-1).mean()
    print(f"{name} {params}: mean tr S at step 0: filtered {tr_f:.3f}, smoothed {tr_s:.3f}")
    assert tr_s < tr_f


def test_failure_rule():
    """The four defects tests/test_gpu_urts.py plants: where the reference fails them."""
    inp, kind = dict(ur.inputs("gnss")), ur.KIND["gnss"]
    mh, Sh = (a.copy() for a in urts.history("gnss"))
    T = mh.shape[1]
    healthy = urts.reference("gnss")["f64"]
    inp["S0"] = inp["S0"].copy()
    Sh[5, 4, 0, 0] = -1.0
    mh[69, 7, 1] = np.nan
    mh[33, T - 1, 0] = np.inf
    inp["S0"][12, 0, 0] = -1.0
    o = urts.smooth(inp, kind, mh, Sh)
    want = {5: 4, 69: 7, 33: T - 1, 12: -1}
    assert sorted(np.flatnonzero(o["status"]).tolist()) == sorted(want)
    for b in range(ur.B):
        k = want.get(b, None)
        if k is None:
            assert o["fail_step"][b] == T
            for key in urts.OUTPUTS:
                np.testing.assert_array_equal(o[key][b], healthy[key][b])
            continue
        assert o["fail_step"][b] == k
        assert np.isnan(o["mu_s"][b, :k + 1]).all() and np.isnan(o["S_s"][b, :k + 1]).all()
        assert np.isnan(o["mu0_s"][b]).all() and np.isnan(o["S0_s"][b]).all()
        np.testing.assert_array_equal(o["mu_s"][b, k + 1:], healthy["mu_s"][b, k + 1:])
        np.testing.assert_array_equal(o["S_s"][b, k + 1:], healthy["S_s"][b, k + 1:])
