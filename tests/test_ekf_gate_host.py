"""Innovation gating and likelihood outputs of the batched EKF (mhe_ekf_run_args,
utils.ekf.run_batch(gate=, innovations=)): everything that needs no device.

  * the symbol is exported, declared in include/mhe.h and bound in mhe._lib; the ABI version
    did not move (nothing that existed changed);
  * the C entry point's refusals, which all precede the launch (NULL device pointers), those of
    mhe_ekf_run reached through the new entry included;
  * utils.ekf.run_batch refuses a bad gate before it loads the library;
  * properties of tests/ekf_gate_reference.py, the reference of tests/test_gpu_ekf_gate.py, on
    that file's inputs.
"""
import ctypes
import os
import re

import numpy as np
import pytest

import ekf_gate_reference as gr
import ekf_ragged as er
from mhe import _lib
from oracle import ekf as oekf
import utils.ekf as ekf
import utils.gnss as gnss

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OK, E_DIMS, E_MODEL, E_NULL = 0, -1, -2, -5
CAR = [1.0e5, 1.2e5, 1500.0, 1.2, 1.4, 2500.0]
REQUIRED = ("mu", "S", "U", "Z", "nz", "PAR", "Q", "R")


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
    """mhe_ekf_args with every required pointer set to p (None: all NULL)."""
    a = _lib.MheEkfArgs(batch=batch, steps=steps)
    for name in REQUIRED:
        setattr(a, name, p)
    for k, v in kw.items():
        setattr(a, k, v)
    return a


def test_symbol_is_exported_declared_and_bound():
    lib = ctypes.CDLL(_lib.LIB_PATH)
    assert hasattr(lib, "mhe_ekf_run_args")
    hdr = open(os.path.join(ROOT, "include", "mhe.h")).read()
    assert re.search(r"\bint mhe_ekf_run_args\(const mhe_ekf_dims\* dims, const mhe_ekf_args\* args, void\* stream\);",
                     hdr)
    assert "#define MHE_ABI_VERSION 11" in hdr
    assert "added within v11; no existing struct or function" in hdr
    res, args = _lib.SIGNATURES["mhe_ekf_run_args"]
    assert res is ctypes.c_int and len(args) == 3
    assert args[0] is ctypes.POINTER(_lib.MheEkfDims) and args[1] is ctypes.POINTER(_lib.MheEkfArgs)
    assert _lib.load().mhe_ekf_run_args.argtypes == args
    # the ctypes mirror declares the header's fields in the header's order
    m = re.search(r"typedef struct mhe_ekf_args \{(.*?)\} mhe_ekf_args;", hdr, re.S)
    body = re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S)
    names = [n for decl in body.split(";") for n in re.findall(r"(\w+)\s*(?:,|$)", decl.strip())]
    assert names == [f[0] for f in _lib.MheEkfArgs._fields_]
    assert _lib.MheEkfArgs._fields_[-4:] == [("gate", ctypes.c_double), ("nis", ctypes.c_void_p),
                                             ("loglik", ctypes.c_void_p), ("rej", ctypes.c_void_p)]


def test_refusals_precede_the_launch():
    run = _lib.load().mhe_ekf_run_args
    buf = (ctypes.c_double * 16)()
    p = ctypes.cast(buf, ctypes.c_void_p).value     # a host address: never dereferenced, nothing is launched
    d = _dims()
    assert run(None, ctypes.byref(_args(p)), None) == E_NULL
    assert run(ctypes.byref(d), None, None) == E_NULL                        # NULL struct
    good = _args(p)
    assert good.struct_size == ctypes.sizeof(_lib.MheEkfArgs)
    for size in (0, good.struct_size - 4, good.struct_size + 8):
        for batch in (4, 0):
            assert run(ctypes.byref(d), ctypes.byref(_args(p, batch=batch, struct_size=size)), None) == E_DIMS
    for gate in (float("nan"), -1.0, -1e-300, -float("inf")):
        for batch in (4, 0):
            assert run(ctypes.byref(d), ctypes.byref(_args(p, batch=batch, gate=gate)), None) == E_DIMS, gate
    for model in ("gnss", "car"):
        d = _dims(model)
        # mhe_ekf_run's refusals, reached through the new entry, with and without a gate
        for extra in ({}, {"gate": 10.83}, {"gate": float("inf"), "nis": p}):
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
        assert run(ctypes.byref(_dims("gnss", **bad)), ctypes.byref(_args(p, gate=1.0)), None) == E_MODEL, bad
    for bad in (dict(n=5), dict(meas_model=1), dict(dyn_model=7)):
        assert run(ctypes.byref(_dims("car", **bad)), ctypes.byref(_args(p, gate=1.0)), None) == E_MODEL, bad
    for i in (2, 5):                                                         # the vehicle's M / I_Z unset
        d = _dims("car")
        d.dyn_par[i] = 0.0
        assert run(ctypes.byref(d), ctypes.byref(_args(p, gate=1.0)), None) == E_DIMS


def test_the_old_entry_keeps_its_refusals():
    run = _lib.load().mhe_ekf_run
    # mu, S, U, u_bs, Z, z_bs, nz, nz_bs, PAR, par_bs, Q, R, r_bs, r_ss, mu_hist, S_hist, status, stream
    nul = [None, None, None, 0, None, 0, None, 0, None, 0, None, None, 0, 0, None, None, None, None]
    d = _dims()
    assert run(None, 4, 5, *nul) == E_NULL
    assert run(ctypes.byref(d), 4, 5, *nul) == E_NULL
    assert run(ctypes.byref(d), 0, 5, *nul) == OK and run(ctypes.byref(d), 4, 0, *nul) == OK
    assert run(ctypes.byref(d), -1, 5, *nul) == E_DIMS
    assert run(ctypes.byref(_dims(pmax=64)), 4, 5, *nul) == E_DIMS
    assert run(ctypes.byref(_dims(struct_size=8)), 0, 5, *nul) == E_DIMS


def test_run_batch_refuses_a_bad_gate_before_loading_the_library(monkeypatch):
    def no_load(*a, **k):
        raise AssertionError("the library was loaded")
    monkeypatch.setattr(_lib, "load", no_load)
    inp = er.gnss_inputs(2, T=6)
    U, Z, nz, sat = er.device_args(inp)
    for bad in (0, 0.0, -1.0, float("nan"), -np.inf, "10.83", True, [10.83], np.array([1.0, 2.0])):
        with pytest.raises(ValueError):
            ekf.run_batch(gnss.gnss_pos_and_bias, gnss.multi_pseudorange, inp["mu0"], inp["S0"], U, Z, nz, inp["Q"],
                          inp["R"], 1.0, sat, gate=bad)
        f = ekf.EKF(gnss.gnss_pos_and_bias, gnss.multi_pseudorange, inp["mu0"][0], inp["S0"][0])
        with pytest.raises(ValueError):
            f.update(U[0, 0], Z[0, 0, :4], inp["Q"], inp["R"][0, 0, :4, :4], {"dt": 1.0}, None,
                     {"sat_pos": sat[0, 0, :4]}, gate=bad)
    for good in (10.83, np.inf, 1, np.float64(0.5), 1e300):
        assert ekf._gate_value(good) == float(good)
    assert ekf._gate_value(None) == 0.0


# ---------------------------------------------------------------- the reference itself

ORACLE = {"gnss301": (oekf.gnss_pos_and_bias, oekf.multi_pseudorange, 0),
          "bias": (oekf.gnss_pos_and_bias, oekf.multi_pseudorange_and_bias, 1),
          "car": (oekf.discrete_vehicle_dynamics, oekf.vehicle_sensors_model, 0)}
SOME = (0, 1, 33, 69)


@pytest.mark.parametrize("name", ["gnss301", "bias", "car"])
def test_reference_without_a_gate_is_the_oracle_bitwise(name):
    inp, kind = gr.inputs(name)
    r = gr.run(inp, kind, np.inf, instances=SOME)
    dyn, meas, extra = ORACLE[name]
    mu, S, _ = er.oracle_run(inp, dyn=dyn, meas=meas, extra=extra, instances=SOME)
    for b in SOME:
        np.testing.assert_array_equal(r["mu"][b], mu[b])
        np.testing.assert_array_equal(r["S"][b], S[b])
    assert not r["rej"].any() and r["margin"] == np.inf
    has = inp["nz"][list(SOME)] > 0
    assert (r["nis"][list(SOME)][has] > 0).all() and not r["nis"][list(SOME)][~has].any()
    assert not r["loglik"][list(SOME)][~has].any()


def test_sequential_scalar_updates_give_the_joint_statistics():
    """sum e_i^2 / s_i and sum log s_i of sequential scalar updates (the lane kernel's form)
    equal the joint nis and log det P to 1e-10 relative on diagonal-R steps."""
    worst = 0.0
    for name in ("gnss301", "bias", "car"):
        inp, kind = gr.inputs(name)
        dyn, meas, extra = kind["odyn"], kind["omeas"], kind["extra"]
        done = 0
        for b in SOME:
            mu, S = inp["mu0"][b], inp["S0"][b]
            for k in range(inp["nz"].shape[1]):
                ns = int(inp["nz"][b, k])
                xp, G = dyn(mu, inp["U"][b, k], params=inp["dparams"], jac=True)
                SP = G @ (S @ G.T) + inp["Q"]
                mu, S = xp, SP
                if ns == 0:
                    continue
                R = (inp["R"][b, k] if inp["R"].ndim == 4 else inp["R"][k])[:ns, :ns]
                assert not (R - np.diag(np.diag(R))).any()
                h, H = meas(xp, params={"sat_pos": inp["sat"][b, k, :ns - extra]}, jac=True)
                e = inp["Z"][b, k, :ns] - h
                P = H @ SP @ H.T + R
                nis, logdet = float(e @ np.linalg.solve(P, e)), np.linalg.slogdet(P)[1]
                m, C, snis, slog = xp.copy(), SP.copy(), 0.0, 0.0
                for i in range(ns):
                    v = C @ H[i]
                    s = H[i] @ v + R[i, i]
                    ei = e[i] - H[i] @ (m - xp)
                    snis, slog = snis + ei * ei / s, slog + np.log(s)
                    m, C = m + v * ei / s, C - np.outer(v, v) / s
                worst = max(worst, abs(snis - nis) / nis, abs(slog - logdet) / abs(logdet))
                mu, S = m, C
                done += 1
        assert done > 10
    print(f"sequential against joint, worst relative difference {worst:.2e}")
    assert worst <= 1e-10


@pytest.mark.parametrize("gate", gr.GATES)
@pytest.mark.parametrize("name", gr.CASES)
def test_margin_condition(name, gate):
    """No row's d2 lies within 1e-6 (relative) of the gate, so the device's reject mask can be
    compared exactly; and the inputs exercise what the device test relies on."""
    inp, _ = gr.inputs(name)
    r = gr.reference(name, gate)
    print(f"{name} gate {gate}: margin {r['margin']:.2e}")
    assert r["margin"] >= gr.MARGIN
    planted = gr.planted_bits(inp)
    assert inp["planted"].sum() > 100 and (inp["nz"] == 0).any()
    assert not (planted & ~r["rej"]).any()                       # every planted row is screened out
    full = (r["nkept"] == 0) & (inp["nz"] > 0)
    part = (r["nkept"] > 0) & (r["nrej"] > 0)
    assert full.any() and part.any()
    if gate == 10.83 and name in ("gnss301", "gnss301c"):
        np.testing.assert_array_equal(r["rej"], planted)         # and no clean row is
    if gate == 0.5:
        clean = int((inp["nz"].sum() - inp["planted"].sum()))
        gone = int(r["nrej"].sum() - inp["planted"].sum())
        print(f"{name}: {gone} of {clean} clean rows screened out at 0.5, {full.sum()} fully rejected steps")
        assert 0.3 * clean <= gone <= 0.7 * clean and full.sum() >= 100      # the threshold itself is exercised
    if name == "bias":
        last = (inp["nz"] > 0) & (((r["rej"].view(np.uint32) >> np.maximum(inp["nz"] - 1, 0).astype(np.uint32)) & 1) == 1)
        assert last.any()                                        # a rejected bias row


def test_detection_on_the_reference():
    """The figures of DESIGN 6b's table, on the reference: screening at 10.83 removes exactly the
    planted rows of gnss301 and brings the final position error down."""
    inp, kind = gr.inputs("gnss301")
    xf = inp["fx"]["mu"][-1][:3]
    gated = gr.reference("gnss301", 10.83)
    plain = gr.run(inp, kind, np.inf)
    err = lambda r: np.linalg.norm(r["mu"][:, -1, :3] - xf, axis=-1)   # noqa: E731
    eg, ep = err(gated), err(plain)
    print(f"final position error, median / max: every row {np.median(ep):.1f} / {ep.max():.1f} m, "
          f"screened {np.median(eg):.1f} / {eg.max():.1f} m; planted rows {inp['planted'].sum()}")
    assert np.median(eg) < np.median(ep) and eg.max() < ep.max()
