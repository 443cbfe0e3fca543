"""Iterated EKF (mhe_iekf_run, utils.ekf.run_batch(iterations=, iter_tol=)): everything that needs
no device.

  * the symbol is exported, declared in include/mhe.h and bound in mhe._lib; mhe_iekf_args is
    mhe_ekf_args' fields in order and then tol, n_iter, max_iter, reserved0 at the offsets a C
    compiler gives them; the ABI version did not move;
  * the C entry point's refusals, which all precede the launch (host addresses, never read);
  * utils.ekf.run_batch and EKF.update refuse bad values before the library is loaded;
  * the conditions on tests/iekf_reference.py that tests/test_gpu_iekf.py relies on;
  * that reference with iterations = 1 against the existing EKF reference (oracle/ekf.py through
    tests/ekf_ragged.oracle_run), and its converged iterate as a stationary point of the step's
    MAP cost.
"""
import ctypes
import inspect
import os
import re

import numpy as np
import pytest

import ekf_ragged as er
import iekf_reference as ir
import ukf_reference as ur
from mhe import _lib
from oracle import ekf as oekf
import utils.ekf as ekf

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


def _args(p=None, batch=4, steps=5, max_iter=3, **kw):
    """mhe_iekf_args with every required pointer set to p (None: all NULL)."""
    a = _lib.MheIekfArgs(batch=batch, steps=steps, max_iter=max_iter)
    for name in REQUIRED:
        setattr(a, name, p)
    for k, v in kw.items():
        setattr(a, k, v)
    return a


def test_symbol_is_exported_declared_and_bound():
    lib = ctypes.CDLL(_lib.LIB_PATH)
    assert hasattr(lib, "mhe_iekf_run")
    hdr = open(os.path.join(ROOT, "include", "mhe.h")).read()
    assert re.search(r"\bint mhe_iekf_run\(const mhe_ekf_dims\* dims, const mhe_iekf_args\* args, void\* stream\);", hdr)
    assert "#define MHE_ABI_VERSION 11" in hdr
    res, args = _lib.SIGNATURES["mhe_iekf_run"]
    assert res is ctypes.c_int and len(args) == 3
    assert args[0] is ctypes.POINTER(_lib.MheEkfDims) and args[1] is ctypes.POINTER(_lib.MheIekfArgs)
    assert _lib.load().mhe_iekf_run.argtypes == args


def test_struct_is_mhe_ekf_args_and_then_the_four_new_fields():
    hdr = open(os.path.join(ROOT, "include", "mhe.h")).read()
    m = re.search(r"typedef struct mhe_iekf_args \{(.*?)\} mhe_iekf_args;", hdr, re.S)
    body = re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S)
    names = [n for decl in body.split(";") for n in re.findall(r"(\w+)\s*(?:,|$)", decl.strip())]
    assert names == [f[0] for f in _lib.MheIekfArgs._fields_]            # the header's fields in the header's order
    I, E = _lib.MheIekfArgs, _lib.MheEkfArgs
    assert I._fields_[:len(E._fields_)] == E._fields_
    assert I._fields_[len(E._fields_):] == [("tol", ctypes.c_double), ("n_iter", ctypes.c_void_p),
                                            ("max_iter", ctypes.c_int32), ("reserved0", ctypes.c_int32)]
    for name, _ in E._fields_:
        assert getattr(I, name).offset == getattr(E, name).offset, name
    # LP64: three int32 and a pad, seventeen 8-byte fields, gate and three pointers: 184 bytes
    assert ctypes.sizeof(E) == 184 and I.tol.offset == 184 and I.n_iter.offset == 192
    assert I.max_iter.offset == 200 and I.reserved0.offset == 204 and ctypes.sizeof(I) == 208
    assert I().struct_size == 208 and E().struct_size == 184


def test_refusals_precede_the_launch():
    run = _lib.load().mhe_iekf_run
    buf = (ctypes.c_double * 16)()
    p = ctypes.cast(buf, ctypes.c_void_p).value     # a host address: never dereferenced, nothing is launched
    d = _dims()
    assert run(None, ctypes.byref(_args(p)), None) == E_NULL
    assert run(ctypes.byref(d), None, None) == E_NULL                        # NULL struct
    good = _args(p)
    assert good.struct_size == ctypes.sizeof(_lib.MheIekfArgs)
    for size in (0, good.struct_size - 4, good.struct_size + 8, ctypes.sizeof(_lib.MheEkfArgs)):
        for batch in (4, 0):
            assert run(ctypes.byref(d), ctypes.byref(_args(p, batch=batch, struct_size=size)), None) == E_DIMS
    for batch in (4, 0):                                                     # before the empty call's MHE_OK
        for gate in (NAN, -1.0, -1e-300, -INF):
            assert run(ctypes.byref(d), ctypes.byref(_args(p, batch=batch, gate=gate)), None) == E_DIMS, gate
        for tol in (NAN, -1.0, -1e-300, -INF):
            assert run(ctypes.byref(d), ctypes.byref(_args(p, batch=batch, tol=tol)), None) == E_DIMS, tol
        for max_iter in (0, -1, 65, 1 << 20):
            assert run(ctypes.byref(d), ctypes.byref(_args(p, batch=batch, max_iter=max_iter)), None) == E_DIMS
        for r0 in (1, -1):
            assert run(ctypes.byref(d), ctypes.byref(_args(p, batch=batch, reserved0=r0)), None) == E_DIMS
    for model in ("gnss", "car"):
        d = _dims(model)
        # mhe_ekf_run_args' refusals, reached through the new entry
        for extra in ({}, {"gate": 10.83}, {"gate": INF, "nis": p}, {"n_iter": p, "tol": 1e-4, "max_iter": 64},
                      {"max_iter": 1, "tol": INF}, {"r_diag": 1}):
            dk = {k: extra[k] for k in ("r_diag",) if k in extra}
            ak = {k: v for k, v in extra.items() if k not in dk}
            d = _dims(model, **dk)
            assert run(ctypes.byref(d), ctypes.byref(_args(None, **ak)), None) == E_NULL
            for name in REQUIRED:                                            # any one required pointer missing
                assert run(ctypes.byref(d), ctypes.byref(_args(p, **dict(ak, **{name: None}))), None) == E_NULL, name
            assert run(ctypes.byref(d), ctypes.byref(_args(p, batch=-1, **ak)), None) == E_DIMS
            assert run(ctypes.byref(d), ctypes.byref(_args(p, steps=-1, **ak)), None) == E_DIMS
            nul = dict(ak, nis=None, n_iter=None)
            assert run(ctypes.byref(d), ctypes.byref(_args(None, batch=0, **nul)), None) == OK   # empty: nothing is read
            assert run(ctypes.byref(d), ctypes.byref(_args(None, steps=0, **nul)), None) == OK
            for pmax in (0, 33, 64):
                assert run(ctypes.byref(_dims(model, pmax=pmax, **dk)), ctypes.byref(_args(p, **ak)), None) == E_DIMS
            assert run(ctypes.byref(_dims(model, q=2, **dk)), ctypes.byref(_args(p, **ak)), None) == E_DIMS
            for size in (0, d.struct_size - 4, d.struct_size + 8):
                assert run(ctypes.byref(_dims(model, struct_size=size)), ctypes.byref(_args(p, **ak)), None) == E_DIMS
    for bad in (dict(dyn_model=0), dict(dyn_model=3), dict(n=9), dict(m=2), dict(meas_model=3), dict(meas_model=0)):
        assert run(ctypes.byref(_dims("gnss", **bad)), ctypes.byref(_args(p)), None) == E_MODEL, bad
    for bad in (dict(n=5), dict(meas_model=1), dict(dyn_model=7)):
        assert run(ctypes.byref(_dims("car", **bad)), ctypes.byref(_args(p)), None) == E_MODEL, bad
    for i in (2, 5):                                                         # the vehicle's M / I_Z unset
        d = _dims("car")
        d.dyn_par[i] = 0.0
        assert run(ctypes.byref(d), ctypes.byref(_args(p)), None) == E_DIMS


def test_python_refuses_bad_values_before_loading_the_library(monkeypatch):
    def no_load(*a, **k):
        raise AssertionError("the library was loaded")
    monkeypatch.setattr(_lib, "load", no_load)
    inp = er.gnss_inputs(2, T=6)
    U, Z, nz, sat = er.device_args(inp)

    def batch(**kw):
        return ekf.run_batch("gnss_pos_and_bias", "multi_pseudorange", inp["mu0"], inp["S0"], U, Z, nz, inp["Q"],
                             inp["R"], 1.0, sat, **kw)

    def single(**kw):
        f = ekf.EKF("gnss_pos_and_bias", "multi_pseudorange", inp["mu0"][0], inp["S0"][0])
        return f.update(U[0, 0], Z[0, 0, :4], inp["Q"], inp["R"][0, 0, :4, :4], {"dt": 1.0}, None,
                        {"sat_pos": sat[0, 0, :4]}, **kw)

    bad_iter = [dict(iterations=v) for v in (True, False, 2.0, 3.5, "3", 0, -1, 65, 1000, [3], np.float64(2.0), NAN)]
    bad_tol = [dict(iterations=3, iter_tol=v) for v in (NAN, -1.0, -1e-300, -INF, "1e-4", None, True, [1e-4])]
    for kw in bad_iter + bad_tol:
        with pytest.raises(ValueError):
            batch(**kw)
        with pytest.raises(ValueError):
            single(**kw)
    with pytest.raises(ValueError):
        batch(iter_tol=-1.0)                                                 # checked without iterations as well
    with pytest.raises(ValueError, match="lane"):
        batch(iterations=3, method="lane")                                   # not formed
    for good in (1, 64, np.int32(5), np.int64(8)):
        assert ekf._iter_values(good, 1e-4) == (int(good), 1e-4)
    assert ekf._iter_values(3, 0) == (3, 0.0) and ekf._iter_values(3, INF) == (3, INF)
    assert ekf._iter_values(None, 0.0) == (None, 0.0)
    sig = inspect.signature(ekf.run_batch).parameters
    assert sig["iterations"].default is None and sig["iter_tol"].default == 0.0
    sig = inspect.signature(ekf.EKF.update).parameters
    assert sig["iterations"].default is None and sig["iter_tol"].default == 0.0
    doc = " ".join(ekf.run_batch.__doc__.split())
    assert "x_{i+1} = mu- + K e" in doc and "absolute max-norm in the state's own units" in doc
    assert "rounding floor" in doc and "1e-8 m" in doc
    assert "iterated run" in " ".join(ekf.smooth_batch.__doc__.split())


# ---------------------------------------------------------------- the reference itself

@pytest.mark.parametrize("name", ir.CASES)
def test_conditions_the_device_test_relies_on(name):
    inp, r = ir.inputs(name), ir.reference(name)     # asserts: counts equal in both precisions, the step margin
    nz, P = inp["nz"], inp["Z"].shape[2]
    hist = np.bincount(r["n_iter"].ravel(), minlength=r["iterations"] + 1)
    moving = (r["n_iter"] == r["iterations"]) & (r["step_last"] > r["tol"])
    print(f"{name}: tol {r['tol']:g}, cap {r['iterations']}, passes per step {hist.tolist()}, at the cap and still "
          f"moving {int(moving.sum())}, smallest |step / tol - 1| {r['step_margin']:.2e}, smallest pivot / diagonal "
          f"{r['margin']:.2e}, floors {r['floor']}, bounds {r['bound']}")
    np.testing.assert_array_equal(r["f64"]["n_iter"], r["n_iter"])
    assert r["step_margin"] >= ir.STEP_MARGIN
    # a pivot's rounding error is below ~ P * 2^-53 of the diagonal entry (7e-15): 1e-10 is four orders above it
    assert r["margin"] > 1e-10
    assert not r["status"].any() and not r["f64"]["status"].any() and not r["rej"].any()
    for key in ir.OUTPUTS:
        assert np.isfinite(r[key]).all() and 0.0 < r["floor"][key] < r["bound"][key]
    np.testing.assert_array_equal(r["S"], np.swapaxes(r["S"], -1, -2))
    # no pass where there is no correction, at least one where there is one, and several counts occur
    assert (nz == 0).any() and (r["n_iter"][nz == 0] == 0).all() and (r["n_iter"][nz > 0] >= 1).all()
    assert (r["n_iter"] <= r["iterations"]).all() and (hist[2:] > 0).sum() >= 3
    assert not r["nis"][nz == 0].any() and (r["nis"][nz > 0] > 0).all()
    if name == "gnss":
        assert {0, 1, P} <= set(nz.ravel().tolist()) and P == 32
    if name == "bias":
        assert P == 13 and moving.any()                  # a step that ends at the cap, still moving by more than tol
    else:
        assert not moving.any()                          # every step converged below the cap
    # the iteration matters on these inputs: the result is not the EKF's
    one = ir.reference(name, 1, 0.0)
    assert (one["n_iter"] == (nz > 0)).all()
    assert float(np.max(np.abs(one["mu"] - r["mu"]))) > 1e3 * r["bound"]["mu"]


@pytest.mark.parametrize("gate", ir.GATES)
@pytest.mark.parametrize("name", ir.GATED)
def test_conditions_of_the_gated_cases(name, gate):
    inp, r = ir.gated_inputs(name), ir.reference(name, ir.CAP[name], ir.TOL[name], gate)
    nz = inp["nz"]
    full = (r["nkept"] == 0) & (nz > 0)
    part = (r["nkept"] > 0) & (r["nkept"] < nz)
    print(f"{name} gate {gate}: gate margin {r['gate_margin']:.2e}, step margin {r['step_margin']:.2e}, steps fully "
          f"screened {int(full.sum())}, partly {int(part.sum())}, passes "
          f"{np.bincount(r['n_iter'].ravel()).tolist()}, floors {r['floor']}")
    assert r["gate_margin"] >= ir.MARGIN and r["step_margin"] >= ir.STEP_MARGIN and r["margin"] > 1e-10
    assert not r["status"].any()
    assert full.any() and part.any() and (r["n_iter"][full] == 0).all() and (r["n_iter"][r["nkept"] > 0] >= 1).all()
    assert not r["nis"][r["nkept"] == 0].any() and not r["loglik"][r["nkept"] == 0].any()
    # the screen and the statistics are pass 0's: at the first step (the later ones start from another
    # state) they are those of the one-pass run, bitwise
    one = ir.run(inp, ir.KIND[name], 1, 0.0, gate)
    k0 = int(np.flatnonzero((r["n_iter"] > 1).any(axis=0))[0])
    assert (r["n_iter"][:, :k0] <= 1).all()
    for key in ("rej", "nis", "loglik"):
        np.testing.assert_array_equal(one[key][:, :k0 + 1], r["f64"][key][:, :k0 + 1])


@pytest.mark.parametrize("name", ["gnss", "car"])
def test_a_gated_run_is_the_ungated_one_on_the_kept_rows(name):
    """The gated reference against the ungated one on inputs from which the host removed the
    screened rows, within the gated case's bound."""
    gate = ir.GATES[0]
    inp, r = ir.gated_inputs(name), ir.reference(name, ir.CAP[name], ir.TOL[name], gate)
    small = ir.ug.compact(inp, r["rej"])
    np.testing.assert_array_equal(small["nz"], r["nkept"])
    want = ir.run(small, ir.KIND[name], ir.CAP[name], ir.TOL[name])
    np.testing.assert_array_equal(want["n_iter"], r["n_iter"])
    for key in ir.OUTPUTS:
        err = float(np.max(np.abs(r["f64"][key] - want[key])))
        print(f"{name} {key}: gated against compacted {err:.2e} (bound {r['bound'][key]:.2e})")
        assert err <= r["bound"][key]


ORACLE = {"gnss": (oekf.gnss_pos_and_bias, oekf.multi_pseudorange, 0),
          "bias": (oekf.gnss_pos_and_bias, oekf.multi_pseudorange_and_bias, 1),
          "car": (oekf.discrete_vehicle_dynamics, oekf.vehicle_sensors_model, 0)}
SOME = (0, 1, 33, 69)


@pytest.mark.parametrize("name", ["gnss", "bias", "car"])
def test_one_pass_is_the_existing_ekf_reference(name):
    """iterations = 1 against oracle/ekf.py (tests/ekf_ragged.oracle_run) on tests/ukf_reference.py's
    input sets (the fixtures' own priors: the oracle forms inv(P), which the cold prior's
    P ~ 1e10 would not let it do to the floor).  Bound: this run's float64-vs-longdouble floor in
    the project's form."""
    inp, kind = ur.inputs(name), ir.KIND[name]
    lo, hi = ir.run(inp, kind, 1, 0.0), ir.run(inp, kind, 1, 0.0, dtype=np.longdouble)
    dyn, meas, extra = ORACLE[name]
    mu, S, spd = er.oracle_run(inp, dyn=dyn, meas=meas, extra=extra, instances=SOME)
    assert spd.all() and not lo["status"].any()
    assert (lo["n_iter"] == (inp["nz"] > 0)).all()
    for key, want in (("mu", mu), ("S", S)):
        floor = float(np.max(np.abs(lo[key].astype(np.longdouble) - hi[key])))
        bound = 8.0 * floor + 1e-10 * (1.0 + float(np.max(np.abs(hi[key]))))
        err = float(np.max(np.abs(lo[key][list(SOME)] - want[list(SOME)])))
        print(f"{name} {key}: one pass against the oracle {err:.2e} (floor {floor:.2e}, bound {bound:.2e})")
        assert err <= bound


@pytest.mark.parametrize("name", ["gnss", "corr", "car"])
def test_the_converged_iterate_is_a_stationary_point_of_the_map_cost(name):
    """g = S-^-1 (x - mu-) - H^T R^-1 (z - h(x)) at the final iterate of every step that converged
    below the cap (not `bias`: its bias row has a zero Jacobian row, so its fixed point is no
    stationary point).  The iterate is within the last step (<= tol in every component, the
    iteration contracting by more than a half) of the fixed point x*, where g = 0, so
    |g| <= |A| sqrt(n) tol with A = S-^-1 + H^T R^-1 H; and that is small beside |g|'s two terms."""
    inp, kind, r = ir.inputs(name), ir.KIND[name], ir.reference(name)
    hi = ir.run(inp, kind, r["iterations"], r["tol"], dtype=np.longdouble)
    Bn, T = inp["nz"].shape
    n = inp["mu0"].shape[1]
    L = np.longdouble
    worst_rel, worst_frac, done = 0.0, 0.0, 0
    for k in range(T):
        rows = inp["nz"][:, k].astype(np.int64)
        h, H = ir.meas_jac(kind, hi["mu"][:, k], inp["sat"][:, k].astype(L), rows)
        for b in range(Bn):
            ns = int(rows[b])
            if ns == 0 or r["n_iter"][b, k] == r["iterations"]:
                continue
            R = (inp["R"][b, k] if inp["R"].ndim == 4 else inp["R"][k])[:ns, :ns].astype(np.float64)
            Hb, e = H[b, :ns].astype(np.float64), (inp["Z"][b, k, :ns].astype(L) - h[b, :ns]).astype(np.float64)
            Si = np.linalg.inv(hi["SP"][b, k].astype(np.float64))
            t1 = Si @ (hi["mu"][b, k] - hi["mp"][b, k]).astype(np.float64)
            t2 = Hb.T @ np.linalg.solve(R, e)
            A = Si + Hb.T @ np.linalg.solve(R, Hb)
            g = np.linalg.norm(t1 - t2)
            lim = np.linalg.norm(A, 2) * np.sqrt(n) * r["tol"] + 1e-9 * max(np.linalg.norm(t1), np.linalg.norm(t2))
            worst_frac = max(worst_frac, g / lim)
            if max(np.linalg.norm(t1), np.linalg.norm(t2)) > 0:
                worst_rel = max(worst_rel, g / max(np.linalg.norm(t1), np.linalg.norm(t2)))
            done += 1
    print(f"{name}: {done} converged steps, worst |g| / limit {worst_frac:.2e}, worst |g| / max(|term|) {worst_rel:.2e}")
    assert done > 50 and worst_frac <= 1.0 and worst_rel <= 1e-3
