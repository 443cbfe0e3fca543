"""Innovation gating of the batched unscented filter (mhe_ukf_run_gated, utils.ukf.run_batch's
`gate`): everything that needs no device.

  * the symbol is exported, declared in include/mhe.h and bound in mhe._lib; mhe_ukf_gate_args is
    mhe_ukf_args' fields in order and then gate and rej, with the offsets a C compiler gives them;
  * the C entry point's refusals, which all precede the launch (host addresses, never read);
  * utils.ukf.run_batch and UKF.update refuse a bad gate before the library is loaded;
  * the conditions on tests/ukf_gate_reference.py that tests/test_gpu_ukf_gate.py relies on, and
    that reference against tests/ukf_reference.py: bitwise with gate = inf, and within the
    float64-vs-longdouble floor on inputs from which the host removed the screened rows.
"""
import ctypes
import os
import re

import numpy as np
import pytest

import ekf_gate_reference as eg
import ekf_ragged as er
import ukf_gate_reference as ug
import ukf_reference as ur
from mhe import _lib
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
    """mhe_ukf_gate_args with every required pointer set to p (None: all NULL) and the default
    alpha, beta, kappa."""
    a = _lib.MheUkfGateArgs(batch=batch, steps=steps, alpha=1.0, beta=0.0, kappa=0.0)
    for name in REQUIRED:
        setattr(a, name, p)
    for k, v in kw.items():
        setattr(a, k, v)
    return a


def test_symbol_is_exported_declared_and_bound():
    lib = ctypes.CDLL(_lib.LIB_PATH)
    assert hasattr(lib, "mhe_ukf_run_gated")
    hdr = open(os.path.join(ROOT, "include", "mhe.h")).read()
    assert re.search(r"\bint mhe_ukf_run_gated\(const mhe_ekf_dims\* dims, const mhe_ukf_gate_args\* args, "
                     r"void\* stream\);", hdr)
    assert "#define MHE_ABI_VERSION 11" in hdr
    res, args = _lib.SIGNATURES["mhe_ukf_run_gated"]
    assert res is ctypes.c_int and len(args) == 3
    assert args[0] is ctypes.POINTER(_lib.MheEkfDims) and args[1] is ctypes.POINTER(_lib.MheUkfGateArgs)
    assert _lib.load().mhe_ukf_run_gated.argtypes == args
    # the ctypes mirror declares the header's fields in the header's order
    m = re.search(r"typedef struct mhe_ukf_gate_args \{(.*?)\} mhe_ukf_gate_args;", hdr, re.S)
    body = re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S)
    names = [n for decl in body.split(";") for n in re.findall(r"(\w+)\s*(?:,|$)", decl.strip())]
    assert names == [f[0] for f in _lib.MheUkfGateArgs._fields_]
    # mhe_ukf_args, untouched, and then the two new fields where that struct ends
    G, U = _lib.MheUkfGateArgs, _lib.MheUkfArgs
    assert G._fields_[:len(U._fields_)] == U._fields_
    assert G._fields_[len(U._fields_):] == [("gate", ctypes.c_double), ("rej", ctypes.c_void_p)]
    for name, _ in U._fields_:
        assert getattr(G, name).offset == getattr(U, name).offset, name
    assert G.gate.offset == ctypes.sizeof(U) == 192 and G.rej.offset == 200 and ctypes.sizeof(G) == 208
    assert G().struct_size == 208 and U().struct_size == 192


def test_refusals_precede_the_launch():
    run = _lib.load().mhe_ukf_run_gated
    buf = (ctypes.c_double * 16)()
    p = ctypes.cast(buf, ctypes.c_void_p).value     # a host address: never dereferenced, nothing is launched
    d = _dims()
    assert run(None, ctypes.byref(_args(p)), None) == E_NULL
    assert run(ctypes.byref(d), None, None) == E_NULL                        # NULL struct
    good = _args(p)
    assert good.struct_size == ctypes.sizeof(_lib.MheUkfGateArgs)
    for size in (0, good.struct_size - 4, good.struct_size + 8, ctypes.sizeof(_lib.MheUkfArgs)):
        for batch in (4, 0):
            assert run(ctypes.byref(d), ctypes.byref(_args(p, batch=batch, struct_size=size)), None) == E_DIMS
    for gate in (NAN, -1.0, -1e-300, -INF):
        for batch in (4, 0):
            assert run(ctypes.byref(d), ctypes.byref(_args(p, batch=batch, gate=gate)), None) == E_DIMS, gate
    bad_abk = [dict(alpha=v) for v in (0.0, -1.0, NAN, INF)] + [dict(beta=NAN), dict(kappa=INF), dict(kappa=-5.0)]
    for model in ("gnss", "car"):
        d = _dims(model)
        # mhe_ukf_run's refusals, reached through the new entry, with and without a gate
        for extra in ({}, {"gate": 10.83}, {"gate": INF, "nis": p}, {"rej": p}):
            for bad in bad_abk[:6] + ([bad_abk[6]] if model == "gnss" else [dict(kappa=-9.0)]):
                assert run(ctypes.byref(d), ctypes.byref(_args(p, **dict(extra, **bad))), None) == E_DIMS, bad
            assert run(ctypes.byref(d), ctypes.byref(_args(None, **dict(extra, rej=None))), None) == E_NULL
            for name in REQUIRED:                                            # any one required pointer missing
                assert run(ctypes.byref(d), ctypes.byref(_args(p, **dict(extra, **{name: None}))), None) == E_NULL, name
            assert run(ctypes.byref(d), ctypes.byref(_args(p, batch=-1, **extra)), None) == E_DIMS
            assert run(ctypes.byref(d), ctypes.byref(_args(p, steps=-1, **extra)), None) == E_DIMS
            nul = dict(extra, rej=None, nis=None)
            assert run(ctypes.byref(d), ctypes.byref(_args(None, batch=0, **nul)), None) == OK   # empty: nothing is read
            assert run(ctypes.byref(d), ctypes.byref(_args(None, steps=0, **nul)), None) == OK
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


def test_python_refuses_a_bad_gate_before_loading_the_library(monkeypatch):
    def no_load(*a, **k):
        raise AssertionError("the library was loaded")
    monkeypatch.setattr(_lib, "load", no_load)
    inp = er.gnss_inputs(2, T=6)
    U, Z, nz, sat = er.device_args(inp)
    for bad in (0, 0.0, -1.0, NAN, -np.inf, "10.83", True, [10.83], np.array([1.0, 2.0])):
        with pytest.raises(ValueError):
            ukf.run_batch("gnss_pos_and_bias", "multi_pseudorange", inp["mu0"], inp["S0"], U, Z, nz, inp["Q"],
                          inp["R"], 1.0, sat, gate=bad)
        f = ukf.UKF("gnss_pos_and_bias", "multi_pseudorange", inp["mu0"][0], inp["S0"][0])
        with pytest.raises(ValueError):
            f.update(U[0, 0], Z[0, 0, :4], inp["Q"], inp["R"][0, 0, :4, :4], {"dt": 1.0}, None,
                     {"sat_pos": sat[0, 0, :4]}, gate=bad)
    import inspect
    sig = inspect.signature(ukf.run_batch).parameters      # gate is keyword only; nothing else is taken
    assert sig["screen"].kind is inspect.Parameter.VAR_KEYWORD
    with pytest.raises(TypeError):
        ukf.run_batch("gnss_pos_and_bias", "multi_pseudorange", inp["mu0"], inp["S0"], U, Z, nz, inp["Q"],
                      inp["R"], 1.0, sat, gates=10.83)
    assert inspect.signature(ukf.UKF.update).parameters["gate"].default is None
    assert "Not formed: a filter-per-lane kernel" in ukf.__doc__
    assert "gated run" in ukf.smooth_batch.__doc__


# ---------------------------------------------------------------- the reference itself

ALL = [(n, g, p) for n in ug.CASES for g in ug.GATES for p in ug.PARAMS]


def _row_bit(inp):
    """(B,T) uint32: the bit of each step's last valid row (0 where the step has none)."""
    nz = inp["nz"].astype(np.int64)
    return np.where(nz > 0, np.uint64(1) << np.maximum(nz - 1, 0).astype(np.uint64), 0).astype(np.uint32)


@pytest.mark.parametrize("name,gate,params", ALL)
def test_conditions_the_device_test_relies_on(name, gate, params):
    inp, r = ug.inputs(name), ug.reference(name, gate, params)     # asserts the two precisions' masks equal
    nz, rej = inp["nz"], r["rej"].view(np.uint32)
    full = int(((r["nkept"] == 0) & (nz > 0)).sum())
    part = int(((r["nkept"] > 0) & (r["nrej"] > 0)).sum())
    print(f"{name} gate {gate} {params}: gate margin {r['gate_margin']:.2e}, rows screened {r['nrej'].sum()} "
          f"(planted {inp['planted'].sum()}), steps fully screened {full}, partly {part}, floors {r['floor']}, "
          f"smallest pivot / diagonal {r['margin']:.2e}, smallest sigma-point x[3] {r['min_vx']:.3f}")
    np.testing.assert_array_equal(r["f64"]["rej"], r["rej"])
    assert not r["status"].any() and not r["f64"]["status"].any() and (r["fail_step"] == -1).all()
    assert r["gate_margin"] >= ug.MARGIN            # no d2 is near the threshold: the masks are exact
    assert r["margin"] > 1e-6                       # no pivot is near zero: status cannot differ
    if name == "car":
        assert r["min_vx"] > 0.0
    for key in ug.OUTPUTS:
        assert np.isfinite(r[key]).all() and 0.0 < r["floor"][key] < r["bound"][key]
    # counts and masks agree; nothing is screened where there is no valid row
    assert ((r["nrej"] + r["nkept"]) == nz).all()
    assert (rej & ~np.where(nz >= 32, 0xffffffff, (1 << nz.astype(np.int64)) - 1).astype(np.uint32) == 0).all()
    # every path: steps partly and fully screened, the last row (bias row / bit 31) screened
    assert full > 0 and part > 0 and ((r["nrej"] == 0) & (nz > 0)).any() and (nz == 0).any()
    if name in ("gnss", "corr"):
        assert (r["rej"] < 0).any() and ((nz == 32) & (r["rej"] >= 0)).any()              # bit 31, both ways
    if name == "bias":
        last = _row_bit(inp)
        assert ((rej & last) != 0).any() and (((rej & last) == 0) & (r["nrej"] > 0)).any()  # the bias row, both ways
    none = r["nkept"] == 0
    assert not r["nis"][none].any() and not r["loglik"][none].any() and (r["nis"][~none] > 0).all()
    np.testing.assert_array_equal(r["S"], np.swapaxes(r["S"], -1, -2))
    planted = eg.planted_bits(inp).view(np.uint32)
    if gate == 10.83:
        if name == "car":
            assert ((rej & planted) == planted).all()             # every planted row, and some more
        else:
            np.testing.assert_array_equal(rej, planted)           # exactly the planted rows


@pytest.mark.parametrize("name", ug.CASES)
def test_an_infinite_gate_is_the_ungated_reference_bitwise(name):
    inp, kind = ug.inputs(name), ug.KIND[name]
    for params in ug.PARAMS:
        got, want = ug.run(inp, kind, np.inf, params), ur.run(inp, kind, params)
        for key in ug.OUTPUTS + ("status", "fail_step"):
            np.testing.assert_array_equal(got[key], want[key])    # NaN where a planted row broke the ungated filter
        assert not got["rej"].any() and not got["nrej"].any() and got["gate_margin"] == np.inf
        np.testing.assert_array_equal(got["nkept"], np.where(inp["nz"] <= inp["Z"].shape[2], inp["nz"], 0))


@pytest.mark.parametrize("gate", ug.GATES)
@pytest.mark.parametrize("name", ["gnss", "corr", "car"])
def test_a_gated_run_is_the_ungated_one_on_the_kept_rows(name, gate):
    """The gated reference against ukf_reference.run on inputs from which the host removed the
    screened rows (not `bias`: removing its last row changes the model).  Bound: the case's
    float64-vs-longdouble floor in ukf_reference's form."""
    inp, kind, r = ug.inputs(name), ug.KIND[name], ug.reference(name, gate)
    small = ug.compact(inp, r["rej"])
    np.testing.assert_array_equal(small["nz"], r["nkept"])
    want = ur.run(small, kind)
    assert not want["status"].any()
    for key in ug.OUTPUTS:
        err = float(np.max(np.abs(r["f64"][key] - want[key])))
        print(f"{name} gate {gate} {key}: gated run against the compacted ungated run {err:.2e} "
              f"(bound {r['bound'][key]:.2e})")
        assert err <= r["bound"][key]
