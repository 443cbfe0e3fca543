"""Pseudo-Huber rows for the iterated EKF (mhe_iekf_run_robust, utils.ekf.run_batch(huber=)):
everything that needs no device.

  * the symbol is exported, declared in include/mhe.h and bound in mhe._lib; mhe_iekf_robust_args is
    mhe_iekf_args' fields at their offsets and then delta, DELTA, weights at the offsets a C compiler
    gives them; the ABI version did not move;
  * the C entry point's refusals, which all precede the launch (host addresses, never read);
  * utils.ekf.run_batch and EKF.update refuse bad values before the library is loaded;
  * the conditions on tests/robust_iekf_reference.py that tests/test_gpu_robust_iekf.py relies on;
  * that reference with delta = inf against tests/iekf_reference.py bitwise, its converged iterate as
    a stationary point of the robust MAP cost, and what the soft weights do on the planted outliers.
"""
import ctypes
import inspect
import os
import re

import numpy as np
import pytest

import ekf_ragged as er
import iekf_reference as ir
import robust_iekf_reference as rr
from mhe import _lib
import utils.ekf as ekf

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OK, E_DIMS, E_MODEL, E_NULL = 0, -1, -2, -5
CAR = [1.0e5, 1.2e5, 1500.0, 1.2, 1.4, 2500.0]
REQUIRED = ("mu", "S", "U", "Z", "nz", "PAR", "Q", "R")
INF, NAN = float("inf"), float("nan")
CASES = rr.PARITY + (rr.ROWS,)
IDS = [f"{n}-gate{g}-delta{d}-tol{t:g}" for n, g, d, t in CASES]


def _dims(model="gnss", **kw):
    d = _lib.MheEkfDims(n=5, m=3, pmax=12, q=3, dyn_model=1, meas_model=1, dt=1.0) if model == "gnss" else \
        _lib.MheEkfDims(n=9, m=2, pmax=8, q=3, dyn_model=2, meas_model=3, dt=0.1)
    if model == "car":
        for i, v in enumerate(CAR):
            d.dyn_par[i] = v
    for k, v in kw.items():
        setattr(d, k, v)
    return d


def _args(p=None, batch=4, steps=5, max_iter=3, delta=15.0, **kw):
    """mhe_iekf_robust_args with every required pointer set to p (None: all NULL)."""
    a = _lib.MheIekfRobustArgs(batch=batch, steps=steps, max_iter=max_iter, delta=delta)
    for name in REQUIRED:
        setattr(a, name, p)
    for k, v in kw.items():
        setattr(a, k, v)
    return a


def test_symbol_is_exported_declared_and_bound():
    lib = ctypes.CDLL(_lib.LIB_PATH)
    assert hasattr(lib, "mhe_iekf_run_robust") and hasattr(lib, "mhe_iekf_run")
    hdr = open(os.path.join(ROOT, "include", "mhe.h")).read()
    assert re.search(r"\bint mhe_iekf_run_robust\(const mhe_ekf_dims\* dims, const mhe_iekf_robust_args\* args, "
                     r"void\* stream\);", hdr)
    assert "#define MHE_ABI_VERSION 11" in hdr
    res, args = _lib.SIGNATURES["mhe_iekf_run_robust"]
    assert res is ctypes.c_int and len(args) == 3
    assert args[0] is ctypes.POINTER(_lib.MheEkfDims) and args[1] is ctypes.POINTER(_lib.MheIekfRobustArgs)
    assert _lib.load().mhe_iekf_run_robust.argtypes == args
    doc = " ".join(re.sub(r"^\s*\*", "", line) for line in hdr.splitlines())
    doc = " ".join(doc.split())
    assert "UNWEIGHTED diagonal" in doc and "REWEIGHTED model" in doc      # what the gate tests; what nis / loglik are


def test_struct_is_mhe_iekf_args_and_then_the_three_new_fields():
    hdr = open(os.path.join(ROOT, "include", "mhe.h")).read()
    m = re.search(r"typedef struct mhe_iekf_robust_args \{(.*?)\} mhe_iekf_robust_args;", hdr, re.S)
    body = re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S)
    names = [n for decl in body.split(";") for n in re.findall(r"(\w+)\s*(?:,|$)", decl.strip())]
    assert names == [f[0] for f in _lib.MheIekfRobustArgs._fields_]      # the header's fields in the header's order
    old = re.search(r"typedef struct mhe_iekf_args \{(.*?)\} mhe_iekf_args;", hdr, re.S).group(1)
    strip = lambda t: " ".join(re.sub(r"/\*.*?\*/", "", t, flags=re.S).split())   # noqa: E731
    assert strip(body).startswith(strip(old))                            # the same declarations, then the new ones
    Rb, I = _lib.MheIekfRobustArgs, _lib.MheIekfArgs
    assert Rb._fields_[:len(I._fields_)] == I._fields_
    assert Rb._fields_[len(I._fields_):] == [("delta", ctypes.c_double), ("DELTA", ctypes.c_void_p),
                                             ("weights", ctypes.c_void_p)]
    for name, _ in I._fields_:
        assert getattr(Rb, name).offset == getattr(I, name).offset, name
    # LP64: mhe_iekf_args is 208 bytes with no tail padding, then three 8-byte fields
    assert ctypes.sizeof(I) == 208 and Rb.delta.offset == 208 and Rb.DELTA.offset == 216
    assert Rb.weights.offset == 224 and ctypes.sizeof(Rb) == 232
    assert Rb().struct_size == 232 and I().struct_size == 208


def test_refusals_precede_the_launch():
    run = _lib.load().mhe_iekf_run_robust
    buf = (ctypes.c_double * 16)()
    p = ctypes.cast(buf, ctypes.c_void_p).value     # a host address: never dereferenced, nothing is launched
    d = _dims()
    assert run(None, ctypes.byref(_args(p)), None) == E_NULL
    assert run(ctypes.byref(d), None, None) == E_NULL                        # NULL struct
    good = _args(p)
    assert good.struct_size == ctypes.sizeof(_lib.MheIekfRobustArgs)
    for size in (0, good.struct_size - 4, good.struct_size + 8, ctypes.sizeof(_lib.MheIekfArgs)):
        for batch in (4, 0):
            assert run(ctypes.byref(d), ctypes.byref(_args(p, batch=batch, struct_size=size)), None) == E_DIMS
    for batch, steps in ((4, 5), (0, 5), (4, 0)):                            # before the empty call's MHE_OK
        kw = dict(batch=batch, steps=steps)
        for delta in (NAN, 0.0, -0.0, -1.0, -1e-300, -INF):                  # one delta for every row: > 0
            assert run(ctypes.byref(d), ctypes.byref(_args(p, delta=delta, **kw)), None) == E_DIMS, delta
        for delta in (15.0, 1e-300, INF, -1.0, NAN):                         # with DELTA given: delta is 0
            assert run(ctypes.byref(d), ctypes.byref(_args(p, delta=delta, DELTA=p, **kw)), None) == E_DIMS, delta
        for gate in (NAN, -1.0, -1e-300, -INF):
            assert run(ctypes.byref(d), ctypes.byref(_args(p, gate=gate, **kw)), None) == E_DIMS, gate
        for tol in (NAN, -1.0, -1e-300, -INF):
            assert run(ctypes.byref(d), ctypes.byref(_args(p, tol=tol, **kw)), None) == E_DIMS, tol
        for max_iter in (0, -1, 65, 1 << 20):
            assert run(ctypes.byref(d), ctypes.byref(_args(p, max_iter=max_iter, **kw)), None) == E_DIMS
        for r0 in (1, -1):
            assert run(ctypes.byref(d), ctypes.byref(_args(p, reserved0=r0, **kw)), None) == E_DIMS
    for model in ("gnss", "car"):
        # mhe_iekf_run's refusals, reached through the new entry, for each way of giving delta
        for ak in ({}, {"delta": INF}, {"delta": 0.0, "DELTA": p}, {"delta": 5.0, "weights": p, "gate": 10.83},
                   {"delta": 0.0, "DELTA": p, "weights": p, "n_iter": p, "tol": 1e-4, "max_iter": 64}):
            d = _dims(model)
            assert run(ctypes.byref(d), ctypes.byref(_args(None, **dict(ak, DELTA=None, delta=ak.get("delta") or 1.0))),
                       None) == E_NULL
            for name in REQUIRED:                                            # any one required pointer missing
                assert run(ctypes.byref(d), ctypes.byref(_args(p, **dict(ak, **{name: None}))), None) == E_NULL, name
            assert run(ctypes.byref(d), ctypes.byref(_args(p, batch=-1, **ak)), None) == E_DIMS
            assert run(ctypes.byref(d), ctypes.byref(_args(p, steps=-1, **ak)), None) == E_DIMS
            nul = dict(ak, weights=None, n_iter=None, DELTA=None, delta=ak.get("delta") or 1.0)
            assert run(ctypes.byref(d), ctypes.byref(_args(None, batch=0, **nul)), None) == OK   # empty: nothing is read
            assert run(ctypes.byref(d), ctypes.byref(_args(None, steps=0, **nul)), None) == OK
            for pmax in (0, 33, 64):
                assert run(ctypes.byref(_dims(model, pmax=pmax)), ctypes.byref(_args(p, **ak)), None) == E_DIMS
            assert run(ctypes.byref(_dims(model, q=2)), ctypes.byref(_args(p, **ak)), None) == E_DIMS
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

    Zs = np.asarray(Z).shape
    scalars = (True, False, 0, 0.0, -1.0, -1e-300, -INF, NAN, "5", np.float64(-2.0), np.bool_(True))
    for v in scalars:
        with pytest.raises(ValueError):
            batch(iterations=3, huber=v)
        with pytest.raises(ValueError):
            single(iterations=3, huber=v)
    arrays = (np.zeros(Zs), np.full(Zs, -1.0), np.full(Zs, NAN), np.full(Zs[:2], 5.0), np.full(Zs[1:], 5.0),
              np.full(Zs[:2] + (Zs[2] + 1,), 5.0), np.full(Zs, "5"), [5.0], (5.0,))
    for v in arrays:
        with pytest.raises(ValueError):
            batch(iterations=3, huber=v)
    one_nan = np.full(Zs, 5.0)
    one_nan[1, 2, 3] = NAN
    one_zero = np.full(Zs, INF)
    one_zero[0, 0, 0] = 0.0
    for v in (one_nan, one_zero):
        with pytest.raises(ValueError):
            batch(iterations=3, huber=v)
    for v in (np.zeros(4), np.full(4, -1.0), [5.0, 5.0, NAN, 5.0], np.full(3, 5.0), np.full(5, 5.0),
              np.full((2, 2), 5.0), ["a", "b", "c", "d"]):
        with pytest.raises(ValueError):
            single(iterations=3, huber=v)
    for v in (5.0, INF, np.full(Zs, 5.0)):                                    # huber is the iterated filter's
        with pytest.raises(ValueError, match="iterations"):
            batch(huber=v)
    for v in (5.0, INF, np.full(4, 5.0)):
        with pytest.raises(ValueError, match="iterations"):
            single(huber=v)
    with pytest.raises(ValueError, match="lane"):
        batch(iterations=3, method="lane", huber=5.0)
    assert ekf._huber_value(None, None) is None and ekf._huber_value(None, 3) is None
    for good in (5, 15.0, INF, np.float64(5.0), np.int32(3), 1e-300):
        assert ekf._huber_value(good, 3) == (float(good), None)
    arr = np.full(Zs, INF)
    got = ekf._huber_value(arr, 3)
    assert got[0] == 0.0 and got[1] is arr
    sig = inspect.signature(ekf.run_batch).parameters
    assert sig["huber"].default is None and list(sig)[-1] == "huber"
    sig = inspect.signature(ekf.EKF.update).parameters
    assert sig["huber"].default is None and list(sig)[-1] == "huber"
    doc = " ".join(ekf.run_batch.__doc__.split())
    assert "UNWEIGHTED" in doc and "REWEIGHTED model" in doc and "after n_iter" in doc
    assert "measurement's own units" in doc


# ---------------------------------------------------------------- the reference itself

@pytest.mark.parametrize("name,gate,delta,tol", CASES, ids=IDS)
def test_conditions_the_device_test_relies_on(name, gate, delta, tol):
    inp = rr.inputs(name)
    r = rr.reference(name, delta, tol, gate)   # asserts: counts, masks, status equal in both precisions; the margins
    nz, P = inp["nz"], inp["Z"].shape[2]
    hist = np.bincount(r["n_iter"].ravel())
    print(f"{name} gate {gate} delta {delta} tol {tol:g}: passes per step {hist.tolist()}, step margin "
          f"{r['step_margin']:.2e}, gate margin {r['gate_margin']:.2e}, smallest pivot / diagonal {r['margin']:.2e}, "
          f"floors {r['floor']}, bounds {r['bound']}")
    for key in ("n_iter", "rej", "status"):
        np.testing.assert_array_equal(r["f64"][key], r[key])
    assert r["step_margin"] >= ir.STEP_MARGIN == 1e-3
    assert r["gate_margin"] >= 1e-6
    assert r["margin"] > 1e-10 and not r["status"].any()
    assert r["n_iter"].max() < rr.CAP == 64                  # no step reached the cap
    assert (r["n_iter"][nz == 0] == 0).all() and (hist[2:] > 0).sum() >= 2     # several counts occur
    for key in rr.OUTPUTS:
        assert np.isfinite(r[key]).all() and 0.0 < r["floor"][key] < r["bound"][key]
    np.testing.assert_array_equal(r["S"], np.swapaxes(r["S"], -1, -2))
    # the weights: in (0, 1] on the applied rows, exactly 0 on every other row
    w = r["weights"]
    word = r["rej"].view(np.uint32)
    kept = (np.arange(P)[None, None, :] < nz[:, :, None]) & ~((word[:, :, None] >> np.arange(P, dtype=np.uint32)) & 1).astype(bool)
    assert w.shape == inp["Z"].shape and ((w > 0) == kept).all() and (w <= 1).all()
    np.testing.assert_array_equal(kept.sum(axis=2), r["nkept"])
    assert (w[kept] > 0.9).any()
    if gate is None:
        assert not r["rej"].any() and (r["n_iter"][nz > 0] >= 1).all()
        assert (w[kept] < 0.1).any()                         # the planted rows are applied, and downweighted
    else:
        none = (r["nkept"] == 0) & (nz > 0)
        assert r["rej"].any() and (r["n_iter"][none] == 0).all() and not r["nis"][r["nkept"] == 0].any()
    if name == "gnss":
        assert {0, 1, 31, 32} <= set(nz.ravel().tolist()) and P == 32 and nz.shape[0] == 70
    if name == "corr":
        R = inp["R"]
        assert np.abs(R - R * np.eye(P)).max() > 0           # a non-diagonal R
    if name == "car":
        assert inp["R"].ndim == 3                            # one R for the batch: r_bstride 0


@pytest.mark.parametrize("name,gate", [(n, None) for n in ir.CASES] + [(n, rr.GATE) for n in ir.GATED])
def test_an_infinite_delta_is_the_plain_reference_bitwise(name, gate):
    """On both families of inputs: the cold priors of tests/iekf_reference.py and the outlier sets."""
    g = np.inf if gate is None else gate
    sets = [rr.inputs(name)] if gate is not None else [ir.inputs(name), rr.inputs(name)]
    for inp in sets:
        plain = ir.run(inp, ir.KIND[name], ir.CAP[name], ir.TOL[name], g)
        for delta in (np.inf, np.full(inp["Z"].shape, np.inf)):
            got = rr.run(inp, ir.KIND[name], ir.CAP[name], ir.TOL[name], delta, g)
            for key in ("mu", "S", "nis", "loglik", "n_iter", "rej", "status", "nkept", "mp", "SP", "step_last"):
                np.testing.assert_array_equal(got[key], plain[key], err_msg=key)
            assert got["step_margin"] == plain["step_margin"] and got["gate_margin"] == plain["gate_margin"]
            P = inp["Z"].shape[2]
            word = plain["rej"].view(np.uint32)
            rejected = ((word[:, :, None] >> np.arange(P, dtype=np.uint32)) & 1).astype(bool)
            nz = np.where(inp["nz"] <= P, inp["nz"], 0)
            applied = (np.arange(P)[None, None, :] < nz[:, :, None]) & ~rejected
            ok = plain["status"] == 0          # (a filter whose state became NaN has NaN residuals, and weights)
            assert ok.sum() >= 60
            np.testing.assert_array_equal(got["om"][ok], applied[ok].astype(np.float64))   # exactly 1 and exactly 0


@pytest.mark.parametrize("name,gate,delta,tol", rr.PARITY[:2] + rr.PARITY[3:4], ids=IDS[:2] + IDS[3:4])
def test_the_converged_iterate_is_a_stationary_point_of_the_robust_map_cost(name, gate, delta, tol):
    """g = S-^-1 (x - mu-) - H^T R~(x)^-1 (z - h(x)), R~_jl = R_jl g_j g_l at x, at the final iterate
    of every step: the fixed-point equation of the recursion, and for a diagonal R half the gradient
    of (x - mu-)^T S-^-1 (x - mu-) + sum_j 2 (delta^2 / R_jj) (s_j - 1).  The form and the limit are
    tests/test_iekf_host.py's (not `bias`, as there: its bias row has a zero Jacobian row): the
    iterate is within the last step (<= tol in every component) of the fixed point x*, and
    |dg/dx| <= |A| with A = S-^-1 + H^T R~^-1 H, since d/dr (r / (R s)) = 1 / (R s^3) <= 1 / (R s);
    so |g| <= |A| sqrt(n) tol, and that is small beside |g|'s two terms.  Everything is taken from
    the longdouble run."""
    inp, kind, r = rr.inputs(name), rr.KIND[name], rr.reference(name, delta, tol, gate)
    L = np.longdouble
    hi = rr.run(inp, kind, rr.CAP, tol, rr.delta_array(inp, delta, L), dtype=L)
    Bn, T = inp["nz"].shape
    n = inp["mu0"].shape[1]
    worst_rel, worst_frac, done = 0.0, 0.0, 0
    for k in range(T):
        rows = inp["nz"][:, k].astype(np.int64)
        h, H = ir.meas_jac(kind, hi["mu"][:, k], inp["sat"][:, k].astype(L), rows)
        for b in range(Bn):
            ns = int(rows[b])
            if ns == 0 or r["n_iter"][b, k] == rr.CAP:
                continue
            R = (inp["R"][b, k] if inp["R"].ndim == 4 else inp["R"][k])[:ns, :ns].astype(np.float64)
            Hb, e = H[b, :ns].astype(np.float64), (inp["Z"][b, k, :ns].astype(L) - h[b, :ns]).astype(np.float64)
            g_ = (1.0 + (e / delta) ** 2) ** 0.25
            np.testing.assert_allclose(1.0 / g_ ** 2, r["weights"][b, k, :ns], rtol=0, atol=1e-3)   # the reported omega
            Rt = R * np.outer(g_, g_)
            Si = np.linalg.inv(hi["SP"][b, k].astype(np.float64))
            t1 = Si @ (hi["mu"][b, k] - hi["mp"][b, k]).astype(np.float64)
            t2 = Hb.T @ np.linalg.solve(Rt, e)
            A = Si + Hb.T @ np.linalg.solve(Rt, Hb)
            g = np.linalg.norm(t1 - t2)
            lim = np.linalg.norm(A, 2) * np.sqrt(n) * tol + 1e-9 * max(np.linalg.norm(t1), np.linalg.norm(t2))
            worst_frac = max(worst_frac, g / lim)
            if max(np.linalg.norm(t1), np.linalg.norm(t2)) > 0:
                worst_rel = max(worst_rel, g / max(np.linalg.norm(t1), np.linalg.norm(t2)))
            done += 1
    print(f"{name}: {done} converged steps, worst |g| / limit {worst_frac:.2e}, worst |g| / max(|term|) {worst_rel:.2e}")
    assert done > 50 and worst_frac <= 1.0 and worst_rel <= 1e-3


def final_position_errors(inp, mu_last):
    """|position - x_f| per filter: the gnss sets' pseudoranges were simulated at the fixture's last state."""
    return np.linalg.norm(mu_last[:, :3] - inp["fx"]["mu"][-1][:3], axis=1)


def test_soft_weights_recover_the_position_on_the_outlier_set():
    """gnss, delta = 5 m, no gate: the median final position error is below a quarter of the plain
    iterated run's on the same inputs."""
    inp, r = rr.inputs("gnss"), rr.reference("gnss", 5.0, 3e-4)
    plain = ir.run(inp, ir.KIND["gnss"], rr.CAP, 3e-4)
    e_r, e_p = final_position_errors(inp, r["mu"][:, -1]), final_position_errors(inp, plain["mu"][:, -1])
    print(f"final position error, median / max: robust {np.median(e_r):.2f} / {e_r.max():.2f} m, plain iterated "
          f"{np.median(e_p):.2f} / {e_p.max():.2f} m")
    assert np.median(e_r) < 0.25 * np.median(e_p)


def test_every_planted_row_weighs_less_than_every_clean_row():
    inp, r = rr.inputs("gnss"), rr.reference("gnss", 5.0, 3e-4)
    w, planted = r["weights"], inp["planted"]
    applied = w > 0
    assert (applied & planted).sum() > 500 and (applied & ~planted).sum() > 5000
    hi, lo = w[applied & planted].max(), w[applied & ~planted].min()
    print(f"omega: largest on a planted row {hi:.3f}, smallest on a clean row {lo:.3f}")
    assert hi < lo
