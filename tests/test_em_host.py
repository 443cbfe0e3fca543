"""Noise identification for the EKF (mhe_ekf_smooth_args, mhe_ekf_em_stats, utils.ekf.smooth_batch
lag_one=, em_stats, fit_noise): everything that needs no device.

  * the two symbols are exported, declared in include/mhe.h and bound in mhe._lib; the structs'
    fields are in the header's order; the ABI version did not move and mhe_ekf_smooth kept its
    signature (nothing that existed changed);
  * the C entry points' refusals, which all precede the launch (host addresses are handed in and
    never dereferenced);
  * properties of tests/em_reference.py, the reference of tests/test_gpu_em.py, on that file's
    inputs (tests/ekf_ragged.py): its plug-ins are the oracle's, its smoother is
    tests/rts_reference.py's, C_k is the off-diagonal block of the joint smoothed covariance of
    a dense batch solve, every W_k is positive semidefinite, a predict-only history counts no
    row, and the committed fit fixture is the recipe's output and passes the recipe's condition;
  * utils.ekf.smooth_batch, em_stats and fit_noise refuse bad shapes, unregistered plug-ins and
    bad keywords before they load the library.
"""
import ctypes
import os
import re

import numpy as np
import pytest

import ekf_ragged as er
import em_reference as em
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
    d = _lib.MheEkfDims(n=5, m=3, pmax=8, q=3, dyn_model=1, meas_model=1, dt=1.0) if model == "gnss" else \
        _lib.MheEkfDims(n=9, m=2, pmax=8, q=3, dyn_model=2, meas_model=3, dt=0.1)
    if model == "car":
        for i, v in enumerate(CAR):
            d.dyn_par[i] = v
    for k, v in kw.items():
        setattr(d, k, v)
    return d


def _header_struct(name):
    hdr = open(os.path.join(ROOT, "include", "mhe.h")).read()
    body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (name, name), hdr, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    names = []
    for decl in body.split(";"):
        decl = decl.strip()
        if decl:
            names += [w.strip(" *") for w in re.sub(r"^(const\s+)?\w+\s*\*?", "", decl, count=1).split(",")]
    return names


# ---------------------------------------------------------------- ABI

def test_symbols_are_exported_declared_and_bound():
    lib = ctypes.CDLL(_lib.LIB_PATH)
    hdr = open(os.path.join(ROOT, "include", "mhe.h")).read()
    assert "#define MHE_ABI_VERSION 11" in hdr
    for sym, struct, cls in (("mhe_ekf_smooth_args", "mhe_ekf_lag_args", _lib.MheEkfLagArgs),
                             ("mhe_ekf_em_stats", "mhe_em_args", _lib.MheEmArgs)):
        assert hasattr(lib, sym)
        assert re.search(r"\bint %s\(const mhe_ekf_dims\* dims, const %s\* args, void\* stream\);" % (sym, struct), hdr)
        res, args = _lib.SIGNATURES[sym]
        assert res is ctypes.c_int and args == [ctypes.POINTER(_lib.MheEkfDims), ctypes.POINTER(cls), ctypes.c_void_p]
        assert getattr(_lib.load(), sym).argtypes == args
        assert [f[0] for f in cls._fields_] == _header_struct(struct)
        assert cls._fields_[0] == ("struct_size", ctypes.c_int32) and cls().struct_size == ctypes.sizeof(cls)
    # what existed is as it was
    assert re.search(r"\bint mhe_ekf_smooth\(const mhe_ekf_dims\* dims, int32_t batch, int32_t steps,", hdr)
    assert len(_lib.SIGNATURES["mhe_ekf_smooth"][1]) == 16
    # the lag-one struct is mhe_ekf_smooth's argument list, then C
    assert [f[0] for f in _lib.MheEkfLagArgs._fields_][1:] == \
        ["batch", "steps", "mu_hist", "S_hist", "U", "u_bstride", "Q", "mu0", "S0", "mu_s", "S_s", "mu0_s", "S0_s",
         "status", "C"]


def _host_ptr():
    buf = (ctypes.c_double * 4096)()
    return buf, ctypes.addressof(buf)


def test_smooth_args_refusals_precede_the_launch():
    run = _lib.load().mhe_ekf_smooth_args
    buf, p = _host_ptr()                              # a host address: never dereferenced, nothing is launched
    A = _lib.MheEkfLagArgs
    assert run(None, ctypes.byref(A(batch=4, steps=5)), None) == E_NULL
    assert run(ctypes.byref(_dims()), None, None) == E_NULL
    req = ("mu_hist", "S_hist", "U", "Q", "mu_s", "S_s")
    for model in ("gnss", "car"):
        d = _dims(model)
        assert run(ctypes.byref(d), ctypes.byref(A(batch=4, steps=5)), None) == E_NULL
        for miss in req + ("C_too",):
            kw = {k: p for k in req if k != miss}
            assert run(ctypes.byref(d), ctypes.byref(A(batch=4, steps=5, C=p, **kw)), None) == \
                (E_DIMS if miss == "C_too" else E_NULL), miss        # all given: C overlaps everything
        full = {k: p for k in req}
        assert run(ctypes.byref(d), ctypes.byref(A(batch=4, steps=5, mu0_s=p, **full)), None) == E_NULL
        assert run(ctypes.byref(d), ctypes.byref(A(batch=4, steps=5, S0_s=p, mu0=p, **full)), None) == E_NULL
        assert run(ctypes.byref(d), ctypes.byref(A(batch=-1, steps=5)), None) == E_DIMS
        assert run(ctypes.byref(d), ctypes.byref(A(batch=4, steps=-1)), None) == E_DIMS
        assert run(ctypes.byref(d), ctypes.byref(A(batch=0, steps=5)), None) == OK      # empty: nothing is read
        assert run(ctypes.byref(d), ctypes.byref(A(batch=4, steps=0)), None) == OK
        for size in (0, ctypes.sizeof(A) - 8, ctypes.sizeof(A) + 8):                    # stale binding of the args
            a = A(batch=0, steps=5)
            a.struct_size = size
            assert run(ctypes.byref(d), ctypes.byref(a), None) == E_DIMS
        for size in (0, d.struct_size - 4, d.struct_size + 8):
            assert run(ctypes.byref(_dims(model, struct_size=size)), ctypes.byref(A(batch=0, steps=5)), None) == E_DIMS
        # C must not share a byte with an input or another output; every other pointer apart
        n = d.n
        step = 4 * 5 * n * n * 8
        sep = {k: p + (i + 1) * step for i, k in enumerate(req)}
        for k in req:
            assert run(ctypes.byref(d), ctypes.byref(A(batch=4, steps=5, C=sep[k] + 8, **sep)), None) == E_DIMS, k
    assert run(ctypes.byref(_dims("gnss", dyn_model=3)), ctypes.byref(A(batch=4, steps=5)), None) == E_MODEL
    assert run(ctypes.byref(_dims("gnss", n=9)), ctypes.byref(A(batch=4, steps=5)), None) == E_MODEL
    dcar = _dims("car")
    dcar.dyn_par[2] = 0.0
    assert run(ctypes.byref(dcar), ctypes.byref(A(batch=4, steps=5)), None) == E_DIMS


def test_em_stats_refusals_precede_the_launch():
    run = _lib.load().mhe_ekf_em_stats
    buf, p = _host_ptr()
    A = _lib.MheEmArgs
    assert run(None, ctypes.byref(A(batch=4, steps=5)), None) == E_NULL
    assert run(ctypes.byref(_dims()), None, None) == E_NULL
    req = ("mu_s", "S_s", "C", "U", "Z", "nz", "PAR", "Qsum", "q_cnt", "r2", "r_cnt")
    for model in ("gnss", "car"):
        d = _dims(model)
        assert run(ctypes.byref(d), ctypes.byref(A(batch=4, steps=5)), None) == E_NULL
        for miss in req:
            kw = {k: p for k in req if k != miss}
            assert run(ctypes.byref(d), ctypes.byref(A(batch=4, steps=5, **kw)), None) == E_NULL, miss
        full = {k: p for k in req}
        assert run(ctypes.byref(d), ctypes.byref(A(batch=4, steps=5, mu0_s=p, **full)), None) == E_NULL
        assert run(ctypes.byref(d), ctypes.byref(A(batch=4, steps=5, S0_s=p, **full)), None) == E_NULL
        assert run(ctypes.byref(d), ctypes.byref(A(batch=-1, steps=5)), None) == E_DIMS
        assert run(ctypes.byref(d), ctypes.byref(A(batch=4, steps=-1)), None) == E_DIMS
        assert run(ctypes.byref(d), ctypes.byref(A(batch=0, steps=5)), None) == OK
        assert run(ctypes.byref(d), ctypes.byref(A(batch=4, steps=0)), None) == OK
        for size in (0, ctypes.sizeof(A) - 8, ctypes.sizeof(A) + 8):
            a = A(batch=0, steps=5)
            a.struct_size = size
            assert run(ctypes.byref(d), ctypes.byref(a), None) == E_DIMS
        for size in (0, d.struct_size - 4, d.struct_size + 8):
            assert run(ctypes.byref(_dims(model, struct_size=size)), ctypes.byref(A(batch=0, steps=5)), None) == E_DIMS
        for bad in (dict(pmax=0), dict(pmax=33), dict(q=2)):
            assert run(ctypes.byref(_dims(model, **bad)), ctypes.byref(A(batch=4, steps=5, **full)), None) == E_DIMS, bad
    for bad in (dict(dyn_model=0), dict(dyn_model=3), dict(n=9), dict(m=2), dict(meas_model=3), dict(meas_model=0)):
        assert run(ctypes.byref(_dims("gnss", **bad)), ctypes.byref(A(batch=4, steps=5)), None) == E_MODEL, bad
    for bad in (dict(n=5), dict(meas_model=1), dict(meas_model=2)):
        assert run(ctypes.byref(_dims("car", **bad)), ctypes.byref(A(batch=4, steps=5)), None) == E_MODEL, bad
    assert run(ctypes.byref(_dims("gnss", meas_model=2)), ctypes.byref(A(batch=4, steps=5)), None) == E_NULL
    for i in (2, 5):
        d = _dims("car")
        d.dyn_par[i] = 0.0
        assert run(ctypes.byref(d), ctypes.byref(A(batch=4, steps=5)), None) == E_DIMS


# ---------------------------------------------------------------- the reference itself

@pytest.fixture(scope="module")
def gnss_case():
    inp = er.gnss_inputs(6)
    inp["hist"] = er.oracle_run(inp)[:2]
    return inp, em.GNSS, oekf.gnss_pos_and_bias, oekf.multi_pseudorange


@pytest.fixture(scope="module")
def car_case():
    inp = er.autocar_inputs(3)
    inp["hist"] = er.oracle_run(inp, dyn=oekf.discrete_vehicle_dynamics, meas=oekf.vehicle_sensors_model)[:2]
    return inp, em.CAR, oekf.discrete_vehicle_dynamics, oekf.vehicle_sensors_model


def test_reference_plugins_are_the_oracles(gnss_case, car_case):
    rng = np.random.default_rng(3)
    for (inp, kind, odyn, omeas) in (gnss_case, car_case):
        mh = inp["hist"][0]
        for b in range(mh.shape[0]):
            k = int(rng.integers(1, mh.shape[1]))
            f, F = em.dynamics(kind, mh[b:b + 1, k], inp["U"][b:b + 1, k], inp["dparams"], np.float64)
            of, oF = odyn(mh[b, k], inp["U"][b, k], params=inp["dparams"], jac=True)
            np.testing.assert_allclose(f[0], of, rtol=1e-14, atol=0)
            np.testing.assert_allclose(F[0], oF, rtol=1e-13, atol=1e-300)
            ns = max(int(inp["nz"][b, k]), 1)
            h, H, valid = em.measurement(kind, mh[b:b + 1, k], inp["sat"][b:b + 1, k], np.array([ns]), np.float64)
            oh, oH = omeas(mh[b, k], params={"sat_pos": inp["sat"][b, k, :ns]}, jac=True)
            np.testing.assert_allclose(h[0, :ns], oh, rtol=1e-15, atol=0)
            np.testing.assert_allclose(H[0, :ns], oH, rtol=1e-13, atol=0)
            assert valid[0].sum() == ns and not h[0, ns:].any() and not H[0, ns:].any()
    x = gnss_case[0]["hist"][0][:1, 3]                       # the bias variant: last row h = x[3], zero Jacobian row
    sat = gnss_case[0]["sat"][:1, 3, :13]
    h, H, _ = em.measurement(em.BIAS, x, sat, np.array([5]), np.float64)
    oh, oH = oekf.multi_pseudorange_and_bias(x[0], params={"sat_pos": sat[0, :4]}, jac=True)
    np.testing.assert_allclose(h[0, :5], oh, rtol=1e-15)
    np.testing.assert_allclose(H[0, :5], oH, rtol=1e-13)
    assert h[0, 4] == x[0, 3] and not H[0, 4].any()


def test_reference_smoother_is_the_rts_reference_and_forward_is_the_oracle(gnss_case, car_case):
    for (inp, kind, odyn, omeas) in (gnss_case, car_case):
        mh, Sh = inp["hist"]
        want = rts.smooth_batch(odyn, mh, Sh, inp["U"], inp["Q"], inp["dparams"], inp["mu0"], inp["S0"])
        got = em.smooth(kind, mh, Sh, inp["U"], inp["Q"], inp["dparams"], inp["mu0"], inp["S0"])
        for g, w in zip((got["mu_s"], got["S_s"], got["mu0_s"], got["S0_s"]), want):
            scale = np.abs(w).max()
            assert np.abs(g - w).max() <= 1e-9 * (1 + scale)
        nop = em.smooth(kind, mh, Sh, inp["U"], inp["Q"], inp["dparams"])
        assert np.isnan(nop["C"][:, 0]).all() and not np.isnan(nop["C"][:, 1:]).any() and "mu0_s" not in nop
        np.testing.assert_array_equal(nop["C"][:, 1:], got["C"][:, 1:])
        assert not np.isnan(got["C"]).any()
        fm, fS, _ = em.forward(kind, inp["mu0"], inp["S0"], inp["U"], inp["Z"], inp["nz"], inp["sat"], inp["Q"],
                               inp["R"], inp["dparams"])
        print(f"{kind['name']}: forward vs oracle mu {np.abs(fm - mh).max():.2e}, S {np.abs(fS - Sh).max():.2e}")
        assert np.abs(fm - mh).max() <= 1e-8 * (1 + np.abs(mh).max()) and np.abs(fS - Sh).max() <= 1e-8 * np.abs(Sh).max()


def test_lag_one_is_the_joint_covariances_off_diagonal_block():
    """gnss dynamics are linear, and the EKF is the Kalman filter of the model linearised where it
    linearised (H at the predictions).  For T = 4 the joint posterior of (x_-1, x_0 .. x_3) has the
    information matrix J = prior + sum_k [-F I]^T Q^-1 [-F I] + sum_k H_k^T R_k^-1 H_k; C_k must be
    block (k, k-1) of J^-1 and Ss_k its diagonal block.  Dense float64 solve: the tolerance is
    cond(J) eps, printed."""
    inp = er.gnss_inputs(4, T=4, pmax=8, nz=np.array([[8, 5, 0, 7], [4, 8, 8, 1], [0, 0, 6, 8], [8, 8, 8, 8]]))
    n, T = 5, 4
    mh, Sh, _, Hs = em.forward(em.GNSS, inp["mu0"], inp["S0"], inp["U"], inp["Z"], inp["nz"], inp["sat"], inp["Q"],
                               inp["R"], inp["dparams"], keep_H=True)
    sm = em.smooth(em.GNSS, mh, Sh, inp["U"], inp["Q"], inp["dparams"], inp["mu0"], inp["S0"])
    F = np.eye(n)
    F[3, 4] = 1.0
    Qi = np.linalg.inv(inp["Q"])
    worst = 0.0
    for b in range(4):
        J = np.zeros(((T + 1) * n, (T + 1) * n))
        J[:n, :n] = np.linalg.inv(inp["S0"][b])
        for k in range(T):
            A = np.zeros((n, (T + 1) * n))
            A[:, k * n:(k + 1) * n], A[:, (k + 1) * n:(k + 2) * n] = -F, np.eye(n)
            J += A.T @ Qi @ A
            H, R = Hs[k][0][b], Hs[k][1][b]                  # rows beyond nz: zero rows of H, unit R
            blk = slice((k + 1) * n, (k + 2) * n)
            J[blk, blk] += H.T @ np.linalg.solve(R, H)
        P = np.linalg.inv(J)
        tol = np.linalg.cond(J) * np.finfo(float).eps * np.abs(P).max() * 8
        for k in range(T):
            cur, prev = slice((k + 1) * n, (k + 2) * n), slice(k * n, (k + 1) * n)
            eC, eS = np.abs(sm["C"][b, k] - P[cur, prev]).max(), np.abs(sm["S_s"][b, k] - P[cur, cur]).max()
            worst = max(worst, eC / tol, eS / tol)
            assert eC <= tol and eS <= tol, (b, k, eC, eS, tol)
        assert np.abs(sm["S0_s"][b] - P[:n, :n]).max() <= tol
        assert np.abs(sm["C"][b, 1] - sm["C"][b, 1].T).max() > 1e-6 * np.abs(sm["C"][b, 1]).max()   # not symmetric
    print(f"lag-one against the dense joint covariance: worst error / (8 cond(J) eps max|P|) = {worst:.2e}")


def test_every_W_is_positive_semidefinite(gnss_case, car_case):
    for (inp, kind, odyn, omeas) in (gnss_case, car_case):
        mh, Sh = inp["hist"]
        sm = em.smooth(kind, mh, Sh, inp["U"], inp["Q"], inp["dparams"], inp["mu0"], inp["S0"])
        st = em.stats(kind, sm["mu_s"], sm["S_s"], sm["C"], inp["U"], inp["Z"], inp["nz"], inp["sat"], inp["dparams"],
                      sm["mu0_s"], sm["S0_s"], keep_W=True)
        W = st["W"]
        assert W.shape[1] == mh.shape[1] and (st["q_cnt"] == mh.shape[1]).all() and not st["status"].any()
        lo = np.linalg.eigvalsh(0.5 * (W + np.swapaxes(W, -1, -2))).min(-1)
        scale = np.abs(W).reshape(W.shape[:2] + (-1,)).max(-1)
        print(f"{kind['name']}: min eig(W_k) / max|W_k| = {(lo / scale).min():.2e}")
        assert (lo >= -1e-9 * scale).all()
        np.testing.assert_array_equal(st["Qsum"], np.swapaxes(st["Qsum"], -1, -2))
        assert (st["r_cnt"] == np.minimum(inp["nz"], inp["Z"].shape[2]).sum(1)).all()
        assert (st["r2"] >= 0).all() and not st["r2"][np.arange(inp["Z"].shape[2])[None, None] >= inp["nz"][..., None]].any()
        nop = em.stats(kind, sm["mu_s"], sm["S_s"], sm["C"], inp["U"], inp["Z"], inp["nz"], inp["sat"], inp["dparams"])
        assert (nop["q_cnt"] == mh.shape[1] - 1).all()


def test_a_predict_only_history_counts_no_row(gnss_case, car_case):
    for (inp, kind, odyn, omeas) in (gnss_case, car_case):
        nz0 = np.zeros_like(inp["nz"])
        mh, Sh, ll = em.forward(kind, inp["mu0"], inp["S0"], inp["U"], inp["Z"], nz0, inp["sat"], inp["Q"], inp["R"],
                                inp["dparams"])
        assert not ll.any()
        sm = em.smooth(kind, mh, Sh, inp["U"], inp["Q"], inp["dparams"], inp["mu0"], inp["S0"])
        st = em.stats(kind, sm["mu_s"], sm["S_s"], sm["C"], inp["U"], inp["Z"], nz0, inp["sat"], inp["dparams"],
                      sm["mu0_s"], sm["S0_s"])
        assert not st["r_cnt"].any() and not st["r2"].any() and not st["status"].any()
        # and with nothing observed the smoothed history is the filtered one, so E[W_k] = Q exactly
        T = mh.shape[1]
        err = np.abs(st["Qsum"] / T - inp["Q"]).max()
        print(f"{kind['name']}: predict-only |Qsum / T - Q| = {err:.2e}")
        assert err <= 1e-9 * np.abs(Sh).max()


def test_the_fit_fixture_is_the_recipe_and_meets_its_condition():
    d = em.fit_inputs()
    made = em.make_fit_recipe()
    for k, v in made.items():
        np.testing.assert_array_equal(d[k], v, err_msg=k)
    assert d["Z"].shape == (8, 40, 8) and os.path.getsize(em.FIT_FIXTURE) < 1 << 20
    r = em.fit_reference()
    ll = np.asarray(r["f64"]["loglik"], dtype=np.float64)
    print("reference loglik per round:", np.array2string(ll, precision=1))
    print(f"smallest gain {np.diff(ll).min():.2f}; r {em.FIT_R_START} -> {100 * float(r['rho']):.3f}; "
          f"diag Q -> {np.diag(r['Q'])}")
    assert ll.shape == (em.FIT_ROUNDS,) and (np.diff(ll) >= 1.0).all()          # the recipe's condition
    assert abs(em.FIT_R_START * float(r["rho"]) - em.FIT_R_TRUE) < abs(em.FIT_R_START - em.FIT_R_TRUE)
    q0, qt = np.diag(em.FIT_Q_SCALE * em.FIT_Q_TRUE), np.diag(em.FIT_Q_TRUE)
    assert (np.abs(np.diag(r["Q"]) - qt) < np.abs(q0 - qt)).all()
    lo = np.linalg.eigvalsh(r["Q"])
    assert lo.min() > 0


# ---------------------------------------------------------------- the host wrappers

def _no_load(monkeypatch):
    def no_load(*a, **k):
        raise AssertionError("the library was loaded")
    monkeypatch.setattr(_lib, "load", no_load)


def test_smooth_batch_lag_one_refuses_before_loading_the_library(monkeypatch, gnss_case):
    _no_load(monkeypatch)
    inp = gnss_case[0]
    mh, Sh = inp["hist"]
    good = (gnss.gnss_pos_and_bias, mh, Sh, inp["U"], inp["Q"], 1.0)
    for bad in (1, 0, None, "yes", np.int32(1)):
        with pytest.raises(ValueError):
            ekf.smooth_batch(*good, lag_one=bad)
    with pytest.raises(ValueError):
        ekf.smooth_batch(good[0], mh[:, :, :4], *good[2:], lag_one=True)
    with pytest.raises(UnsupportedPlugin):
        ekf.smooth_batch(lambda x, u, params=None, jac=False: (x, np.eye(5)), *good[1:], lag_one=True)
    import inspect
    assert list(inspect.signature(ekf.smooth_batch).parameters)[-1] == "lag_one"


def test_em_stats_refuses_before_loading_the_library(monkeypatch, gnss_case):
    _no_load(monkeypatch)
    inp = gnss_case[0]
    mh, Sh = inp["hist"]
    B, T, n = mh.shape
    good = [gnss.gnss_pos_and_bias, gnss.multi_pseudorange, mh, Sh, Sh.copy(), inp["U"], inp["Z"], inp["nz"], 1.0,
            inp["sat"]]
    for i, bad in ((2, mh[:, :, :4]), (2, mh[0]), (3, Sh[:, :-1]), (4, Sh[:, :, :4]), (5, inp["U"][:, :-1]),
                   (6, inp["Z"][:-1]), (6, np.zeros((B, T, 33))), (7, inp["nz"][:, :-1]), (9, inp["sat"][..., :2]),
                   (9, inp["sat"][:, :, :-1])):
        a = list(good)
        a[i] = bad
        with pytest.raises(ValueError):
            ekf.em_stats(*a)
    with pytest.raises(ValueError):
        ekf.em_stats(*good, inputs="batch_inner")                  # the inputs are batch-outermost
    with pytest.raises(ValueError):
        ekf.em_stats(*good, inputs="sideways")
    with pytest.raises(ValueError):
        ekf.em_stats(*good, mu0_s=inp["mu0"])                      # a smoothed prior is mu0_s and S0_s
    with pytest.raises(ValueError):
        ekf.em_stats(*good, mu0_s=inp["mu0"][:-1], S0_s=inp["S0"])
    with pytest.raises(ValueError):
        ekf.em_stats(*good, rejected=np.zeros((B, T + 1), np.int32))
    with pytest.raises(UnsupportedPlugin):
        ekf.em_stats("gnss_pos_and_bias", "vehicle_sensors_model", *good[2:])       # not a compiled pair

    def multi_pseudorange(x, params=None, jac=False):              # registered name, other math
        y, J = oekf.multi_pseudorange(x, params=params, jac=True)
        return y + 1e-3, J
    with pytest.raises(UnsupportedPlugin):
        ekf.em_stats(good[0], multi_pseudorange, *good[2:])
    with pytest.raises(UnsupportedPlugin):
        ekf.em_stats(lambda x, u, params=None, jac=False: (x, np.eye(5)), *good[1:])


def test_fit_noise_refuses_before_loading_the_library(monkeypatch, gnss_case):
    _no_load(monkeypatch)
    inp = gnss_case[0]
    good = [gnss.gnss_pos_and_bias, gnss.multi_pseudorange, inp["mu0"], inp["S0"], inp["U"], inp["Z"], inp["nz"],
            inp["Q"], inp["R"], 1.0, inp["sat"]]
    for kw in (dict(rounds=0), dict(rounds=-3), dict(rounds=2.0), dict(rounds=True), dict(rounds=None),
               dict(rounds=ekf.MAX_ROUNDS + 1), dict(fit_Q=1), dict(fit_R="no"), dict(fit_R=None),
               dict(q_structure="band"), dict(q_structure=None), dict(gate=0.0), dict(gate=-1.0), dict(gate=True),
               dict(inputs="sideways"), dict(inputs="batch_inner")):
        with pytest.raises(ValueError):
            ekf.fit_noise(*good, **kw)
    for i, bad in ((2, inp["mu0"][:, :4]), (3, inp["S0"][:-1]), (4, inp["U"][:, :-1]), (5, inp["Z"][0]),
                   (6, inp["nz"][:-1]), (7, inp["Q"][:4, :4]), (8, inp["R"][:, :, :-1]), (8, inp["R"][0, 0]),
                   (10, inp["sat"][..., :2])):
        a = list(good)
        a[i] = bad
        with pytest.raises(ValueError):
            ekf.fit_noise(*a)
    with pytest.raises(UnsupportedPlugin):
        ekf.fit_noise("gnss_pos_and_bias", "vehicle_sensors_model", *good[2:])
    with pytest.raises(UnsupportedPlugin):
        ekf.fit_noise(lambda x, u, params=None, jac=False: (x, np.eye(5)), *good[1:])
