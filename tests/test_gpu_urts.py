"""Unscented RTS smoother on the device (csrc/mhe_ukf.hip k_ukf_rts, mhe_ukf_smooth,
utils.ukf.smooth_batch).

Reference: tests/urts_reference.py, the recursion of include/mhe.h in NumPy, run in float64 and in
np.longdouble on the float64 forward history of tests/ukf_reference.py, once per process.  The
device smoother runs on that same uploaded history and is compared with the longdouble run; per
case and output, floor = max |float64 run - longdouble run| and
    bound = 8 * floor + 1e-10 * (1 + max |ref|).
tests/test_urts_host.py asserts that every reference run ends with status 0 and that no Cholesky
pivot is near zero, so the device cannot disagree about status.
Inputs: B = 70 (17 full workgroups and one of two waves), T = 12 (T = 61 for the car).
"""
import ctypes

import numpy as np
import pytest
import torch

import ukf_reference as ur
import urts_reference as urts
from mhe import _lib
import utils.ekf as ekf
import utils.ukf as ukf

pytestmark = pytest.mark.gpu

ALONE = (0, 5, 69)
ALL = [(name, params) for name in ur.CASES for params in ur.PARAMS]
DEV = "cuda"


def _np(t):
    return None if t is None else t.cpu().numpy()


def _hist(a, layout):
    """A (B, T, ...) history on the device: contiguous batch-outermost, or run_batch's form (a
    batch-outermost view of batch-innermost storage)."""
    a = np.asarray(a)
    if layout == "outer":
        return torch.as_tensor(np.array(a), device=DEV)
    st = torch.as_tensor(np.array(np.moveaxis(a, 0, -1), order="C"), device=DEV)
    return st.permute(st.dim() - 1, *range(st.dim() - 1))


def _smooth(name, mh, Sh, params=ur.PARAMS[0], inputs="batch_outer", prior=True, inp=None, **kw):
    """utils.ukf.smooth_batch on a case's U, Q, dt, dyn_params (and prior); NumPy copies."""
    inp = ur.inputs(name) if inp is None else inp
    T = mh.shape[1]
    U = inp["U"][:, :T]
    U = U if inputs == "batch_outer" else np.ascontiguousarray(np.moveaxis(U, 0, -1))
    pr = dict(mu0=inp["mu0"], S0=inp["S0"]) if prior else {}
    out = ukf.smooth_batch(ur.KIND[name]["dyn"], mh, Sh, U, inp["Q"], inp["dparams"]["dt"], dyn_params=inp["dparams"],
                           inputs=inputs, alpha=params[0], beta=params[1], kappa=params[2], **pr, **kw)
    if "stream" in kw:
        kw["stream"].synchronize()
    return [_np(t) for t in out]


def _sub(inp, idx):
    out = dict(inp)
    for key in ("mu0", "S0", "U"):
        out[key] = np.ascontiguousarray(inp[key][idx])
    return out


@pytest.fixture(scope="module")
def device():
    """The device smoother on the uploaded reference history with the prior, batch-innermost
    history and batch-outermost U, per (case, parameters)."""
    cache = {}

    def get(name, params=ur.PARAMS[0]):
        if (name, params) not in cache:
            mh, Sh = urts.history(name, params)
            cache[name, params] = _smooth(name, _hist(mh, "inner"), _hist(Sh, "inner"), params)
        return cache[name, params]
    return get


@pytest.mark.parametrize("name,params", ALL)
def test_parity(device, name, params):
    """Both history layouts x both U layouts x with and without the prior against the longdouble
    run; the eight calls agree bitwise with one another."""
    ref = urts.reference(name, params)
    mh, Sh = urts.history(name, params)
    base = device(name, params)
    for layout in ("inner", "outer"):
        dm, dS = _hist(mh, layout), _hist(Sh, layout)
        assert ekf._hist_storage(dm, (mh.shape[2],))[1] == (layout == "inner")
        for inputs in ("batch_outer", "batch_inner"):
            for prior in (True, False):
                got = _smooth(name, dm, dS, params, inputs, prior)
                assert len(got) == (5 if prior else 3)
                np.testing.assert_array_equal(got[2], ref["status"])
                assert not got[2].any()
                for g, w in zip(got, base):
                    np.testing.assert_array_equal(g, w)
    got = dict(zip(("mu_s", "S_s", "status", "mu0_s", "S0_s"), base))
    errs = {k: float(np.max(np.abs(got[k] - ref[k]))) for k in urts.OUTPUTS}
    print(f"{name} {params}: " + ", ".join(
        f"{k} observed {errs[k]:.2e} floor {ref['floor'][k]:.2e} bound {ref['bound'][k]:.2e}" for k in urts.OUTPUTS))
    for k in urts.OUTPUTS:
        assert np.isfinite(got[k]).all()
        assert errs[k] <= ref["bound"][k], (k, errs[k], ref["bound"][k])


@pytest.mark.parametrize("name,params", [("gnss", ur.PARAMS[0]), ("car", ur.PARAMS[1])])
def test_end_to_end(name, params):
    """utils.ukf.run_batch on the device, then smooth_batch on its batch-innermost views (no
    copy), against the reference smoother run on that device history; same form of bound."""
    inp, k = ur.inputs(name), ur.KIND[name]
    U, Z, nz, sat = ur.er.device_args(inp)
    mh, Sh, _, _, st = ukf.run_batch(k["dyn"], k["meas"], inp["mu0"], inp["S0"], U, Z, nz, inp["Q"], inp["R"],
                                     inp["dparams"]["dt"], sat, dyn_params=inp["dparams"], alpha=params[0],
                                     beta=params[1], kappa=params[2])
    assert not _np(st).any()
    n = mh.shape[2]
    st_mu, bi_mu = ekf._hist_storage(mh, (n,))
    st_S, bi_S = ekf._hist_storage(Sh, (n, n))
    assert bi_mu and bi_S and st_mu.data_ptr() == mh.data_ptr() and st_S.data_ptr() == Sh.data_ptr()
    got = dict(zip(("mu_s", "S_s", "status", "mu0_s", "S0_s"), _smooth(name, mh, Sh, params)))
    ref = urts.on_history(name, params, _np(mh), _np(Sh))
    assert not ref["status"].any() and not got["status"].any() and ref["margin"] >= 0.05
    for key in urts.OUTPUTS:
        err = float(np.max(np.abs(got[key] - ref[key])))
        print(f"end to end {name} {params} {key}: observed {err:.2e} floor {ref['floor'][key]:.2e} "
              f"bound {ref['bound'][key]:.2e}")
        assert err <= ref["bound"][key], (key, err, ref["bound"][key])


@pytest.mark.parametrize("name", ["gnss", "car"])
def test_symmetry_last_step_and_lower_triangle(device, name):
    mh, Sh = urts.history(name)
    ms, Ss, st, m0s, S0s = device(name)
    np.testing.assert_array_equal(Ss, np.swapaxes(Ss, -1, -2))           # bitwise symmetric
    np.testing.assert_array_equal(S0s, np.swapaxes(S0s, -1, -2))
    np.testing.assert_array_equal(ms[:, -1], mh[:, -1])                   # the last step is the filtered one
    np.testing.assert_array_equal(Ss[:, -1], Sh[:, -1])
    assert np.abs(ms[:, :-1] - mh[:, :-1]).max() > 0
    # only the upper triangle of S_hist is read
    n = mh.shape[2]
    poisoned = np.array(Sh)
    poisoned[:, :, np.tril_indices(n, -1)[0], np.tril_indices(n, -1)[1]] = np.nan
    for layout in ("inner", "outer"):
        got = _smooth(name, _hist(mh, layout), _hist(poisoned, layout))
        for g, w in zip(got, device(name)):
            np.testing.assert_array_equal(g, w)


@pytest.mark.parametrize("name", ["gnss", "car"])
def test_a_filter_alone_is_bitwise_its_result_in_the_batch(device, name):
    full = device(name)
    inp = ur.inputs(name)
    mh, Sh = urts.history(name)
    for b in ALONE:
        alone = _smooth(name, _hist(mh[[b]], "inner"), _hist(Sh[[b]], "inner"), inp=_sub(inp, [b]))
        for a, f in zip(alone, full):
            np.testing.assert_array_equal(a[0], f[b])
    idx = list(ALONE)                                                     # and in another batch, at another place
    some = _smooth(name, _hist(mh[idx], "outer"), _hist(Sh[idx], "outer"), inp=_sub(inp, idx))
    for a, f in zip(some, full):
        np.testing.assert_array_equal(a, f[idx])


@pytest.mark.parametrize("bi", [0, 1])
@pytest.mark.parametrize("name", ["gnss", "car"])
def test_in_place_equals_out_of_place(device, name, bi):
    """The C entry point with mu_s == mu_hist and S_s == S_hist, in both history layouts."""
    inp = ur.inputs(name)
    want = device(name)
    mh, Sh = urts.history(name)
    B, T, n = mh.shape
    m = inp["U"].shape[2]
    mu_io = torch.as_tensor(np.array(np.moveaxis(mh, 0, -1) if bi else mh, order="C"), device=DEV)
    S_io = torch.as_tensor(np.array(np.moveaxis(Sh, 0, -1) if bi else Sh, order="C"), device=DEV)
    U, Q, mu0, S0 = (torch.as_tensor(np.array(inp[k], order="C"), device=DEV) for k in ("U", "Q", "mu0", "S0"))
    m0s, S0s = torch.empty_like(mu0), torch.empty_like(S0)
    st = torch.full((B,), -1, dtype=torch.int32, device=DEV)
    dyn = ur.KIND[name]["dyn"]
    did, _, _ = ekf.dynamics(dyn)
    dims = _lib.MheEkfDims(n=n, m=m, dyn_model=did, dt=float(inp["dparams"]["dt"]), hist_batch_inner=bi)
    for i, v in enumerate(ekf.dyn_par(dyn, inp["dparams"])):
        dims.dyn_par[i] = float(v)
    p = lambda t: t.data_ptr()   # noqa: E731
    args = _lib.MheUkfSmoothArgs(batch=B, steps=T, mu_hist=p(mu_io), S_hist=p(S_io), U=p(U), u_bstride=T * m, Q=p(Q),
                                 mu0=p(mu0), S0=p(S0), mu_s=p(mu_io), S_s=p(S_io), mu0_s=p(m0s), S0_s=p(S0s),
                                 status=p(st), alpha=1.0, beta=0.0, kappa=0.0)
    rc = _lib.load().mhe_ukf_smooth(ctypes.byref(dims), ctypes.byref(args),
                                    ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert rc == 0
    torch.cuda.synchronize()
    assert not _np(st).any()
    np.testing.assert_array_equal(_np(mu_io.permute(2, 0, 1) if bi else mu_io), want[0])
    np.testing.assert_array_equal(_np(S_io.permute(3, 0, 1, 2) if bi else S_io), want[1])
    np.testing.assert_array_equal(_np(m0s), want[3])
    np.testing.assert_array_equal(_np(S0s), want[4])


def test_a_side_stream_gives_the_default_streams_result(device):
    mh, Sh = urts.history("corr")
    got = _smooth("corr", _hist(mh, "inner"), _hist(Sh, "inner"), stream=torch.cuda.Stream())
    for g, w in zip(got, device("corr")):
        np.testing.assert_array_equal(g, w)


@pytest.mark.parametrize("name", ["gnss", "car"])
def test_one_and_two_steps(name):
    """T = 1 returns the history, and with a prior does one step; T = 2 works.  The reference on
    the same short history gives the bound."""
    inp, kind = ur.inputs(name), ur.KIND[name]
    mh, Sh = urts.history(name)
    for T in (1, 2):
        m, S = mh[:, :T], Sh[:, :T]
        lo, hi = (urts.smooth(inp, kind, m, S, dtype=dt) for dt in (np.float64, np.longdouble))
        assert not lo["status"].any() and not hi["status"].any()
        ref, floor, bound = urts.bounds(lo, hi)
        for layout in ("inner", "outer"):
            ms, Ss, st = _smooth(name, _hist(m, layout), _hist(S, layout), prior=False)
            ms2, Ss2, st2, m0s, S0s = _smooth(name, _hist(m, layout), _hist(S, layout))
            assert ms.shape == m.shape and Ss.shape == S.shape and not st.any() and not st2.any()
            np.testing.assert_array_equal(ms, ms2)
            np.testing.assert_array_equal(Ss, Ss2)
            np.testing.assert_array_equal(ms[:, -1], m[:, -1])
            np.testing.assert_array_equal(Ss[:, -1], S[:, -1])
            for key, g in (("mu_s", ms), ("S_s", Ss), ("mu0_s", m0s), ("S0_s", S0s)):
                err = float(np.max(np.abs(g - ref[key])))
                assert err <= bound[key], (T, key, err, bound[key])
            assert np.abs(m0s - inp["mu0"]).max() > 0                     # the prior's step was taken


@pytest.mark.parametrize("params", ur.PARAMS)
@pytest.mark.parametrize("name", ["gnss", "car"])
def test_a_predict_only_history_comes_back_bitwise(name, params):
    """A device forward run with nz = 0 throughout, smoothed with that run's own U, Q, dt,
    dyn_params and (alpha, beta, kappa): the recomputed (mu-, S-) are the history's own, every
    difference is an exact zero, and the history comes back bitwise."""
    inp, k = ur.inputs(name), ur.KIND[name]
    U, Z, nz, sat = ur.er.device_args(inp)
    mh, Sh, _, _, st = ukf.run_batch(k["dyn"], k["meas"], inp["mu0"], inp["S0"], U, Z, np.zeros_like(nz), inp["Q"],
                                     inp["R"], inp["dparams"]["dt"], sat, dyn_params=inp["dparams"], alpha=params[0],
                                     beta=params[1], kappa=params[2])
    assert not _np(st).any()
    ms, Ss, st = _smooth(name, mh, Sh, params, prior=False)
    assert not st.any()
    np.testing.assert_array_equal(ms, _np(mh))
    np.testing.assert_array_equal(Ss, _np(Sh))


def test_failures_are_reported_and_isolated(device):
    """Four planted defects: status 1 exactly for those filters, NaN from the step the reference
    names down to step 0 and in the smoothed prior, the steps above and the wave neighbours in the
    same workgroups bitwise the healthy run's."""
    healthy = device("gnss")
    inp = dict(ur.inputs("gnss"))
    mh, Sh = (np.array(a) for a in urts.history("gnss"))
    T = mh.shape[1]
    inp["S0"] = inp["S0"].copy()
    Sh[5, 4, 0, 0] = -1.0
    mh[69, 7, 1] = np.nan
    mh[33, T - 1, 0] = np.inf
    inp["S0"][12, 0, 0] = -1.0
    ref = urts.smooth(inp, ur.KIND["gnss"], mh, Sh)
    failed = {5: 4, 69: 7, 33: T - 1, 12: -1}
    assert {b: int(ref["fail_step"][b]) for b in failed} == failed and ref["status"].sum() == 4
    for layout in ("inner", "outer"):
        ms, Ss, st, m0s, S0s = _smooth("gnss", _hist(mh, layout), _hist(Sh, layout), inp=inp)
        np.testing.assert_array_equal(st, ref["status"])
        assert sorted(np.flatnonzero(st).tolist()) == sorted(failed)
        for b, k in failed.items():
            assert np.isnan(ms[b, :k + 1]).all() and np.isnan(Ss[b, :k + 1]).all()
            assert np.isnan(m0s[b]).all() and np.isnan(S0s[b]).all()
            np.testing.assert_array_equal(ms[b, k + 1:], healthy[0][b, k + 1:])
            np.testing.assert_array_equal(Ss[b, k + 1:], healthy[1][b, k + 1:])
        others = ~np.isin(np.arange(ur.B), list(failed))
        assert others[[4, 6, 7, 68, 32]].all()                           # the failed filters' workgroups
        for g, w in zip((ms, Ss, m0s, S0s), (healthy[0], healthy[1], healthy[3], healthy[4])):
            np.testing.assert_array_equal(g[others], w[others])
            assert np.isfinite(g[others]).all()
