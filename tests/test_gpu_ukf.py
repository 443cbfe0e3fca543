"""Batched unscented Kalman filter on the device (csrc/mhe_ukf.hip k_ukf, mhe_ukf_run,
utils.ukf.run_batch / UKF).

Reference: tests/ukf_reference.py, the recursion of include/mhe.h in NumPy, run in float64 and
in np.longdouble once per process.  The device is compared with the longdouble run; per case
and output, floor = max |float64 run - longdouble run| and
    bound = 8 * floor + 1e-10 * (1 + max |ref|)
(the 8 covers the device's different but fixed summation order and FMA contraction).
tests/test_ukf_host.py asserts that every reference run ends with status 0 and that no Cholesky
pivot is near zero, so the device cannot disagree about status.
Inputs: tests/ekf_ragged.py's builders, B = 70 (17 full workgroups and one of two waves), T = 12
(T = 61 for the car), row counts 0, 1, 7, 8, 9, ..., 31, 32 planted in every group.
"""
import numpy as np
import pytest
import torch

import ukf_reference as ur
import utils.ukf as ukf

pytestmark = pytest.mark.gpu

ALONE = (0, 5, 69)
PARITY = [(n, p, "batch_outer") for n in ur.CASES for p in ur.PARAMS] + [("gnss", p, "batch_inner") for p in ur.PARAMS]
BATCHED = ("mu0", "S0", "U", "Z", "nz", "sat")


def _np(t):
    return None if t is None else t.cpu().numpy()


def _run(name, inp=None, params=ur.PARAMS[0], inputs="batch_outer", **kw):
    """run_batch on a case's inputs (or `inp`); NumPy copies of what it returns."""
    inp = ur.inputs(name) if inp is None else inp
    U, Z, nz, sat = ur.er.device_args(inp, inputs)
    k = ur.KIND[name]
    out = ukf.run_batch(k["dyn"], k["meas"], inp["mu0"], inp["S0"], U, Z, nz, inp["Q"], inp["R"],
                        inp["dparams"]["dt"], sat, inputs=inputs, dyn_params=inp["dparams"], alpha=params[0],
                        beta=params[1], kappa=params[2], **kw)
    return [_np(t) for t in out]


def _sub(inp, idx):
    """The instances idx of a builder's inputs, as a batch of their own."""
    out = dict(inp)
    for key in BATCHED:
        out[key] = np.ascontiguousarray(inp[key][idx])
    if inp["R"].ndim == 4:
        out["R"] = np.ascontiguousarray(inp["R"][idx])
    return out


def _copy(inp):
    return {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in inp.items()}


@pytest.fixture(scope="module")
def device():
    """The full call (histories and statistics), per (case, parameters, layout)."""
    cache = {}

    def get(name, params=ur.PARAMS[0], inputs="batch_outer"):
        key = (name, params, inputs)
        if key not in cache:
            cache[key] = _run(name, params=params, inputs=inputs, innovations=True)
        return cache[key]
    return get


@pytest.mark.parametrize("name,params,inputs", PARITY)
def test_parity(device, name, params, inputs):
    ref = ur.reference(name, params)
    mh, Sh, mu, S, st, nis, ll = device(name, params, inputs)
    got = {"mu": mh, "S": Sh, "nis": nis, "loglik": ll}
    errs = {k: float(np.max(np.abs(got[k] - ref[k]))) for k in ur.OUTPUTS}
    errs["mu_final"] = float(np.max(np.abs(mu - ref["mu"][:, -1])))
    errs["S_final"] = float(np.max(np.abs(S - ref["S"][:, -1])))
    print(f"{name} {params} {inputs}: " + ", ".join(
        f"{k} err {errs[k]:.2e} floor {ref['floor'][k]:.2e} bound {ref['bound'][k]:.2e}" for k in ur.OUTPUTS))
    np.testing.assert_array_equal(st, ref["status"])
    for k in ur.OUTPUTS:
        assert np.isfinite(got[k]).all()
        assert errs[k] <= ref["bound"][k], (k, errs[k], ref["bound"][k])
    assert errs["mu_final"] <= ref["bound"]["mu"] and errs["S_final"] <= ref["bound"]["S"]
    np.testing.assert_array_equal(mu, mh[:, -1])
    np.testing.assert_array_equal(S, Sh[:, -1])


@pytest.mark.parametrize("name", ur.CASES)
def test_covariance_is_bitwise_symmetric_and_statistics_vanish_without_a_correction(device, name):
    for params in ur.PARAMS:
        _, Sh, _, S, _, nis, ll = device(name, params)
        np.testing.assert_array_equal(Sh, np.swapaxes(Sh, -1, -2))
        np.testing.assert_array_equal(S, np.swapaxes(S, -1, -2))
        none = ur.inputs(name)["nz"] == 0
        assert none.any() and (nis[none] == 0.0).all() and (ll[none] == 0.0).all()
        assert (nis[~none] > 0.0).all()


@pytest.mark.parametrize("name", ["gnss", "car"])
def test_a_filter_alone_is_bitwise_its_result_in_the_batch(device, name):
    full = device(name)
    inp = ur.inputs(name)
    for b in ALONE:
        alone = _run(name, _sub(inp, [b]), innovations=True)
        for a, f in zip(alone, full):
            np.testing.assert_array_equal(a[0], f[b])
    some = _run(name, _sub(inp, list(ALONE)), innovations=True)      # and in another batch, at another place
    for a, f in zip(some, full):
        np.testing.assert_array_equal(a, f[list(ALONE)])


@pytest.mark.parametrize("name", ["corr", "car"])
def test_optional_outputs_do_not_change_the_result(device, name):
    full = device(name)
    out = _run(name, keep_history=False, innovations=False)
    assert len(out) == 5 and out[0] is None and out[1] is None
    for i in (2, 3, 4):
        np.testing.assert_array_equal(out[i], full[i])
    out = _run(name, keep_history=True, innovations=False)
    assert len(out) == 5
    for i in range(5):
        np.testing.assert_array_equal(out[i], full[i])


def test_a_step_with_more_rows_than_capacity_is_predict_only(device):
    """Status 2: one planted nz = pmax + 1; that step is predict-only, the filter goes on, and
    every other instance is bitwise unchanged."""
    full = device("gnss")
    inp = _copy(ur.inputs("gnss"))
    b = 6
    k = int(np.flatnonzero(inp["nz"][b, 2:-2] > 0)[0]) + 2
    inp["nz"][b, k] = inp["Z"].shape[2] + 1
    ref = ur.run(inp, ur.KIND["gnss"])
    assert ref["status"][b] == 2 and ref["status"].sum() == 2
    got = _run("gnss", inp, innovations=True)
    np.testing.assert_array_equal(got[4], ref["status"])
    bound = ur.reference("gnss")["bound"]
    for i, key in enumerate(("mu", "S")):
        assert np.isfinite(got[i][b]).all()
        assert np.max(np.abs(got[i][b] - ref[key][b])) <= bound[key]
        np.testing.assert_array_equal(got[i][b, :k], full[i][b, :k])
        assert np.max(np.abs(got[i][b, k:] - full[i][b, k:])) > 100 * bound[key]     # the step was skipped
    assert got[5][b, k] == 0.0 and got[6][b, k] == 0.0
    others = np.arange(ur.B) != b
    for g, f in zip(got, full):
        np.testing.assert_array_equal(g[others], f[others])


def test_a_failed_filter_is_nan_from_that_step_on_and_alone(device):
    """Status 1, by ordinary numerical inputs: a prior covariance with a negative diagonal
    entry (fails at step 0) and an R whose leading entry makes Pzz indefinite at a known
    step.  The reference says where; the neighbours in the workgroup are bitwise the healthy run."""
    full = device("gnss")
    inp = _copy(ur.inputs("gnss"))
    b1, b2 = 5, 42
    k2 = int(np.flatnonzero(inp["nz"][b2, 3:] >= 2)[0]) + 3
    inp["S0"][b1, 2, 2] = -inp["S0"][b1, 2, 2]
    inp["R"][b2, k2, 0, 0] = -1.0e9
    ref = ur.run(inp, ur.KIND["gnss"])
    assert ref["status"][b1] == 1 and ref["status"][b2] == 1 and ref["status"].sum() == 2
    assert ref["fail_step"][b1] == 0 and ref["fail_step"][b2] == k2
    got = _run("gnss", inp, innovations=True)
    np.testing.assert_array_equal(got[4], ref["status"])
    for b, k in ((b1, 0), (b2, k2)):
        for i in (0, 1, 5, 6):
            assert np.isnan(got[i][b, k:]).all()
            np.testing.assert_array_equal(got[i][b, :k], full[i][b, :k])
        assert np.isnan(got[2][b]).all() and np.isnan(got[3][b]).all()
    others = ~np.isin(np.arange(ur.B), (b1, b2))
    assert others[[4, 6, 7, 40, 41, 43]].all()                       # the failed filters' workgroups
    for g, f in zip(got, full):
        if g is not got[4]:
            np.testing.assert_array_equal(g[others], f[others])
            assert np.isfinite(g[others]).all()


def test_class_api_is_run_batch_step_by_step():
    """Three UKF.update calls, one of them without a measurement, equal run_batch over the same
    three steps bitwise; a failing update raises."""
    inp = ur.inputs("gnss")
    params = ur.PARAMS[1]
    b, nzs, P = 3, (4, 0, 6), 6
    one = _sub(inp, [b])
    one["U"], one["Z"], one["sat"] = one["U"][:, :3], one["Z"][:, :3, :P].copy(), one["sat"][:, :3, :P].copy()
    one["R"] = np.ascontiguousarray(one["R"][:, :3, :P, :P])
    one["nz"] = np.array([nzs], dtype=np.int32)
    mh, Sh, mu, S, st = _run("gnss", one, params=params)
    assert st[0] == 0
    f = ukf.UKF("gnss_pos_and_bias", "multi_pseudorange", one["mu0"][0], one["S0"][0], alpha=params[0],
                beta=params[1], kappa=params[2])
    for k, ns in enumerate(nzs):
        if ns == 0:
            f.update(one["U"][0, k], None, one["Q"], None, {"dt": 1.0})
        else:
            f.update(one["U"][0, k], one["Z"][0, k, :ns], one["Q"], one["R"][0, k, :ns, :ns], {"dt": 1.0}, None,
                     {"sat_pos": one["sat"][0, k, :ns]})
        np.testing.assert_array_equal(f.mu, mh[0, k])
        np.testing.assert_array_equal(f.S, Sh[0, k])
    held = f.mu.copy()
    with pytest.raises(np.linalg.LinAlgError):
        f.update(one["U"][0, 0], one["Z"][0, 0, :4], one["Q"], -1.0e9 * np.eye(4), {"dt": 1.0}, None,
                 {"sat_pos": one["sat"][0, 0, :4]})
    np.testing.assert_array_equal(f.mu, held)


def test_a_side_stream_gives_the_default_streams_result(device):
    full = device("corr")
    side = torch.cuda.Stream()
    inp = ur.inputs("corr")
    U, Z, nz, sat = ur.er.device_args(inp)
    k = ur.KIND["corr"]
    out = ukf.run_batch(k["dyn"], k["meas"], inp["mu0"], inp["S0"], U, Z, nz, inp["Q"], inp["R"], 1.0, sat,
                        stream=side, innovations=True)
    side.synchronize()
    for g, f in zip(out, full):
        np.testing.assert_array_equal(_np(g), f)
