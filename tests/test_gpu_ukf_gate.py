"""Innovation gating of the batched unscented filter on the device (csrc/mhe_ukf.hip
k_ukf<.., GATE>, mhe_ukf_run_gated, utils.ukf.run_batch(gate=...) / UKF.update(gate=...)).

Reference: tests/ukf_gate_reference.py, the recursion of include/mhe.h with the screen, in NumPy,
run in float64 and in np.longdouble once per process.  The device is compared with the longdouble
run; per case, gate, parameter set and output, floor = max |float64 run - longdouble run| of the
two GATED runs and
    bound = 8 * floor + 1e-10 * (1 + max |ref|)
(tests/ukf_reference.py's form).  The rejection masks are compared exactly: the reference's
smallest |d2 / gate - 1| is asserted to be at least MARGIN = 1e-6 first, orders of magnitude above
any rounding of d2.  tests/test_ukf_gate_host.py asserts the reference's other conditions.
Inputs: tests/ukf_reference.py's four cases (B = 70, T = 12, T = 61 for the car) with a prior
consistent with its covariance (gnss cases) and +400 m on a seeded 8 % of the valid rows.
"""
import ctypes

import numpy as np
import pytest
import torch

import ukf_gate_reference as ug
import ukf_reference as ur
import urts_reference as urts
import utils.ukf as ukf
from mhe import _lib

pytestmark = pytest.mark.gpu

ALONE = (0, 5, 69)
PARITY = [(n, g, p, "batch_outer") for n in ug.CASES for g in ug.GATES for p in ug.PARAMS] + \
         [("gnss", g, ug.PARAMS[1], "batch_inner") for g in ug.GATES]
BATCHED = ("mu0", "S0", "U", "Z", "nz", "sat")
E_DIMS, E_NULL = -1, -5


def _np(t):
    return None if t is None else t.cpu().numpy()


def _run(name, inp=None, params=ug.PARAMS[0], inputs="batch_outer", **kw):
    """run_batch on a case's gated-test inputs (or `inp`); NumPy copies of what it returns."""
    inp = ug.inputs(name) if inp is None else inp
    U, Z, nz, sat = ur.er.device_args(inp, inputs)
    k = ug.KIND[name]
    out = ukf.run_batch(k["dyn"], k["meas"], inp["mu0"], inp["S0"], U, Z, nz, inp["Q"], inp["R"],
                        inp["dparams"]["dt"], sat, inputs=inputs, dyn_params=inp["dparams"], alpha=params[0],
                        beta=params[1], kappa=params[2], **kw)
    return [_np(t) for t in out]


def _sub(inp, idx):
    """The instances idx of an input set, as a batch of their own."""
    out = dict(inp)
    for key in BATCHED:
        out[key] = np.ascontiguousarray(inp[key][idx])
    if inp["R"].ndim == 4:
        out["R"] = np.ascontiguousarray(inp["R"][idx])
    return out


def _copy(inp):
    return {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in inp.items()}


def _equal(got, want, rows=slice(None)):
    for g, w in zip(got, want):
        np.testing.assert_array_equal(g[rows], w[rows])


@pytest.fixture(scope="module")
def device():
    """The full gated call (histories, statistics, masks), per (case, gate, parameters, layout)."""
    cache = {}

    def get(name, gate=ug.GATES[0], params=ug.PARAMS[0], inputs="batch_outer"):
        key = (name, gate, params, inputs)
        if key not in cache:
            cache[key] = _run(name, params=params, inputs=inputs, gate=gate, innovations=True)
        return cache[key]
    return get


# ---------------------------------------------------------------- 1. parity

@pytest.mark.parametrize("name,gate,params,inputs", PARITY)
def test_parity(device, name, gate, params, inputs):
    ref = ug.reference(name, gate, params)
    mh, Sh, mu, S, st, nis, ll, rej = device(name, gate, params, inputs)
    got = {"mu": mh, "S": Sh, "nis": nis, "loglik": ll}
    errs = {k: float(np.max(np.abs(got[k] - ref[k]))) for k in ug.OUTPUTS}
    errs["mu_final"] = float(np.max(np.abs(mu - ref["mu"][:, -1])))
    errs["S_final"] = float(np.max(np.abs(S - ref["S"][:, -1])))
    print(f"{name} gate {gate} {params} {inputs}: gate margin {ref['gate_margin']:.2e}, " + ", ".join(
        f"{k} err {errs[k]:.2e} floor {ref['floor'][k]:.2e} bound {ref['bound'][k]:.2e}" for k in ug.OUTPUTS))
    np.testing.assert_array_equal(st, ref["status"])
    assert ref["gate_margin"] >= ug.MARGIN
    assert rej.dtype == np.int32
    np.testing.assert_array_equal(rej, ref["rej"])
    for k in ug.OUTPUTS:
        assert np.isfinite(got[k]).all()
        assert errs[k] <= ref["bound"][k], (k, errs[k], ref["bound"][k])
    assert errs["mu_final"] <= ref["bound"]["mu"] and errs["S_final"] <= ref["bound"]["S"]
    np.testing.assert_array_equal(Sh, np.swapaxes(Sh, -1, -2))
    np.testing.assert_array_equal(S, np.swapaxes(S, -1, -2))
    none, nz = ref["nkept"] == 0, ug.inputs(name)["nz"]
    assert none.any() and (nis[none] == 0.0).all() and (ll[none] == 0.0).all() and (nis[~none] > 0.0).all()
    assert (nz == 0).any() and (rej[nz == 0] == 0).all()
    np.testing.assert_array_equal(mu, mh[:, -1])
    np.testing.assert_array_equal(S, Sh[:, -1])


# ---------------------------------------------------------------- 2. kept rows only

@pytest.mark.parametrize("gate", ug.GATES)
@pytest.mark.parametrize("name", ["gnss", "car"])
def test_a_gated_step_is_the_ungated_one_fed_the_kept_rows(device, name, gate):
    """Both runs through the gated instance: the gated run, and a gate = inf run on inputs from
    which the host removed the rows the device screened out.  The histories are bitwise equal
    (every entry of e, Pzz and Pxz is a sum over the sigma points of that row's own values, and
    the sweep and the closing sums run over the same rows in the same order); nis and loglik are
    reduced over the lanes in another order and are held to the bound."""
    ref = ug.reference(name, gate)
    full = device(name, gate)
    small = ug.compact(ug.inputs(name), full[7])
    kept = _run(name, small, gate=np.inf, innovations=True)
    np.testing.assert_array_equal(kept[4], full[4])
    assert not kept[7].any()
    for i in range(4):
        np.testing.assert_array_equal(kept[i], full[i])
    for i, key in ((5, "nis"), (6, "loglik")):
        err = float(np.max(np.abs(kept[i] - full[i])))
        print(f"{name} gate {gate} {key}: gated against compacted {err:.2e} (bound {ref['bound'][key]:.2e})")
        assert err <= ref["bound"][key]


# ---------------------------------------------------------------- 3. off means off

@pytest.mark.parametrize("name", ug.CASES)
def test_a_gate_that_screens_nothing_is_the_plain_call(name):
    """gate = inf with statistics and gate = 1e300 (the gated instance) against the call without
    a gate (mhe_ukf_run, the plain instance), on the clean inputs of tests/ukf_reference.py.
    On the MI355X no entry of any case differed bitwise, so equality is asserted."""
    inp = ur.inputs(name)
    plain = _run(name, inp, innovations=True)
    assert len(plain) == 7
    inf = _run(name, inp, innovations=True, gate=np.inf)
    big = _run(name, inp, gate=1e300)
    assert len(inf) == 8 and len(big) == 5
    assert not inf[7].any()
    differ = sum(int((g != p).sum()) for got in (inf, big) for g, p in zip(got, plain))
    print(f"{name}: entries of the gated instance's results that differ bitwise from the plain call's: {differ}")
    for got in (inf, big):
        for g, p in zip(got, plain):
            np.testing.assert_array_equal(g, p)


# ---------------------------------------------------------------- 4. independence and isolation

@pytest.mark.parametrize("name", ["gnss", "car"])
def test_a_filter_alone_is_bitwise_its_result_in_the_batch(device, name):
    full = device(name)
    inp = ug.inputs(name)
    assert any(full[7][b].any() for b in ALONE)
    for b in ALONE:
        alone = _run(name, _sub(inp, [b]), gate=ug.GATES[0], innovations=True)
        for a, f in zip(alone, full):
            np.testing.assert_array_equal(a[0], f[b])
    some = _run(name, _sub(inp, list(ALONE)), gate=ug.GATES[0], innovations=True)
    for a, f in zip(some, full):                                     # and in another batch, at another place
        np.testing.assert_array_equal(a, f[list(ALONE)])


def test_a_step_with_more_rows_than_capacity_is_predict_only(device):
    """Status 2: one planted nz = pmax + 1; that step is predict-only with an empty mask, the
    filter goes on, and every other instance is bitwise unchanged."""
    gate = ug.GATES[0]
    full = device("gnss")
    inp = _copy(ug.inputs("gnss"))
    b = 6
    k = int(np.flatnonzero(inp["nz"][b, 2:-2] > 0)[0]) + 2
    inp["nz"][b, k] = inp["Z"].shape[2] + 1
    ref = ug.run(inp, ug.KIND["gnss"], gate)
    assert ref["status"][b] == 2 and ref["status"].sum() == 2 and ref["gate_margin"] >= ug.MARGIN
    got = _run("gnss", inp, gate=gate, innovations=True)
    np.testing.assert_array_equal(got[4], ref["status"])
    np.testing.assert_array_equal(got[7], ref["rej"])
    assert got[7][b, k] == 0 and got[5][b, k] == 0.0 and got[6][b, k] == 0.0
    bound = ug.reference("gnss", gate)["bound"]
    for i, key in enumerate(("mu", "S")):
        assert np.isfinite(got[i][b]).all()
        assert np.max(np.abs(got[i][b] - ref[key][b])) <= bound[key]
        np.testing.assert_array_equal(got[i][b, :k], full[i][b, :k])
    _equal(got, full, np.arange(ur.B) != b)


def test_a_row_with_a_negative_innovation_variance_is_kept_and_fails_the_filter(device):
    """Status 1: an R whose leading entry makes Pzz[0, 0] negative at a known step.  The screen
    keeps that row, its pivot fails, the filter is NaN from the step the reference names, and the
    neighbours in the workgroup are bitwise the healthy run."""
    gate = ug.GATES[0]
    full = device("gnss")
    inp = _copy(ug.inputs("gnss"))
    b, healthy = 42, ug.reference("gnss", gate)
    k = int(np.flatnonzero((inp["nz"][b, 3:] >= 2) & ((healthy["rej"][b, 3:] & 1) == 0))[0]) + 3
    inp["R"][b, k, 0, 0] = -1.0e9
    ref = ug.run(inp, ug.KIND["gnss"], gate)
    assert ref["status"][b] == 1 and ref["status"].sum() == 1 and ref["fail_step"][b] == k
    assert (ref["rej"][b, k] & 1) == 0 and ref["gate_margin"] >= ug.MARGIN
    got = _run("gnss", inp, gate=gate, innovations=True)
    np.testing.assert_array_equal(got[4], ref["status"])
    np.testing.assert_array_equal(got[7], ref["rej"])
    assert (got[7][b, k] & 1) == 0 and not got[7][b, k + 1:].any()
    for i in (0, 1, 5, 6):
        assert np.isnan(got[i][b, k:]).all()
        np.testing.assert_array_equal(got[i][b, :k], full[i][b, :k])
    assert np.isnan(got[2][b]).all() and np.isnan(got[3][b]).all()
    others = np.arange(ur.B) != b
    assert others[[40, 41, 43]].all()                                        # the failed filter's workgroup
    for g, f in zip(got, full):
        if g is not got[4]:
            np.testing.assert_array_equal(g[others], f[others])
            assert np.isfinite(g[others]).all()


# ---------------------------------------------------------------- 5. interfaces

def test_class_api_is_run_batch_step_by_step():
    """Three UKF.update(gate=...) calls, one of them without a measurement, equal run_batch over
    the same three steps bitwise, and hold that step's nis, loglik and rejected rows."""
    inp = ug.inputs("gnss")
    params, gate = ug.PARAMS[1], ug.GATES[0]
    nzs, P = (6, 0, 4), 6
    b = int(np.flatnonzero(inp["planted"][:, 0, :nzs[0]].any(axis=1) & (inp["nz"][:, 0] >= nzs[0]))[0])
    one = _sub(inp, [b])
    one["U"], one["Z"], one["sat"] = one["U"][:, :3], one["Z"][:, :3, :P].copy(), one["sat"][:, :3, :P].copy()
    one["R"] = np.ascontiguousarray(one["R"][:, :3, :P, :P])
    one["nz"] = np.array([nzs], dtype=np.int32)
    mh, Sh, mu, S, st, nis, ll, rej = _run("gnss", one, params=params, gate=gate, innovations=True)
    assert st[0] == 0 and rej[0, 0] != 0 and rej[0, 1] == 0
    f = ukf.UKF("gnss_pos_and_bias", "multi_pseudorange", one["mu0"][0], one["S0"][0], alpha=params[0],
                beta=params[1], kappa=params[2])
    for k, ns in enumerate(nzs):
        if ns == 0:
            f.update(one["U"][0, k], None, one["Q"], None, {"dt": 1.0}, gate=gate)
        else:
            f.update(one["U"][0, k], one["Z"][0, k, :ns], one["Q"], one["R"][0, k, :ns, :ns], {"dt": 1.0}, None,
                     {"sat_pos": one["sat"][0, k, :ns]}, gate=gate)
        np.testing.assert_array_equal(f.mu, mh[0, k])
        np.testing.assert_array_equal(f.S, Sh[0, k])
        assert f.nis == nis[0, k] and f.loglik == ll[0, k]
        assert f.rejected.dtype == bool and f.rejected.shape == (ns,)
        assert f.rejected.tolist() == [bool((int(rej[0, k]) >> i) & 1) for i in range(ns)]
    g = ukf.UKF("gnss_pos_and_bias", "multi_pseudorange", one["mu0"][0], one["S0"][0])
    g.update(one["U"][0, 0], one["Z"][0, 0, :4], one["Q"], one["R"][0, 0, :4, :4], {"dt": 1.0}, None,
             {"sat_pos": one["sat"][0, 0, :4]})
    assert not hasattr(g, "rejected") and not hasattr(g, "nis")              # without a gate nothing changes


def test_a_side_stream_gives_the_default_streams_result(device):
    full = device("corr")
    side = torch.cuda.Stream()
    inp = ug.inputs("corr")
    U, Z, nz, sat = ur.er.device_args(inp)
    k = ug.KIND["corr"]
    out = ukf.run_batch(k["dyn"], k["meas"], inp["mu0"], inp["S0"], U, Z, nz, inp["Q"], inp["R"], 1.0, sat,
                        stream=side, innovations=True, gate=ug.GATES[0])
    side.synchronize()
    for g, f in zip(out, full):
        np.testing.assert_array_equal(_np(g), f)


@pytest.mark.parametrize("name", ["gnss", "car"])
def test_the_smoother_takes_a_gated_history(name):
    """utils.ukf.smooth_batch over the history of a gated run (its batch-innermost views), against
    tests/urts_reference.py's smoother on that same history, in that file's form of bound."""
    inp, k, gate = ug.inputs(name), ug.KIND[name], ug.GATES[0]
    U, Z, nz, sat = ur.er.device_args(inp)
    mh, Sh, _, _, st = ukf.run_batch(k["dyn"], k["meas"], inp["mu0"], inp["S0"], U, Z, nz, inp["Q"], inp["R"],
                                     inp["dparams"]["dt"], sat, dyn_params=inp["dparams"], gate=gate)
    assert not _np(st).any()
    out = ukf.smooth_batch(k["dyn"], mh, Sh, U, inp["Q"], inp["dparams"]["dt"], mu0=inp["mu0"], S0=inp["S0"],
                           dyn_params=inp["dparams"])
    got = dict(zip(("mu_s", "S_s", "status", "mu0_s", "S0_s"), [_np(t) for t in out]))
    lo = urts.smooth(inp, k, _np(mh), _np(Sh), dtype=np.float64)
    hi = urts.smooth(inp, k, _np(mh), _np(Sh), dtype=np.longdouble)
    ref, floor, bound = urts.bounds(lo, hi)
    assert not got["status"].any() and not hi["status"].any() and not lo["status"].any()
    for key in urts.OUTPUTS:
        err = float(np.max(np.abs(got[key] - ref[key])))
        print(f"smoother on a gated history, {name} {key}: observed {err:.2e} floor {floor[key]:.2e} "
              f"bound {bound[key]:.2e}")
        assert err <= bound[key], (key, err, bound[key])


def test_the_c_entry_refuses_as_mhe_ukf_run_and_runs_it_when_nothing_is_asked():
    """mhe_ukf_run_gated: a NULL struct, a wrong struct_size and a NaN or negative gate are
    refused with mhe_ukf_run's codes; with gate = 0 and rej = NULL it matches mhe_ukf_run bitwise."""
    lib = _lib.load()
    inp = ug.inputs("gnss")
    B, T = inp["nz"].shape
    P, n, m = inp["Z"].shape[2], 5, 3
    dev = torch.device("cuda", 0)
    t = {k: torch.as_tensor(np.ascontiguousarray(inp[k]), device=dev) for k in ("U", "Z", "sat", "Q", "R")}
    t["nz"] = torch.as_tensor(inp["nz"], dtype=torch.int32, device=dev)
    dims = _lib.MheEkfDims(n=n, m=m, pmax=P, q=3, dyn_model=1, meas_model=1, dt=1.0)

    def call(fn, cls, **extra):
        o = {"mu": torch.as_tensor(inp["mu0"], device=dev).clone(), "S": torch.as_tensor(inp["S0"], device=dev).clone(),
             "mu_hist": torch.full((B, T, n), -7.0, dtype=torch.float64, device=dev),
             "S_hist": torch.full((B, T, n, n), -7.0, dtype=torch.float64, device=dev),
             "status": torch.full((B,), -7, dtype=torch.int32, device=dev),
             "nis": torch.full((B, T), -7.0, dtype=torch.float64, device=dev),
             "loglik": torch.full((B, T), -7.0, dtype=torch.float64, device=dev)}
        a = cls(batch=B, steps=T, U=t["U"].data_ptr(), u_bstride=T * m, Z=t["Z"].data_ptr(), z_bstride=T * P,
                nz=t["nz"].data_ptr(), nz_bstride=T, PAR=t["sat"].data_ptr(), par_bstride=T * P * 3,
                Q=t["Q"].data_ptr(), R=t["R"].data_ptr(), r_bstride=T * P * P, r_sstride=P * P, alpha=1.0, beta=0.0,
                kappa=0.0, **{k: v.data_ptr() for k, v in o.items()})
        for k, v in extra.items():
            setattr(a, k, v)
        rc = fn(ctypes.byref(dims), ctypes.byref(a), ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
        torch.cuda.synchronize()
        return rc, {k: _np(v) for k, v in o.items()}

    gated, G = lib.mhe_ukf_run_gated, _lib.MheUkfGateArgs
    assert gated(ctypes.byref(dims), None, None) == E_NULL
    for extra in (dict(struct_size=ctypes.sizeof(_lib.MheUkfArgs)), dict(struct_size=0), dict(gate=float("nan")),
                  dict(gate=-1.0)):
        rc, out = call(gated, G, **extra)
        assert rc == E_DIMS, extra
        assert all((v == -7).all() for k, v in out.items() if k not in ("mu", "S"))      # nothing ran
    rc0, want = call(lib.mhe_ukf_run, _lib.MheUkfArgs)
    rc1, got = call(gated, G, gate=0.0, rej=None)
    assert rc0 == 0 and rc1 == 0
    for key in want:
        np.testing.assert_array_equal(got[key], want[key])
    # and a mask alone (gate 0) is the gated instance screening nothing
    rej = torch.full((B, T), -7, dtype=torch.int32, device=dev)
    rc2, got = call(gated, G, gate=0.0, rej=rej.data_ptr())
    assert rc2 == 0 and not _np(rej).any()
    np.testing.assert_array_equal(got["status"], want["status"])
