"""Iterated EKF on the device (csrc/mhe_iekf.hip k_iekf, mhe_iekf_run,
utils.ekf.run_batch(iterations=, iter_tol=) / EKF.update(iterations=)).

Reference: tests/iekf_reference.py, the recursion of include/mhe.h in NumPy, run in float64 and in
np.longdouble once per process.  The device is compared with the longdouble run; per case and
output, floor = max |float64 run - longdouble run| and
    bound = 8 * floor + 1e-10 * (1 + max |ref|)
(tests/ukf_reference.py's form).  The pass counts and the rejection masks are compared exactly: the
reference asserts first that every pass of every step has |step / tol - 1| >= 1e-3 and every row
|d2 / gate - 1| >= 1e-6, orders of magnitude above any rounding of either, and that the counts and
masks of its two precisions agree.  tests/test_iekf_host.py asserts the reference's other conditions.
Inputs: tests/ekf_ragged.py's builders at B = 70 (17 workgroups and a partial one) with a cold prior
(1e5 m off in position; the car 2000 m); the gated cases use tests/ukf_gate_reference.py's sets.
"""
import numpy as np
import pytest

import ekf_ragged as er
import iekf_reference as ir
import utils.ekf as ekf

pytestmark = pytest.mark.gpu

ALONE = (0, 5, 69)
PARITY = [(n, "batch_outer") for n in ir.CASES] + [("gnss", "batch_inner")]
BATCHED = ("mu0", "S0", "U", "Z", "nz", "sat")


def _np(t):
    return None if t is None else t.cpu().numpy()


def _run(name, inp=None, inputs="batch_outer", **kw):
    """run_batch on a case's cold-prior inputs (or `inp`); NumPy copies of what it returns."""
    inp = ir.inputs(name) if inp is None else inp
    U, Z, nz, sat = er.device_args(inp, inputs)
    k = ir.KIND[name]
    out = ekf.run_batch(k["dyn"], k["meas"], inp["mu0"], inp["S0"], U, Z, nz, inp["Q"], inp["R"],
                        inp["dparams"]["dt"], sat, inputs=inputs, dyn_params=inp["dparams"], **kw)
    return [_np(t) for t in out]


def _iter(name, **kw):
    return dict(dict(iterations=ir.CAP[name], iter_tol=ir.TOL[name]), **kw)


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


def _check(tag, got, ref, stats=True):
    """Histories, final state and statistics within bound; status and n_iter exact; S bitwise
    symmetric; the final state is the last history entry."""
    mh, Sh, mu, S, st = got[:5]
    n_iter = got[-1]
    vals = {"mu": mh, "S": Sh}
    if stats:
        vals.update(nis=got[5], loglik=got[6])
    errs = {k: float(np.max(np.abs(v - ref[k]))) for k, v in vals.items()}
    print(f"{tag}: passes {np.bincount(ref['n_iter'].ravel()).tolist()}, step margin {ref['step_margin']:.2e}, " +
          ", ".join(f"{k} err {errs[k]:.2e} floor {ref['floor'][k]:.2e} bound {ref['bound'][k]:.2e}" for k in vals))
    np.testing.assert_array_equal(st, ref["status"])
    assert n_iter.dtype == np.int32 and n_iter.shape == ref["n_iter"].shape
    np.testing.assert_array_equal(n_iter, ref["n_iter"])
    for k, v in vals.items():
        assert np.isfinite(v).all()
        assert errs[k] <= ref["bound"][k], (k, errs[k], ref["bound"][k])
    np.testing.assert_array_equal(Sh, np.swapaxes(Sh, -1, -2))
    np.testing.assert_array_equal(S, np.swapaxes(S, -1, -2))
    np.testing.assert_array_equal(mu, mh[:, -1])
    np.testing.assert_array_equal(S, Sh[:, -1])


@pytest.fixture(scope="module")
def device():
    """The full iterated call (histories, statistics, counts) on the cold-prior inputs, per case."""
    cache = {}

    def get(name, inputs="batch_outer"):
        if (name, inputs) not in cache:
            cache[name, inputs] = _run(name, inputs=inputs, innovations=True, **_iter(name))
        return cache[name, inputs]
    return get


@pytest.fixture(scope="module")
def gated():
    """The gated iterated call on tests/ukf_gate_reference.py's inputs, per (case, gate)."""
    cache = {}

    def get(name, gate):
        if (name, gate) not in cache:
            cache[name, gate] = _run(name, ir.gated_inputs(name), gate=gate, innovations=True, **_iter(name))
        return cache[name, gate]
    return get


# ---------------------------------------------------------------- 1. parity

@pytest.mark.parametrize("name,inputs", PARITY)
def test_parity(device, name, inputs):
    ref = ir.reference(name)
    got = device(name, inputs)
    assert len(got) == 9 and not got[7].any()
    _check(f"{name} {inputs}", got, ref)
    assert (got[-1] > 2).any() and (got[-1] == 0).any()


# ---------------------------------------------------------------- 2. a fixed number of passes

@pytest.mark.parametrize("name", ir.CASES)
def test_zero_tolerance_makes_every_pass(name):
    ref = ir.reference(name, 3, 0.0)
    got = _run(name, innovations=True, iterations=3, iter_tol=0.0)
    nz, P = ir.inputs(name)["nz"], ir.inputs(name)["Z"].shape[2]
    np.testing.assert_array_equal(got[-1], np.where((nz > 0) & (nz <= P), 3, 0))
    _check(f"{name} 3 passes", got, ref)


# ---------------------------------------------------------------- 3. one pass is the EKF

@pytest.mark.parametrize("name", ir.CASES)
def test_one_pass_is_the_wave_ekf(name):
    """iterations = 1 against run_batch(method="wave") without the keyword (k_ekf), within the bound
    of the one-pass reference on the same inputs."""
    ref = ir.reference(name, 1, 0.0)
    one = _run(name, iterations=1)
    ekf_ = _run(name, method="wave")
    assert len(one) == 6 and len(ekf_) == 5
    np.testing.assert_array_equal(one[4], ekf_[4])
    nz = ir.inputs(name)["nz"]
    np.testing.assert_array_equal(one[5], (nz > 0).astype(np.int32))
    differ = sum(int((a != b).sum()) for a, b in zip(one[:4], ekf_[:4]))
    print(f"{name}: entries of the one-pass result that differ bitwise from k_ekf's: {differ}"
          f" ({'bitwise equal' if differ == 0 else 'not bitwise'})")
    for i, key in ((0, "mu"), (1, "S"), (2, "mu"), (3, "S")):
        err = float(np.max(np.abs(one[i] - ekf_[i])))
        print(f"{name} {key}: one pass against k_ekf {err:.2e} (bound {ref['bound'][key]:.2e})")
        assert err <= ref["bound"][key]
    _check(f"{name} one pass", one, ref, stats=False)


# ---------------------------------------------------------------- 4. the gate

@pytest.mark.parametrize("gate", ir.GATES)
@pytest.mark.parametrize("name", ir.GATED)
def test_gated_parity(gated, name, gate):
    ref = ir.reference(name, ir.CAP[name], ir.TOL[name], gate)
    got = gated(name, gate)
    print(f"{name} gate {gate}: gate margin {ref['gate_margin']:.2e}")
    assert got[7].dtype == np.int32
    np.testing.assert_array_equal(got[7], ref["rej"])                        # the masks, exactly
    _check(f"{name} gate {gate}", got, ref)
    none = ref["nkept"] == 0
    assert none.any() and (got[5][none] == 0.0).all() and (got[6][none] == 0.0).all() and (got[5][~none] > 0.0).all()
    assert (got[-1][none] == 0).all() and (got[-1][~none] >= 1).all()


@pytest.mark.parametrize("gate", ir.GATES)
@pytest.mark.parametrize("name", ir.GATED)
def test_a_gated_run_is_the_ungated_one_fed_the_kept_rows(gated, name, gate):
    ref = ir.reference(name, ir.CAP[name], ir.TOL[name], gate)
    full = gated(name, gate)
    small = ir.ug.compact(ir.gated_inputs(name), full[7])
    kept = _run(name, small, innovations=True, **_iter(name))
    np.testing.assert_array_equal(kept[4], full[4])
    np.testing.assert_array_equal(kept[-1], full[-1])
    assert not kept[7].any()
    for i, key in ((0, "mu"), (1, "S"), (2, "mu"), (3, "S"), (5, "nis"), (6, "loglik")):
        err = float(np.max(np.abs(kept[i] - full[i])))
        print(f"{name} gate {gate} {key}: gated against compacted {err:.2e} (bound {ref['bound'][key]:.2e})")
        assert err <= ref["bound"][key]


@pytest.mark.parametrize("name", ir.GATED)
def test_a_gate_that_screens_nothing_is_the_call_without_one(name):
    plain = _run(name, **_iter(name))
    inf = _run(name, gate=np.inf, innovations=True, **_iter(name))
    assert len(plain) == 6 and len(inf) == 9 and not inf[7].any()
    for i in (0, 1, 2, 3, 4, -1):                                            # mu, S (histories and final), n_iter
        np.testing.assert_array_equal(inf[i], plain[i])


# ---------------------------------------------------------------- 5. independence

@pytest.mark.parametrize("name", ["gnss", "car"])
def test_a_filter_alone_is_bitwise_its_result_in_the_batch(device, name):
    """Neighbours in the workgroup make other numbers of passes; nothing of them leaks."""
    full = device(name)
    inp = ir.inputs(name)
    counts = [full[-1][b0:b0 + 4].max(axis=0) != full[-1][b0:b0 + 4].min(axis=0) for b0 in (0, 4)]
    assert all(c.any() for c in counts)                # the pass counts differ within the workgroups of 0 and of 5
    for b in ALONE:
        alone = _run(name, _sub(inp, [b]), innovations=True, **_iter(name))
        for a, f in zip(alone, full):
            np.testing.assert_array_equal(a[0], f[b])
    some = _run(name, _sub(inp, list(ALONE)), innovations=True, **_iter(name))
    for a, f in zip(some, full):                                             # and in another batch, at another place
        np.testing.assert_array_equal(a, f[list(ALONE)])


# ---------------------------------------------------------------- 6. status

def test_an_indefinite_innovation_covariance_is_status_1_and_stays_with_its_filter(device):
    full = device("gnss")
    inp = _copy(ir.inputs("gnss"))
    b = 42
    k = int(np.flatnonzero(inp["nz"][b, 3:] >= 2)[0]) + 3
    inp["R"][b, k, 0, 0] = -1.0e9                                            # P[0, 0] < 0 once S has contracted
    ref = ir.run(inp, ir.KIND["gnss"], ir.CAP["gnss"], ir.TOL["gnss"])
    assert ref["status"][b] == 1 and ref["status"].sum() == 1
    got = _run("gnss", inp, innovations=True, **_iter("gnss"))
    np.testing.assert_array_equal(got[4], ref["status"])
    others = np.arange(ir.B) != b
    assert others[[40, 41, 43]].all()                                        # the failed filter's workgroup
    for g, f in zip(got, full):
        np.testing.assert_array_equal(g[others], f[others])
    for i in (0, 1, 5, 6, 8):
        np.testing.assert_array_equal(got[i][b, :k], full[i][b, :k])


def test_a_step_with_more_rows_than_capacity_is_predict_only(device):
    full = device("gnss")
    inp = _copy(ir.inputs("gnss"))
    b = 6
    k = int(np.flatnonzero(inp["nz"][b, 2:-2] > 0)[0]) + 2
    inp["nz"][b, k] = inp["Z"].shape[2] + 1
    ref = ir.run(inp, ir.KIND["gnss"], ir.CAP["gnss"], ir.TOL["gnss"], dtype=np.longdouble)
    assert ref["status"][b] == 2 and ref["status"].sum() == 2 and ref["n_iter"][b, k] == 0
    got = _run("gnss", inp, innovations=True, **_iter("gnss"))
    np.testing.assert_array_equal(got[4], ref["status"])
    assert got[-1][b, k] == 0 and got[7][b, k] == 0 and got[5][b, k] == 0.0 and got[6][b, k] == 0.0
    bound = ir.reference("gnss")["bound"]
    # the predicted state: mu-, S- of that step
    assert np.max(np.abs(got[0][b, k] - ref["mp"][b, k].astype(np.float64))) <= bound["mu"]
    assert np.max(np.abs(got[1][b, k] - ref["SP"][b, k].astype(np.float64))) <= bound["S"]
    for i in (0, 1, 5, 6, 7, 8):
        np.testing.assert_array_equal(got[i][b, :k], full[i][b, :k])
    others = np.arange(ir.B) != b
    for g, f in zip(got, full):
        np.testing.assert_array_equal(g[others], f[others])


# ---------------------------------------------------------------- 7. the class

def test_class_api_is_a_batch_of_one():
    """EKF.update(iterations=...) step by step, one step without a measurement, equals run_batch
    over the same steps bitwise and holds that step's n_iter."""
    inp = ir.inputs("gnss")
    nzs, P, b = (6, 0, 4), 6, 3
    one = _sub(inp, [b])
    one["U"], one["Z"], one["sat"] = one["U"][:, :3], one["Z"][:, :3, :P].copy(), one["sat"][:, :3, :P].copy()
    one["R"] = np.ascontiguousarray(one["R"][:, :3, :P, :P])
    one["nz"] = np.array([nzs], dtype=np.int32)
    kw = _iter("gnss")
    mh, Sh, mu, S, st, n_iter = _run("gnss", one, **kw)
    assert st[0] == 0 and n_iter[0, 0] >= 2 and n_iter[0, 1] == 0
    f = ekf.EKF("gnss_pos_and_bias", "multi_pseudorange", one["mu0"][0], one["S0"][0])
    for k, ns in enumerate(nzs):
        if ns == 0:
            f.update(one["U"][0, k], None, one["Q"], None, {"dt": 1.0}, **kw)
        else:
            f.update(one["U"][0, k], one["Z"][0, k, :ns], one["Q"], one["R"][0, k, :ns, :ns], {"dt": 1.0}, None,
                     {"sat_pos": one["sat"][0, k, :ns]}, **kw)
        np.testing.assert_array_equal(f.mu, mh[0, k])
        np.testing.assert_array_equal(f.S, Sh[0, k])
        assert isinstance(f.n_iter, int) and f.n_iter == n_iter[0, k]
    g = ekf.EKF("gnss_pos_and_bias", "multi_pseudorange", one["mu0"][0], one["S0"][0])
    g.update(one["U"][0, 0], one["Z"][0, 0, :4], one["Q"], one["R"][0, 0, :4, :4], {"dt": 1.0}, None,
             {"sat_pos": one["sat"][0, 0, :4]})
    assert not hasattr(g, "n_iter")                                          # without the keyword nothing changes
