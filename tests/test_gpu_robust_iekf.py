"""Pseudo-Huber rows for the iterated EKF on the device (csrc/mhe_iekf.hip k_iekf<.., ROBUST>,
mhe_iekf_run_robust, utils.ekf.run_batch(huber=) / EKF.update(huber=)).

Reference: tests/robust_iekf_reference.py, the recursion of include/mhe.h in NumPy, run in float64
and in np.longdouble once per process.  The device is compared with the longdouble run; per case and
output (mu, S, nis, loglik, weights), floor = max |float64 run - longdouble run| and
    bound = 8 * floor + 1e-10 * (1 + max |ref|)
(tests/ukf_reference.py's form).  The pass counts, the rejection masks and the statuses are compared
exactly: the reference asserts first that every pass of every step has |step / tol - 1| >= 1e-3 and
every row |d2 / gate - 1| >= 1e-6, and that the counts and masks of its two precisions agree.
tests/test_robust_iekf_host.py asserts the reference's other conditions.  Inputs:
tests/ukf_gate_reference.py's outlier sets at B = 70 (17 workgroups and a partial one; 8 % of the
rows shifted by +400 m), cap 64.
"""
import numpy as np
import pytest
import torch

import ekf_ragged as er
import iekf_reference as ir
import robust_iekf_reference as rr
import utils.ekf as ekf

pytestmark = pytest.mark.gpu

ALONE = (0, 5, 69)
PARITY = [c + ("batch_outer",) for c in rr.PARITY] + [rr.PARITY[0] + ("batch_inner",)]
IDS = [f"{n}-gate{g}-delta{d}-tol{t:g}-{i}" for n, g, d, t, i in PARITY]
BATCHED = ("mu0", "S0", "U", "Z", "nz", "sat")
MU, S_, MUF, SF, ST, NIS, LL, REJ, NIT, W = range(10)     # what the full call returns


def _np(t):
    return None if t is None else t.cpu().numpy()


def _layout(D, inputs):
    """A (B,T,P) array in Z's layout."""
    return D if inputs == "batch_outer" else np.ascontiguousarray(np.transpose(D, (1, 2, 0)))


def _run(name, inp, inputs="batch_outer", **kw):
    """run_batch on an input set; NumPy copies of what it returns."""
    U, Z, nz, sat = er.device_args(inp, inputs)
    k = ir.KIND[name]
    out = ekf.run_batch(k["dyn"], k["meas"], inp["mu0"], inp["S0"], U, Z, nz, inp["Q"], inp["R"],
                        inp["dparams"]["dt"], sat, inputs=inputs, dyn_params=inp["dparams"], **kw)
    return [_np(t) for t in out]


def _full(name, inp, gate, delta, tol, inputs="batch_outer", cap=rr.CAP):
    """The full robust call: histories, statistics, counts and weights (10 entries)."""
    huber = _layout(delta, inputs) if isinstance(delta, np.ndarray) else delta
    kw = {} if gate is None else {"gate": gate}
    return _run(name, inp, inputs, innovations=True, iterations=cap, iter_tol=tol, huber=huber, **kw)


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


def _applied(inp, rej):
    """(B,T,P) bool: the rows that were applied, from nz and the rejection mask."""
    P = inp["Z"].shape[2]
    nz = np.where(inp["nz"] <= P, inp["nz"], 0)
    word = rej.view(np.uint32)
    return (np.arange(P)[None, None, :] < nz[:, :, None]) & \
        ~((word[:, :, None] >> np.arange(P, dtype=np.uint32)) & 1).astype(bool)


def _check(tag, got, ref):
    """Histories, final state, statistics and weights within bound; status, n_iter and rej exact;
    S bitwise symmetric; the final state is the last history entry."""
    assert len(got) == 10
    vals = {"mu": got[MU], "S": got[S_], "nis": got[NIS], "loglik": got[LL], "weights": got[W]}
    errs = {k: float(np.max(np.abs(v - ref[k]))) for k, v in vals.items()}
    print(f"{tag}: passes {np.bincount(ref['n_iter'].ravel()).tolist()}, step margin {ref['step_margin']:.2e}, gate "
          f"margin {ref['gate_margin']:.2e}, " +
          ", ".join(f"{k} err {errs[k]:.2e} floor {ref['floor'][k]:.2e} bound {ref['bound'][k]:.2e}" for k in vals))
    np.testing.assert_array_equal(got[ST], ref["status"])
    assert got[NIT].dtype == np.int32 and got[NIT].shape == ref["n_iter"].shape
    np.testing.assert_array_equal(got[NIT], ref["n_iter"])
    assert got[REJ].dtype == np.int32
    np.testing.assert_array_equal(got[REJ], ref["rej"])
    for k, v in vals.items():
        assert v.shape == ref[k].shape and np.isfinite(v).all()
        assert errs[k] <= ref["bound"][k], (k, errs[k], ref["bound"][k])
    np.testing.assert_array_equal(got[S_], np.swapaxes(got[S_], -1, -2))
    np.testing.assert_array_equal(got[SF], np.swapaxes(got[SF], -1, -2))
    np.testing.assert_array_equal(got[MUF], got[MU][:, -1])
    np.testing.assert_array_equal(got[SF], got[S_][:, -1])
    assert ((got[W] > 0) == (ref["weights"] > 0)).all()          # 0 exactly where no row was applied


@pytest.fixture(scope="module")
def device():
    """The full robust call on the outlier inputs, per (case, gate, delta, tol, layout)."""
    cache = {}

    def get(name, gate, delta, tol, inputs="batch_outer"):
        key = (name, gate, delta, tol, inputs)
        if key not in cache:
            inp = rr.inputs(name)
            d = rr.delta_array(inp, delta) if isinstance(delta, tuple) else delta
            cache[key] = _full(name, inp, gate, d, tol, inputs)
        return cache[key]
    return get


# ---------------------------------------------------------------- 1. parity

@pytest.mark.parametrize("name,gate,delta,tol,inputs", PARITY, ids=IDS)
def test_parity(device, name, gate, delta, tol, inputs):
    ref = rr.reference(name, delta, tol, gate)
    got = device(name, gate, delta, tol, inputs)
    _check(f"{name} gate {gate} delta {delta} {inputs}", got, ref)
    assert (got[NIT] > 2).any() and (got[NIT] == 0).any()
    assert got[REJ].any() == (gate is not None)


# ---------------------------------------------------------------- 2. a delta per row

def test_a_delta_per_row(device):
    """`bias`: the pseudoranges' delta and another one for the bias row, as an array in Z's layout."""
    name, gate, delta, tol = rr.ROWS
    assert delta[0] != delta[1]
    _check(f"bias per-row delta {delta}", device(name, gate, delta, tol), rr.reference(name, delta, tol, gate))


@pytest.mark.parametrize("inputs", ["batch_outer", "batch_inner"])
def test_a_constant_array_is_the_scalar_call_bitwise(device, inputs):
    name, gate, delta, tol = rr.PARITY[0]
    inp = rr.inputs(name)
    scalar = device(name, gate, delta, tol, inputs)
    array = _full(name, inp, gate, np.full(inp["Z"].shape, delta), tol, inputs)
    on_device = _full(name, inp, gate, torch.as_tensor(_layout(np.full(inp["Z"].shape, delta), inputs), device="cuda"),
                      tol, inputs)
    for a, t, s in zip(array, on_device, scalar):
        np.testing.assert_array_equal(a, s)
        np.testing.assert_array_equal(t, s)


# ---------------------------------------------------------------- 3. delta = inf is the plain iterated run

@pytest.mark.parametrize("name", ir.CASES)
def test_an_infinite_delta_is_the_plain_run_bitwise(name):
    """On tests/iekf_reference.py's cold-prior sets at its cap and tol: the scalar and the array."""
    inp = ir.inputs(name)
    kw = dict(innovations=True, iterations=ir.CAP[name], iter_tol=ir.TOL[name])
    plain = _run(name, inp, **kw)
    assert len(plain) == 9 and (plain[NIT] > 2).any() and not plain[ST].any()
    applied = _applied(inp, plain[REJ])
    for huber in (np.inf, np.full(inp["Z"].shape, np.inf)):
        got = _run(name, inp, huber=huber, **kw)
        assert len(got) == 10
        for g, p in zip(got[:9], plain):
            np.testing.assert_array_equal(g, p)
        np.testing.assert_array_equal(got[W], applied.astype(np.float64))      # exactly 1 and exactly 0


# ---------------------------------------------------------------- 4. the gate sees the unweighted rows

@pytest.mark.parametrize("name,gate,delta,tol", rr.PARITY[4:], ids=[i for i in IDS[4:6]])
def test_the_mask_is_the_plain_runs_at_the_same_prediction(device, name, gate, delta, tol):
    """Up to and including its first step with rows, a filter of the gated robust run has seen what
    the gated plain run has seen: the prior and predictions.  The masks there are equal."""
    inp = rr.inputs(name)
    robust = device(name, gate, delta, tol)
    plain = _run(name, inp, gate=gate, innovations=True, iterations=rr.CAP, iter_tol=tol)
    nz = inp["nz"]
    first = np.argmax(nz > 0, axis=1)
    upto = (np.arange(nz.shape[1])[None, :] <= first[:, None]) & (nz > 0).any(axis=1)[:, None]
    assert (nz > 0).any(axis=1).all() and (plain[REJ][upto] != 0).sum() >= 5
    np.testing.assert_array_equal(robust[REJ][upto], plain[REJ][upto])


# ---------------------------------------------------------------- 5. independence

@pytest.mark.parametrize("name,gate,delta,tol", [rr.PARITY[0], rr.PARITY[3], rr.PARITY[4]],
                         ids=[IDS[0], IDS[3], IDS[4]])
def test_a_filter_alone_is_bitwise_its_result_in_the_batch(device, name, gate, delta, tol):
    """Neighbours in the workgroup make other numbers of passes; nothing of them leaks."""
    full = device(name, gate, delta, tol)
    inp = rr.inputs(name)
    counts = [full[NIT][b0:b0 + 4].max(axis=0) != full[NIT][b0:b0 + 4].min(axis=0) for b0 in (0, 4)]
    assert all(c.any() for c in counts)                # the pass counts differ within the workgroups of 0 and of 5
    for b in ALONE:
        alone = _full(name, _sub(inp, [b]), gate, delta, tol)
        for a, f in zip(alone, full):
            np.testing.assert_array_equal(a[0], f[b])
    some = _full(name, _sub(inp, list(ALONE)), gate, delta, tol)
    for a, f in zip(some, full):                                             # and in another batch, at another place
        np.testing.assert_array_equal(a, f[list(ALONE)])


# ---------------------------------------------------------------- 6. status

def test_a_nan_delta_is_status_1_and_stays_with_its_filter(device):
    """A device tensor is not checked on the host; the NaN makes a non-finite pivot."""
    name, gate, delta, tol = rr.PARITY[0]
    full = device(name, gate, delta, tol)
    inp = rr.inputs(name)
    b = 42
    k = int(np.flatnonzero(inp["nz"][b, 3:] >= 2)[0]) + 3
    D = np.full(inp["Z"].shape, delta)
    D[b, k, 0] = np.nan
    got = _full(name, inp, gate, torch.as_tensor(D, device="cuda"), tol)
    want = np.zeros(rr.B, dtype=np.int32)
    want[b] = 1
    np.testing.assert_array_equal(got[ST], want)
    others = np.arange(rr.B) != b
    assert others[[40, 41, 43]].all()                                        # the failed filter's workgroup
    for g, f in zip(got, full):
        np.testing.assert_array_equal(g[others], f[others])
    for i in (MU, S_, NIS, LL, REJ, NIT, W):
        np.testing.assert_array_equal(got[i][b, :k], full[i][b, :k])


def test_a_step_with_more_rows_than_capacity_is_predict_only(device):
    name, gate, delta, tol = rr.PARITY[0]
    full = device(name, gate, delta, tol)
    inp = _copy(rr.inputs(name))
    b = 6
    k = int(np.flatnonzero(inp["nz"][b, 2:-2] > 0)[0]) + 2
    inp["nz"][b, k] = inp["Z"].shape[2] + 1
    ref = rr.run(inp, rr.KIND[name], rr.CAP, tol, delta, dtype=np.longdouble)
    assert ref["status"][b] == 2 and (ref["status"] != 0).sum() == 1 and ref["n_iter"][b, k] == 0
    got = _full(name, inp, gate, delta, tol)
    np.testing.assert_array_equal(got[ST], ref["status"])
    assert got[NIT][b, k] == 0 and got[REJ][b, k] == 0 and got[NIS][b, k] == 0.0 and got[LL][b, k] == 0.0
    assert not got[W][b, k].any()                                            # zero weights
    bound = rr.reference(name, delta, tol, gate)["bound"]
    # the predicted state: mu-, S- of that step
    assert np.max(np.abs(got[MU][b, k] - ref["mp"][b, k].astype(np.float64))) <= bound["mu"]
    assert np.max(np.abs(got[S_][b, k] - ref["SP"][b, k].astype(np.float64))) <= bound["S"]
    for i in (MU, S_, NIS, LL, REJ, NIT, W):
        np.testing.assert_array_equal(got[i][b, :k], full[i][b, :k])
    others = np.arange(rr.B) != b
    for g, f in zip(got, full):
        np.testing.assert_array_equal(g[others], f[others])


# ---------------------------------------------------------------- 7. the class

def test_class_api_is_a_batch_of_one():
    """EKF.update(huber=...) step by step, one step without a measurement, equals run_batch over the
    same steps bitwise and holds that step's weights."""
    inp = rr.inputs("gnss")
    nzs, P, b = (6, 0, 4), 6, 3
    one = _sub(inp, [b])
    one["U"], one["Z"], one["sat"] = one["U"][:, :3], one["Z"][:, :3, :P].copy(), one["sat"][:, :3, :P].copy()
    one["R"] = np.ascontiguousarray(one["R"][:, :3, :P, :P])
    one["nz"] = np.array([nzs], dtype=np.int32)
    kw = dict(iterations=rr.CAP, iter_tol=3e-4, huber=5.0)
    mh, Sh, mu, S, st, n_iter, w = _run("gnss", one, **kw)
    assert st[0] == 0 and n_iter[0, 0] >= 2 and n_iter[0, 1] == 0 and w.shape == (1, 3, P)
    assert (w[0, 0] > 0).all() and not w[0, 1].any() and (w[0, 2, :4] > 0).all() and not w[0, 2, 4:].any()
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
        assert f.weights.shape == (ns,) and f.weights.dtype == np.float64
        np.testing.assert_array_equal(f.weights, w[0, k, :ns])
    # one delta per row of z
    h = ekf.EKF("gnss_pos_and_bias", "multi_pseudorange", one["mu0"][0], one["S0"][0])
    h.update(one["U"][0, 0], one["Z"][0, 0, :6], one["Q"], one["R"][0, 0, :6, :6], {"dt": 1.0}, None,
             {"sat_pos": one["sat"][0, 0, :6]}, **dict(kw, huber=np.full(6, 5.0)))
    np.testing.assert_array_equal(h.mu, mh[0, 0])
    np.testing.assert_array_equal(h.weights, w[0, 0])
    g = ekf.EKF("gnss_pos_and_bias", "multi_pseudorange", one["mu0"][0], one["S0"][0])
    g.update(one["U"][0, 0], one["Z"][0, 0, :4], one["Q"], one["R"][0, 0, :4, :4], {"dt": 1.0}, None,
             {"sat_pos": one["sat"][0, 0, :4]}, iterations=rr.CAP, iter_tol=3e-4)
    assert not hasattr(g, "weights") and hasattr(g, "n_iter")                # without the keyword nothing changes


# ---------------------------------------------------------------- 8. what the weights do

def test_the_device_reproduces_the_behaviour_on_the_outlier_set(device):
    """gnss, delta = 5 m, no gate: the median final position error is below a quarter of the plain
    iterated run's, and every applied planted row weighs less than every applied clean row."""
    name, gate, delta, tol = rr.PARITY[0]
    inp = rr.inputs(name)
    xf = inp["fx"]["mu"][-1][:3]
    robust = device(name, gate, delta, tol)
    plain = _run(name, inp, iterations=rr.CAP, iter_tol=tol)
    e_r = np.linalg.norm(robust[MUF][:, :3] - xf, axis=1)
    e_p = np.linalg.norm(plain[MUF][:, :3] - xf, axis=1)
    w, planted = robust[W], inp["planted"]
    applied = w > 0
    hi, lo = w[applied & planted].max(), w[applied & ~planted].min()
    print(f"final position error, median / max: robust {np.median(e_r):.2f} / {e_r.max():.2f} m, plain iterated "
          f"{np.median(e_p):.2f} / {e_p.max():.2f} m; omega: largest on a planted row {hi:.3f}, smallest on a "
          f"clean row {lo:.3f}")
    assert np.median(e_r) < 0.25 * np.median(e_p)
    assert (applied & planted).sum() > 500 and hi < lo
