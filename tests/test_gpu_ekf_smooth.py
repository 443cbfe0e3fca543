"""RTS smoother on the device (csrc/mhe_ekf.hip k_ekf_rts, mhe_ekf_smooth, utils.ekf.smooth_batch).

Reference: tests/rts_reference.py (np.linalg.solve on full matrices, oracle/ekf.py's dynamics),
run per filter, once per module.  Bound: the project's EKF bound (test_ekf.MU_TOL / S_TOL:
|dmu| <= 1e-9 (1 + |mu|), |dS| <= 1e-9 max|S| per filter and step).  The backward pass alone
is compared on the device's own filtered history, so only the smoother's rounding enters.
End to end (device filter + device smoother against oracle filter + reference smoother) the
forward difference enters too: the bound stays the project's unless the change of the
REFERENCE's result under that forward difference (reference smoother on the device history
against reference smoother on the oracle history) alone exceeds it, and is then 8 x that
change (the "8 x floor" convention of tests/cov_reference.py).

Batches: B = 301 (gnss, T = 12: a second block with 45 lanes; ragged row counts 0..32 and a
per-filter R in the forward pass), B = 70 (one wave plus six lanes: gnss T = 1, 2, the bias-row
variant, and the 9-state vehicle at T = 61).
"""
import ctypes

import numpy as np
import pytest

import ekf_ragged as er
import rts_reference as rts
from mhe import _lib
from oracle import ekf as oekf
from test_ekf import MU_TOL, S_TOL, _close
import utils.ekf as ekf
import utils.gnss as gnss

pytestmark = pytest.mark.gpu

B_MAIN, B_SMALL = 301, 70
ALONE = (0, 63, 64)                      # and B - 1
GNSS = dict(dyn=gnss.gnss_pos_and_bias, meas=gnss.multi_pseudorange, odyn=oekf.gnss_pos_and_bias,
            omeas=oekf.multi_pseudorange, extra=0)
BIAS = dict(GNSS, meas=gnss.multi_pseudorange_and_bias, omeas=oekf.multi_pseudorange_and_bias, extra=1)
CAR = dict(dyn="discrete_vehicle_dynamics", meas="vehicle_sensors_model", odyn=oekf.discrete_vehicle_dynamics,
           omeas=oekf.vehicle_sensors_model, extra=0)


def _np(t):
    return None if t is None else t.cpu().numpy()


def _forward(inp, kind, method, inputs="batch_outer"):
    """Device filter; (mu_hist, S_hist) as run_batch returns them (device views)."""
    U, Z, nz, sat = er.device_args(inp, inputs)
    mh, Sh, _, _, st = ekf.run_batch(kind["dyn"], kind["meas"], inp["mu0"], inp["S0"], U, Z, nz, inp["Q"], inp["R"],
                                     inp["dparams"]["dt"], sat, method=method, inputs=inputs,
                                     dyn_params=inp["dparams"])
    assert not _np(st).any()
    return mh, Sh


def _smooth(inp, kind, mh, Sh, inputs="batch_outer", prior=False, **kw):
    U = inp["U"] if inputs == "batch_outer" else np.ascontiguousarray(np.moveaxis(inp["U"], 0, -1))
    pr = dict(mu0=inp["mu0"], S0=inp["S0"]) if prior else {}
    return ekf.smooth_batch(kind["dyn"], mh, Sh, U, inp["Q"], inp["dparams"]["dt"], dyn_params=inp["dparams"],
                            inputs=inputs, **pr, **kw)


def _ref(inp, kind, mh, Sh, prior=False):
    pr = (inp["mu0"], inp["S0"]) if prior else ()
    return rts.smooth_batch(kind["odyn"], mh, Sh, inp["U"], inp["Q"], inp["dparams"], *pr)


def _assert_close(what, mu, S, rmu, rS, tol=(MU_TOL, S_TOL)):
    emu, eS = _close(mu, S, rmu, rS)
    print(f"{what}: mu {emu:.2e} (bound {tol[0]:.1e}), S {eS:.2e} (bound {tol[1]:.1e})")
    assert emu <= tol[0] and eS <= tol[1], (what, emu, eS)


class Case:
    """One input set: the device forward histories of both kernels, the reference smoother
    on each of them, the oracle forward and the reference smoother on it -- computed once."""

    def __init__(self, inp, kind):
        self.inp, self.kind = inp, kind
        self.fwd, self.ref = {}, {}
        for method in ("lane", "wave"):
            mh, Sh = _forward(inp, kind, method)
            self.fwd[method] = (mh, Sh)
            self.ref[method] = _ref(inp, kind, _np(mh), _np(Sh), prior=True)
        omu, oS, _ = er.oracle_run(inp, dyn=kind["odyn"], meas=kind["omeas"], extra=kind["extra"])
        self.oracle = _ref(inp, kind, omu, oS, prior=True)


def _short(T):
    return er.gnss_inputs(B_SMALL, T=T, nz=np.random.default_rng(T).integers(0, 33, size=(B_SMALL, T)))


@pytest.fixture(scope="module")
def main():
    return Case(er.gnss_inputs(B_MAIN), GNSS)


@pytest.fixture(scope="module")
def cases(main):
    return {"gnss301": main, "gnssT1": Case(_short(1), GNSS), "gnssT2": Case(_short(2), GNSS),
            "bias": Case(er.bias_inputs(), BIAS), "car": Case(er.autocar_inputs(), CAR)}


NAMES = ["gnss301", "gnssT1", "gnssT2", "bias", "car"]


@pytest.mark.parametrize("method", ["lane", "wave"])
@pytest.mark.parametrize("name", NAMES)
def test_backward_pass_alone(cases, name, method):
    """Device smoother on the device's own filtered history against the reference on the same
    history; the forward inputs are ragged (row counts 0..32, predict-only steps, per-filter R)."""
    c = cases[name]
    if name in ("gnss301", "bias"):
        assert (c.inp["nz"] == 0).any() and c.inp["nz"].max() > 8
    mh, Sh = c.fwd[method]
    ms, Ss, st, m0s, S0s = _smooth(c.inp, c.kind, mh, Sh, prior=True)
    assert not _np(st).any(), np.flatnonzero(_np(st))
    r = c.ref[method]
    _assert_close(f"backward {name}/{method}", _np(ms), _np(Ss), r[0], r[1])
    _assert_close(f"backward {name}/{method} prior", _np(m0s), _np(S0s), r[2], r[3])


@pytest.mark.parametrize("method", ["lane", "wave"])
@pytest.mark.parametrize("name", NAMES)
def test_end_to_end(cases, name, method):
    c = cases[name]
    mh, Sh = c.fwd[method]
    ms, Ss, st, m0s, S0s = _smooth(c.inp, c.kind, mh, Sh, prior=True)
    r, o = c.ref[method], c.oracle
    fmu, fS = _close(r[0], r[1], o[0], o[1])          # the reference's own move under the forward difference
    tol = (MU_TOL if fmu <= MU_TOL else 8 * fmu, S_TOL if fS <= S_TOL else 8 * fS)
    print(f"end to end {name}/{method}: reference moves by mu {fmu:.2e}, S {fS:.2e} under the forward difference")
    _assert_close(f"end to end {name}/{method}", _np(ms), _np(Ss), o[0], o[1], tol)
    pmu, pS = _close(r[2], r[3], o[2], o[3])
    ptol = (MU_TOL if pmu <= MU_TOL else 8 * pmu, S_TOL if pS <= S_TOL else 8 * pS)
    _assert_close(f"end to end {name}/{method} prior", _np(m0s), _np(S0s), o[2], o[3], ptol)


@pytest.mark.parametrize("name", ["gnss301", "car"])
def test_layouts_agree_bitwise(cases, name):
    """Batch-innermost (run_batch's views, no copy) and batch-outermost histories, both U layouts."""
    c = cases[name]
    mh, Sh = c.fwd["lane"]
    st_mu, bi_mu = ekf._hist_storage(mh, (mh.shape[2],))
    st_S, bi_S = ekf._hist_storage(Sh, tuple(Sh.shape[2:]))
    assert bi_mu and bi_S and st_mu.data_ptr() == mh.data_ptr() and st_S.data_ptr() == Sh.data_ptr()
    assert st_mu.is_contiguous() and st_S.is_contiguous() and st_mu.shape[-1] == mh.shape[0]
    base = [_np(t) for t in _smooth(c.inp, c.kind, mh, Sh, prior=True)]
    outer = mh.contiguous(), Sh.contiguous()
    assert not ekf._hist_storage(outer[0], (mh.shape[2],))[1]
    for hist, inputs in ((outer, "batch_outer"), (outer, "batch_inner"), ((mh, Sh), "batch_inner"),
                         ((_np(mh), _np(Sh)), "batch_outer")):
        got = [_np(t) for t in _smooth(c.inp, c.kind, hist[0], hist[1], inputs=inputs, prior=True)]
        for g, w in zip(got, base):
            np.testing.assert_array_equal(g, w)


@pytest.mark.parametrize("bi", [0, 1])
@pytest.mark.parametrize("name", ["gnss301", "car"])
def test_in_place_equals_out_of_place(cases, name, bi):
    """The C entry point with mu_s == mu_hist and S_s == S_hist, in both history layouts."""
    import torch
    c = cases[name]
    mh, Sh = c.fwd["lane"]
    want = [_np(t) for t in _smooth(c.inp, c.kind, mh, Sh)]
    B, T, n = mh.shape
    m = c.inp["U"].shape[2]
    if bi:
        mu_io, S_io = mh.permute(1, 2, 0).contiguous().clone(), Sh.permute(1, 2, 3, 0).contiguous().clone()
    else:
        mu_io, S_io = mh.contiguous().clone(), Sh.contiguous().clone()
    U = torch.as_tensor(c.inp["U"], device=mh.device).contiguous()
    Q = torch.as_tensor(c.inp["Q"], device=mh.device).contiguous()
    st = torch.full((B,), -1, dtype=torch.int32, device=mh.device)
    did, _, _ = ekf.dynamics(c.kind["dyn"])
    dims = _lib.MheEkfDims(n=n, m=m, dyn_model=did, dt=float(c.inp["dparams"]["dt"]), hist_batch_inner=bi)
    for i, v in enumerate(ekf.dyn_par(c.kind["dyn"], c.inp["dparams"])):
        dims.dyn_par[i] = float(v)
    p = lambda t: ctypes.c_void_p(t.data_ptr())   # noqa: E731
    rc = _lib.load().mhe_ekf_smooth(ctypes.byref(dims), B, T, p(mu_io), p(S_io), p(U), T * m, p(Q), None, None,
                                    p(mu_io), p(S_io), None, None, p(st),
                                    ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert rc == 0
    torch.cuda.synchronize()
    assert not _np(st).any()
    got_mu = _np(mu_io.permute(2, 0, 1) if bi else mu_io)
    got_S = _np(S_io.permute(3, 0, 1, 2) if bi else S_io)
    np.testing.assert_array_equal(got_mu, want[0])
    np.testing.assert_array_equal(got_S, want[1])


@pytest.mark.parametrize("name", ["gnss301", "car"])
def test_a_filter_alone_equals_its_batch_result(cases, name):
    c = cases[name]
    mh, Sh = c.fwd["lane"]
    B = mh.shape[0]
    full = [_np(t) for t in _smooth(c.inp, c.kind, mh, Sh, prior=True)]
    for j in ALONE + (B - 1,):
        one = {k: c.inp[k][j:j + 1] for k in ("U", "mu0", "S0")}
        one.update(Q=c.inp["Q"], dparams=c.inp["dparams"])
        got = [_np(t) for t in _smooth(one, c.kind, mh[j:j + 1], Sh[j:j + 1], prior=True)]
        for g, w in zip(got, full):
            np.testing.assert_array_equal(g, w[j:j + 1])


@pytest.mark.parametrize("method", ["lane", "wave"])
@pytest.mark.parametrize("name", ["gnss301", "car"])
def test_symmetry_and_ordering(cases, name, method):
    c = cases[name]
    mh, Sh = c.fwd[method]
    ms, Ss, st = [_np(t) for t in _smooth(c.inp, c.kind, mh, Sh)]     # no prior: three outputs
    mh, Sh = _np(mh), _np(Sh)
    np.testing.assert_array_equal(Ss, np.swapaxes(Ss, -1, -2))         # bitwise symmetric
    iu = np.triu_indices(mh.shape[2])
    np.testing.assert_array_equal(ms[:, -1], mh[:, -1])                # the last step is the filtered one,
    np.testing.assert_array_equal(Ss[:, -1][:, iu[0], iu[1]], Sh[:, -1][:, iu[0], iu[1]])   # its upper triangle
    dS = Sh - Ss
    lo = np.linalg.eigvalsh(0.5 * (dS + np.swapaxes(dS, -1, -2))).min(-1)
    scale = np.abs(Sh).reshape(Sh.shape[:2] + (-1,)).max(-1)
    print(f"{name}/{method}: min eig(S - Ss) / max|S| = {(lo / scale).min():.2e}")
    assert (lo >= -1e-9 * scale).all()


@pytest.mark.parametrize("name", ["gnss301", "car"])
def test_predict_only_run_is_left_unchanged(cases, name):
    c = cases[name]
    free = dict(c.inp, nz=np.zeros_like(c.inp["nz"]))
    mh, Sh = _forward(free, c.kind, "lane")
    ms, Ss, st = _smooth(free, c.kind, mh, Sh)
    assert not _np(st).any()
    _assert_close(f"predict-only {name}", _np(ms), _np(Ss), _np(mh), _np(Sh))


def test_prior_is_optional(main):
    mh, Sh = main.fwd["lane"]
    assert len(_smooth(main.inp, GNSS, mh, Sh)) == 3
    out = _smooth(main.inp, GNSS, mh, Sh, prior=True)
    assert len(out) == 5 and out[3].shape == (B_MAIN, 5) and out[4].shape == (B_MAIN, 5, 5)
    np.testing.assert_array_equal(_np(out[4]), np.swapaxes(_np(out[4]), -1, -2))


def test_failures_are_reported_and_isolated(main):
    """A NaN in one filter's history and a predicted covariance without a Cholesky factor in
    another's: status 1 and NaN from that step down for those two, every other filter and the
    steps above bitwise as in the healthy run.  NaN arithmetic only."""
    mh, Sh = main.fwd["lane"]
    healthy = [_np(t) for t in _smooth(main.inp, GNSS, mh, Sh, prior=True)]
    mu_bad, S_bad = _np(mh).copy(), _np(Sh).copy()
    (j1, k1), (j2, k2) = (130, 5), (65, 7)
    mu_bad[j1, k1, 2] = np.nan
    S_bad[j2, k2, 1, 1] = -1e9
    ms, Ss, st, m0s, S0s = [_np(t) for t in _smooth(main.inp, GNSS, mu_bad, S_bad, prior=True)]
    want = np.zeros(B_MAIN, dtype=st.dtype)
    want[[j1, j2]] = 1
    np.testing.assert_array_equal(st, want)
    ok = want == 0
    for g, w in zip((ms, Ss, m0s, S0s), (healthy[0], healthy[1], healthy[3], healthy[4])):
        np.testing.assert_array_equal(g[ok], w[ok])
    for j, k in ((j1, k1), (j2, k2)):
        assert np.isnan(ms[j, :k + 1]).all() and np.isnan(Ss[j, :k + 1]).all()
        assert np.isnan(m0s[j]).all() and np.isnan(S0s[j]).all()
        np.testing.assert_array_equal(ms[j, k + 1:], healthy[0][j, k + 1:])
        np.testing.assert_array_equal(Ss[j, k + 1:], healthy[1][j, k + 1:])


def test_side_stream_gives_the_same_result(main):
    import torch
    mh, Sh = main.fwd["lane"]
    want = [_np(t) for t in _smooth(main.inp, GNSS, mh, Sh, prior=True)]
    side = torch.cuda.Stream()
    out = _smooth(main.inp, GNSS, mh, Sh, prior=True, stream=side)
    side.synchronize()
    for g, w in zip(out, want):
        np.testing.assert_array_equal(_np(g), w)
