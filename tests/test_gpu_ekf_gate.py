"""Innovation gating and likelihood outputs of the batched EKF on the device (csrc/mhe_ekf.hip
k_ekf_lane<.., true> / k_ekf<.., true>, mhe_ekf_run_args, utils.ekf.run_batch(gate=, innovations=)).

Reference: tests/ekf_gate_reference.py (the screen from oracle/ekf.py's functions, then
oracle.ekf.EKF.update on the kept rows; nis by np.linalg.solve, log det by slogdet), computed
once per process.  Inputs: tests/ekf_ragged.py's builders with a consistent prior and a seeded
8 % of the valid rows shifted by +400 m; gates 10.83 and 0.5.  The reference asserts that no
row's d2 is within 1e-6 (relative) of the gate, so the reject masks are compared exactly.
Bounds: the project's EKF bound on the histories (test_ekf.MU_TOL / S_TOL through _close);
|dnis| <= 1e-9 (1 + nis) + 2 eta ||P_a^-1 e_a||_1 with eta = 4 spacing(max |z|) (the first-order
effect on nis of the rounding of z - h, both terms ~2e7 m), and half that plus
1e-9 (1 + |loglik|) on loglik.
"""
import numpy as np
import pytest

import ekf_gate_reference as gr
import rts_reference as rts
from test_ekf import MU_TOL, S_TOL, _close
import utils.ekf as ekf
import utils.gnss as gnss

pytestmark = pytest.mark.gpu

PLUG = {"gnss301": (gnss.gnss_pos_and_bias, gnss.multi_pseudorange),
        "gnss301c": (gnss.gnss_pos_and_bias, gnss.multi_pseudorange),
        "bias": (gnss.gnss_pos_and_bias, gnss.multi_pseudorange_and_bias),
        "car": ("discrete_vehicle_dynamics", "vehicle_sensors_model")}
ALONE = (0, 63, 64)                      # and B - 1
PARITY = [(n, m) for n in ("gnss301", "bias", "car") for m in ("lane", "wave")] + [("gnss301c", "wave")]


def _np(t):
    return None if t is None else t.cpu().numpy()


def _run(name, method, inp=None, inputs="batch_outer", **kw):
    """run_batch on a case's inputs (or `inp`); NumPy copies of what it returns."""
    inp = gr.inputs(name)[0] if inp is None else inp
    U, Z, nz, sat = gr.er.device_args(inp, inputs)
    dyn, meas = PLUG[name]
    out = ekf.run_batch(dyn, meas, inp["mu0"], inp["S0"], U, Z, nz, inp["Q"], inp["R"], inp["dparams"]["dt"], sat,
                        method=method, inputs=inputs, dyn_params=inp["dparams"], **kw)
    return out


@pytest.fixture(scope="module")
def plain():
    """The ungated call (today's instances), per (case, method)."""
    cache = {}

    def get(name, method):
        if (name, method) not in cache:
            cache[name, method] = [_np(t) for t in _run(name, method)]
        return cache[name, method]
    return get


@pytest.fixture(scope="module")
def gated():
    """gate = 10.83 with statistics, per (case, method): device tensors."""
    cache = {}

    def get(name, method):
        if (name, method) not in cache:
            cache[name, method] = _run(name, method, gate=10.83, innovations=True)
        return cache[name, method]
    return get


# ---------------------------------------------------------------- 1. parity

@pytest.mark.parametrize("gate", gr.GATES)
@pytest.mark.parametrize("name,method", PARITY)
def test_parity(name, method, gate):
    inp, _ = gr.inputs(name)
    r = gr.reference(name, gate)
    assert r["margin"] >= gr.MARGIN, r["margin"]             # the condition under which masks are exact
    mh, Sh, mu, S, st, nis, ll, rej = [_np(t) for t in _run(name, method, gate=gate, innovations=True)]
    assert nis.shape == ll.shape == rej.shape == inp["nz"].shape and rej.dtype == np.int32
    assert not st.any(), np.flatnonzero(st)
    np.testing.assert_array_equal(rej, r["rej"])
    emu, eS = _close(mh, Sh, r["mu"], r["S"])
    bound = 1e-9 * (1.0 + r["nis"]) + 2.0 * r["eta"]
    dn = np.abs(nis - r["nis"])
    dl = np.abs(ll - r["loglik"])
    lbound = 0.5 * bound + 1e-9 * (1.0 + np.abs(r["loglik"]))
    print(f"{name}/{method} gate {gate}: mu {emu:.2e} (bound {MU_TOL:.1e}), S {eS:.2e} (bound {S_TOL:.1e}), "
          f"nis worst |d| / bound {(dn / bound).max():.2e}, loglik {(dl / lbound).max():.2e}; "
          f"rounding share of the nis bound up to {(2.0 * r['eta'] / bound).max():.2f}")
    assert emu <= MU_TOL and eS <= S_TOL, (emu, eS)
    assert (dn <= bound).all(), (dn / bound).max()
    assert (dl <= lbound).all(), (dl / lbound).max()
    np.testing.assert_array_equal(mu, mh[:, -1])
    np.testing.assert_array_equal(S, Sh[:, -1])
    none = r["nkept"] == 0                                   # nz = 0 or every row screened out: exact zeros
    assert not nis[none].any() and not ll[none].any()


def test_parity_inputs_exercise_the_paths():
    """Partly and fully rejected steps, nz = 0 steps, a rejected bias row, bit 31, every 8-row
    chunk of the lane kernel holding a rejected row and a kept one."""
    for name in gr.CASES:
        inp, _ = gr.inputs(name)
        nz = inp["nz"]
        for gate in gr.GATES:
            r = gr.reference(name, gate)
            assert ((r["nkept"] == 0) & (nz > 0)).any() and ((r["nkept"] > 0) & (r["nrej"] > 0)).any()
        assert (nz == 0).any()
    inp, _ = gr.inputs("bias")
    r = gr.reference("bias", 10.83)
    w, nz = r["rej"].view(np.uint32), inp["nz"]
    assert (((w >> np.maximum(nz - 1, 0).astype(np.uint32)) & 1)[nz > 0] == 1).any()
    w = gr.reference("gnss301", 0.5)["rej"].view(np.uint32)
    full = gr.inputs("gnss301")[0]["nz"] == 32
    assert ((w[full] >> 31) & 1).any() and ((~w[full] >> 31) & 1).any()
    for lo in (0, 8, 16, 24):
        chunk = (w[full] >> lo) & 0xFF
        assert ((chunk != 0) & (chunk != 0xFF)).any()


# ---------------------------------------------------------------- 2. off means off

@pytest.mark.parametrize("name,method", [(n, m) for n in ("gnss301", "car") for m in ("lane", "wave")])
def test_off_means_off(plain, name, method):
    """gate = inf with the statistics, and a gate no row reaches, through the new instances:
    bitwise the plain call's mu, S, histories and status."""
    want = plain(name, method)
    stats = [_np(t) for t in _run(name, method, gate=np.inf, innovations=True)]
    huge = [_np(t) for t in _run(name, method, gate=1e300)]
    assert len(stats) == 8 and len(huge) == 5
    for got in (stats, huge):
        for g, w in zip(got[:5], want):
            np.testing.assert_array_equal(g, w)
    assert not stats[7].any()
    nz = gr.inputs(name)[0]["nz"]
    assert not stats[5][nz == 0].any() and not stats[6][nz == 0].any()
    if name == "gnss301":                                    # every row applied: the planted ones show in nis
        assert (stats[5][nz > 0] > 0).all()
        some = gr.run(gr.inputs(name)[0], gr.GNSS, np.inf, instances=ALONE)
        for b in ALONE:                                      # statistics alone against the reference
            bound = 1e-9 * (1.0 + some["nis"][b]) + 2.0 * some["eta"][b]
            assert (np.abs(stats[5][b] - some["nis"][b]) <= bound).all()
            assert (np.abs(stats[6][b] - some["loglik"][b])
                    <= 0.5 * bound + 1e-9 * (1.0 + np.abs(some["loglik"][b]))).all()


# ---------------------------------------------------------------- 3. detection

@pytest.mark.parametrize("method", ["lane", "wave"])
def test_detection(plain, gated, method):
    inp, _ = gr.inputs("gnss301")
    planted = gr.planted_bits(inp)
    np.testing.assert_array_equal(gr.reference("gnss301", 10.83)["rej"], planted)   # holds for the reference
    out = [_np(t) for t in gated("gnss301", method)]
    np.testing.assert_array_equal(out[7], planted)           # every planted row and no clean one
    xf = inp["fx"]["mu"][-1][:3]
    eg = np.linalg.norm(out[2][:, :3] - xf, axis=-1)
    ep = np.linalg.norm(plain("gnss301", method)[2][:, :3] - xf, axis=-1)
    print(f"{method}: final position error median / max, every row applied {np.median(ep):.1f} / {ep.max():.1f} m, "
          f"screened at 10.83 {np.median(eg):.1f} / {eg.max():.1f} m ({int(inp['planted'].sum())} planted rows)")
    assert np.median(eg) < np.median(ep)


# ---------------------------------------------------------------- 4. layouts and placement

@pytest.mark.parametrize("name,method", [("gnss301", "lane"), ("gnss301", "wave"), ("car", "lane"), ("car", "wave")])
def test_layouts_and_placement(gated, name, method):
    import torch
    want = [_np(t) for t in gated(name, method)]
    inner = _run(name, method, inputs="batch_inner", gate=10.83, innovations=True)
    for g, w in zip(inner, want):
        np.testing.assert_array_equal(_np(g), w)
    for t in inner[5:]:                                      # views of batch-innermost storage
        assert t.permute(1, 0).is_contiguous()
    inp, _ = gr.inputs(name)
    B = inp["nz"].shape[0]
    for j in ALONE + (B - 1,):
        one = {k: (v[j:j + 1] if k in ("mu0", "S0", "U", "Z", "nz", "sat") or (k == "R" and v.ndim == 4) else v)
               for k, v in inp.items()}
        got = _run(name, method, inp=one, gate=10.83, innovations=True)
        for g, w in zip(got, want):
            np.testing.assert_array_equal(_np(g), w[j:j + 1])
    side = torch.cuda.Stream()
    out = _run(name, method, gate=10.83, innovations=True, stream=side)
    side.synchronize()
    for g, w in zip(out, want):
        np.testing.assert_array_equal(_np(g), w)


# ---------------------------------------------------------------- 5. degenerate steps

@pytest.mark.parametrize("method", ["lane", "wave"])
def test_a_step_with_too_many_rows(gated, method):
    """nz > pmax at one step of one filter: status 2 and zero statistics for that step (it is
    predict-only, as today); every other filter is bitwise unaffected."""
    inp, kind = gr.inputs("bias")                            # pmax = 13
    want = [_np(t) for t in gated("bias", method)]
    j, k = 37, 4
    nz = inp["nz"].copy()
    nz[j, k] = 14
    got = [_np(t) for t in _run("bias", method, inp=dict(inp, nz=nz), gate=10.83, innovations=True)]
    st = np.zeros_like(want[4])
    st[j] = 2
    np.testing.assert_array_equal(got[4], st)
    assert got[5][j, k] == 0 and got[6][j, k] == 0 and got[7][j, k] == 0
    others = np.arange(nz.shape[0]) != j
    for g, w in zip(got, want):
        np.testing.assert_array_equal(g[others], w[others])
    for g, w in zip((got[0], got[1], got[5], got[6], got[7]), (want[0], want[1], want[5], want[6], want[7])):
        np.testing.assert_array_equal(g[j, :k], w[j, :k])     # and the steps before it
    ref = gr.run(dict(inp, nz=np.where(nz == 14, 0, nz)), kind, 10.83, instances=[j])
    emu, eS = _close(got[0][j], got[1][j], ref["mu"][j], ref["S"][j])
    assert emu <= MU_TOL and eS <= S_TOL, (emu, eS)
    np.testing.assert_array_equal(got[7][j], ref["rej"][j])


# ---------------------------------------------------------------- 6. the EKF class

def test_ekf_update_with_a_gate():
    inp, kind = gr.inputs("gnss301")
    b = 5
    k = 0
    ns = 9
    z = inp["Z"][b, k, :ns] - gr.SHIFT * inp["planted"][b, k, :ns]   # a clean step
    z[6] += gr.SHIFT                                         # and one planted outlier
    R = inp["R"][b, k, :ns, :ns]
    sat = inp["sat"][b, k, :ns]
    u = inp["U"][b, k]
    rej, d2 = gr.screen(kind["odyn"], kind["omeas"], 0, inp["mu0"][b], inp["S0"][b], u, z, R, sat, inp["Q"],
                        inp["dparams"], 10.83)
    assert rej.tolist() == [i == 6 for i in range(ns)] and np.abs(d2 / 10.83 - 1.0).min() >= gr.MARGIN
    f = ekf.EKF(gnss.gnss_pos_and_bias, gnss.multi_pseudorange, inp["mu0"][b].copy(), inp["S0"][b].copy())
    f.update(u, z, inp["Q"], R, {"dt": 1.0}, None, {"sat_pos": sat}, gate=10.83)
    assert f.rejected.dtype == bool and f.rejected.tolist() == rej.tolist()
    keep = ~rej
    o = gr.oekf.EKF(kind["odyn"], kind["omeas"], inp["mu0"][b], inp["S0"][b])
    nis, ll, eta = gr.step(o, kind["odyn"], kind["omeas"], 0, u, z, R, sat, inp["Q"], inp["dparams"], 10.83)[2:]
    w = gr.oekf.EKF(kind["odyn"], kind["omeas"], inp["mu0"][b], inp["S0"][b])     # the update without that row
    w.update(u, z[keep], inp["Q"], R[keep][:, keep], {"dt": 1.0}, None, {"sat_pos": sat[keep]})
    np.testing.assert_array_equal(o.mu, w.mu)
    emu, eS = _close(f.mu[None], f.S[None], w.mu[None], w.S[None])
    assert emu <= MU_TOL and eS <= S_TOL, (emu, eS)
    bound = 1e-9 * (1.0 + nis) + 2.0 * eta
    assert abs(f.nis - nis) <= bound and abs(f.loglik - ll) <= 0.5 * bound + 1e-9 * (1.0 + abs(ll))
    # statistics only
    g = ekf.EKF(gnss.gnss_pos_and_bias, gnss.multi_pseudorange, inp["mu0"][b].copy(), inp["S0"][b].copy())
    g.update(u, z, inp["Q"], R, {"dt": 1.0}, None, {"sat_pos": sat}, gate=np.inf)
    assert not g.rejected.any() and g.nis > f.nis
    # a following update without a gate behaves as today: the plain update, and the statistics stay
    h = ekf.EKF(gnss.gnss_pos_and_bias, gnss.multi_pseudorange, f.mu.copy(), f.S.copy())
    seen = (f.nis, f.loglik, f.rejected.copy())
    z1, R1, sat1 = inp["Z"][b, 1, :ns], inp["R"][b, 1, :ns, :ns], inp["sat"][b, 1, :ns]
    f.update(u, z1, inp["Q"], R1, {"dt": 1.0}, None, {"sat_pos": sat1})
    h.update(u, z1, inp["Q"], R1, {"dt": 1.0}, None, {"sat_pos": sat1})
    np.testing.assert_array_equal(f.mu, h.mu)
    np.testing.assert_array_equal(f.S, h.S)
    assert not hasattr(h, "nis") and (f.nis, f.loglik) == seen[:2] and f.rejected.tolist() == seen[2].tolist()
    # predict only
    f.update(u, None, inp["Q"], None, {"dt": 1.0}, gate=10.83)
    assert f.nis == 0.0 and f.loglik == 0.0 and f.rejected.shape == (0,)


# ---------------------------------------------------------------- 7. smoothing

@pytest.mark.parametrize("name", ["gnss301", "car"])
def test_a_gated_history_smooths_as_any_other(gated, name):
    inp, kind = gr.inputs(name)
    out = gated(name, "lane")
    mh, Sh = out[0], out[1]
    ms, Ss, st = ekf.smooth_batch(PLUG[name][0], mh, Sh, inp["U"], inp["Q"], inp["dparams"]["dt"],
                                  dyn_params=inp["dparams"])
    assert not _np(st).any()
    rmu, rS = rts.smooth_batch(kind["odyn"], _np(mh), _np(Sh), inp["U"], inp["Q"], inp["dparams"])
    emu, eS = _close(_np(ms), _np(Ss), rmu, rS)
    print(f"smoothed gated history {name}: mu {emu:.2e}, S {eS:.2e}")
    assert emu <= MU_TOL and eS <= S_TOL, (emu, eS)
