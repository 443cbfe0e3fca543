"""Noise identification on the device: the lag-one output of k_ekf_rts (mhe_ekf_smooth_args,
utils.ekf.smooth_batch(lag_one=True)), k_ekf_em (csrc/mhe_em.hip, mhe_ekf_em_stats,
utils.ekf.em_stats) and utils.ekf.fit_noise.

Reference: tests/em_reference.py (full matrices, no LAPACK), run in float64 and in np.longdouble
on exactly what the device stage under test was given: the smoother on the device filter's
history, the statistics on the device smoother's output.  So only the stage's own rounding
enters, and per case and output
    floor = max |float64 run - longdouble run|,   bound = 8 floor + 1e-10 (1 + max |ref|)
(the convention of tests/test_gpu_urts.py); observed, floor and bound are printed for every
assertion.  Counts and statuses are compared exactly.

Inputs (tests/ekf_ragged.py): gnss B = 70 (one wave plus six lanes), T = 12, row counts over
EDGE_COUNTS and a per-filter R; the bias-row variant (pmax = 13, steps with no row); the 9-state
vehicle at T = 61; and gnss with B = 1, T = 1 and T = 2.
"""
import numpy as np
import pytest
import torch

import ekf_ragged as er
import em_reference as em
import utils.ekf as ekf
import utils.gnss as gnss

pytestmark = pytest.mark.gpu

DEV = "cuda"
KIND = {"gnss": em.GNSS, "bias": em.BIAS, "car": em.CAR}
PLUG = {"gnss": (gnss.gnss_pos_and_bias, gnss.multi_pseudorange),
        "bias": (gnss.gnss_pos_and_bias, gnss.multi_pseudorange_and_bias),
        "car": ("discrete_vehicle_dynamics", "vehicle_sensors_model")}
NAMES = ["gnss", "bias", "car", "gnssB1", "gnssT1", "gnssT2"]
BIG = ["gnss", "bias", "car"]
ALONE = (0, 63, 64, 69)
SMOOTH_KEYS = ("mu_s", "S_s", "C", "mu0_s", "S0_s")


def _np(t):
    """A C-ordered NumPy copy (a view of batch-innermost storage would keep its strides)."""
    return None if t is None else np.array(t.cpu().numpy(), order="C")


def _inputs(name):
    if name == "gnss":
        return er.gnss_inputs(70, T=12)
    if name == "bias":
        return er.bias_inputs()
    if name == "car":
        return er.autocar_inputs(70, 61)
    if name == "gnssB1":
        return er.gnss_inputs(1, T=12)
    T = {"gnssT1": 1, "gnssT2": 2}[name]
    return er.gnss_inputs(70, T=T, nz=np.random.default_rng(T).integers(0, 33, size=(70, T)))


def _hist(a, layout):
    """A (B, T, ...) history on the device: contiguous batch-outermost, or run_batch's form (a
    batch-outermost view of batch-innermost storage)."""
    a = np.asarray(a)
    if layout == "outer":
        return torch.as_tensor(np.array(a), device=DEV)
    st = torch.as_tensor(np.array(np.moveaxis(a, 0, -1), order="C"), device=DEV)
    return st.permute(st.dim() - 1, *range(st.dim() - 1))


class Case:
    """One input set: the device filter's history, the device smoother with lag-one on it, the
    device statistics on that, and the references of both stages -- computed once, read-only."""

    def __init__(self, name):
        self.name, self.kind = name, KIND[name[:4] if name.startswith("gnss") else name]
        self.dyn, self.meas = PLUG[name[:4] if name.startswith("gnss") else name]
        inp = self.inp = _inputs(name)
        U, Z, nz, sat = er.device_args(inp)
        out = ekf.run_batch(self.dyn, self.meas, inp["mu0"], inp["S0"], U, Z, nz, inp["Q"], inp["R"],
                            inp["dparams"]["dt"], sat, dyn_params=inp["dparams"])
        assert not _np(out[4]).any()
        self.mh, self.Sh = _np(out[0]), _np(out[1])
        a = (self.kind, self.mh, self.Sh, inp["U"], inp["Q"], inp["dparams"], inp["mu0"], inp["S0"])
        self.ref_smooth = em.both(em.smooth, SMOOTH_KEYS, *a)
        self.sm = dict(zip(("mu_s", "S_s", "status", "mu0_s", "S0_s", "C"),
                           [_np(t) for t in self.smooth(_hist(self.mh, "inner"), _hist(self.Sh, "inner"))]))
        s = self.sm
        b = (self.kind, s["mu_s"], s["S_s"], s["C"], inp["U"], inp["Z"], inp["nz"], inp["sat"], inp["dparams"])
        self.ref_stats = em.both(em.stats, ("Qsum", "r2"), *b, mu0_s=s["mu0_s"], S0_s=s["S0_s"])
        self.ref_stats_noprior = em.both(em.stats, ("Qsum", "r2"), *b)
        self.st = self.stats()

    def smooth(self, mh, Sh, inputs="batch_outer", prior=True, lag_one=True, inp=None, **kw):
        inp = self.inp if inp is None else inp
        U = inp["U"] if inputs == "batch_outer" else np.ascontiguousarray(np.moveaxis(inp["U"], 0, -1))
        pr = dict(mu0=inp["mu0"], S0=inp["S0"]) if prior else {}
        out = ekf.smooth_batch(self.dyn, mh, Sh, U, inp["Q"], inp["dparams"]["dt"], dyn_params=inp["dparams"],
                               inputs=inputs, lag_one=lag_one, **pr, **kw)
        if "stream" in kw:
            kw["stream"].synchronize()
        return out

    def stats(self, layout="inner", inputs="batch_outer", prior=True, sm=None, inp=None, **kw):
        """utils.ekf.em_stats on the device smoother's output (or `sm`), as NumPy arrays."""
        inp, sm = self.inp if inp is None else inp, self.sm if sm is None else sm
        U, Z, nz, sat = er.device_args(inp, inputs)
        pr = dict(mu0_s=sm["mu0_s"], S0_s=sm["S0_s"]) if prior else {}
        out = ekf.em_stats(self.dyn, self.meas, _hist(sm["mu_s"], layout), _hist(sm["S_s"], layout),
                           _hist(sm["C"], layout), U, Z, nz, inp["dparams"]["dt"], sat, dyn_params=inp["dparams"],
                           inputs=inputs, **pr, **kw)
        if "stream" in kw:
            kw["stream"].synchronize()
        return dict(zip(("Qsum", "q_cnt", "r2", "r_cnt", "status"), [_np(t) for t in out]))

    def sub(self, idx):
        inp = dict(self.inp)
        for key in ("mu0", "S0", "U", "Z", "nz", "sat"):
            inp[key] = np.ascontiguousarray(self.inp[key][idx])
        if self.inp["R"].ndim == 4:
            inp["R"] = np.ascontiguousarray(self.inp["R"][idx])
        return inp


_CASES = {}


@pytest.fixture(scope="module")
def case():
    def get(name):
        if name not in _CASES:
            _CASES[name] = Case(name)
        return _CASES[name]
    yield get
    _CASES.clear()


def _same(a, b):
    for key in a:
        np.testing.assert_array_equal(a[key], b[key], err_msg=key)


# ---------------------------------------------------------------- 1. parity

@pytest.mark.parametrize("name", NAMES)
def test_parity(case, name):
    """C, Qsum and r2 against the longdouble reference: both history layouts x both input layouts x
    with and without the prior.  Counts and statuses exact; C_0 is NaN without a prior."""
    c = case(name)
    B, T, n = c.mh.shape
    for layout in ("inner", "outer"):
        dm, dS = _hist(c.mh, layout), _hist(c.Sh, layout)
        inner = layout == "inner" and B > 1         # a batch of one is contiguous either way
        assert ekf._hist_storage(dm, (n,))[1] == inner
        for inputs in ("batch_outer", "batch_inner"):
            for prior in (True, False):
                what = f"{name} {layout}/{inputs}/{'prior' if prior else 'no prior'}"
                out = c.smooth(dm, dS, inputs, prior)
                assert len(out) == (6 if prior else 4)
                C = out[-1]
                assert tuple(C.shape) == (B, T, n, n) and ekf._hist_storage(C, (n, n))[1] == inner
                C = _np(C)
                assert not _np(out[2]).any()
                if prior:
                    em.check(what, C, c.ref_smooth, "C")
                    em.check(what, _np(out[0]), c.ref_smooth, "mu_s")
                    em.check(what, _np(out[1]), c.ref_smooth, "S_s")
                else:
                    assert np.isnan(C[:, 0]).all()                  # not formed, and said so
                    ref = dict(c.ref_smooth, C=c.ref_smooth["C"].copy())
                    ref["C"][:, 0] = np.nan
                    em.check(what, C, ref, "C")
                st = c.stats(layout, inputs, prior)
                ref = c.ref_stats if prior else c.ref_stats_noprior
                em.check(what, st["Qsum"], ref, "Qsum")
                em.check(what, st["r2"], ref, "r2")
                np.testing.assert_array_equal(st["q_cnt"], ref["q_cnt"])
                np.testing.assert_array_equal(st["r_cnt"], ref["r_cnt"])
                np.testing.assert_array_equal(st["status"], ref["status"])
                assert (st["q_cnt"] == T - 1 + int(prior)).all() and not st["status"].any()
                assert st["r2"].shape == (B, T, c.inp["Z"].shape[2])
    if T == 1:
        assert not c.stats(prior=False)["Qsum"].any()               # no step pairs: an empty sum


# ---------------------------------------------------------------- 2. lag-one leaves the smoother alone

@pytest.mark.parametrize("name", NAMES)
def test_lag_one_does_not_disturb_the_smoother(case, name):
    c = case(name)
    for layout in ("inner", "outer"):
        dm, dS = _hist(c.mh, layout), _hist(c.Sh, layout)
        for prior in (True, False):
            plain = [_np(t) for t in c.smooth(dm, dS, prior=prior, lag_one=False)]
            lag = [_np(t) for t in c.smooth(dm, dS, prior=prior)]
            assert len(lag) == len(plain) + 1
            for g, w in zip(lag, plain):
                np.testing.assert_array_equal(g, w)


# ---------------------------------------------------------------- 3. symmetry

@pytest.mark.parametrize("name", NAMES)
def test_qsum_is_bitwise_symmetric(case, name):
    c = case(name)
    for prior in (True, False):
        Qs = c.stats(prior=prior)["Qsum"]
        np.testing.assert_array_equal(Qs, np.swapaxes(Qs, -1, -2))
    lo = np.linalg.eigvalsh(c.st["Qsum"]).min(-1)
    print(f"{name}: min eig(Qsum) / max|Qsum| = {(lo / np.abs(c.st['Qsum']).max((1, 2))).min():.2e}")


# ---------------------------------------------------------------- 4. isolation

@pytest.mark.parametrize("name", BIG)
def test_a_filter_alone_equals_its_rows_in_the_batch(case, name):
    c = case(name)
    for j in ALONE:
        idx = slice(j, j + 1)
        one = c.sub(idx)
        out = [_np(t) for t in c.smooth(_hist(c.mh[idx], "inner"), _hist(c.Sh[idx], "inner"), inp=one)]
        for g, key in zip(out, ("mu_s", "S_s", "status", "mu0_s", "S0_s", "C")):
            np.testing.assert_array_equal(g, c.sm[key][idx], err_msg=key)
        sm = {k: v[idx] for k, v in c.sm.items()}
        _same(c.stats(sm=sm, inp=one), {k: v[idx] for k, v in c.st.items()})


# ---------------------------------------------------------------- 5. stream

@pytest.mark.parametrize("name", ["gnss", "car"])
def test_side_stream_gives_the_same_result(case, name):
    c = case(name)
    side = torch.cuda.Stream()
    out = [_np(t) for t in c.smooth(_hist(c.mh, "inner"), _hist(c.Sh, "inner"), stream=side)]
    np.testing.assert_array_equal(out[-1], c.sm["C"])
    _same(c.stats(stream=side), c.st)


# ---------------------------------------------------------------- 6. rejection mask

@pytest.mark.parametrize("name", BIG)
def test_rejection_mask(case, name):
    """Masked rows are exactly 0 and leave the count; every other row, and Qsum, bitwise the
    unmasked run's.  The mask goes in as a NumPy array and as a gated run's own device view."""
    c = case(name)
    nz, pmax = c.inp["nz"], c.inp["Z"].shape[2]
    rng = np.random.default_rng(17)
    bits = rng.uniform(size=nz.shape + (pmax,)) < 0.3            # bits beyond nz are set too: they count nothing
    valid = np.arange(pmax)[None, None, :] < nz[:, :, None]
    word = (bits.astype(np.uint64) << np.arange(pmax, dtype=np.uint64)).sum(-1).astype(np.uint32).view(np.int32)
    got = c.stats(rejected=word)
    hit = bits & valid
    assert hit.any() and (hit[..., pmax - 1].any() or pmax < 32)
    assert not got["r2"][hit].any()
    np.testing.assert_array_equal(got["r_cnt"], c.st["r_cnt"] - hit.sum((1, 2)))
    np.testing.assert_array_equal(got["r2"][~hit], c.st["r2"][~hit])
    for key in ("Qsum", "q_cnt", "status"):
        np.testing.assert_array_equal(got[key], c.st[key])
    ref = em.stats(c.kind, c.sm["mu_s"], c.sm["S_s"], c.sm["C"], c.inp["U"], c.inp["Z"], nz, c.inp["sat"],
                   c.inp["dparams"], c.sm["mu0_s"], c.sm["S0_s"], rejected=word)
    np.testing.assert_array_equal(got["r_cnt"], ref["r_cnt"])
    np.testing.assert_array_equal(got["r2"] == 0, ref["r2"] == 0)
    _same(c.stats(rejected=np.zeros_like(word)), c.st)            # an empty mask is no mask
    # a gated run's mask, as run_batch hands it back (a view of (T, B) storage)
    U, Z, nzd, sat = er.device_args(c.inp)
    run = ekf.run_batch(c.dyn, c.meas, c.inp["mu0"], c.inp["S0"], U, Z, nzd, c.inp["Q"], c.inp["R"],
                        c.inp["dparams"]["dt"], sat, dyn_params=c.inp["dparams"], gate=0.5, innovations=True)
    rej = run[7]
    assert not rej.is_contiguous() and _np(rej).any()
    _same(c.stats(rejected=rej), c.stats(rejected=_np(rej)))


# ---------------------------------------------------------------- 7. ragged counts

@pytest.mark.parametrize("name", BIG)
def test_ragged_counts(case, name):
    c = case(name)
    nz, pmax = c.inp["nz"], c.inp["Z"].shape[2]
    beyond = np.arange(pmax)[None, None, :] >= nz[:, :, None]
    assert beyond.any() and (nz == 0).any()
    assert not c.st["r2"][beyond].any()                             # exactly 0
    assert (c.st["r2"][~beyond] > 0).all()
    np.testing.assert_array_equal(c.st["r_cnt"], nz.sum(1))
    # a step that claims more rows than the arrays hold: status 2, the step skipped, nobody else touched
    j, k = 66, int(np.flatnonzero(nz[66])[0])
    over = dict(c.inp, nz=nz.copy())
    over["nz"][j, k] = pmax + 1
    got = c.stats(inp=over)
    want = np.zeros_like(c.st["status"])
    want[j] = 2
    np.testing.assert_array_equal(got["status"], want)
    assert not got["r2"][j, k].any() and got["r_cnt"][j] == c.st["r_cnt"][j] - nz[j, k]
    keep = np.ones(nz.shape, dtype=bool)
    keep[j, k] = False
    np.testing.assert_array_equal(got["r2"][keep], c.st["r2"][keep])
    np.testing.assert_array_equal(got["Qsum"], c.st["Qsum"])       # the dynamics' sum does not read nz


# ---------------------------------------------------------------- 8. fault isolation

@pytest.mark.parametrize("name", BIG)
def test_a_nan_is_reported_and_isolated(case, name):
    """NaN arithmetic only: a NaN planted in one filter's smoothed mean, in another's lag-one
    record; status 1 and NaN sums for those two, every other filter bitwise the healthy run's."""
    c = case(name)
    T = c.mh.shape[1]
    sm = {k: v.copy() for k, v in c.sm.items()}
    (j1, k1), (j2, k2) = (5, T // 2), (65, T - 1)
    sm["mu_s"][j1, k1, 1] = np.nan
    sm["C"][j2, k2, 0, 2] = np.nan
    got = c.stats(sm=sm)
    want = np.zeros_like(c.st["status"])
    want[[j1, j2]] = 1
    np.testing.assert_array_equal(got["status"], want)
    ok = want == 0
    for key in got:
        np.testing.assert_array_equal(got[key][ok], c.st[key][ok], err_msg=key)
    for j in (j1, j2):
        assert np.isnan(got["Qsum"][j]).all() and np.isnan(got["r2"][j]).all()
    # and the smoother: a NaN in the filtered history leaves C NaN from the step above it down
    mh = c.mh.copy()
    mh[j1, k1, 1] = np.nan
    out = [_np(t) for t in c.smooth(_hist(mh, "inner"), _hist(c.Sh, "inner"))]
    np.testing.assert_array_equal(out[2], (np.arange(mh.shape[0]) == j1).astype(out[2].dtype))
    assert np.isnan(out[-1][j1, :k1 + 2]).all()
    np.testing.assert_array_equal(out[-1][j1, k1 + 2:], c.sm["C"][j1, k1 + 2:])
    others = np.arange(mh.shape[0]) != j1
    np.testing.assert_array_equal(out[-1][others], c.sm["C"][others])


# ---------------------------------------------------------------- 9. the fitting loop

def test_fit_noise_on_synthetic_data_with_a_known_truth():
    """tests/golden/em_fit_gnss.npz (em_reference.make_fit_recipe): truth Q = diag(0.5, 0.5, 0.5, 2,
    0.01), r = 9; start 50 Q and r = 100; 12 rounds."""
    d = em.fit_inputs()
    ref = em.fit_reference()
    out = ekf.fit_noise(gnss.gnss_pos_and_bias, gnss.multi_pseudorange, d["mu0"], d["S0"], d["U"], d["Z"], d["nz"],
                        d["Q"], d["R"], 1.0, d["sat"], rounds=em.FIT_ROUNDS)
    assert out["n_iter"] == em.FIT_ROUNDS and int(out["n_used"].item()) == d["Z"].shape[0]
    for key in ("Q", "R", "rho", "loglik"):
        assert out[key].is_cuda
    ll = _np(out["loglik"])
    print("device loglik per round:", np.array2string(ll, precision=2))
    print(f"smallest gain {np.diff(ll).min():.3f}")
    assert ll.shape == (em.FIT_ROUNDS,) and (np.diff(ll) >= 0).all()
    em.check("fit", _np(out["Q"]), ref, "Q")
    em.check("fit", _np(out["rho"]), ref, "rho")
    rho = float(out["rho"].item())
    assert np.abs(_np(out["R"]) - rho * d["R"]).max() <= 1e-12 * rho * em.FIT_R_START
    print(f"r: {em.FIT_R_START} -> {rho * em.FIT_R_START:.4f} (truth {em.FIT_R_TRUE}); diag Q -> {np.diag(_np(out['Q']))}")
    assert abs(rho * em.FIT_R_START - em.FIT_R_TRUE) < abs(em.FIT_R_START - em.FIT_R_TRUE)
    q0, qt = np.diag(d["Q"]), np.diag(em.FIT_Q_TRUE)
    assert (np.abs(np.diag(_np(out["Q"])) - qt) < np.abs(q0 - qt)).all()


def test_fit_noise_keywords():
    d = em.fit_inputs()
    a = (gnss.gnss_pos_and_bias, gnss.multi_pseudorange, d["mu0"], d["S0"], d["U"], d["Z"], d["nz"], d["Q"], d["R"], 1.0,
         d["sat"])
    full = ekf.fit_noise(*a, rounds=2)
    only_r = ekf.fit_noise(*a, rounds=2, fit_Q=False)
    np.testing.assert_array_equal(_np(only_r["Q"]), d["Q"])
    assert float(only_r["rho"].item()) != 1.0
    only_q = ekf.fit_noise(*a, rounds=2, fit_R=False)
    np.testing.assert_array_equal(_np(only_q["R"]), d["R"])
    assert float(only_q["rho"].item()) == 1.0
    diag = ekf.fit_noise(*a, rounds=2, q_structure="diag")
    Qd = _np(diag["Q"])
    np.testing.assert_array_equal(Qd, np.diag(np.diag(Qd)))
    one = ekf.fit_noise(*a, rounds=1)
    np.testing.assert_array_equal(_np(one["loglik"]), _np(full["loglik"])[:1])     # the entering parameters' likelihood
    inner = ekf.fit_noise(a[0], a[1], d["mu0"], d["S0"], *er.device_args(dict(d), "batch_inner")[:3], d["Q"], d["R"], 1.0,
                          er.device_args(dict(d), "batch_inner")[3], rounds=2, inputs="batch_inner")
    np.testing.assert_array_equal(_np(inner["Q"]), _np(full["Q"]))
    gated = ekf.fit_noise(*a, rounds=2, gate=np.inf)              # screens nothing: the same fit through the gated kernels
    np.testing.assert_allclose(_np(gated["Q"]), _np(full["Q"]), rtol=1e-9)
    Rfull = d["R"] + 0.5                                          # off-diagonal entries
    with pytest.raises(ValueError):
        ekf.fit_noise(*a[:8], Rfull, *a[9:], rounds=1)
    wave = ekf.fit_noise(*a[:8], Rfull, *a[9:], rounds=1, fit_R=False)
    assert np.isfinite(_np(wave["Q"])).all()
