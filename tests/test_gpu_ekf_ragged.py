"""Ragged batches through both EKF kernels (csrc/mhe_ekf.hip: k_ekf_lane, k_ekf).

The other EKF device tests tile one row-count vector over the batch, so all lanes of a
wave do the same work.  Here every instance has its own row count at every step (0..32,
with the counts either side of k_ekf_lane's 8-row chunks planted in every wave), its own
R (r_bstride != 0), and B = 301: two blocks of k_ekf_lane with 45 lanes in the second,
75 full workgroups of k_ekf and one with a single wave.  Builders: tests/ekf_ragged.py.

Reference: oracle/ekf.py (the reference's update with an explicit inv(P)), run for every
instance at every step, once per module.  Tolerance: the project's existing EKF bound,
|dmu| <= 1e-9 (1 + |mu|) and |dS| <= 1e-9 max|S| per instance and step (test_ekf._close).
"""
import numpy as np
import pytest

import ekf_ragged as er
from oracle import ekf as oekf
from test_ekf import MU_TOL, S_TOL, _close
import utils.ekf as ekf
import utils.gnss as gnss

B_MAIN = 301
CAP_B, CAP_PMAX, CAP_J, CAP_K = 70, 12, 37, 5     # the planted nz = 13 of the capacity test
SPD_J = 130                                        # the planted not-SPD instance


@pytest.fixture(scope="module")
def ragged():
    inp = er.gnss_inputs(B_MAIN)
    inp["ref"] = er.oracle_run(inp)
    return inp


@pytest.fixture(scope="module")
def capacity():
    rng = np.random.default_rng(99)
    nz = er.ragged_counts(rng, CAP_B, 12, CAP_PMAX, edges=(0, 1, 7, 8, 9, 12))
    nz[CAP_J, CAP_K] = CAP_PMAX + 1
    inp = er.gnss_inputs(CAP_B, 12, CAP_PMAX, seed=100, nz=nz)
    inp["ref"] = er.oracle_run(inp, predict_only={(CAP_J, CAP_K)})
    return inp


@pytest.fixture(scope="module")
def bias_case():
    inp = er.bias_inputs()
    inp["ref"] = er.oracle_run(inp, meas=oekf.multi_pseudorange_and_bias, extra=1)
    return inp


@pytest.fixture(scope="module")
def autocar_case():
    inp = er.autocar_inputs()
    inp["ref"] = er.oracle_run(inp, dyn=oekf.discrete_vehicle_dynamics, meas=oekf.vehicle_sensors_model)
    return inp


def _spd_case(ragged):
    """The module's ragged input with one negative R entry; (inputs, j, k)."""
    k = int(np.flatnonzero(ragged["nz"][SPD_J] >= 1)[0])
    inp = dict(ragged, R=ragged["R"].copy())
    inp["R"][SPD_J, k, 0, 0] = -1e9
    return inp, SPD_J, k


def _run(inp, method, inputs="batch_outer", dyn=gnss.gnss_pos_and_bias, meas=gnss.multi_pseudorange, **kw):
    U, Z, nz, sat = er.device_args(inp, inputs)
    mh, Sh, mu, S, st = ekf.run_batch(dyn, meas, inp["mu0"], inp["S0"], U, Z, nz, inp["Q"], inp["R"],
                                      inp["dparams"]["dt"], sat, method=method, inputs=inputs,
                                      dyn_params=inp["dparams"], **kw)
    c = lambda t: None if t is None else t.cpu().numpy()   # noqa: E731
    return c(mh), c(Sh), c(mu), c(S), c(st)


def _assert_close(what, mh, Sh, ref, rows=None):
    rmu, rS = ref[0], ref[1]
    if rows is not None:
        mh, Sh, rmu, rS = mh[rows], Sh[rows], rmu[rows], rS[rows]
    emu, eS = _close(mh, Sh, rmu, rS)
    print(f"{what}: mu {emu:.2e}, S {eS:.2e} (bound {MU_TOL:.0e})")
    assert emu <= MU_TOL and eS <= S_TOL, (what, emu, eS)


# ---------------------------------------------------------------- preconditions (no device)

def test_ragged_builders_meet_their_preconditions(ragged, capacity):
    nz = ragged["nz"]
    assert nz.shape == (B_MAIN, 12) and ragged["R"].shape == (B_MAIN, 12, 32, 32)
    assert er.edges_in_every_window(nz, er.EDGE_COUNTS)
    assert nz.min() == 0 and nz.max() == 32
    # lanes of one wave disagree on the chunk count at every step
    chunks = (nz + 7) // 8
    for w0 in range(0, B_MAIN, er.WAVE):
        assert (chunks[w0:w0 + er.WAVE].max(0) > chunks[w0:w0 + er.WAVE].min(0)).all()
    offd = ragged["R"] - ragged["R"] * np.eye(32)
    assert not offd.any() and np.unique(ragged["R"][:, :, 0, 0]).size == B_MAIN * 12
    assert ragged["ref"][2].all()                       # P is SPD at every correction
    assert np.isfinite(ragged["ref"][0]).all() and np.isfinite(ragged["ref"][1]).all()
    # satellites: above the horizon, at the fixture's radius, fixture slots kept
    fx, sat = ragged["fx"], ragged["sat"]
    assert (sat[..., 2] > 0).all()
    rad = np.linalg.norm(sat, axis=-1)
    assert rad.min() > 2.0e7 and rad.max() < 2.6e7
    np.testing.assert_array_equal(sat[5, 3, :12], fx["sat_pos"][3, :12])
    # capacity case: one planted cell beyond pmax, not in the last instance or at the last step
    cnz = capacity["nz"]
    over = np.argwhere(cnz > CAP_PMAX)
    assert over.tolist() == [[CAP_J, CAP_K]] and CAP_J < CAP_B - 1 and CAP_K <= 12 - 2
    assert capacity["ref"][2].all()
    # not-SPD case: only the planted correction has no Cholesky factor
    inp, j, k = _spd_case(ragged)
    spd = er.oracle_run(inp, instances=[j])[2]
    assert not spd[j, k] and spd.sum() == spd.size - 1
    # bias-row variant: the oracle takes an empty sat_pos with the bias row
    bi = er.bias_inputs()
    assert bi["Z"].shape[2] == 13 and bi["nz"].max() == 13
    assert (bi["nz"] == 0).any() and (bi["nz"] == 1).any()
    y, J = oekf.multi_pseudorange_and_bias(np.arange(5.0), {"sat_pos": np.zeros((0, 3))}, jac=True)
    assert y.shape == (1,) and y[0] == 3.0 and not J.any()
    # autocar: prefixes of the fixture's rows, both ends of the range present
    ac = er.autocar_inputs()
    assert ac["nz"].shape == (70, 61) and (ac["nz"] <= ac["nz_fixture"][None]).all()
    steps = np.flatnonzero(ac["nz_fixture"])
    assert steps.size == 7 and (ac["nz"][:, steps] == 0).any()
    assert (ac["nz"][:, steps] == ac["nz_fixture"][steps]).any()
    assert (ac["nz"][:, steps].max(0) > ac["nz"][:, steps].min(0)).all()


def _update_raises_on_not_spd(fx):
    """The drop-in class turns status 1 into the reference's LinAlgError."""
    f = ekf.EKF(gnss.gnss_pos_and_bias, gnss.multi_pseudorange, fx["mu0"].copy(), fx["S0"].copy())
    R = np.diag(float(fx["r_pr"]) * np.ones(12))
    R[0, 0] = -1e9
    with pytest.raises(np.linalg.LinAlgError):
        f.update(np.zeros(3), fx["pr"][0, :12], fx["Q"], R, dyn_func_params={"dt": 1.0},
                 meas_func_params={"sat_pos": fx["sat_pos"][0, :12]})


# ---------------------------------------------------------------- device

@pytest.mark.gpu
@pytest.mark.parametrize("inputs", ["batch_outer", "batch_inner"])
@pytest.mark.parametrize("method", ["lane", "wave", "auto"])
def test_ragged_rows_match_oracle(ragged, method, inputs):
    assert er.edges_in_every_window(ragged["nz"], er.EDGE_COUNTS)
    mh, Sh, _, _, st = _run(ragged, method, inputs)
    assert not st.any(), np.flatnonzero(st)
    _assert_close(f"ragged {method}/{inputs}", mh, Sh, ragged["ref"])


@pytest.mark.gpu
@pytest.mark.parametrize("method", ["lane", "wave"])
def test_final_state_equals_last_history_entry(ragged, method):
    mh, Sh, mu, S, st = _run(ragged, method)
    none_h, none_S, mu2, S2, st2 = _run(ragged, method, keep_history=False)
    assert none_h is None and none_S is None
    assert not st.any() and not st2.any()
    np.testing.assert_array_equal(mu, mu2)
    np.testing.assert_array_equal(S, S2)
    np.testing.assert_array_equal(mu, mh[:, -1])
    np.testing.assert_array_equal(S, Sh[:, -1])


@pytest.mark.gpu
@pytest.mark.parametrize("method", ["lane", "wave"])
def test_ragged_bias_row_variant(bias_case, method):
    inp = bias_case
    assert (inp["nz"] == 0).any() and (inp["nz"] == 1).any() and inp["nz"].max() == 13
    mh, Sh, _, _, st = _run(inp, method, meas=gnss.multi_pseudorange_and_bias)
    assert not st.any(), np.flatnonzero(st)
    _assert_close(f"bias row {method}", mh, Sh, inp["ref"])


@pytest.mark.gpu
def test_ragged_correlated_R_per_instance():
    B = 9
    nz = er.ragged_counts(np.random.default_rng(5), B, 12, 32, edges=(1, 7, 8, 9, 17, 31, 32), lo=1, group=B)
    inp = er.gnss_inputs(B, seed=6, nz=nz, corr=(0.7, 0.3))
    assert inp["nz"].min() >= 1 and inp["R"].shape == (B, 12, 32, 32)
    assert np.unique(inp["R"][:, 0, 0, 1]).size == B     # a scale of its own per instance
    mh, Sh, _, _, st = _run(inp, "auto")
    assert not st.any(), np.flatnonzero(st)
    _assert_close("correlated R auto", mh, Sh, er.oracle_run(inp))
    wh, wS, _, _, _ = _run(inp, "wave")                   # auto took the general kernel
    np.testing.assert_array_equal(mh, wh)
    np.testing.assert_array_equal(Sh, wS)


@pytest.mark.gpu
@pytest.mark.parametrize("method", ["lane", "wave"])
def test_ragged_autocar(autocar_case, method):
    inp = autocar_case
    mh, Sh, _, _, st = _run(inp, method, dyn="discrete_vehicle_dynamics", meas="vehicle_sensors_model")
    assert not st.any(), np.flatnonzero(st)
    _assert_close(f"autocar {method}", mh, Sh, inp["ref"])


@pytest.mark.gpu
@pytest.mark.parametrize("inputs", ["batch_outer", "batch_inner"])
@pytest.mark.parametrize("method", ["lane", "wave"])
def test_rows_beyond_capacity_are_refused(capacity, method, inputs):
    """A step that claims more rows than Z / PAR / R hold (nz = 13, pmax = 12) is refused:
    status 2 and a predict-only step, as for nz > 32.  (Placed so that a kernel that does read
    row 13 reads the next step's first row, inside every allocation.)"""
    mh, Sh, _, _, st = _run(capacity, method, inputs)
    want = np.zeros(CAP_B, dtype=st.dtype)
    want[CAP_J] = 2
    np.testing.assert_array_equal(st, want)
    _assert_close(f"capacity {method}/{inputs} refused instance", mh, Sh, capacity["ref"], rows=[CAP_J])
    _assert_close(f"capacity {method}/{inputs} others", mh, Sh, capacity["ref"],
                  rows=np.arange(CAP_B) != CAP_J)


@pytest.mark.gpu
@pytest.mark.parametrize("method", ["lane", "wave"])
def test_not_spd_is_reported_and_isolated(ragged, method):
    inp, j, k = _spd_case(ragged)
    mh, Sh, _, _, st = _run(inp, method)
    want = np.zeros(B_MAIN, dtype=st.dtype)
    want[j] = 1
    np.testing.assert_array_equal(st, want)
    _assert_close(f"not SPD {method} others", mh, Sh, ragged["ref"], rows=np.arange(B_MAIN) != j)
    _update_raises_on_not_spd(ragged["fx"])
