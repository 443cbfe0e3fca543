"""Seeded builders for the ragged-batch EKF device tests (tests/test_gpu_ekf_ragged.py).

A "ragged" batch is one in which the instances of one launch do different amounts of
work: every instance has its own row count at every step, its own R, and the batch is no
multiple of the kernels' block sizes.  Everything here is NumPy on the host; the oracle
is oracle/ekf.py, run for every instance at every step.
"""
import os

import numpy as np

from oracle import ekf as oekf

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
CAR_KEYS = ("C_AF", "C_AR", "M", "D_F", "D_R", "I_Z")

# row counts every wave of k_ekf_lane must see: none, one, the rows either side of each
# boundary of its 8-row chunks, and the full capacity of 32
EDGE_COUNTS = (0, 1, 7, 8, 9, 15, 16, 17, 24, 25, 31, 32)
WAVE = 64


def gnss_fixture():
    return dict(np.load(os.path.join(GOLDEN, "ekf_gnss_stationary.npz")))


def autocar_fixture():
    g = np.load(os.path.join(GOLDEN, "ekf_autocar.npz"))
    d = {k: g[k] for k in g.files}
    d["dparams"] = {"dt": float(d["dt"]), "car_params": dict(zip(CAR_KEYS, d["car"]))}
    return d


def satellites(fx, rng, T, pmax):
    """(T, pmax, 3): the fixture's satellites of steps 0..T-1 in the leading slots, the
    rest (and any fixture slot beyond that step's nsat, which the log leaves empty) seeded
    unit directions above the horizon at the mean radius of the fixture's satellites."""
    nfx = min(pmax, fx["sat_pos"].shape[1])
    valid = np.arange(fx["sat_pos"].shape[1])[None, :] < fx["nsat"][:T, None]
    radius = float(np.linalg.norm(fx["sat_pos"][:T][valid[:T]], axis=-1).mean())
    d = rng.normal(size=(T, pmax, 3))
    d[..., 2] = np.abs(d[..., 2]) + 0.05
    sat = radius * d / np.linalg.norm(d, axis=-1, keepdims=True)
    keep = valid[:, :nfx]
    sat[:, :nfx][keep] = fx["sat_pos"][:T, :nfx][keep]
    return sat


def ragged_counts(rng, B, T, hi, edges=(), lo=0, group=WAVE // 2):
    """(B, T) int32 counts uniform in lo..hi; then every value of `edges` is planted at
    its own cell of every aligned group of `group` instances (the short last group
    included).  With group = 32 every run of 64 consecutive instances, aligned to a
    wave or not, holds a whole group and so every edge value."""
    nz = rng.integers(lo, hi + 1, size=(B, T)).astype(np.int32)
    for g0 in range(0, B, group):
        nb = min(group, B - g0)
        assert nb * T >= len(edges)
        cells = rng.choice(nb * T, size=len(edges), replace=False)
        for cell, v in zip(cells, edges):
            nz[g0 + cell // T, cell % T] = v
    return nz


def edges_in_every_window(nz, edges, width=WAVE):
    """True when every run of `width` consecutive instances, and the last wave's partial
    one, holds every value of `edges` at some step."""
    B = nz.shape[0]
    starts = list(range(0, max(B - width, 0) + 1)) + [(B - 1) // width * width]
    return all(set(edges) <= set(nz[s:s + width].ravel().tolist()) for s in starts)


def gnss_inputs(B, T=12, pmax=32, seed=2024, nz=None, corr=None):
    """Inputs of the gnss_pos_and_bias / multi_pseudorange pair for run_batch, batch
    outermost.  R is per instance and per step, (B, T, pmax, pmax): diagonal with entries
    r_pr U(0.5, 1.5), or with corr = (a, c) the correlated r_pr s_b (a I + c 1 1^T) with a
    per-instance scale s_b in U(0.5, 1.5)."""
    fx = gnss_fixture()
    rng = np.random.default_rng(seed)
    sat1 = satellites(fx, rng, T, pmax)
    sat = np.repeat(sat1[None], B, 0)
    xf = fx["mu"][-1]
    Z = np.linalg.norm(sat - xf[:3], axis=-1) + xf[3] + 3.0 * rng.normal(size=(B, T, pmax))
    U = 0.1 * rng.normal(size=(B, T, 3))
    mu0 = np.tile(fx["mu0"], (B, 1))
    mu0[1:] += rng.normal(size=(B - 1, 5)) * np.array([3, 3, 3, 30, 0.1])
    S0 = np.tile(fx["S0"], (B, 1, 1))
    r = float(fx["r_pr"])
    R = np.zeros((B, T, pmax, pmax))
    if corr is None:
        i = np.arange(pmax)
        R[:, :, i, i] = r * rng.uniform(0.5, 1.5, size=(B, T, pmax))
    else:
        s = rng.uniform(0.5, 1.5, size=B)
        R[:] = (r * s)[:, None, None, None] * (corr[0] * np.eye(pmax) + corr[1] * np.ones((pmax, pmax)))
    if nz is None:
        nz = ragged_counts(rng, B, T, pmax, EDGE_COUNTS)
    return {"fx": fx, "mu0": mu0, "S0": S0, "U": U, "Z": Z, "nz": np.asarray(nz, dtype=np.int32), "sat": sat,
            "R": R, "Q": fx["Q"], "dparams": {"dt": 1.0}}


def bias_inputs(B=70, T=12, seed=77):
    """multi_pseudorange_and_bias: pmax = 13, nz = nsat + 1 with nsat in 0..12 (nsat = 0: a
    step with the bias row alone), and some steps with no measurement at all.  The bias
    row's z sits in slot nsat; its satellite slot is unused."""
    rng = np.random.default_rng(seed)
    nsat = ragged_counts(rng, B, T, 12, edges=(0, 1, 7, 8, 9, 12))
    inp = gnss_inputs(B, T, 13, seed=seed + 1, nz=nsat + 1)
    xf = inp["fx"]["mu"][-1]
    b, k = np.meshgrid(np.arange(B), np.arange(T), indexing="ij")
    inp["Z"][b, k, nsat] = xf[3] + 3.0 * rng.normal(size=(B, T))
    none = rng.uniform(size=(B, T)) < 0.15
    cells = rng.choice(B * T, size=B // 32 + 1, replace=False)
    none[cells // T, cells % T] = True
    inp["nz"][none] = 0
    return inp


def autocar_inputs(B=70, T=61, seed=7):
    """discrete_vehicle_dynamics / vehicle_sensors_model on the first T steps of
    ekf_autocar.npz: priors and measurements perturbed as tests/test_ekf_autocar.py does,
    and at every step with measurements each instance keeps a random prefix of 0..nz rows.
    R is one (T, pmax, pmax) array shared by the batch (r_bstride = 0)."""
    fx = autocar_fixture()
    rng = np.random.default_rng(seed)
    mu0 = np.repeat(fx["mu0"][None], B, 0)
    mu0[1:, :2] += rng.normal(size=(B - 1, 2))
    mu0[1:, 6] += 5.0 * rng.normal(size=B - 1)
    S0 = np.repeat(fx["S0"][None], B, 0)
    Z = np.repeat(fx["Z"][None, :T], B, 0)
    nzr = fx["nz"][:T]
    pmax = Z.shape[2]
    for k in range(T):
        Z[1:, k, :nzr[k]] += 0.5 * rng.normal(size=(B - 1, nzr[k]))
    nz = rng.integers(0, nzr[None, :] + 1, size=(B, T)).astype(np.int32)
    meas = np.flatnonzero(nzr)
    nz[0, meas[0]], nz[1, meas[0]] = 0, nzr[meas[0]]     # both ends of the range occur
    sat = np.repeat(fx["sat_pos"][None, :T], B, 0)
    R = np.repeat(np.diag(float(fx["r_pr"]) * np.ones(pmax))[None], T, 0)
    U = np.repeat(fx["U"][None, :T], B, 0)
    return {"fx": fx, "mu0": mu0, "S0": S0, "U": U, "Z": Z, "nz": nz, "sat": sat, "R": R, "Q": fx["Q"],
            "dparams": fx["dparams"], "nz_fixture": nzr}


def device_args(inp, inputs="batch_outer"):
    """(U, Z, nz, sat_pos) in the layout run_batch's `inputs` names."""
    a = (inp["U"], inp["Z"], inp["nz"], inp["sat"])
    if inputs == "batch_inner":
        a = tuple(np.ascontiguousarray(np.moveaxis(x, 0, -1)) for x in a)
    return a


def oracle_run(inp, dyn=oekf.gnss_pos_and_bias, meas=oekf.multi_pseudorange, extra=0, predict_only=(),
               instances=None):
    """oracle.ekf.EKF for every instance (or `instances`) at every step, fed the leading
    nz x nz block of that instance's and step's R; the (b, k) pairs of `predict_only` skip the
    correction.  Returns (mu (B,T,n), S (B,T,n,n), spd (B,T)): spd is False where the
    innovation covariance P = H S- H^T + R of a correction has no Cholesky factor."""
    B, T = inp["nz"].shape
    n = inp["mu0"].shape[1]
    mus, Ss, spd = np.zeros((B, T, n)), np.zeros((B, T, n, n)), np.ones((B, T), dtype=bool)
    Rall = inp["R"]
    for b in (range(B) if instances is None else instances):
        f = oekf.EKF(dyn, meas, inp["mu0"][b], inp["S0"][b])
        for k in range(T):
            ns = int(inp["nz"][b, k])
            if ns == 0 or (b, k) in predict_only:
                f.update(inp["U"][b, k], None, inp["Q"], None, inp["dparams"])
            else:
                R = (Rall[b, k] if Rall.ndim == 4 else Rall[k])[:ns, :ns]
                par = {"sat_pos": inp["sat"][b, k, :ns - extra]}
                xp, G = dyn(f.mu, inp["U"][b, k], params=inp["dparams"], jac=True)
                _, H = meas(xp, params=par, jac=True)
                P = H @ ((G @ (f.S @ G.T) + inp["Q"]) @ H.T) + R
                try:
                    np.linalg.cholesky(P)
                except np.linalg.LinAlgError:
                    spd[b, k] = False
                f.update(inp["U"][b, k], inp["Z"][b, k, :ns], inp["Q"], R, inp["dparams"], None, par)
            mus[b, k], Ss[b, k] = f.mu, f.S
    return mus, Ss, spd
