"""Innovation-gated EKF in NumPy -- TEST INFRASTRUCTURE ONLY.

The reference of tests/test_ekf_gate_host.py and tests/test_gpu_ekf_gate.py.  Per filter and
step, with (mu-, S-) the prediction of oracle/ekf.py's dynamics and (h, H) the measurement
model at mu- over the step's nz rows:

    d2_i = (z_i - h_i)^2 / (H_i S- H_i^T + R_ii);   row i is screened out iff d2_i > gate

(a NaN or a non-positive denominator keeps the row).  The correction is oracle.ekf.EKF.update
fed only the kept rows -- z[keep], R[keep][:, keep], sat[keep]; a kept bias row (the last row
of multi_pseudorange_and_bias) keeps that model, a dropped one turns the update into
multi_pseudorange; no kept row: predict only.  Over the kept rows a,

    nis = e_a^T P_a^-1 e_a (np.linalg.solve),  loglik = -(nis + log det P_a + |a| log 2 pi) / 2 (slogdet)

and both are 0 when no row is applied.  `eta` is eta ||P_a^-1 e_a||_1 with
eta = 4 spacing(max |z|) over the step's rows: the first-order effect on nis of rounding in
z - h, both terms ~2e7 m.

Also here: the seeded inputs of the two test files (tests/ekf_ragged.py's builders with a
prior that is consistent with its covariance and 8 % of the valid rows shifted by +400 m) and
their references, computed once per process.
"""
import functools

import numpy as np

import ekf_ragged as er
from oracle import ekf as oekf

GATES = (10.83, 0.5)       # chi-square(1) 0.999 quantile; a threshold inside the clean rows' bulk
MARGIN = 1e-6              # every row: |d2 / gate - 1| >= MARGIN, so the reject mask is compared exactly
SHIFT, FRACTION, PLANT_SEED, PRIOR_SEED = 400.0, 0.08, 11, 5
PRIOR_SIGMA = np.array([3.0, 3.0, 3.0, 30.0, 0.1])

GNSS = dict(odyn=oekf.gnss_pos_and_bias, omeas=oekf.multi_pseudorange, extra=0)
BIAS = dict(GNSS, omeas=oekf.multi_pseudorange_and_bias, extra=1)
CAR = dict(odyn=oekf.discrete_vehicle_dynamics, omeas=oekf.vehicle_sensors_model, extra=0)


def screen(dyn, meas, extra, mu, S, u, z, R, sat, Q, dparams, gate):
    """(rejected (nz,) bool, d2 (nz,)) of one step's rows at the prediction from (mu, S)."""
    ns = z.shape[0]
    xp, G = dyn(mu, u, params=dparams, jac=True)
    SP = G @ (S @ G.T) + Q
    h, H = meas(xp, params={"sat_pos": sat[:ns - extra]}, jac=True)
    den = np.einsum("ij,jk,ik->i", H, SP, H) + np.diag(R)
    with np.errstate(divide="ignore", invalid="ignore"):
        d2 = (z - h) ** 2 / den
        return (den > 0) & (d2 > gate), d2


def step(f, dyn, meas, extra, u, z, R, sat, Q, dparams, gate):
    """One gated update of the oracle.ekf.EKF object f (z: the step's nz rows, R its nz x nz
    block, sat its nz - extra satellites).  Returns (rejected, d2, nis, loglik, eta)."""
    ns = z.shape[0]
    if ns == 0:
        f.update(u, None, Q, None, dparams)
        return np.zeros(0, dtype=bool), np.zeros(0), 0.0, 0.0, 0.0
    rej, d2 = screen(dyn, meas, extra, f.mu, f.S, u, z, R, sat, Q, dparams, gate)
    keep = ~rej
    if not keep.any():
        f.update(u, None, Q, None, dparams)
        return rej, d2, 0.0, 0.0, 0.0
    model = meas
    ksat = keep[:ns - extra]
    if extra and not keep[-1]:
        model = oekf.multi_pseudorange       # the bias row is dropped: the update has satellite rows only
    par = {"sat_pos": sat[:ns - extra][ksat]}
    za, Ra = z[keep], R[keep][:, keep]
    xp, G = dyn(f.mu, u, params=dparams, jac=True)
    SP = G @ (f.S @ G.T) + Q
    h, H = model(xp, params=par, jac=True)
    P = H @ (SP @ H.T) + Ra
    e = za - h
    x = np.linalg.solve(P, e)
    nis = float(e @ x)
    sign, logdet = np.linalg.slogdet(P)
    loglik = -0.5 * (nis + logdet + keep.sum() * np.log(2.0 * np.pi))
    eta = 4.0 * np.spacing(np.abs(z).max()) * float(np.abs(x).sum())
    f.update(u, za, Q, Ra, dparams, model, par)
    return rej, d2, nis, loglik, eta


def run(inp, kind, gate, instances=None):
    """Every filter (or `instances`) of a tests/ekf_ragged.py input set at every step.  Returns a
    dict: mu (B,T,n), S (B,T,n,n), nis, loglik, eta (B,T), rej (B,T) int32 bit masks, nrej and
    nkept (B,T) counts, margin = min over all rows of |d2 / gate - 1| (inf for gate = inf)."""
    B, T = inp["nz"].shape
    n = inp["mu0"].shape[1]
    out = {"mu": np.zeros((B, T, n)), "S": np.zeros((B, T, n, n)), "nis": np.zeros((B, T)),
           "loglik": np.zeros((B, T)), "eta": np.zeros((B, T)), "rej": np.zeros((B, T), dtype=np.uint32),
           "nrej": np.zeros((B, T), dtype=int), "nkept": np.zeros((B, T), dtype=int)}
    margin = np.inf
    Rall = inp["R"]
    dyn, meas, extra = kind["odyn"], kind["omeas"], kind["extra"]
    for b in (range(B) if instances is None else instances):
        f = oekf.EKF(dyn, meas, inp["mu0"][b], inp["S0"][b])
        for k in range(T):
            ns = int(inp["nz"][b, k])
            R = (Rall[b, k] if Rall.ndim == 4 else Rall[k])[:ns, :ns]
            rej, d2, nis, ll, eta = step(f, dyn, meas, extra, inp["U"][b, k], inp["Z"][b, k, :ns], R,
                                         inp["sat"][b, k], inp["Q"], inp["dparams"], gate)
            out["mu"][b, k], out["S"][b, k] = f.mu, f.S
            out["nis"][b, k], out["loglik"][b, k], out["eta"][b, k] = nis, ll, eta
            out["rej"][b, k] = sum(1 << i for i in np.flatnonzero(rej))
            out["nrej"][b, k], out["nkept"][b, k] = rej.sum(), ns - rej.sum()
            if ns and np.isfinite(gate):
                margin = min(margin, float(np.abs(d2 / gate - 1.0).min()))
    out["rej"] = out["rej"].view(np.int32)
    out["margin"] = margin
    return out


# ---------------------------------------------------------------- the tests' inputs

def consistent_prior(inp, seed=PRIOR_SEED):
    """A gnss input set with a prior that is consistent with its covariance: mu0 = x_f +
    N(0, diag(PRIOR_SIGMA)^2) with x_f the fixture's last state (the point the measurements
    were simulated at) and its drift set to 0, S0 that covariance, U = 0.  (The fixture's own
    prior is far outside its S0, and a gate then rightly rejects everything.)"""
    B = inp["mu0"].shape[0]
    xf = inp["fx"]["mu"][-1].copy()
    xf[4] = 0.0
    rng = np.random.default_rng(seed)
    out = dict(inp)
    out["mu0"] = xf + rng.normal(size=(B, 5)) * PRIOR_SIGMA
    out["S0"] = np.tile(np.diag(PRIOR_SIGMA ** 2), (B, 1, 1))
    out["U"] = np.zeros_like(inp["U"])
    return out


def plant(inp, seed=PLANT_SEED):
    """Shift a seeded FRACTION of the valid rows by +SHIFT m; out["planted"] (B,T,pmax) bool."""
    rng = np.random.default_rng(seed)
    Z = inp["Z"].copy()
    valid = np.arange(Z.shape[2])[None, None, :] < inp["nz"][:, :, None]
    planted = valid & (rng.uniform(size=Z.shape) < FRACTION)
    Z[planted] += SHIFT
    return dict(inp, Z=Z, planted=planted)


def planted_bits(inp):
    """(B,T) int32: the planted rows as rej-style bit masks."""
    w = (inp["planted"].astype(np.uint64) << np.arange(inp["planted"].shape[2], dtype=np.uint64)).sum(-1)
    return w.astype(np.uint32).view(np.int32)


@functools.lru_cache(maxsize=None)
def inputs(name):
    if name == "gnss301":
        return plant(consistent_prior(er.gnss_inputs(301))), GNSS
    if name == "gnss301c":
        return plant(consistent_prior(er.gnss_inputs(301, corr=(1.0, 0.3)))), GNSS
    if name == "bias":
        return plant(consistent_prior(er.bias_inputs())), BIAS
    if name == "car":
        return plant(er.autocar_inputs()), CAR
    raise KeyError(name)


CASES = ("gnss301", "gnss301c", "bias", "car")


@functools.lru_cache(maxsize=None)
def reference(name, gate):
    """run() on inputs(name), once per process (both test files share it; treat as read-only)."""
    inp, kind = inputs(name)
    return run(inp, kind, gate)
