"""Throughput of the batched unscented filter (mhe_ukf_run, k_ukf) beside the same build's
extended filter of the same shape (utils.ekf.run_batch(method="wave"): k_ekf, one wavefront per
filter, augmented Cholesky sweep), and the cost of its statistics and of innovation gating
(mhe_ukf_run_gated, k_ukf<.., GATE>).

    python tools/bench_ukf.py [gnss|autocar] [B] [reps] [--plain-only] [--out FILE]

Workloads: the gnss_stationary recipe (n = 5, 12 slots, 51 steps) and the autonomous-car recipe
(n = 9, 300 steps, 8-11 rows at every 10th step), B filters (default 65536), identical inputs
for both filters, batch-innermost and resident on the device, histories kept.  The gnss inputs
are consistent with the filter's model as in tools/bench_ekf_gate.py: prior mu0 = x_f + N(0, S0)
with S0 = diag(3, 3, 3, 30, 0.1)^2, pseudoranges simulated at x_f with the fixture's satellites
and N(0, r_pr) noise per filter.

Launch kinds:

    k_ukf            no keyword: mhe_ukf_run, the plain instances
    k_ukf_stats      innovations=True: the plain instances with nis / loglik
    k_ukf_gate       gate = 10.83, innovations=True, the data as they are: the gated instances
    k_ukf_gate_8pct  the same with a seeded 8 % of the valid rows shifted by +400 m
    k_ekf            the extended filter, method "wave"

Timing: HIP events around one launch; the kinds alternate, `reps` launches each after a
warm-up of all, the median per kind is reported.  One JSON line per run is printed and
appended to --out (default profiles/ukf.jsonl).  Metric: filter-steps/s = B * T / time.

--plain-only measures k_ukf alone and does not bind mhe_ukf_run_gated, so that a library built
from an earlier revision (tools/build_from.sh, loaded through MHE_LIB) can be measured by the
same script, builds alternating between processes.
"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "nlp-filter_amd"))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402

from mhe import _lib  # noqa: E402
import utils.ekf as ekf  # noqa: E402
import utils.ukf as ukf  # noqa: E402

argv = [a for a in sys.argv[1:] if not a.startswith("--")]
PLAIN_ONLY = "--plain-only" in sys.argv
OUT = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else os.path.join(ROOT, "profiles", "ukf.jsonl")
if "--out" in sys.argv:
    argv.remove(OUT)
WHICH = argv[0] if argv else "gnss"
B = int(argv[1]) if len(argv) > 1 else 65536
REPS = int(argv[2]) if len(argv) > 2 else 5
GATE, SHIFT, FRACTION = 10.83, 400.0, 0.08
if PLAIN_ONLY:
    _lib.SIGNATURES.pop("mhe_ukf_run_gated")
dev = torch.device("cuda", 0)
G = os.path.join(ROOT, "tests", "golden")


def rep(a, dtype=torch.float64):
    """(..., B): one array replicated over the batch, batch innermost, made on the device."""
    t = torch.as_tensor(np.asarray(a), dtype=dtype, device=dev)
    return t.unsqueeze(-1).expand(*t.shape, B).contiguous()


gen = torch.Generator(device=dev)
gen.manual_seed(7)
if WHICH == "gnss":
    fx = dict(np.load(os.path.join(G, "ekf_gnss_stationary.npz")))
    T, pmax, n, m = fx["pr"].shape[0], 12, 5, 3
    sigma = torch.tensor([3.0, 3.0, 3.0, 30.0, 0.1], dtype=torch.float64, device=dev)
    xf = fx["mu"][-1].copy()
    xf[4] = 0.0
    mu0 = torch.as_tensor(xf, device=dev) + torch.randn((B, n), dtype=torch.float64, device=dev, generator=gen) * sigma
    S0 = torch.diag(sigma ** 2).expand(B, n, n).contiguous()
    U = torch.zeros((T, m, B), dtype=torch.float64, device=dev)
    nz, sat = rep(fx["nsat"], torch.int32), rep(fx["sat_pos"])
    Z = rep(np.linalg.norm(fx["sat_pos"] - xf[:3], axis=-1) + xf[3])
    Z += float(fx["r_pr"]) ** 0.5 * torch.randn(Z.shape, dtype=torch.float64, device=dev, generator=gen)
    dyn, meas, dparams = "gnss_pos_and_bias", "multi_pseudorange", {"dt": 1.0}
elif WHICH == "autocar":
    fx = dict(np.load(os.path.join(G, "ekf_autocar.npz")))
    car = dict(zip(("C_AF", "C_AR", "M", "D_F", "D_R", "I_Z"), fx["car"]))
    dparams = {"dt": float(fx["dt"]), "car_params": car}
    T, pmax, n, m = fx["U"].shape[0], fx["Z"].shape[1], 9, 2
    mu0 = torch.as_tensor(fx["mu0"], device=dev).expand(B, n).contiguous()
    mu0[1:, :2] += torch.randn((B - 1, 2), dtype=torch.float64, device=dev, generator=gen)
    S0 = torch.as_tensor(fx["S0"], device=dev).expand(B, n, n).contiguous()
    U, Z, nz, sat = rep(fx["U"]), rep(fx["Z"]), rep(fx["nz"], torch.int32), rep(fx["sat_pos"])
    dyn, meas = "discrete_vehicle_dynamics", "vehicle_sensors_model"
else:
    raise SystemExit(f"unknown workload {WHICH!r}")
R = torch.as_tensor(np.stack([np.diag(float(fx["r_pr"]) * np.ones(pmax)) for _ in range(T)]), device=dev)
Q = torch.as_tensor(fx["Q"], device=dev)

# the same measurements with outliers: +SHIFT m on a seeded FRACTION of the valid rows (Z is (T, pmax, B))
valid = torch.arange(pmax, device=dev)[None, :, None] < nz[:, None, :]
planted = valid & (torch.rand(Z.shape, dtype=torch.float64, device=dev, generator=gen) < FRACTION)
Z8 = Z + SHIFT * planted


def run_ukf(z=Z, **kw):
    return ukf.run_batch(dyn, meas, mu0, S0, U, z, nz, Q, R, dparams["dt"], sat, inputs="batch_inner",
                         dyn_params=dparams, **kw)


KINDS = {"k_ukf": run_ukf}
if not PLAIN_ONLY:
    KINDS.update({"k_ukf_stats": lambda: run_ukf(innovations=True),
                  "k_ukf_gate": lambda: run_ukf(innovations=True, gate=GATE),
                  "k_ukf_gate_8pct": lambda: run_ukf(Z8, innovations=True, gate=GATE),
                  "k_ekf": lambda: ekf.run_batch(dyn, meas, mu0, S0, U, Z, nz, Q, R, dparams["dt"], sat,
                                                 method="wave", inputs="batch_inner", dyn_params=dparams)})

final, screened = {}, {}
for name, fn in KINDS.items():      # warm-up, and what each kind did
    out = fn()
    torch.cuda.synchronize()
    assert int((out[4] != 0).sum().item()) == 0, f"{name}: a filter ended with a non-zero status"
    final[name] = out[2].clone()
    if len(out) == 8:               # rows screened out / valid rows, and of the planted ones
        bits = (out[7].permute(1, 0)[:, None, :] >> torch.arange(pmax, device=dev)[None, :, None]) & 1
        screened[name] = {"rows": float(bits.sum().item()) / float(valid.sum().item())}
        if name == "k_ukf_gate_8pct":
            screened[name]["of_planted"] = float((bits.bool() & planted).sum().item()) / float(planted.sum().item())
    del out
dmu = None if PLAIN_ONLY else float((final["k_ukf"] - final["k_ekf"]).abs().max().item())

times = {name: [] for name in KINDS}
for _ in range(REPS):
    for name, fn in KINDS.items():  # the kinds alternate
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        times[name].append(e0.elapsed_time(e1))
med = {name: float(np.median(t)) for name, t in times.items()}
rec = {"metric": "filter-steps/s, unscented beside extended (one wavefront per filter)", "workload": WHICH, "n": n,
       "B": B, "T": T, "pmax": pmax, "reps": REPS, "lib": os.path.basename(_lib.LIB_PATH),
       "lib_sha256_16": _lib.lib_digest(), "unit": "filter-steps/s", "gate": GATE,
       "kinds": {name: dict(ms_per_launch=med[name], launches_ms=times[name], value=B * T / (med[name] * 1e-3))
                 for name in KINDS}}
if not PLAIN_ONLY:
    rec.update(max_abs_dmu_final_ukf_vs_ekf=dmu, ukf_over_ekf_time=med["k_ukf"] / med["k_ekf"],
               stats_over_plain_time=med["k_ukf_stats"] / med["k_ukf"],
               gate_over_plain_time=med["k_ukf_gate"] / med["k_ukf"],
               gate_8pct_over_plain_time=med["k_ukf_gate_8pct"] / med["k_ukf"], screened=screened)
line = json.dumps(rec)
print(line)
os.makedirs(os.path.dirname(os.path.abspath(OUT)), exist_ok=True)
with open(OUT, "a") as f:
    f.write(line + "\n")
