"""Cost of innovation gating and the likelihood outputs (mhe_ekf_run_args, k_ekf_lane<.., true>)
beside the same build's plain filter (mhe_ekf_run).

    python tools/bench_ekf_gate.py [gnss|autocar] [B] [reps] [--plain-only] [--out FILE]

Workloads: the gnss_stationary recipe (n = 5, 12 slots, 51 steps; default B = 262144) and the
autonomous-car recipe (n = 9, 300 steps, 8-11 rows at every 10th step; default B = 131072),
B filters, inputs batch-innermost and resident on the device, method "lane", history kept.
The gnss inputs are consistent with the filter's model, as a gate presumes: the prior is
mu0 = x_f + N(0, S0) with S0 = diag(3, 3, 3, 30, 0.1)^2 and x_f the fixture's last state, and
the pseudoranges are simulated at x_f with the fixture's satellites and N(0, r_pr) noise per
filter (with the log's own pseudoranges and prior, far outside R and S0, a gate rejects nearly
every row).  Four launch kinds:

    plain       no keyword: mhe_ekf_run's instances
    stats       gate = inf, innovations=True: statistics only (no screening pass)
    gate_clean  gate = 10.83, innovations=True, the data as they are
    gate_8pct   the same with a seeded 8 % of the valid rows shifted by +400 m

Timing: HIP events around `reps` launches of one kind; the kinds alternate within a window,
three windows, the median per kind is reported.  One JSON line per run is printed and
appended to --out (default profiles/ekf_gate.jsonl).  Metric: filter-steps/s = B * T / time.

--plain-only measures the plain launch alone and does not bind mhe_ekf_run_args, so that a
library built from an earlier revision (tools/build_from.sh, loaded through MHE_LIB) can be
measured by the same script, builds alternating between processes.
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
import utils.gnss as gnss  # noqa: E402
import utils.vehicle as veh  # noqa: E402

argv = [a for a in sys.argv[1:] if not a.startswith("--")]
PLAIN_ONLY = "--plain-only" in sys.argv
OUT = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else os.path.join(ROOT, "profiles", "ekf_gate.jsonl")
if "--out" in sys.argv:
    argv.remove(OUT)
WHICH = argv[0] if argv else "gnss"
B = int(argv[1]) if len(argv) > 1 else {"gnss": 262144, "autocar": 131072}[WHICH]
REPS = int(argv[2]) if len(argv) > 2 else 5
GATE, SHIFT, FRACTION = 10.83, 400.0, 0.08
dev = torch.device("cuda", 0)
G = os.path.join(ROOT, "tests", "golden")
if PLAIN_ONLY:
    _lib.SIGNATURES.pop("mhe_ekf_run_args")


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
    dyn, meas, dparams = gnss.gnss_pos_and_bias, gnss.multi_pseudorange, {"dt": 1.0}
elif WHICH == "autocar":
    fx = dict(np.load(os.path.join(G, "ekf_autocar.npz")))
    car = dict(zip(("C_AF", "C_AR", "M", "D_F", "D_R", "I_Z"), fx["car"]))
    dparams = {"dt": float(fx["dt"]), "car_params": car}
    T, pmax, n, m = fx["U"].shape[0], fx["Z"].shape[1], 9, 2
    mu0 = torch.as_tensor(fx["mu0"], device=dev).expand(B, n).contiguous()
    mu0[1:, :2] += torch.randn((B - 1, 2), dtype=torch.float64, device=dev, generator=gen)
    S0 = torch.as_tensor(fx["S0"], device=dev).expand(B, n, n).contiguous()
    U, Z, nz, sat = rep(fx["U"]), rep(fx["Z"]), rep(fx["nz"], torch.int32), rep(fx["sat_pos"])
    dyn, meas = veh.discrete_vehicle_dynamics, veh.vehicle_sensors_model
else:
    raise SystemExit(f"unknown workload {WHICH!r}")
R = torch.as_tensor(np.stack([np.diag(float(fx["r_pr"]) * np.ones(pmax)) for _ in range(T)]), device=dev)
Q = torch.as_tensor(fx["Q"], device=dev)
valid = torch.arange(pmax, device=dev)[None, :, None] < nz[:, None, :]
planted = valid & (torch.rand(Z.shape, dtype=torch.float64, device=dev, generator=gen) < FRACTION)
Z8 = Z + SHIFT * planted


def run(z=Z, **kw):
    return ekf.run_batch(dyn, meas, mu0, S0, U, z, nz, Q, R, dparams["dt"], sat, method="lane", inputs="batch_inner",
                         dyn_params=dparams, **kw)


KINDS = {"plain": lambda: run(),
         "stats": lambda: run(gate=np.inf, innovations=True),
         "gate_clean": lambda: run(gate=GATE, innovations=True),
         "gate_8pct": lambda: run(Z8, gate=GATE, innovations=True)}
if PLAIN_ONLY:
    KINDS = {"plain": KINDS["plain"]}

facts = {}
for name, fn in KINDS.items():      # warm-up, and what each kind did
    out = fn()
    torch.cuda.synchronize()
    facts[name] = {"status_nonzero": int((out[4] != 0).sum().item())}
    if len(out) > 5:
        rows = int(nz.sum().item())
        gone = int(sum(((out[7] >> i) & 1).sum().item() for i in range(pmax)))
        facts[name].update(rows=rows, rows_screened_out=gone, nis_mean_per_kept_row=float(out[5].sum().item()) / max(rows - gone, 1))
        if name == "gate_8pct":
            word = sum(planted[:, i, :].to(torch.int32) << i for i in range(pmax)).permute(1, 0)
            facts[name].update(planted=int(planted.sum().item()), planted_missed=int((word & ~out[7] != 0).sum().item()))
    del out

windows = {name: [] for name in KINDS}
for _ in range(3):
    for name, fn in KINDS.items():  # the kinds alternate within a window
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(REPS):
            fn()
        e1.record()
        torch.cuda.synchronize()
        windows[name].append(e0.elapsed_time(e1) / REPS)
med = {name: sorted(w)[1] for name, w in windows.items()}
rec = {"metric": "EKF filter-steps/s by launch kind", "workload": WHICH, "n": n, "B": B, "T": T, "pmax": pmax,
       "method": "lane", "gate": GATE, "reps": REPS, "lib": os.path.basename(_lib.LIB_PATH),
       "lib_sha256_16": _lib.lib_digest(), "unit": "filter-steps/s",
       "kinds": {name: dict(facts[name], ms_per_launch=med[name], windows_ms=windows[name],
                            value=B * T / (med[name] * 1e-3), over_plain=med[name] / med["plain"])
                 for name in KINDS}}
line = json.dumps(rec)
print(line)
os.makedirs(os.path.dirname(os.path.abspath(OUT)), exist_ok=True)
with open(OUT, "a") as f:
    f.write(line + "\n")
