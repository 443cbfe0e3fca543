"""Unscented RTS smoother throughput (mhe_ukf_smooth, k_ukf_rts) beside the same build's forward
filter (mhe_ukf_run, k_ukf) on the same shape.

    python tools/bench_ukf_smooth.py [gnss|autocar] [B] [reps] [--out FILE]

Workloads: those of tools/bench_ukf.py -- the gnss_stationary recipe (n = 5, 12 slots, 51 steps)
and the autonomous-car recipe (n = 9, 300 steps, 8-11 rows at every 10th step), B filters
(default 65536), inputs batch-innermost and resident on the device.  The forward filter runs once
to produce the history; the smoother then runs on its batch-innermost views (no copy), with the
prior, writing to its own output buffers.

Timing: HIP events around one launch; smoother and forward filter alternate, `reps` launches each
after a warm-up of both, the median per kernel is reported.  One JSON line per run is printed and
appended to --out (default profiles/ukf_smooth.jsonl).  Metric: filter-steps/s = B * T / time.

Algorithmic bytes of the smoother per filter-step: mu (n), the upper triangle of S
(n (n + 1) / 2) and u (m) doubles read, mu_s (n) and S_s (n^2) doubles written; the share of
HBM bandwidth is those bytes over the time against 8 TB/s.
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
OUT = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else \
    os.path.join(ROOT, "profiles", "ukf_smooth.jsonl")
if "--out" in sys.argv:
    argv.remove(OUT)
WHICH = argv[0] if argv else "gnss"
B = int(argv[1]) if len(argv) > 1 else 65536
REPS = int(argv[2]) if len(argv) > 2 else 5
HBM = 8.0e12
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
    U = 0.1 * torch.randn((T, m, B), dtype=torch.float64, device=dev, generator=gen)
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


def forward():
    return ukf.run_batch(dyn, meas, mu0, S0, U, Z, nz, Q, R, dparams["dt"], sat, inputs="batch_inner",
                         dyn_params=dparams)


mh, Sh, _, _, st = forward()
torch.cuda.synchronize()
assert int((st != 0).sum().item()) == 0, "k_ukf: a filter ended with a non-zero status"
assert ekf._hist_storage(mh, (n,))[0].data_ptr() == mh.data_ptr()     # consumed without a copy


def backward():
    return ukf.smooth_batch(dyn, mh, Sh, U, Q, dparams["dt"], mu0=mu0, S0=S0, dyn_params=dparams,
                            inputs="batch_inner")


out = backward()
torch.cuda.synchronize()
assert int((out[2] != 0).sum().item()) == 0, "k_ukf_rts: a filter ended with a non-zero status"
shrink = float((torch.diagonal(Sh[:, 0], dim1=-2, dim2=-1).sum(-1)
                / torch.diagonal(out[1][:, 0], dim1=-2, dim2=-1).sum(-1)).median().item())
del out

KINDS = {"k_ukf_rts": backward, "k_ukf": forward}
times = {name: [] for name in KINDS}
for _ in range(REPS):
    for name, fn in KINDS.items():  # the two kernels alternate
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        o = fn()
        e1.record()
        torch.cuda.synchronize()
        del o
        times[name].append(e0.elapsed_time(e1))
med = {name: float(np.median(t)) for name, t in times.items()}
by = 8.0 * (n + n * (n + 1) // 2 + m + n + n * n)
rate = B * T / (med["k_ukf_rts"] * 1e-3)
rec = {"metric": "filter-steps/s, unscented RTS smoother beside the unscented filter (one wavefront per filter)",
       "workload": WHICH, "n": n, "B": B, "T": T, "pmax": pmax, "reps": REPS, "lib_sha256_16": _lib.lib_digest(),
       "unit": "filter-steps/s", "bytes_per_step": by, "achieved_GBs": by * rate / 1e9, "hbm_frac": by * rate / HBM,
       "tr_S0_filtered_over_smoothed_median": shrink,
       "kinds": {name: dict(ms_per_launch=med[name], launches_ms=times[name], value=B * T / (med[name] * 1e-3))
                 for name in KINDS},
       "rts_over_ukf_time": med["k_ukf_rts"] / med["k_ukf"]}
line = json.dumps(rec)
print(line)
os.makedirs(os.path.dirname(os.path.abspath(OUT)), exist_ok=True)
with open(OUT, "a") as f:
    f.write(line + "\n")
