"""RTS smoother throughput (mhe_ekf_smooth, k_ekf_rts) beside the same build's forward filter.

    python tools/bench_ekf_smooth.py [gnss|autocar] [B] [reps]

Workloads: the shapes of tools/bench_ekf.py (gnss_stationary recipe, n = 5, 51 epochs) and
tools/bench_ekf_autocar.py (autonomous-car plug-ins, n = 9, 300 steps), B filters with
perturbed priors, inputs batch-innermost and resident on the device.  The forward filter
(k_ekf_lane) runs once to produce the history; the smoother then runs on that history, writing
to its own output buffers.  Timing: HIP events around `reps` launches after a warm-up launch,
three windows, median reported; the forward kernel is timed the same way on the same shape.
Metric: filter-steps/s = B * T / time per launch.

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

import utils.ekf as ekf  # noqa: E402
import utils.gnss as gnss  # noqa: E402
import utils.vehicle as veh  # noqa: E402

WHICH = sys.argv[1] if len(sys.argv) > 1 else "gnss"
B = int(sys.argv[2]) if len(sys.argv) > 2 else 65536
REPS = int(sys.argv[3]) if len(sys.argv) > 3 else 10
HBM = 8.0e12
dev = torch.device("cuda", 0)
G = os.path.join(ROOT, "tests", "golden")

if WHICH == "gnss":
    fx = dict(np.load(os.path.join(G, "ekf_gnss_stationary.npz")))
    T, pmax, n, m = fx["pr"].shape[0], 12, 5, 3
    rng = np.random.default_rng(7)
    mu0 = np.tile(fx["mu0"], (B, 1))
    mu0[1:] += rng.normal(size=(B - 1, 5)) * np.array([3, 3, 3, 30, 0.1])
    U = np.ascontiguousarray(np.moveaxis(rng.normal(size=(B, T, 3)) * 0.1, 0, -1))
    Z = np.ascontiguousarray(np.repeat(fx["pr"][..., None], B, -1))
    nz = np.ascontiguousarray(np.repeat(fx["nsat"][:, None], B, -1).astype(np.int32))
    sat = np.ascontiguousarray(np.repeat(fx["sat_pos"][..., None], B, -1))
    dyn, meas, dparams = gnss.gnss_pos_and_bias, gnss.multi_pseudorange, {"dt": 1.0}
elif WHICH == "autocar":
    fx = dict(np.load(os.path.join(G, "ekf_autocar.npz")))
    car = dict(zip(("C_AF", "C_AR", "M", "D_F", "D_R", "I_Z"), fx["car"]))
    dparams = {"dt": float(fx["dt"]), "car_params": car}
    T, pmax, n, m = fx["U"].shape[0], fx["Z"].shape[1], 9, 2
    rng = np.random.default_rng(11)
    mu0 = np.tile(fx["mu0"], (B, 1))
    mu0[1:, :2] += rng.normal(size=(B - 1, 2))
    U = np.ascontiguousarray(np.repeat(fx["U"][..., None], B, -1))
    Z = np.ascontiguousarray(np.repeat(fx["Z"][..., None], B, -1))
    nz = np.ascontiguousarray(np.repeat(fx["nz"][:, None], B, -1).astype(np.int32))
    sat = np.ascontiguousarray(np.repeat(fx["sat_pos"][..., None], B, -1))
    dyn, meas = veh.discrete_vehicle_dynamics, veh.vehicle_sensors_model
else:
    raise SystemExit(f"unknown workload {WHICH!r}")
S0 = np.tile(fx["S0"], (B, 1, 1))
R = np.stack([np.diag(float(fx["r_pr"]) * np.ones(pmax)) for _ in range(T)])
mu0, S0, U, Z, nz, sat, R, Q = (torch.as_tensor(a, device=dev) for a in (mu0, S0, U, Z, nz, sat, R, fx["Q"]))


def forward():
    return ekf.run_batch(dyn, meas, mu0, S0, U, Z, nz, Q, R, dparams["dt"], sat, method="lane", inputs="batch_inner",
                         dyn_params=dparams)


def backward(mh, Sh):
    return ekf.smooth_batch(dyn, mh, Sh, U, Q, dparams["dt"], mu0=mu0, S0=S0, dyn_params=dparams,
                            inputs="batch_inner")


def timed(fn):
    """Median over three windows of ms per launch (buffers of the warm-up call are reused)."""
    fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(3):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(REPS):
            fn()
        e1.record()
        torch.cuda.synchronize()
        ms.append(e0.elapsed_time(e1) / REPS)
    return sorted(ms)[1], ms


mh, Sh, _, _, st = forward()
torch.cuda.synchronize()
assert int(st.abs().sum().item()) == 0
out = backward(mh, Sh)
torch.cuda.synchronize()
assert int(out[2].abs().sum().item()) == 0
assert ekf._hist_storage(mh, (n,))[0].data_ptr() == mh.data_ptr()     # consumed without a copy
shrink = float((torch.diagonal(Sh[:, 0], dim1=-2, dim2=-1).sum(-1)
                / torch.diagonal(out[1][:, 0], dim1=-2, dim2=-1).sum(-1)).median().item())
del out
s_ms, s_all = timed(lambda: backward(mh, Sh))
f_ms, f_all = timed(forward)
by = 8.0 * (n + n * (n + 1) // 2 + m + n + n * n)
rate = B * T / (s_ms * 1e-3)
print(json.dumps({"metric": "RTS smoother filter-steps/s", "workload": WHICH, "n": n, "B": B, "T": T,
                  "kernel": "mhe_ekf::k_ekf_rts (one filter per lane)", "ms_per_launch": s_ms, "windows_ms": s_all,
                  "value": rate, "unit": "filter-steps/s", "bytes_per_step": by,
                  "achieved_GBs": by * rate / 1e9, "hbm_frac": by * rate / HBM,
                  "tr_S0_filtered_over_smoothed_median": shrink,
                  "forward": {"kernel": "mhe_ekf::k_ekf_lane", "ms_per_launch": f_ms, "windows_ms": f_all,
                              "value": B * T / (f_ms * 1e-3), "unit": "filter-steps/s"}}))
