"""Cost of the iterated EKF (mhe_iekf_run, k_iekf) beside the same build's wave-method EKF (k_ekf).

    python tools/bench_iekf.py [gnss|autocar] [B] [reps] [--out FILE] [--robust]

Workloads: the gnss_stationary recipe (n = 5, 12 slots, 51 steps) and the autonomous-car recipe
(n = 9, 300 steps, 8-11 rows at every 10th step), B = 65536 filters by default, inputs
batch-innermost and resident on the device, history kept.  The gnss inputs are consistent with the
filter's model (tools/bench_ekf_gate.py's: prior x_f + N(0, S0), S0 = diag(3, 3, 3, 30, 0.1)^2,
pseudoranges simulated at x_f).  The cold prior is x_f + N(0, S0c), S0c = diag(1e5, 1e5, 1e5, 1e3,
0.1)^2 (gnss); px, py of the prior moved by N(0, 2000^2) and that variance added to S0 (car).
Launch kinds:

    ekf_wave      no keyword, method="wave": k_ekf, the yardstick of iter1
    ekf_predict   the same with every nz = 0: k_ekf's predict and history stores alone, so that
                  ekf_wave - ekf_predict is k_ekf's correct phase, the yardstick of a further pass
    iter1         iterations=1
    iter3         iterations=3, iter_tol=0: two further passes at every corrected step
    cold8         iterations=8, iter_tol=TOL on the cold prior (the mean pass count is recorded)

--robust adds the pseudo-Huber rows (mhe_iekf_run_robust, huber=) and its outlier recipe, the one of
tools/bench_ekf_gate.py: a seeded 8 % of the valid rows shifted by +400 m, the consistent prior:

    robust_inf3   iterations=3, iter_tol=0, huber=inf: iter3's work plus the reweighting alone
    out_plain     iterations=16, iter_tol=TOL on the outlier inputs
    out_gate      the same with gate=10.83
    out_huber     the same with huber=DELTA (15, the measurement's units), no gate
    out_both      the same with huber=DELTA and gate=10.83

and records robust_inf3 / iter3, and for the out_* kinds the passes per corrected step and (gnss)
the position error after the last step.

Timing: HIP events around `reps` launches of one kind; the kinds alternate within a window, three
windows, the median per kind is reported.  One JSON line per run is printed and appended to --out
(default profiles/iekf.jsonl) with the two ratios: iter1 / ekf_wave, and
(iter3 - iter1) / 2 over (ekf_wave - ekf_predict).  For gnss the line also holds the cold-start
table: position error of the EKF and of the iterated filter after the first and the last step.
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

ROBUST = "--robust" in sys.argv
argv = [a for a in sys.argv[1:] if not a.startswith("--")]
OUT = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else os.path.join(ROOT, "profiles", "iekf.jsonl")
if "--out" in sys.argv:
    argv.remove(OUT)
WHICH = argv[0] if argv else "gnss"
B = int(argv[1]) if len(argv) > 1 else 65536
REPS = int(argv[2]) if len(argv) > 2 else 3
TOL = {"gnss": 1e-4, "autocar": 1e-6}[WHICH]
GATE, SHIFT, FRACTION, DELTA = 10.83, 400.0, 0.08, 15.0
dev = torch.device("cuda", 0)
G = os.path.join(ROOT, "tests", "golden")


def rep(a, dtype=torch.float64):
    """(..., B): one array replicated over the batch, batch innermost, made on the device."""
    t = torch.as_tensor(np.asarray(a), dtype=dtype, device=dev)
    return t.unsqueeze(-1).expand(*t.shape, B).contiguous()


gen = torch.Generator(device=dev)
gen.manual_seed(7)
randn = lambda *s: torch.randn(s, dtype=torch.float64, device=dev, generator=gen)   # noqa: E731
if WHICH == "gnss":
    fx = dict(np.load(os.path.join(G, "ekf_gnss_stationary.npz")))
    T, pmax, n, m = fx["pr"].shape[0], 12, 5, 3
    sigma = torch.tensor([3.0, 3.0, 3.0, 30.0, 0.1], dtype=torch.float64, device=dev)
    cold = torch.tensor([1e5, 1e5, 1e5, 1e3, 0.1], dtype=torch.float64, device=dev)
    xf = fx["mu"][-1].copy()
    xf[4] = 0.0
    mu0 = torch.as_tensor(xf, device=dev) + randn(B, n) * sigma
    S0 = torch.diag(sigma ** 2).expand(B, n, n).contiguous()
    mu0c = torch.as_tensor(xf, device=dev) + randn(B, n) * cold
    S0c = torch.diag(cold ** 2).expand(B, n, n).contiguous()
    U = torch.zeros((T, m, B), dtype=torch.float64, device=dev)
    nz, sat = rep(fx["nsat"], torch.int32), rep(fx["sat_pos"])
    Z = rep(np.linalg.norm(fx["sat_pos"] - xf[:3], axis=-1) + xf[3])
    Z += float(fx["r_pr"]) ** 0.5 * randn(*Z.shape)
    dyn, meas, dparams = gnss.gnss_pos_and_bias, gnss.multi_pseudorange, {"dt": 1.0}
elif WHICH == "autocar":
    fx = dict(np.load(os.path.join(G, "ekf_autocar.npz")))
    car = dict(zip(("C_AF", "C_AR", "M", "D_F", "D_R", "I_Z"), fx["car"]))
    dparams = {"dt": float(fx["dt"]), "car_params": car}
    T, pmax, n, m = fx["U"].shape[0], fx["Z"].shape[1], 9, 2
    mu0 = torch.as_tensor(fx["mu0"], device=dev).expand(B, n).contiguous()
    mu0[1:, :2] += randn(B - 1, 2)
    S0 = torch.as_tensor(fx["S0"], device=dev).expand(B, n, n).contiguous()
    mu0c, S0c = mu0.clone(), S0.clone()
    mu0c[:, :2] += 2000.0 * randn(B, 2)
    S0c[:, 0, 0] += 2000.0 ** 2
    S0c[:, 1, 1] += 2000.0 ** 2
    U, Z, nz, sat = rep(fx["U"]), rep(fx["Z"]), rep(fx["nz"], torch.int32), rep(fx["sat_pos"])
    dyn, meas = veh.discrete_vehicle_dynamics, veh.vehicle_sensors_model
else:
    raise SystemExit(f"unknown workload {WHICH!r}")
R = torch.as_tensor(np.stack([np.diag(float(fx["r_pr"]) * np.ones(pmax)) for _ in range(T)]), device=dev)
Q = torch.as_tensor(fx["Q"], device=dev)
nz0 = torch.zeros_like(nz)


def run(m0=mu0, s0=S0, rows=nz, **kw):
    return ekf.run_batch(dyn, meas, m0, s0, U, Z, rows, Q, R, dparams["dt"], sat, inputs="batch_inner",
                         dyn_params=dparams, **kw)


KINDS = {"ekf_wave": lambda: run(method="wave"),
         "ekf_predict": lambda: run(rows=nz0, method="wave"),
         "iter1": lambda: run(iterations=1),
         "iter3": lambda: run(iterations=3, iter_tol=0.0),
         "cold8": lambda: run(mu0c, S0c, iterations=8, iter_tol=TOL)}


def pos_err(mh):
    """Median and max position error after the first and the last step (gnss: x_f is known)."""
    p = torch.as_tensor(xf[:3], device=dev)
    e = [torch.linalg.norm(mh[:, k, :3] - p, dim=-1) for k in (0, -1)]
    return {"first_median": float(e[0].median().item()), "last_median": float(e[1].median().item()),
            "last_max": float(e[1].max().item())}


if ROBUST:
    valid = torch.arange(pmax, device=dev)[None, :, None] < nz[:, None, :]
    planted = valid & (torch.rand(Z.shape, dtype=torch.float64, device=dev, generator=gen) < FRACTION)
    Z8 = Z + SHIFT * planted

    def run8(**kw):
        return ekf.run_batch(dyn, meas, mu0, S0, U, Z8, nz, Q, R, dparams["dt"], sat, inputs="batch_inner",
                             dyn_params=dparams, iterations=16, iter_tol=TOL, **kw)

    KINDS.update({"robust_inf3": lambda: run(iterations=3, iter_tol=0.0, huber=float("inf")),
                  "out_plain": lambda: run8(),
                  "out_gate": lambda: run8(gate=GATE),
                  "out_huber": lambda: run8(huber=DELTA),
                  "out_both": lambda: run8(huber=DELTA, gate=GATE)})

facts = {}
for name, fn in KINDS.items():      # warm-up, and what each kind did
    out = fn()
    torch.cuda.synchronize()
    facts[name] = {"status_nonzero": int((out[4] != 0).sum().item())}
    if len(out) > 5:
        cnt = out[-2] if name in ("robust_inf3", "out_huber", "out_both") else out[-1]   # weights come after n_iter
        done = cnt > 0
        facts[name].update(corrected_steps=int(done.sum().item()),
                           mean_passes=float(cnt[done].double().mean().item()) if bool(done.any()) else 0.0,
                           max_passes=int(cnt.max().item()))
    if WHICH == "gnss" and (name == "cold8" or name.startswith("out_")):
        facts[name]["position_error_m"] = pos_err(out[0])
    del out
if WHICH == "gnss":
    out = run(mu0c, S0c, method="wave")
    torch.cuda.synchronize()
    facts["ekf_wave"]["cold_position_error_m"] = pos_err(out[0])
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
correct = med["ekf_wave"] - med["ekf_predict"]
further = (med["iter3"] - med["iter1"]) / 2.0
rec = {"metric": "iterated-EKF filter-steps/s by launch kind", "workload": WHICH, "n": n, "B": B, "T": T, "pmax": pmax,
       "iter_tol_cold8": TOL, "reps": REPS, "lib": os.path.basename(_lib.LIB_PATH), "lib_sha256_16": _lib.lib_digest(),
       "unit": "filter-steps/s",
       "kinds": {name: dict(facts[name], ms_per_launch=med[name], windows_ms=windows[name],
                            value=B * T / (med[name] * 1e-3), over_ekf_wave=med[name] / med["ekf_wave"])
                 for name in KINDS},
       "iter1_over_ekf_wave": med["iter1"] / med["ekf_wave"],
       "k_ekf_correct_phase_ms": correct, "further_pass_ms": further,
       "further_pass_over_k_ekf_correct_phase": further / correct if correct > 0 else None}
if ROBUST:
    rec.update(robust_inf3_over_iter3=med["robust_inf3"] / med["iter3"], outliers={"shift_m": SHIFT, "fraction": FRACTION},
               gate=GATE, huber_delta=DELTA, planted_rows=int(planted.sum().item()))
line = json.dumps(rec)
print(line)
os.makedirs(os.path.dirname(os.path.abspath(OUT)), exist_ok=True)
with open(OUT, "a") as f:
    f.write(line + "\n")
