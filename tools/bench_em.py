"""Cost of the noise-identification kernels beside the smoother they follow.

    python tools/bench_em.py all   [gnss|autocar] [B] [reps]
    python tools/bench_em.py plain [gnss|autocar] [B] [reps] [LIB]

all:   on one filtered history, the same build's plain smoother (k_ekf_rts<.., false>,
       mhe_ekf_smooth), the smoother with the lag-one output (k_ekf_rts<.., true>,
       mhe_ekf_smooth_args) and the statistics kernel (k_ekf_em, mhe_ekf_em_stats) on the
       smoother's output.
plain: the plain smoother alone through the library file LIB (default: the product's), opened
       on its own with only mhe_ekf_smooth bound, so a library built from an earlier revision
       (tools/build_from.sh) that lacks the newer symbols can be measured by this same tool;
       alternate the two builds in one sitting, one process each.

Workloads: the smoother's shapes of tools/bench_ekf_smooth.py (gnss_stationary recipe, n = 5, 51
epochs; autonomous-car plug-ins, n = 9, 300 steps), B filters with perturbed priors, inputs and
histories batch-innermost and resident on the device, the forward filter (k_ekf_lane) run once to
produce the history.  Every timed call goes straight to the C entry point with buffers allocated
once: no allocation inside a window.  Timing: HIP events around `reps` launches after a warm-up
launch, five windows, median, mean and spread ((max - min) / median) reported.
"""
import ctypes
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

MODE = sys.argv[1] if len(sys.argv) > 1 else "all"
WHICH = sys.argv[2] if len(sys.argv) > 2 else "gnss"
B = int(sys.argv[3]) if len(sys.argv) > 3 else 65536
REPS = int(sys.argv[4]) if len(sys.argv) > 4 else 10
LIB = os.path.abspath(sys.argv[5]) if len(sys.argv) > 5 else _lib.LIB_PATH
WINDOWS = 5
dev = torch.device("cuda", 0)
G = os.path.join(ROOT, "tests", "golden")


def rep(a, dtype=torch.float64):
    """(..., B) on the device: the fixture's array repeated along a new innermost batch axis."""
    t = torch.as_tensor(np.ascontiguousarray(a), dtype=dtype, device=dev)
    return t.unsqueeze(-1).expand(*t.shape, B).contiguous()


if WHICH == "gnss":
    fx = dict(np.load(os.path.join(G, "ekf_gnss_stationary.npz")))
    T, pmax, n, m = fx["pr"].shape[0], 12, 5, 3
    rng = np.random.default_rng(7)
    mu0 = np.tile(fx["mu0"], (B, 1))
    mu0[1:] += rng.normal(size=(B - 1, 5)) * np.array([3, 3, 3, 30, 0.1])
    U = torch.as_tensor(np.ascontiguousarray(np.moveaxis(rng.normal(size=(B, T, 3)) * 0.1, 0, -1)), device=dev)
    Z, nz, sat = rep(fx["pr"]), rep(fx["nsat"], torch.int32), rep(fx["sat_pos"])
    dyn, meas, dparams = gnss.gnss_pos_and_bias, gnss.multi_pseudorange, {"dt": 1.0}
elif WHICH == "autocar":
    fx = dict(np.load(os.path.join(G, "ekf_autocar.npz")))
    car = dict(zip(("C_AF", "C_AR", "M", "D_F", "D_R", "I_Z"), fx["car"]))
    dparams = {"dt": float(fx["dt"]), "car_params": car}
    T, pmax, n, m = fx["U"].shape[0], fx["Z"].shape[1], 9, 2
    rng = np.random.default_rng(11)
    mu0 = np.tile(fx["mu0"], (B, 1))
    mu0[1:, :2] += rng.normal(size=(B - 1, 2))
    U, Z, nz, sat = rep(fx["U"]), rep(fx["Z"]), rep(fx["nz"], torch.int32), rep(fx["sat_pos"])
    dyn, meas = veh.discrete_vehicle_dynamics, veh.vehicle_sensors_model
else:
    raise SystemExit(f"unknown workload {WHICH!r}")
S0 = torch.as_tensor(np.tile(fx["S0"], (B, 1, 1)), device=dev)
mu0 = torch.as_tensor(mu0, device=dev)
R = torch.as_tensor(np.stack([np.diag(float(fx["r_pr"]) * np.ones(pmax)) for _ in range(T)]), device=dev)
Q = torch.as_tensor(fx["Q"], device=dev).contiguous()

mh, Sh, _, _, st = ekf.run_batch(dyn, meas, mu0, S0, U, Z, nz, Q, R, dparams["dt"], sat, method="lane",
                                 inputs="batch_inner", dyn_params=dparams)
torch.cuda.synchronize()
assert int(st.abs().sum().item()) == 0
mh_st, Sh_st = ekf._hist_storage(mh, (n,))[0], ekf._hist_storage(Sh, (n, n))[0]
assert mh_st.data_ptr() == mh.data_ptr() and Sh_st.data_ptr() == Sh.data_ptr()     # consumed without a copy

(did, _, _), (mid, _, q) = ekf.models(dyn, meas)
dims = _lib.MheEkfDims(n=n, m=m, pmax=pmax, q=q, dyn_model=did, meas_model=mid, dt=float(dparams["dt"]),
                       hist_batch_inner=1, in_batch_inner=1)
for i, v in enumerate(ekf.dyn_par(dyn, dparams)):
    dims.dyn_par[i] = float(v)
ms, Ss = torch.empty_like(mh_st), torch.empty_like(Sh_st)
m0s, S0s = torch.empty_like(mu0), torch.empty_like(S0)
status = torch.empty(B, dtype=torch.int32, device=dev)
stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
p = lambda t: ctypes.c_void_p(t.data_ptr())   # noqa: E731


def timed(fn):
    fn()
    torch.cuda.synchronize()
    w = []
    for _ in range(WINDOWS):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(REPS):
            fn()
        e1.record()
        torch.cuda.synchronize()
        w.append(e0.elapsed_time(e1) / REPS)
    med = sorted(w)[len(w) // 2]
    return {"ms_median": med, "ms_mean": float(np.mean(w)), "spread": (max(w) - min(w)) / med, "windows_ms": w,
            "filter_steps_per_s": B * T / (med * 1e-3)}


def plain_call(lib):
    def call():
        rc = lib.mhe_ekf_smooth(ctypes.byref(dims), B, T, p(mh_st), p(Sh_st), p(U), T * m, p(Q), p(mu0), p(S0), p(ms),
                                p(Ss), p(m0s), p(S0s), p(status), stream)
        assert rc == 0, rc
    return call


base = {"workload": WHICH, "n": n, "B": B, "T": T, "reps": REPS, "windows": WINDOWS}
if MODE == "plain":
    raw = ctypes.CDLL(LIB)
    raw.mhe_ekf_smooth.restype = ctypes.c_int
    raw.mhe_ekf_smooth.argtypes = _lib.SIGNATURES["mhe_ekf_smooth"][1]
    out = timed(plain_call(raw))
    assert int(status.abs().sum().item()) == 0
    print(json.dumps(dict(base, mode="plain", kernel="mhe_ekf::k_ekf_rts (plain instance)",
                          lib=os.path.relpath(LIB, ROOT), lib_sha256_16=_lib.lib_digest(LIB), **out)))
elif MODE == "all":
    lib = _lib.load()
    C = torch.empty_like(Sh_st)
    lag = _lib.MheEkfLagArgs(batch=B, steps=T, mu_hist=mh_st.data_ptr(), S_hist=Sh_st.data_ptr(), U=U.data_ptr(),
                             u_bstride=T * m, Q=Q.data_ptr(), mu0=mu0.data_ptr(), S0=S0.data_ptr(), mu_s=ms.data_ptr(),
                             S_s=Ss.data_ptr(), mu0_s=m0s.data_ptr(), S0_s=S0s.data_ptr(), status=status.data_ptr(),
                             C=C.data_ptr())
    Qsum = torch.empty((B, n, n), dtype=torch.float64, device=dev)
    r2 = torch.empty((T, pmax, B), dtype=torch.float64, device=dev)
    q_cnt, r_cnt, est = (torch.empty(B, dtype=torch.int32, device=dev) for _ in range(3))
    ea = _lib.MheEmArgs(batch=B, steps=T, mu_s=ms.data_ptr(), S_s=Ss.data_ptr(), C=C.data_ptr(), mu0_s=m0s.data_ptr(),
                        S0_s=S0s.data_ptr(), U=U.data_ptr(), u_bstride=T * m, Z=Z.data_ptr(), z_bstride=T * pmax,
                        nz=nz.data_ptr(), nz_bstride=T, PAR=sat.data_ptr(), par_bstride=T * pmax * q,
                        Qsum=Qsum.data_ptr(), q_cnt=q_cnt.data_ptr(), r2=r2.data_ptr(), r_cnt=r_cnt.data_ptr(),
                        status=est.data_ptr())

    def lag_call():
        rc = lib.mhe_ekf_smooth_args(ctypes.byref(dims), ctypes.byref(lag), stream)
        assert rc == 0, rc

    def em_call():
        rc = lib.mhe_ekf_em_stats(ctypes.byref(dims), ctypes.byref(ea), stream)
        assert rc == 0, rc

    t_plain = timed(plain_call(lib))
    t_lag = timed(lag_call)
    assert int(status.abs().sum().item()) == 0
    t_em = timed(em_call)
    assert int(est.abs().sum().item()) == 0 and int(q_cnt.min().item()) == T
    Qhat = (Qsum.sum(0) / q_cnt.sum()).cpu().numpy()
    # algorithmic bytes per filter-step (doubles): the smoother reads mu, the triangle of S and u and
    # writes mu_s and S_s (+ C); the statistics kernel reads mu_s, the triangle of S_s, C, u, nz and
    # the rows' z and satellite, and writes r2
    tri = n * (n + 1) // 2
    rows = float(nz.to(torch.float64).mean().item())
    by = {"plain": 8.0 * (n + tri + m + n + n * n), "lag_one": 8.0 * (n + tri + m + n + 2 * n * n),
          "em": 8.0 * (n + tri + n * n + m + 4 * rows + pmax) + 4.0}
    for k, t in (("plain", t_plain), ("lag_one", t_lag), ("em", t_em)):
        t["bytes_per_step"] = by[k]
        t["achieved_GBs"] = by[k] * t["filter_steps_per_s"] / 1e9
    print(json.dumps(dict(base, mode="all", lib_sha256_16=_lib.lib_digest(), smooth_plain=t_plain,
                          smooth_lag_one=t_lag, em_stats=t_em,
                          lag_over_plain=t_lag["ms_median"] / t_plain["ms_median"],
                          em_over_plain=t_em["ms_median"] / t_plain["ms_median"],
                          diag_Q_estimate=np.diag(Qhat).tolist(), diag_Q_given=np.diag(fx["Q"]).tolist())))
else:
    raise SystemExit(f"unknown mode {MODE!r}")
