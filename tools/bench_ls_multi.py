"""Multi-epoch stationary-receiver least squares: throughput of k_ls_multi's two instances.

    python tools/bench_ls_multi.py [--out FILE]     every shape, one child process each
    python tools/bench_ls_multi.py --shape NAME     one shape, one JSON line

utils.leastsquares.run_batch_multi's kernel (mhe_ls_multi_run, csrc/mhe_ls.hip) with 16 and
with 64 lanes per log (mhe_set_option(MHE_OPT_LSM_GROUP), which the product never sets) on
  log      the receiver-A log of tests/golden/least_squares.npz, 326 rows (40 epochs),
           x C = 1, 256, 16384, 262144 logs
  short    its first 6 epochs (55 rows: the 16-lane instance holds them in registers)
           x C = 256, 16384, 262144
  shortpad the same 55 rows in a row capacity of 65, which the held-rows instance does not
           take (rows read again in every iteration)      x C = 16384, 262144
  x2, x3, x6   the log tiled 2, 3 and 6 times, times running on (652, 978, 1956 rows)
           x C = 256, 16384
  long     the log tiled 12 times (3912 rows)      x C = 1, 256, 16384
with a 0.8 m/s drift and 3 m noise per log (made on the device from a seed), cold starts.
Inputs are resident; outputs are allocated once; HIP events around `reps` back-to-back calls
of the C entry point after a warm-up of every instance, reps sized to a window of >= 0.2 s;
the two instances alternate and each figure is the median of 3 windows.
Metrics per instance: ms per launch, logs/s (fixes/s), rows/s (rows x GN iterations), and
GB/s of the algorithmic 40 B per row per log read ONCE -- a lower bound on the traffic, not
what the kernel moves: it reads the rows again in every iteration.
CPU figure: tests/ls_multi_reference.py (a port of the reference's pinv iteration) on one
core over a bounded sample.

The parent never opens the GPU: it starts one child per shape under `timeout`, in order, and
stops at the first that fails.
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = {  # name: (epochs kept, tiles, C, time limit of the child in seconds[, row capacity])
    "log_1": (40, 1, 1, 120), "log_256": (40, 1, 256, 120), "log_16384": (40, 1, 16384, 180),
    "log_262144": (40, 1, 262144, 300),
    "short_256": (6, 1, 256, 120), "short_16384": (6, 1, 16384, 120), "short_262144": (6, 1, 262144, 180),
    "shortpad_16384": (6, 1, 16384, 120, 65), "shortpad_262144": (6, 1, 262144, 180, 65),
    "x2_256": (40, 2, 256, 120), "x2_16384": (40, 2, 16384, 180),
    "x3_256": (40, 3, 256, 120), "x3_16384": (40, 3, 16384, 180),
    "x6_256": (40, 6, 256, 120), "x6_16384": (40, 6, 16384, 180),
    "long_1": (40, 12, 1, 120), "long_256": (40, 12, 256, 180), "long_16384": (40, 12, 16384, 300),
}
DRIFT, SIGMA = 0.8, 3.0


def run_shape(name):
    sys.path[:0] = [os.path.join(ROOT, "nlp-filter_amd"), ROOT, os.path.join(ROOT, "tests")]
    import ctypes

    import numpy as np
    import torch

    import ls_multi_reference as lm
    from mhe import _lib

    T, tiles, C = SHAPES[name][:3]
    fx = lm.fixture()
    cnt = fx["A_count"][:T]
    t_ep = np.asarray(fx["A_t"], dtype=np.float64)
    period = t_ep[-1] - t_ep[0] + (t_ep[1] - t_ep[0])
    t1, sp1, pr1 = lm.stack_log(t_ep[:T], [fx["A_sat_pos"][k, :cnt[k]] for k in range(T)],
                                [fx["A_pr"][k, :cnt[k]] for k in range(T)])
    t_rows = np.concatenate([t1 + i * period for i in range(tiles)])
    sp_rows, pr_rows = np.tile(sp1, (tiles, 1)), np.tile(pr1, tiles) + DRIFT * t_rows
    R = t_rows.shape[0]
    cap = SHAPES[name][4] if len(SHAPES[name]) > 4 else R
    pad = lambda a: np.concatenate((a, np.zeros((cap - R,) + a.shape[1:])))  # noqa: E731
    dev = torch.device("cuda", 0)
    gen = torch.Generator(device=dev).manual_seed(5)
    sp = torch.as_tensor(pad(sp_rows), device=dev)[None].expand(C, cap, 3).contiguous()
    tt = torch.as_tensor(pad(t_rows), device=dev)[None].expand(C, cap).contiguous()
    pr = torch.as_tensor(pad(pr_rows), device=dev)[None] + SIGMA * torch.randn((C, cap), generator=gen, device=dev,
                                                                              dtype=torch.float64)
    nrows = torch.full((C,), R, dtype=torch.int32, device=dev)
    p0 = torch.zeros((C, 5), dtype=torch.float64, device=dev)
    p = torch.empty((C, 5), dtype=torch.float64, device=dev)
    iters = torch.empty((C,), dtype=torch.int32, device=dev)
    lib = _lib.load()
    dims = _lib.MheLsmDims(max_iter=100, tol=1e-7)
    stream = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    ptr = lambda a: ctypes.c_void_p(a.data_ptr())  # noqa: E731

    def launch(G):
        assert lib.mhe_set_option(_lib.OPT_LSM_GROUP, G) >= 0
        _lib.check(lib.mhe_ls_multi_run(ctypes.byref(dims), C, cap, ptr(sp), ptr(pr), ptr(tt), ptr(nrows), ptr(p0),
                                        ptr(p), ptr(iters), stream), "mhe_ls_multi_run")

    def window(G, reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(reps):
            launch(G)
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / reps

    res = {"shape": name, "rows": R, "row_cap": cap, "logs": C, "lib": _lib.lib_digest(), "rule_picks": None}
    sols = {}
    for G in (16, 64):                      # warm-up, and the two instances' answers
        launch(G)
        torch.cuda.synchronize()
        sols[G] = (p.cpu().numpy().copy(), iters.cpu().numpy().copy())
    assert (sols[16][1] > 0).all() and (sols[64][1] > 0).all()
    res["logs_with_other_iteration_count_16_vs_64"] = int((sols[16][1] != sols[64][1]).sum())
    res["max_abs_diff_16_vs_64"] = float(np.abs(sols[16][0] - sols[64][0]).max())
    mean_it = float(sols[16][1].mean())
    reps = {G: max(3, min(2000, int(200.0 / max(window(G, 3), 1e-3)) + 1)) for G in (16, 64)}
    ms = {16: [], 64: []}
    for _ in range(3):
        for G in (16, 64):
            ms[G].append(window(G, reps[G]))
    lib.mhe_set_option(_lib.OPT_LSM_GROUP, 0)
    res["rule_picks"] = lib.mhe_ls_multi_group(cap)
    res["mean_gn_iterations"] = mean_it
    for G in (16, 64):
        m = statistics.median(ms[G])
        res[f"G{G}"] = {"ms_per_launch": m, "windows_ms": ms[G], "reps": reps[G], "logs_per_s": C / (m * 1e-3),
                        "row_iterations_per_s": C * R * mean_it / (m * 1e-3),
                        "GBps_of_40B_per_row_read_once": 40.0 * R * C / (m * 1e-3) / 1e9}
    nb, t0 = 0, time.perf_counter()
    while time.perf_counter() - t0 < 1.0:
        lm.iterate(t_rows, sp_rows, pr_rows + SIGMA * np.random.default_rng(nb).normal(size=R), np.zeros(3))
        nb += 1
    dt = time.perf_counter() - t0
    res["cpu_baseline"] = {"logs_per_s": nb / dt, "cores": 1, "kind": "port",
                           "sample": f"{nb} logs of {R} rows, tests/ls_multi_reference.py on one core, {dt:.1f} s"}
    print(json.dumps(res))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", choices=sorted(SHAPES))
    ap.add_argument("--out", help="append the JSON lines to this file")
    ap.add_argument("--only", nargs="*", help="subset of shapes for the parent run")
    a = ap.parse_args()
    if a.shape:
        return run_shape(a.shape)
    for name in (a.only or SHAPES):
        limit = SHAPES[name][3]
        r = subprocess.run(["timeout", "-k", "10", str(limit), sys.executable, os.path.abspath(__file__), "--shape", name],
                           stdout=subprocess.PIPE, text=True)
        if r.returncode != 0:
            print(f"{name}: exit status {r.returncode}; stopping", file=sys.stderr)
            sys.exit(r.returncode)
        line = r.stdout.strip().splitlines()[-1]
        print(line, flush=True)
        if a.out:
            with open(a.out, "a") as f:
                f.write(line + "\n")


if __name__ == "__main__":
    main()
