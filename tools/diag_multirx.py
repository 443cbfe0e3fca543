"""Why the oracle replica of gnss-multi-receiver.py disagrees with the stored IPOPT
fixes (data/gnss-multi-receiver/NLP_{A,B}.csv) -- a CPU diagnostic on the reference's
logs and stored results, read from tests/golden/gnss-multi-receiver/ (.mat / .csv).

For each window the replica (tests/general_problems.two_rx_mhe_oracle, Gauss-Newton on
the reference objective, W eliminated) reaches J*.  Fixing the horizontal positions of
A and B at t = T to the stored IPOPT values and re-minimising everything else gives
J_c >= J*.  If the stored values were a stationary point of the same objective,
J_c - J* would be at the rounding level; a large gap means the stored fixes are not
the optimum of the objective the script builds (IPOPT stopped elsewhere).  Windows
after the first inherit different priors (the previous window's solution), so only
window 0 -- identical inputs on both sides -- is a clean comparison; later windows are
reported with our own chain's prior.
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "nlp-filter_amd"), ROOT, os.path.join(ROOT, "tests")]

from general_problems import TWO_RX, row, two_rx_weights, two_rx_window_rows  # noqa: E402
from oracle import collocation as oc  # noqa: E402
from oracle import gn_general as gg  # noqa: E402
from oracle import leastsquares as ols  # noqa: E402
from utils import data as gd, utils as gu  # noqa: E402

REF = os.path.join(ROOT, "tests", "golden", "gnss-multi-receiver")


def main(n_windows=6, penalty=1e8):
    dA = gd.load_gnss_logs(REF + "/rec1/rec1_gnss_log_50y_moving_")
    dB = gd.load_gnss_logs(REF + "/rec2/rec2_gnss_log_50y_moving_")
    p_ref = gu.lla2ecef(np.array([37.4276, -122.1670, 0.0]))
    tA, tB = np.asarray(dA["t"], float), np.asarray(dB["t"], float)
    t0 = min(tA.min(), tB.min())
    dA["t"], dB["t"] = tA - t0, tB - t0
    x = np.zeros(3)

    def ls(d):
        o = ols.run_least_squares(d["sat_pos"], d["pr"], d["sat_vel"], d["pr_rate"], x=x)
        e = np.array([gu.ecef2enu(p, p_ref) for p in o["x"]])
        v = np.array([gu.ecef2enu(q, p_ref, rotation_only=True) for q in o["v"]])
        return {"x_ENU": e[:, 0], "y_ENU": e[:, 1], "z_ENU": e[:, 2], "bias": o["b"],
                "xd_ENU": v[:, 0], "yd_ENU": v[:, 1], "zd_ENU": v[:, 2]}

    lsA, lsB = ls(dA), ls(dB)
    refA = np.loadtxt(REF + "/NLP_A.csv", delimiter=",")
    refB = np.loadtxt(REF + "/NLP_B.csv", delimiter=",")
    c = dict(TWO_RX)
    T, N, n, DT = c["T"], c["N"], c["n"], c["DT"]
    P = N + 1
    Qw, Pw = two_rx_weights()
    D, cw = oc.diff_matrix(N), (T / 2.0) * oc.quad_weights(N)
    t_nodes = oc.tau2t(oc.nodes(N), 0.0, T)
    eq = np.array([[k * n + 2, k * n + 7] for k in range(P)])
    xhat0 = np.array([lsA["x_ENU"][0], lsA["y_ENU"][0], lsA["z_ENU"][0], lsA["bias"][0], 0.0,
                      lsB["x_ENU"][0], lsB["y_ENU"][0], lsB["z_ENU"][0], lsB["bias"][0], 0.0])
    t_off = dB["t"][0] - dA["t"][0]
    from scipy.interpolate import interp1d
    enu = lambda s: gu.ecef2enu(s, p_ref)  # noqa: E731
    X = np.zeros((1, P, n))
    lines = []
    for w in range(n_windows):
        t0w = w * DT
        iA = np.nonzero((dA["t"] >= t0w) & (dA["t"] <= t0w + T))[0]
        iB = np.nonzero((dB["t"] >= t0w + t_off) & (dB["t"] <= t0w + t_off + T))[0]
        sA, sB = dA["t"][iA] - t0w, dB["t"][iB] - t0w - t_off
        uA = np.vstack([lsA[k][iA] for k in ("xd_ENU", "yd_ENU", "zd_ENU")])
        uB = interp1d(sB, np.vstack([lsB[k][iB] for k in ("xd_ENU", "yd_ENU", "zd_ENU")]), fill_value="extrapolate")(sA)
        U = interp1d(sA, np.vstack((uA, uB)), fill_value="extrapolate")(t_nodes).T[None]
        satA = [np.array([enu(s) for s in dA["sat_pos"][k]]).reshape(-1, 3) for k in iA]
        satB = [np.array([enu(s) for s in dB["sat_pos"][k]]).reshape(-1, 3) for k in iB]
        t, rows, Rw, Y = two_rx_window_rows(c, satA, [dA["pr"][k] for k in iA], satB, [dB["pr"][k] for k in iB])

        def solve(extra_t, extra_rows, extra_R, extra_Y, X0):
            tt, rr, RR, YY = (np.concatenate([t, extra_t]), np.concatenate([rows, extra_rows]),
                              np.concatenate([Rw, extra_R]), np.concatenate([Y, extra_Y]))
            o = np.argsort(tt, kind="stable")
            pb = gg.GeneralProblem(N, T, n, 6, "gnss_two_receiver", "mixed", D, cw, oc.interp_matrix(N, T, tt[o]),
                                   Qw, RR[o], Pw=Pw, eq=eq)
            Xs, _, _, _, st = gg.gauss_newton_general(pb, X0, None, U, YY[o].reshape(1, -1, 1), rr[o][None],
                                                      xhat0[None], max_iter=100, tol=1e-12)
            # objective WITHOUT the extra rows
            o0 = np.argsort(t, kind="stable")
            pb0 = gg.GeneralProblem(N, T, n, 6, "gnss_two_receiver", "mixed", D, cw, oc.interp_matrix(N, T, t[o0]),
                                    Qw, Rw[o0], Pw=Pw, eq=eq)
            J = gg.cost_full(pb0, Xs, None, U, Y[o0].reshape(1, -1, 1), rows[o0][None], xhat0[None])[0]
            return Xs, J, int(st[0])

        Xs, Js, st = solve(np.zeros(0), np.zeros((0, rows.shape[1])), np.zeros(0), np.zeros(0), X)
        eA = enu(gu.lla2ecef(np.array([refA[w, 0], refA[w, 1], 0.0])))
        eB = enu(gu.lla2ecef(np.array([refB[w, 0], refB[w, 1], 0.0])))
        pen_rows = np.array([row(gg.ROW_COMP, [k]) for k in (0, 1, 5, 6)])
        Xc, Jc, stc = solve(np.full(4, T), pen_rows, np.full(4, penalty), np.array([eA[0], eA[1], eB[0], eB[1]]), Xs)
        dpos = np.array([np.hypot(*(Xs[0, -1, 0:2] - eA[:2])), np.hypot(*(Xs[0, -1, 5:7] - eB[:2]))])
        miss = np.array([np.hypot(*(Xc[0, -1, 0:2] - eA[:2])), np.hypot(*(Xc[0, -1, 5:7] - eB[:2]))])
        # the penalty rows hold the fixed coordinates with force 2 R miss: the objective's
        # gradient there, nonzero unless the stored fixes were stationary
        force = 2.0 * penalty * miss.max()
        lines.append(f"window {w}: J* = {Js:.6f} (status {st}), |A-A_ipopt| = {dpos[0]:.2f} m, |B-B_ipopt| = "
                     f"{dpos[1]:.2f} m; with A, B fixed to the IPOPT fixes: J_c = {Jc:.6f} (status {stc}, "
                     f"residual miss {miss.max():.1e} m, |dJ/dx| there ~ {force:.0f} per m), J_c - J* = {Jc - Js:.4f}")
        print(lines[-1], flush=True)
        X = Xs
        xhat0 = oc.interp_matrix(N, T, [DT])[0] @ Xs[0]
    return lines


if __name__ == "__main__":
    main(int(sys.argv[1]) if len(sys.argv) > 1 else 6)
