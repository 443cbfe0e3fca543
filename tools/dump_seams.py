"""Outputs of the shapes of tests/test_gpu_gn_seams.py, for comparing two builds bit for bit.

  MHE_LIB=<libA.so> python tools/dump_seams.py dump a.npz      (GPU)
  MHE_LIB=<libB.so> python tools/dump_seams.py dump b.npz      (GPU)
  python tools/dump_seams.py cmp a.npz b.npz                   -> exit status 0 if every array is equal

Per (P, M) of the test file, without and with a prior in the constants: X, cost, iters, status of
the four trajectories in a batch of CUs + 8 copies, once as built and once with a NaN in one
trajectory's X_init; and the two per-solve prior weight cases (120 arrays).  Build the libraries
with tools/build_ab.sh (profiles/seams_bitwise.txt is this tool's record of round 9).
"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in ("nlp-filter_amd", "tests", ""):
    sys.path.insert(0, os.path.join(ROOT, p))
import numpy as np  # noqa: E402

NAMES = ("X", "cost", "iters", "status")


def dump(path):
    import test_gpu_gn_seams as t
    out = {}
    rep = t._rep()
    for PM in sorted(t.SHAPES):
        for prior in (False, True):
            w, s, _ = t._case(*PM, prior)
            Xn = w.X_init.copy()
            Xn[1, 3, 0] = np.nan
            for tag, Xi in (("", w.X_init), ("nan_", Xn)):
                for nm, a in zip(NAMES, t._solve(s, w, Xi, rep)):
                    out[f"P{PM[0]}_M{PM[1]}_{int(prior)}_{tag}{nm}"] = a
    for P in (72, 101):
        w, Pw, x0, s = t._pw_case(P)
        r = s.solve(w.X_init[rep], w.U, w.Y[rep], x0=x0[rep], max_iter=t.ITERS, tol=0.0, Pw=Pw[rep])
        for nm, a in zip(NAMES, r):
            out[f"pw_P{P}_{nm}"] = a.cpu().numpy()
    np.savez(path, **out)
    print("dumped", len(out), "arrays")


def cmp(pa, pb):
    a, b = np.load(pa), np.load(pb)
    bad = [k for k in a.files if k not in b.files or a[k].dtype != b[k].dtype or a[k].tobytes() != b[k].tobytes()]
    print(f"{len(a.files) - len(bad)}/{len(a.files)} arrays bitwise equal {bad}")
    return 1 if bad or set(a.files) != set(b.files) else 0


if __name__ == "__main__":
    sys.exit(dump(sys.argv[2]) if sys.argv[1] == "dump" else cmp(*sys.argv[2:4]))
