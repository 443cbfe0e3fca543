"""Outputs of the cases of tests/test_gpu_gn_streams.py, for comparing two builds bit for bit.

  MHE_LIB=<libA.so> python tools/dump_streams.py dump a.npz      (GPU)
  MHE_LIB=<libB.so> python tools/dump_streams.py dump b.npz      (GPU)
  python tools/dump_streams.py cmp a.npz b.npz                   -> exit status 0 if every array is equal

Per (P, M) of the test file, without and with a prior in the constants: X, cost, iters, status of
the four trajectories in a batch of CUs + 8 copies and of the four alone (the small-batch
instance); the per-solve prior weight case, the n = 4 pair and the bounded solve (184 arrays).
Both libraries must hold every pair (a full build, not the van der Pol variant build).
profiles/streams_bitwise.txt is this tool's record of round 10.
"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in ("nlp-filter_amd", "tests", ""):
    sys.path.insert(0, os.path.join(ROOT, p))
import numpy as np  # noqa: E402

NAMES = ("X", "cost", "iters", "status")


def dump(path):
    import test_gpu_gn_streams as t
    from mhe import solver
    out = {}
    rep = t._rep()

    def put(key, arrays):
        for nm, a in zip(NAMES, arrays):
            out[f"{key}_{nm}"] = a.cpu().numpy()

    def both(key, s, w, x0=None, **kw):
        for tag, r in (("large", rep), ("alone", np.arange(t.B))):
            put(f"{key}_{tag}", s.solve(w.X_init[r], w.U, w.Y[r], x0=None if x0 is None else x0[r],
                                        max_iter=t.ITERS, tol=0.0, **{k: v[r] for k, v in kw.items()}))

    for PM in sorted(t.SHAPES):
        for prior in (False, True):
            w = t.make_vdp(*PM, prior=prior)
            both(f"P{PM[0]}_M{PM[1]}_{int(prior)}", solver.from_workload(w), w, w.x0)
    w = t.make_vdp(101, 101)
    Pw, x0 = t.ar.prior_inputs(w)
    w.Pw = t.ar.const_prior(w)
    both("pw_P101", solver.from_workload(w), w, x0, Pw=Pw)
    from test_gpu_pairs import case
    c = case("di_P17_M16")
    both("di_P17_M16", c.solver(), c.w)
    w = t.make_vdp(21, 21)
    both("bounded_P21", solver.from_workload(w, bounds=[(1, 0.5, np.inf), (0, -np.inf, 1.5)]), w)
    np.savez(path, **out)
    print("dumped", len(out), "arrays")


def cmp(pa, pb):
    a, b = np.load(pa), np.load(pb)
    bad = [k for k in a.files if k not in b.files or a[k].dtype != b[k].dtype or a[k].tobytes() != b[k].tobytes()]
    print(f"{len(a.files) - len(bad)}/{len(a.files)} arrays bitwise equal {bad}")
    return 1 if bad or set(a.files) != set(b.files) else 0


if __name__ == "__main__":
    sys.exit(dump(sys.argv[2]) if sys.argv[1] == "dump" else cmp(*sys.argv[2:4]))
