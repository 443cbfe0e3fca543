"""Writes tests/golden/ls_multi.npz: the reference's own multi-epoch fixes, as data only.

CPU only; run by hand next to a checkout of the reference (gen_golden.py's REF), never on a
device and never by the tests:

    python tests/golden/gen_ls_multi.py

It calls the reference's two functions (utils/leastsquares.py) on the receiver-A and
receiver-B logs of least_squares.npz as they are:
  * runBatchLeastSquares (:144-169) on A and B (all 40 epochs), then on A's and B's epochs
    [0, 6), in this order in one process and with the fixture's reference point -- each call starts
    from the previous call's fix through iterativeLeastSquares_multiTimeStep's shared
    default x, which is zero before the first;
  * iterativeLeastSquares_multiTimeStep (:66-94) twice in a row with the default x (reset
    to zero first): A's epochs [0, 6), then B's epochs [0, 3) -- the second call's warm
    start through the shared default is what is recorded.
Stored: the returned values, nothing of the reference's program text.
"""
import contextlib
import io
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from gen_golden import load_reference  # noqa: E402

RUNS = (("A40", "A", 40), ("B40", "B", 40), ("A6", "A", 6), ("B6", "B", 6))
PAIR = (("A", 6), ("B", 3))
KEYS = ("b0", "alpha", "x_ECEF", "y_ECEF", "z_ECEF", "lat", "lon", "h", "x_ENU", "y_ENU", "z_ENU")


def log(fx, tag, T):
    """Per-epoch lists of the first T epochs."""
    cnt, t = fx[f"{tag}_count"], np.asarray(fx[f"{tag}_t"], dtype=np.float64)[:T]
    sp = [fx[f"{tag}_sat_pos"][k, :cnt[k]] for k in range(T)]
    pr = [fx[f"{tag}_pr"][k, :cnt[k]] for k in range(T)]
    return t, sp, pr


def main():
    ref = load_reference()
    fx = dict(np.load(os.path.join(HERE, "least_squares.npz")))
    default_x = ref.ls.iterativeLeastSquares_multiTimeStep.__defaults__[0]
    default_x[:] = 0.0
    out = {}
    with contextlib.redirect_stdout(io.StringIO()):   # the reference prints on convergence
        for name, tag, T in RUNS:
            sol = ref.ls.runBatchLeastSquares(*log(fx, tag, T), fx["p_ref"])
            for k in KEYS:
                out[f"{name}_{k}"] = np.float64(sol[k])
        default_x[:] = 0.0
        for i, (tag, T) in enumerate(PAIR):
            t, sp, pr = log(fx, tag, T)
            tr = np.concatenate([np.full(len(pr[k]), t[k]) for k in range(T)])
            x, b0, alpha = ref.ls.iterativeLeastSquares_multiTimeStep(tr, np.vstack(sp), np.concatenate(pr))
            assert x is default_x
            out[f"pair{i}_p"] = np.concatenate((x, [b0, alpha]))
    np.savez_compressed(os.path.join(HERE, "ls_multi.npz"), **out)
    for k in sorted(out):
        print(k, out[k])


if __name__ == "__main__":
    main()
