"""Reference for the multi-epoch stationary-receiver fix -- TEST INFRASTRUCTURE.

A NumPy restatement of kingdwd/nlp-filter utils/leastsquares.py:66-94
(iterativeLeastSquares_multiTimeStep): one position x, a clock bias b0 at t = 0 and a
drift alpha over ALL rows of a log, Gauss-Newton steps dx = pinv(G) drho with rows
[-los, 1, t_k] and drho_k = pr_k - |s_k - x| - b0 - alpha t_k, stop after the update when
||dx|| < 1e-7.  It returns the iteration count as well.  Pinned to the reference's own
results (tests/golden/ls_multi.npz, written by tests/golden/gen_ls_multi.py) to 1e-9 m by
tests/test_ls_multi_host.py.

normal_equations() is the kernel's formulation (csrc/mhe_ls.hip: k_ls_multi) in NumPy:
G^T G dx = G^T drho by Cholesky, same stop rule.

The builders below make the inputs that tests/test_ls_multi_host.py checks without a
device and tests/test_gpu_ls_multi.py runs on one; the references are computed once per
process (lru_cache) and must not be modified.
"""
import functools
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
TOL = 1e-7


def geometry(sat_pos, x):
    """buildGeometryMatrix (utils/leastsquares.py:6-16), row by row as the reference."""
    G = np.zeros((sat_pos.shape[0], 3))
    for k in range(sat_pos.shape[0]):
        los = sat_pos[k, :] - x
        G[k, :] = -los / np.linalg.norm(los)
    return G


def _ranges(sat_pos, x):
    return np.array([np.linalg.norm(sat_pos[k, :] - x) for k in range(sat_pos.shape[0])])


def iterate(t, sat_pos, pr, x, b0=0.0, alpha=0.0, maxiter=100):
    """(x, b0, alpha, iterations); x is modified in place like the reference."""
    N = sat_pos.shape[0]
    it = 0
    for it in range(1, maxiter + 1):
        G = np.hstack((geometry(sat_pos, x), np.ones((N, 1)), t.reshape(N, 1)))
        drho = pr - _ranges(sat_pos, x) - b0 - alpha * t
        dx = np.matmul(np.linalg.pinv(G), drho)
        x += dx[0:3]
        b0 += dx[3]
        alpha += dx[4]
        if np.linalg.norm(dx) < TOL:
            break
    return x, b0, alpha, it


def normal_equations(t, sat_pos, pr, x, b0=0.0, alpha=0.0, maxiter=100):
    """The kernel's form: 5x5 normal equations by Cholesky.  (x, b0, alpha, iterations)."""
    x = x.copy()
    N = sat_pos.shape[0]
    it = 0
    for it in range(1, maxiter + 1):
        los = sat_pos - x
        nrm = np.linalg.norm(los, axis=1)
        G = np.hstack((-los / nrm[:, None], np.ones((N, 1)), t.reshape(N, 1)))
        L = np.linalg.cholesky(G.T @ G)
        dx = np.linalg.solve(L.T, np.linalg.solve(L, G.T @ (pr - nrm - b0 - alpha * t)))
        x += dx[0:3]
        b0 += dx[3]
        alpha += dx[4]
        if np.linalg.norm(dx) < TOL:
            break
    return x, b0, alpha, it


def stack_log(t, sat_pos, pr):
    """runBatchLeastSquares' stacking (utils/leastsquares.py:148-155): per-epoch lists -> flat rows."""
    tr = np.concatenate([np.full(len(pr[i]), t[i], dtype=np.float64) for i in range(len(pr))])
    return tr, np.vstack(sat_pos), np.concatenate(pr)


# ---------------------------------------------------------------- test inputs

TAG = "A"          # receiver A: see tests/test_gpu_ls_ragged.py on receiver B's thin prefixes
C = 37             # logs per batch: no multiple of the 4 (G = 16) or 16 (G = 64) logs a block holds
SPANS = (2, 3, 6, 40)
S = 12             # satellite slots per epoch in the fixture
DRIFT, SIGMA = 0.8, 3.0   # clock drift added to the pseudoranges (m/s), noise (m)
# Row capacities of the two batches: all 40 epochs x 12 slots, which the library's rule sends
# to the 16-lane instance, and the smallest capacity it sends to the 64-lane instance.
CAPS = (480, 513)


@functools.lru_cache(maxsize=None)
def fixture():
    return dict(np.load(os.path.join(GOLDEN, "least_squares.npz")))


def fix_A():
    fx = fixture()
    return np.array([fx[f"{TAG}_ls_{a}_ECEF"][0] for a in "xyz"])


def _build(cap, seed):
    """C ragged logs in run_batch's epoch-packed layout (C,40,S) and as flat rows of capacity cap.

    Log c spans SPANS[c % 4] leading epochs; about a tenth of its epochs are dropped
    entirely (never the first or the last of the span, so the span is what it says), the
    others keep a leading count in [5, count] (while a log has more rows than cap, one more
    inner epoch is dropped: not at the capacities in use).  Log 0 is cut to two epochs of five: 10 rows, fewer than
    either group has lanes.  Pseudoranges get a DRIFT m/s clock drift and SIGMA m noise.
    Starts alternate: even logs at the origin, odd logs within 10 m of the fixture's fix."""
    fx = fixture()
    rng = np.random.default_rng(seed)
    T = fx[f"{TAG}_count"].shape[0]
    t_ep = np.asarray(fx[f"{TAG}_t"], dtype=np.float64)
    nsat = np.zeros((C, T), dtype=np.int32)
    for c in range(C):
        span = SPANS[c % 4]
        cnt = rng.integers(5, fx[f"{TAG}_count"][:span] + 1)
        inner = np.arange(1, span - 1)
        cnt[inner[rng.uniform(size=inner.size) < 0.1]] = 0
        if c == 0:
            cnt[:] = 5
        while cnt.sum() > cap:
            live = inner[cnt[inner] > 0]
            cnt[rng.choice(live)] = 0
        nsat[c, :span] = cnt
    sp = np.tile(fx[f"{TAG}_sat_pos"][None], (C, 1, 1, 1))
    pr = (np.tile(fx[f"{TAG}_pr"][None], (C, 1, 1)) + DRIFT * t_ep[None, :, None]
          + SIGMA * rng.normal(size=(C, T, S)))
    t2 = np.tile(t_ep[None], (C, 1))
    d = {"cap": cap, "sp4": sp, "pr3": pr, "t2": t2, "nsat": nsat, "nrows": nsat.sum(1).astype(np.int32)}
    d["sp"], d["pr"], d["t"] = np.zeros((C, cap, 3)), np.zeros((C, cap)), np.zeros((C, cap))
    for c in range(C):
        keep = np.arange(S)[None, :] < nsat[c][:, None]
        n = d["nrows"][c]
        d["sp"][c, :n], d["pr"][c, :n] = sp[c][keep], pr[c][keep]
        d["t"][c, :n] = np.broadcast_to(t_ep[:, None], (T, S))[keep]
    p0 = np.zeros((C, 5))
    off = rng.normal(size=(C, 3))
    off *= (10.0 * rng.uniform(size=(C, 1))) / np.linalg.norm(off, axis=1, keepdims=True)
    p0[1::2, :3] = (fix_A() + off)[1::2]
    d["p0"] = p0
    # starts with a bias and a drift of their own (test 3)
    d["p0_bias"] = p0.copy()
    d["p0_bias"][:, 3] = rng.normal(size=C) * 50.0
    d["p0_bias"][:, 4] = rng.normal(size=C) * 2.0
    return d


def rows(d, c):
    n = d["nrows"][c]
    return d["t"][c, :n], d["sp"][c, :n], d["pr"][c, :n]


def solve_all(d, fn, p0, maxiter=100):
    """fn (iterate or normal_equations) over every log of d from p0 (C,5): p (C,5), iters (C)."""
    p, it = np.zeros((C, 5)), np.zeros(C, dtype=np.int32)
    for c in range(C):
        x, b0, al, it[c] = fn(*rows(d, c), p0[c, :3].copy(), p0[c, 3], p0[c, 4], maxiter=maxiter)
        p[c, :3], p[c, 3], p[c, 4] = x, b0, al
    return p, it


@functools.lru_cache(maxsize=None)
def batch(which):
    """The batch of CAPS[which] with its references: ref (converged), ref2 (two steps from
    p0), ref_bias (from p0_bias); each (p (C,5), iters (C))."""
    d = _build(CAPS[which], seed=71 + which)
    d["ref"] = solve_all(d, iterate, d["p0"])
    d["ref2"] = solve_all(d, iterate, d["p0"], maxiter=2)
    d["ref_bias"] = solve_all(d, iterate, d["p0_bias"])
    return d


# planted logs of test 4: with 16 lanes per log a wave holds logs 4w..4w+3, so waves 0 and 5
# each hold the three planted kinds beside one healthy log (log 0 is the 10-row one); with
# 64 lanes per log every log is a wave of its own
PLANT_FEW, PLANT_ONE_T, PLANT_EMPTY = (1, 21), (2, 22), (3, 23)


def planted(d):
    """d's flat rows with the planted logs: 4 rows; all rows at one t; nrows = 0."""
    nrows, t = d["nrows"].copy(), d["t"].copy()
    nrows[list(PLANT_FEW)] = 4
    for c in PLANT_ONE_T:
        t[c, :] = t[c, 0]
    nrows[list(PLANT_EMPTY)] = 0
    return nrows, t
