"""Ragged batches through the least-squares kernel (csrc/mhe_ls.hip: k_ls, one task per lane).

tests/test_leastsquares.py runs 64 chains with equal satellite counts and compares every
ninth.  Here every chain has its own count at every epoch, cold and warm starts alternate
inside each wave (so neighbouring lanes run 6 and 2-3 iterations), the task counts are no
multiple of the block (301 chains: one block and 45 lanes; 280 epochs: one block and 24),
and every task is compared.

Inputs: receiver A of tests/golden/least_squares.npz, pseudoranges + N(0, 3 m), per chain
and epoch a count in [5, count] (the leading slots are kept).  Receiver A, because with the
leading 5-6 satellites of receiver B's epoch 4 the geometry matrix has a condition number
of 190-400: the normal equations square it, the step length stalls near the 1e-7 stop rule,
and the iteration count there is decided by rounding (the reference's pinv and a NumPy
normal-equation solve disagree on it in about 1 chain in 10).  Receiver A's worst prefix of
five or more has a condition number of 34, and the two formulations agree in every epoch
(checked below without a device).

Reference: oracle/leastsquares.py (the reference's pinv iteration).  Tolerances are those
of tests/test_leastsquares.py: positions and bias 1e-6 m, velocities 1e-6 m/s; iteration
counts equal.
"""
import numpy as np
import pytest

from oracle import leastsquares as ols
from test_leastsquares import V_TOL, X_TOL

TAG = "A"
C_WARM, T_WARM = 301, 6
C_COLD, T_COLD = 7, 40
FLAG_EPOCH, FLAG_LANE = 3, 13       # one chain per wave gets an epoch with 3 satellites


@pytest.fixture(scope="module")
def lsfx(golden):
    return golden["least_squares"]


def _fix(fx, k=0):
    return np.array([fx[f"{TAG}_ls_{a}_ECEF"][k] for a in "xyz"])


def _chains(fx, C, T, seed, starts):
    """C perturbed copies of the first T epochs with ragged counts; starts: "mixed" (even
    chains ~1e3 m N(0,1) from the origin, odd chains within 10 m of the fixture's fix) or "cold"."""
    rng = np.random.default_rng(seed)
    cnt0 = fx[f"{TAG}_count"][:T]
    d = {"cnt": rng.integers(5, cnt0[None, :] + 1, size=(C, T)).astype(np.int32),
         "sp": np.tile(fx[f"{TAG}_sat_pos"][None, :T], (C, 1, 1, 1)),
         "pr": np.tile(fx[f"{TAG}_pr"][None, :T], (C, 1, 1)) + 3.0 * rng.normal(size=(C, T, 12)),
         "sv": np.tile(fx[f"{TAG}_sat_vel"][None, :T], (C, 1, 1, 1)),
         "rr": np.tile(fx[f"{TAG}_pr_rate"][None, :T], (C, 1, 1)) + 0.05 * rng.normal(size=(C, T, 12))}
    x0 = 1e3 * rng.normal(size=(C, 3))
    if starts == "mixed":
        off = rng.normal(size=(C, 3))
        off *= (10.0 * rng.uniform(size=(C, 1))) / np.linalg.norm(off, axis=1, keepdims=True)
        x0[1::2] = (_fix(fx) + off)[1::2]
    d["x0"] = x0
    return d


def _oracle_chain(d, c, skip=()):
    """The reference loop over chain c's epochs through one shared warm-start array; the
    epochs of `skip` are left out (the array passes through them unchanged)."""
    T = d["cnt"].shape[1]
    x = d["x0"][c].copy()
    out = {"x": np.zeros((T, 3)), "b": np.zeros(T), "iters": np.zeros(T, dtype=np.int32),
           "v": np.zeros((T, 3)), "bd": np.zeros(T)}
    for k in range(T):
        if k in skip:
            out["x"][k], out["iters"][k], out["v"][k], out["bd"][k] = x, -1, np.nan, np.nan
            continue
        n = d["cnt"][c, k]
        p, b, it = ols.iterative_least_squares(d["sp"][c, k, :n], d["pr"][c, k, :n], x)
        v, bd = ols.iterative_least_squares_vel(d["sp"][c, k, :n], d["sv"][c, k, :n], d["rr"][c, k, :n], p)
        out["x"][k], out["b"][k], out["iters"][k], out["v"][k], out["bd"][k] = p, b, it, v, bd
    return out


def _stack(rows):
    return {k: np.stack([r[k] for r in rows]) for k in rows[0]}


@pytest.fixture(scope="module")
def warm(lsfx):
    d = _chains(lsfx, C_WARM, T_WARM, seed=41, starts="mixed")
    d["ref"] = _stack([_oracle_chain(d, c) for c in range(C_WARM)])
    return d


@pytest.fixture(scope="module")
def cold(lsfx):
    """C_COLD x T_COLD independent epochs, each from its chain's cold start; ref2: the
    oracle's iterate after two steps."""
    d = _chains(lsfx, C_COLD, T_COLD, seed=43, starts="cold")
    ref = {"x": np.zeros((C_COLD, T_COLD, 3)), "b": np.zeros((C_COLD, T_COLD)),
           "iters": np.zeros((C_COLD, T_COLD), dtype=np.int32)}
    ref2 = {k: v.copy() for k, v in ref.items()}
    for c in range(C_COLD):
        for k in range(T_COLD):
            n = d["cnt"][c, k]
            for r, mi in ((ref, 100), (ref2, 2)):
                r["x"][c, k], r["b"][c, k], r["iters"][c, k] = ols.iterative_least_squares(
                    d["sp"][c, k, :n], d["pr"][c, k, :n], d["x0"][c].copy(), maxiter=mi)
    d["ref"], d["ref2"] = ref, ref2
    return d


def _flagged(warm):
    """The warm input with a 3-satellite epoch in one chain of every wave; (counts, chains)."""
    chains = np.arange(FLAG_LANE, C_WARM, 64)
    cnt = warm["cnt"].copy()
    cnt[chains, FLAG_EPOCH] = 3
    return cnt, chains


def _normal_equations(sp, pr, x, maxiter=100, tol=1e-7):
    """The kernel's formulation in NumPy: G^T G dx = G^T drho by Cholesky, same stop rule."""
    x, b, it = x.copy(), 0.0, 0
    for _ in range(maxiter):
        G = np.hstack((ols.geometry(sp, x), np.ones((len(pr), 1))))
        L = np.linalg.cholesky(G.T @ G)
        dx = np.linalg.solve(L.T, np.linalg.solve(L, G.T @ (pr - np.linalg.norm(sp - x, axis=1) - b)))
        x += dx[:3]
        b += dx[3]
        it += 1
        if np.linalg.norm(dx) < tol:
            break
    return x, b, it


# ---------------------------------------------------------------- preconditions (no device)

def test_ragged_ls_builders_meet_their_preconditions(lsfx, warm, cold):
    for d, T in ((warm, T_WARM), (cold, T_COLD)):
        assert d["cnt"].min() == 5 and (d["cnt"] <= lsfx[f"{TAG}_count"][None, :T]).all()
        assert (d["cnt"].max(0) > d["cnt"].min(0))[lsfx[f"{TAG}_count"][:T] > 5].all()   # ragged at every epoch
    cnt, chains = _flagged(warm)
    assert chains.size == 5 and (chains // 64 == np.arange(5)).all()
    planted = np.zeros(cnt.shape, dtype=bool)
    planted[chains, FLAG_EPOCH] = True
    assert (cnt[planted] == 3).all() and (cnt[~planted] >= 5).all()
    # cold and warm starts alternate inside every wave, and do different amounts of work
    far = np.linalg.norm(warm["x0"] - _fix(lsfx), axis=1)
    assert (far[1::2] <= 10.0).all() and (far[0::2] > 1e5).all()
    it0 = warm["ref"]["iters"][:, 0]
    assert it0[0::2].min() > it0[1::2].max() and it0[1::2].min() >= 2
    assert (cold["ref2"]["iters"] == 2).all() and (cold["ref"]["iters"] > 2).all()
    # the two formulations agree at these inputs: same iteration counts, fixes to X_TOL
    worst = 0.0
    for c in range(0, C_WARM, 3):
        x = warm["x0"][c].copy()
        for k in range(T_WARM):
            n = warm["cnt"][c, k]
            x, b, it = _normal_equations(warm["sp"][c, k, :n], warm["pr"][c, k, :n], x)
            assert it == warm["ref"]["iters"][c, k], (c, k)
            worst = max(worst, np.abs(x - warm["ref"]["x"][c, k]).max(), abs(b - warm["ref"]["b"][c, k]))
    for k in range(T_COLD):
        n = cold["cnt"][3, k]
        x, b, it = _normal_equations(cold["sp"][3, k, :n], cold["pr"][3, k, :n], cold["x0"][3])
        assert it == cold["ref"]["iters"][3, k], k
        worst = max(worst, np.abs(x - cold["ref"]["x"][3, k]).max(), abs(b - cold["ref"]["b"][3, k]))
    print(f"normal equations vs pinv on the ragged inputs: {worst:.2e} m (bound {X_TOL:.0e})")
    assert worst <= X_TOL


# ---------------------------------------------------------------- device

def _run(d, cnt=None, vel=True, **kw):
    import utils.leastsquares as uls
    r = uls.run_batch(d["sp"], d["pr"], d["cnt"] if cnt is None else cnt, x_init=d["x0"],
                      sat_vel=d["sv"] if vel else None, pr_rate=d["rr"] if vel else None, **kw)
    return {k: v.cpu().numpy() for k, v in r.items()}


def _assert_fixes(what, r, ref, rows=slice(None), vel=True):
    ex = max(np.abs(r["x"][rows] - ref["x"][rows]).max(), np.abs(r["b"][rows] - ref["b"][rows]).max())
    ev = max(np.abs(r["v"][rows] - ref["v"][rows]).max(), np.abs(r["bd"][rows] - ref["bd"][rows]).max()) if vel else 0.0
    print(f"{what}: x, b {ex:.2e} m (bound {X_TOL:.0e}); v, bd {ev:.2e} m/s (bound {V_TOL:.0e})")
    np.testing.assert_array_equal(r["iters"][rows], ref["iters"][rows])
    assert ex <= X_TOL and ev <= V_TOL, (what, ex, ev)


@pytest.mark.gpu
def test_warm_chains_ragged(warm):
    r = _run(warm)
    _assert_fixes("warm chains", r, warm["ref"])
    np.testing.assert_array_equal(r["x_last"], r["x"][:, -1])


@pytest.mark.gpu
def test_warm_chain_with_a_flagged_epoch(warm):
    cnt, chains = _flagged(warm)
    r = _run(warm, cnt=cnt)
    others = np.ones(C_WARM, dtype=bool)
    others[chains] = False
    _assert_fixes("chains beside a flagged one", r, warm["ref"], rows=others)
    keep = [k for k in range(T_WARM) if k != FLAG_EPOCH]
    for c in chains:
        ref = _oracle_chain(warm, c, skip=(FLAG_EPOCH,))
        assert r["iters"][c, FLAG_EPOCH] == -1
        assert np.isnan(r["v"][c, FLAG_EPOCH]).all() and np.isnan(r["bd"][c, FLAG_EPOCH])
        np.testing.assert_array_equal(r["x"][c, FLAG_EPOCH], r["x"][c, FLAG_EPOCH - 1])   # the fix is carried
        _assert_fixes(f"chain {c} around its flagged epoch", {k: v[c] for k, v in r.items() if k != "x_last"},
                      ref, rows=keep)
    np.testing.assert_array_equal(r["x_last"], r["x"][:, -1])


@pytest.mark.gpu
def test_cold_epochs_tail(cold):
    assert C_COLD * T_COLD == 256 + 24
    r = _run(cold, vel=False, warm=False)
    _assert_fixes("cold epochs", r, cold["ref"], vel=False)


@pytest.mark.gpu
def test_iteration_cap(cold):
    r = _run(cold, vel=False, warm=False, maxiter=2)
    assert (r["iters"] == 2).all()
    _assert_fixes("two iterations from cold", r, cold["ref2"], vel=False)
