"""Reference for pseudo-Huber measurement rows -- TEST INFRASTRUCTURE (imports oracle/).

Row i with weight R_i, residual e_i = y_i - h(x(t_i)) and scale delta_i costs the
reference's pseudo_huber_loss with Q = R_i (cost_functions.py:25-31),

    2 R_i delta_i^2 (sqrt(1 + e_i^2 / delta_i^2) - 1) = 2 R_i e_i^2 / (1 + s_i),
    s_i = sqrt(1 + e_i^2 / delta_i^2)

(the second form does not cancel for |e| << delta), and is solved by iteratively
reweighted least squares: every step is the oracle's Gauss-Newton step of the quadratic
problem whose row weights are lambda_i = R_i / s_i at the current iterate.  The quadratic
majorises the loss at that iterate (oracle.gn.huber_weights), so undamped steps decrease
the robust cost monotonically.  Everything is built from oracle.gn / oracle.gn_general
as they are: residuals with the original weights, normal equations on a copy of the
problem that carries lambda in Rw's place.  delta = +inf gives s = 1 exactly: the
quadratic row.
"""
import numpy as np

from oracle import gn
from oracle import gn_general as gg


def _bm(a, B, M):
    """(M,), (1, M) or (B, M) [, 1, 1] -> (B, M)."""
    a = np.asarray(a, dtype=np.float64)
    a = a.reshape(a.shape[:-2]) if a.ndim >= 3 else a
    return np.broadcast_to(a if a.ndim == 2 else a[None], (B, M))


def row_weights(Rw, e, delta):
    """lambda (B, M) and the rows' robust cost (B,) from weights Rw, residuals e (B, M)
    (0 on masked rows) and scales delta."""
    B, M = e.shape
    R, dl = _bm(Rw, B, M), _bm(delta, B, M)
    s = np.sqrt(1.0 + e ** 2 / dl ** 2)
    return R / s, np.sum(2.0 * R * e ** 2 / (1.0 + s), axis=1)


def _dyn_cost(pb, X, U, Y, PAR, x0):
    """Dynamics + prior cost: the oracle's cost with every measurement row masked."""
    return gn.residuals(gn._with_rw(pb, np.zeros_like(pb.Rw)), X, U, Y, PAR, x0)[3]


def weights(pb, X, U, Y, PAR, delta, x0=None):
    """lambda (B, M, 1, 1) at X (the Rw of the reweighted problem) and the robust cost (B,)."""
    _, _, e, _ = gn.residuals(pb, X, U, Y, PAR, x0)
    lam, cm = row_weights(pb.Rw, e[..., 0], delta)
    return lam[..., None, None], _dyn_cost(pb, X, U, Y, PAR, x0) + cm


def cost(pb, X, U, Y, PAR, delta, x0=None):
    return weights(pb, X, U, Y, PAR, delta, x0)[1]


def reweighted(pb, X, U, Y, PAR, delta, x0=None):
    """The quadratic problem whose Gauss-Newton system at X is the IRLS system."""
    return gn._with_rw(pb, weights(pb, X, U, Y, PAR, delta, x0)[0])


def normal_equations(pb, X, U, Y, PAR, delta, x0=None):
    """IRLS system at X: H (B, d, d), g (B, d) -- half the gradient of the robust cost --
    and the robust cost (B,)."""
    lam, c = weights(pb, X, U, Y, PAR, delta, x0)
    H, g, _ = gn.normal_equations(gn._with_rw(pb, lam), X, U, Y, PAR, x0)
    return H, g, c


def _gn_loop(system, cost_at, X0, max_iter, tol, perturb):
    """oracle.gn.gauss_newton's loop and stopping rule, one trajectory at a time, on
    system(b, X_b) -> (H, g) and cost_at(X) -> (B,)."""
    X = np.array(X0, dtype=np.float64, copy=True)
    B = X.shape[0]
    iters = np.zeros(B, dtype=np.int32)
    status = np.full(B, gn.MAXITER, dtype=np.int32)
    for b in range(B):
        for _ in range(max_iter):
            H, g = system(b, X[b:b + 1])
            if perturb is not None:
                H, g = gn.perturb_rel(H, perturb), gn.perturb_rel(g, perturb + 1)
            try:
                L = np.linalg.cholesky(H)
            except np.linalg.LinAlgError:
                status[b] = gn.NOT_SPD
                break
            delta = -np.linalg.solve(L.T, np.linalg.solve(L, g))
            if not np.all(np.isfinite(delta)):
                status[b] = gn.NONFINITE
                break
            step = delta.reshape(X.shape[1:])
            X[b] = X[b] + step
            iters[b] += 1
            if np.max(np.abs(step)) <= tol * (1.0 + np.max(np.abs(X[b]))):
                status[b] = gn.OK
                break
    return X, cost_at(X), iters, status


def _one(A, b, B):
    return None if A is None else (A[b:b + 1] if A.shape[0] == B else A)


def gauss_newton(pb, X0, U, Y, PAR, delta, x0=None, max_iter=20, tol=1e-10, perturb=None):
    """IRLS with oracle.gn.gauss_newton's stopping rule.  Returns X, robust cost (at the
    returned X), iters, status.  ``perturb`` as oracle.gn.gauss_newton."""
    B = np.shape(X0)[0]
    M = pb.M
    dl = _bm(delta, B, M)

    def system(b, Xb):
        pbb = gn._with_rw(pb, pb.Rw[b:b + 1]) if pb.Rw.ndim == 4 else pb
        H, g, _ = normal_equations(pbb, Xb, _one(U, b, B), Y[b:b + 1], _one(PAR, b, B), dl[b:b + 1], _one(x0, b, B))
        return H[0], g[0]

    return _gn_loop(system, lambda X: cost(pb, X, U, Y, PAR, delta, x0), X0, max_iter, tol, perturb)


# ---------------------------------------------------------------- mixed rows (oracle.gn_general)
def general_residuals(pb, X, Y, PAR):
    """e (B, M) of a gg.GeneralProblem without extra variables (0 on masked rows)."""
    X = np.asarray(X, dtype=np.float64)
    B = X.shape[0]
    R = _bm(pb.Rw, B, pb.M)
    e = np.zeros((B, pb.M))
    for b in range(B):
        for i in range(pb.M):
            if R[b, i] == 0.0:
                continue
            h, _ = gg.mixed_row(PAR[min(b, PAR.shape[0] - 1), i], pb.Phi[i] @ X[b])
            e[b, i] = float(np.ravel(Y[b, i])[0]) - h
    return e


def _general_with_rw(pb, Rw):
    q = gg.GeneralProblem.__new__(gg.GeneralProblem)
    q.__dict__.update(pb.__dict__)
    q.Rw = Rw
    return q


def general_normal_equations(pb, X, U, Y, PAR, delta, x0=None):
    """IRLS system of a mixed-row problem (no extra variables, no constraints) at X."""
    assert pb.n_extra == 0 and pb.eq.shape[0] == 0
    lam, cm = row_weights(pb.Rw, general_residuals(pb, X, Y, PAR), delta)
    H, g, _ = gg.normal_equations_full(_general_with_rw(pb, lam), X, None, U, Y, PAR, x0)
    return H, g, gg._dynamics_part(pb, np.asarray(X, dtype=np.float64), U, x0)[2] + cm


def general_gauss_newton(pb, X0, U, Y, PAR, delta, x0=None, max_iter=20, tol=1e-10, perturb=None):
    B = np.shape(X0)[0]
    dl = _bm(delta, B, pb.M)
    R = _bm(pb.Rw, B, pb.M)

    def system(b, Xb):
        H, g, _ = general_normal_equations(_general_with_rw(pb, R[b]), Xb, _one(U, b, B), Y[b:b + 1],
                                           _one(PAR, b, B), dl[b:b + 1], _one(x0, b, B))
        return H[0], g[0]

    def cost_at(X):
        return general_normal_equations(_general_with_rw(pb, R), X, U, Y, PAR, dl, x0)[2]

    return _gn_loop(system, cost_at, X0, max_iter, tol, perturb)


# ---------------------------------------------------------------- the issue's inputs
SEED, OUTLIER_FRACTION, OUTLIER, DELTA = 7, 0.08, 400.0, 15.0


def with_outliers(Y):
    """Y with 8 % of the rows shifted by +400 m (rng seed 7) and the mask."""
    rng = np.random.default_rng(SEED)
    out = rng.random(Y.shape) < OUTLIER_FRACTION
    Y = np.array(Y, dtype=np.float64, copy=True)
    Y[out] += OUTLIER
    return Y, out


def position_error(w, X):
    """Per trajectory: the largest distance of a node's position estimate from the (stationary)
    true position."""
    return np.linalg.norm(X[:, :, :3] - w.X_true[:, :1, :3], axis=-1).max(axis=1)


# ---------------------------------------------------------------- bounds (projected Newton)
def gauss_newton_bounded(pb, X0, U, Y, PAR, delta, x0=None, max_iter=20, tol=1e-10, trace=None):
    """oracle.gn.gauss_newton_bounded with the IRLS system and the robust cost: the same
    epsilon-active set, reduced step and Armijo search along the projection arc (pb.lb /
    pb.ub), the noise term with |lambda e| (oracle.gn.cost_noise of the reweighted problem)."""
    X = np.array(X0, dtype=np.float64, copy=True)
    B = X.shape[0]
    dl = _bm(delta, B, pb.M)
    lo, hi = gn.box(pb, X.shape[1:])
    X = np.clip(X, lo, hi)
    iters = np.zeros(B, dtype=np.int32)
    status = np.full(B, gn.MAXITER, dtype=np.int32)
    for b in range(B):
        pbb = gn._with_rw(pb, pb.Rw[b:b + 1]) if pb.Rw.ndim == 4 else pb
        a = (_one(U, b, B), Y[b:b + 1], _one(PAR, b, B))
        kw = dict(delta=dl[b:b + 1], x0=_one(x0, b, B))
        noise = lambda Xb: gn.cost_noise(reweighted(pbb, Xb, *a, **kw), Xb, *a, kw["x0"])[0]  # noqa: E731
        Xb = X[b:b + 1].copy()
        while iters[b] < max_iter:
            H, g, J = (v[0] for v in normal_equations(pbb, Xb, *a, **kw))
            x = Xb[0]
            act = gn.active_set(pb, x, g.reshape(x.shape)).ravel()
            dH = np.diag(H).copy()
            H[act, :] = 0.0
            H[:, act] = 0.0
            H[act, act] = dH[act]
            try:
                L = np.linalg.cholesky(H)
            except np.linalg.LinAlgError:
                status[b] = gn.NOT_SPD
                break
            d = -np.linalg.solve(L.T, np.linalg.solve(L, g)).reshape(x.shape)
            if not np.all(np.isfinite(d)):
                status[b] = gn.NONFINITE
                break
            s = np.clip(x + d, lo, hi) - x
            actr, gr = act.reshape(x.shape), g.reshape(x.shape)
            alpha, nz0 = 1.0, noise(Xb)
            for _ in range(gn.LS_MAX):
                xt = np.clip(x + alpha * d, lo, hi)
                pred = alpha * np.sum(np.where(actr, 0.0, gr * d)) + np.sum(np.where(actr, gr * (xt - x), 0.0))
                Jt = cost(pbb, xt[None], *a, **kw)[0]
                if Jt <= J + 2.0 * gn.ARMIJO_SIGMA * pred + nz0 + noise(xt[None]) + gn.COST_SLACK * abs(J):
                    break
                alpha *= 0.5
            Xb = xt[None]
            if trace is not None:
                trace.append((b, int(iters[b]), alpha, int(act.sum())))
            iters[b] += 1
            if np.max(np.abs(s)) <= tol * (1.0 + np.max(np.abs(xt))):
                status[b] = gn.OK
                break
        X[b] = Xb[0]
    return X, cost(pb, X, U, Y, PAR, delta, x0), iters, status


def active_set_margins(pb, X0, U, Y, PAR, delta, g_floor, max_iter):
    """How far the projected Newton method's active-set decisions of its first ``max_iter``
    iterations are from flipping, on the reference alone: (m_g, m_x) with
      m_g  the smallest |g| / g_floor over the bounded entries within eps of their bound
           (their sign of g decides active / free; g_floor(pb', X) is g's entrywise rounding
           level, e.g. big_oracle.g_rounding_floor, given the reweighted problem pb'),
      m_x  the smallest distance of any other bounded entry from the eps band.
    A case with m_g near 1 has a decision that rounding makes, not the method: two correct
    evaluations then take different (equally valid) paths to the same KKT point and differ
    by far more than rounding at a fixed iteration count."""
    m_g, m_x = np.inf, np.inf
    B = np.shape(X0)[0]
    for it in range(max_iter):
        X = gauss_newton_bounded(pb, X0, U, Y, PAR, delta, max_iter=it, tol=0.0)[0]
        g = normal_equations(pb, X, U, Y, PAR, delta)[1].reshape(X.shape)
        fl = g_floor(reweighted(pb, X, U, Y, PAR, delta), X).reshape(X.shape)
        lo, hi = gn.box(pb, X.shape)
        bounded = np.isfinite(lo) | np.isfinite(hi)
        for b in range(B):
            wv = np.max(np.abs(X[b] - np.clip(X[b] - g[b], lo[b], hi[b])), where=bounded[b], initial=0.0)
            eps = min(gn.EPS_ACT * (1.0 + np.abs(X[b]).max()), wv)
            near = bounded[b] & ((X[b] <= lo[b] + eps) | (X[b] >= hi[b] - eps))
            if near.any():
                m_g = min(m_g, float((np.abs(g[b]) / fl[b])[near].min()))
            far = bounded[b] & ~near
            if far.any():
                m_x = min(m_x, float(np.minimum(np.abs(X[b] - lo[b] - eps), np.abs(hi[b] - eps - X[b]))[far].min()))
    return m_g, m_x
