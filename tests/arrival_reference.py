"""Reference for the per-solve prior weight and the arrival cost -- TEST INFRASTRUCTURE
(imports oracle/).

Per-trajectory oracle.  ``oracle.gn.Problem`` carries ONE (n, n) prior weight, so the
reference of a batch whose trajectories each have their own Pw_b is B problems of batch 1,
each solved by ``gn.gauss_newton`` (``gauss_newton_bounded`` when the problem has bounds)
from the same start, stacked.

Arrival weight.  With C_ref = S_t inv(H) S_t^T (cov_reference.cov_from_H) at the point X,

    A_ref = sym(inv(C_ref)),     bound = FLOOR_MULT * floor + 1e-12 * max|A_ref|

where floor is the change of A_ref when every entry of H moves by eps of its magnitude
(gn.perturb_rel(H, tolerance.SEED_H)) -- the rule of cov_reference.py, carried through the
n x n inverse.  One bound per trajectory.

Inputs (``prior_inputs``).  rng = default_rng(7); G (B, n, n) then the x0 noise (B, n) are
drawn in that order; Pw_b = d S_b d with S_b = G_b G_b^T / n + 0.5 I (symmetrised exactly)
and d = sqrt(scale): scale = [10, 10] for van der Pol (the size of its measurement
information 1 / 0.01 .. 1 / 0.02 over ten), [10] for the single integrator by the same
reasoning, [1e-2, 1e-2, 1e-2, 1e-2, 1] for the GNSS shapes (100 m^2 position / clock
variances, 1 (m/s)^2 drift); x0_b = X_init[b, 0] + 0.1 N(0, 1).  The make_* workloads carry
no prior: the tests add one.
"""
import numpy as np

from oracle import gn

import cov_reference as cr
import tolerance as tl

SCALES = {1: [10.0], 2: [10.0, 10.0], 5: [1e-2, 1e-2, 1e-2, 1e-2, 1.0]}


def prior_inputs(w, seed=7):
    """(Pw (B, n, n), x0 (B, n)) for the workload, see the module docstring."""
    rng = np.random.default_rng(seed)
    n, B = w.n, w.B
    G = rng.normal(size=(B, n, n))
    noise = rng.normal(size=(B, n))
    d = np.sqrt(np.asarray(SCALES[n], dtype=np.float64))
    S = G @ np.swapaxes(G, 1, 2) / n + 0.5 * np.eye(n)
    S = 0.5 * (S + np.swapaxes(S, 1, 2))
    Pw = d[None, :, None] * S * d[None, None, :]
    assert np.array_equal(Pw, np.swapaxes(Pw, 1, 2))
    return Pw, w.X_init[:, 0] + 0.1 * noise


def const_prior(w):
    """A prior weight for the device constants that no trajectory uses: diag(scale)."""
    return np.diag(np.asarray(SCALES[w.n], dtype=np.float64))


def problem(w, Pw_b, **kw):
    """The oracle's problem of one trajectory with its own prior weight."""
    return gn.Problem(w.N, w.T, w.n, w.m, w.dyn, w.meas, w.cpm.D, (w.T / 2) * w.cpm.w,
                      w.cpm.lagrange_matrix(w.t_meas), w.Qw, w.Rw, Pw=Pw_b, meas_static=w.meas_static, **kw)


def _one(w, b, Y):
    """Inputs of trajectory b as a batch of one (U, Y, PAR)."""
    U = w.U if w.U.shape[0] == 1 else w.U[b:b + 1]
    PAR = None if w.PAR is None else (w.PAR if w.PAR.shape[0] == 1 else w.PAR[b:b + 1])
    return U, Y[b:b + 1], PAR


def solve(w, Pw, x0, max_iter, tol, X0=None, Y=None, perturb=None, trace=None, **kw):
    """The per-trajectory oracle: X (B, P, n), cost, iters, status, stacked."""
    X0 = w.X_init if X0 is None else X0
    Y = w.Y if Y is None else Y
    out = []
    for b in range(X0.shape[0]):
        U, Yb, PAR = _one(w, b, Y)
        pb = problem(w, Pw[b], **kw)
        extra = {} if (pb.lb is not None or pb.ub is not None) else {"perturb": perturb}
        tr = None if trace is None else []
        out.append(gn.gauss_newton(pb, X0[b:b + 1], U, Yb, PAR, x0[b:b + 1], max_iter=max_iter, tol=tol,
                                   trace=tr, **extra))
        if trace is not None:
            trace.extend((b, it, a) for _, it, a in tr)
    return tuple(np.concatenate([o[k] for o in out]) for k in range(4))


def normal_equations(w, Pw, x0, X, Y=None):
    """H (B, d, d), g (B, d), cost (B) of the per-trajectory problems at X."""
    Y = w.Y if Y is None else Y
    out = []
    for b in range(X.shape[0]):
        U, Yb, PAR = _one(w, b, Y)
        out.append(gn.normal_equations(problem(w, Pw[b]), X[b:b + 1], U, Yb, PAR, x0[b:b + 1]))
    return tuple(np.concatenate([o[k] for o in out]) for k in range(3))


def sym_inv(C):
    A = np.linalg.inv(C)
    return 0.5 * (A + A.T)


def arrival(w, Pw, x0, X, t, Y=None):
    """(x_ref (B, n), A_ref (B, n, n), C_ref (B, n, n), bound (B,)) at X for the shift time t."""
    Phi = w.cpm.lagrange_matrix(np.asarray([t], dtype=np.float64))
    H, _, _ = normal_equations(w, Pw, x0, X, Y)
    C = cr.cov_from_H(H, Phi, w.n)[:, 0]
    Cp = cr.cov_from_H(gn.perturb_rel(H, tl.SEED_H), Phi, w.n)[:, 0]
    A = np.stack([sym_inv(c) for c in C])
    Ap = np.stack([sym_inv(c) for c in Cp])
    floor = np.abs(Ap - A).reshape(A.shape[0], -1).max(axis=1)
    bound = tl.FLOOR_MULT * floor + 1e-12 * np.abs(A).reshape(A.shape[0], -1).max(axis=1)
    x = np.stack([w.cpm.evaluateSolution(t, list(X[b])) for b in range(X.shape[0])])
    return x, A, C, bound


def x_bound(w, X, t):
    """4 eps sum_j |phi_j X_j| per trajectory and component: the rounding of the ordered sum."""
    phi = w.cpm.lagrange_matrix(np.asarray([t], dtype=np.float64))[0]
    return 4.0 * tl.EPS * np.einsum("j,bjc->bc", np.abs(phi), np.abs(X))
