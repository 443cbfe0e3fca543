"""Reference for the covariance of mixed-row and bordered problems (mhe_kkt_cov) -- TEST
INFRASTRUCTURE (imports oracle/).

Unknowns v = [vec(X) node-major ; z], information H = J^T W J over all of them
(oracle.gn_general.normal_equations_full), equality rows C v = r (constraint_rows).  The
covariance of the estimate under the rows is the leading (d + nz) block of

    inv([[H, C^T], [C, 0]])

formed densely with numpy -- independent of the device's Cholesky + Schur-complement route.
A variable with an all-zero row of H and no constraint is held by the solve
(gn_general.kkt_step's rule) and removed from the system here; its own row and column of
the result are NaN.  The x blocks are the diagonal n x n blocks of S (.) S^T with
S = phi(t) (x) I_n (cov_reference.selector); the z block is the trailing nz x nz block.

Tolerance, the rule of cov_reference.py: floor = the change of the reference when H moves by
gn.perturb_rel(H, tolerance.SEED_H) (C is exact: +-1 / 0), and

    bound = FLOOR_MULT * floor + 1e-12 * max|ref|          (x blocks and z block apart)
"""
import numpy as np

from oracle import gn
from oracle import gn_general as gg

import cov_reference as cr
import tolerance as tl


def kkt_inverse_block(H, C):
    """(d + nz, d + nz): the unknowns' block of inv([[H, C^T], [C, 0]]); held variables NaN."""
    D, K = H.shape[0], C.shape[0]
    free = ~((np.abs(H).sum(1) == 0.0) & (np.abs(C).sum(0) == 0.0))
    nf = int(free.sum())
    A = np.zeros((nf + K, nf + K))
    A[:nf, :nf] = H[np.ix_(free, free)]
    A[:nf, nf:] = C[:, free].T
    A[nf:, :nf] = C[:, free]
    inv = np.linalg.inv(A)[:nf, :nf]
    out = np.full((D, D), np.nan)
    out[np.ix_(free, free)] = inv
    return out


def _blocks(H, C, Phi, n, d):
    S = cr.selector(Phi, n)
    Tq = S.shape[0] // n
    B, nz = H.shape[0], H.shape[1] - d
    cov = np.empty((B, Tq, n, n))
    covz = np.empty((B, nz, nz))
    for b in range(B):
        V = kkt_inverse_block(H[b], C)
        assert np.all(np.isfinite(V[:d, :d])), "a state unknown was held"
        full = S @ V[:d, :d] @ S.T
        for q in range(Tq):
            cov[b, q] = full[q * n:(q + 1) * n, q * n:(q + 1) * n]
        covz[b] = V[d:, d:]
    return cov, covz


def _bound(ref, pert):
    m = np.isfinite(ref)
    assert np.array_equal(m, np.isfinite(pert))
    if not m.any():
        return 0.0
    return tl.FLOOR_MULT * float(np.abs(pert[m] - ref[m]).max()) + 1e-12 * float(np.abs(ref[m]).max())


def kkt_cov_reference(pb, Phi, X, Z, U, Y, PAR, x0=None):
    """cov (B, Tq, n, n), covz (B, nz, nz) at (X, Z) for the basis rows Phi (Tq, P), and
    their bounds (two floats)."""
    B, P, n = X.shape
    d, nz = P * n, pb.n_extra
    H, _, _ = gg.normal_equations_full(pb, X, Z, U, Y, PAR, x0)
    C = gg.constraint_rows(pb, d, nz)
    cov, covz = _blocks(H, C, Phi, n, d)
    covp, covzp = _blocks(gn.perturb_rel(H, tl.SEED_H), C, Phi, n, d)
    return cov, covz, _bound(cov, covp), _bound(covz, covzp)


def query_rows(N, T):
    """Lagrange rows at [0, 0.37 T, T, 0.2 T] (the endpoints are nodes: unit rows)."""
    from oracle import collocation as oc
    return oc.interp_matrix(N, T, np.array([0.0, 0.37 * T, T, 0.2 * T]))
