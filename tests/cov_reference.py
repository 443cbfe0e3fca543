"""Reference for the posterior covariance at query times -- TEST INFRASTRUCTURE (imports oracle/).

The estimation objective is r^T W r, so H = J^T W J at a point X (oracle.gn.normal_equations)
is the information matrix of the whole trajectory; with S = phi(t) (x) I_n, the Lagrange rows
extractSolution evaluates the state with,

    C_ref[q] = S_q inv(H) S_q^T                                   (n x n per query time)

formed with numpy.  The tolerance follows tests/tolerance.py: floor_H is the change of C_ref
when every entry of H moves by eps of its magnitude (oracle.gn.perturb_rel, seed
tolerance.SEED_H) -- the backward error of ANY evaluation order of H's sums, amplified by
cond(H) -- and

    bound = FLOOR_MULT * floor_H + 1e-12 * max|C_ref|
"""
import numpy as np

from oracle import gn

import tolerance as tl


def selector(Phi, n):
    """S = phi (x) I_n: (Tq n, P n), row q n + c picks component c of x(t_q)."""
    return np.kron(np.asarray(Phi, dtype=np.float64), np.eye(n))


def cov_from_H(H, Phi, n):
    """(B, Tq, n, n): the diagonal n x n blocks of S inv(H) S^T for each H (B, d, d)."""
    S = selector(Phi, n)
    Tq = S.shape[0] // n
    out = np.empty((H.shape[0], Tq, n, n))
    for b in range(H.shape[0]):
        C = S @ np.linalg.inv(H[b]) @ S.T
        for q in range(Tq):
            out[b, q] = C[q * n:(q + 1) * n, q * n:(q + 1) * n]
    return out


def cov_reference(pb, cpm, t, X, U, Y, PAR=None, x0=None):
    """C_ref (B, Tq, n, n) at X for the query times t, and its bound (a float)."""
    H, _, _ = gn.normal_equations(pb, X, U, Y, PAR, x0)
    Phi = cpm.lagrange_matrix(np.asarray(t, dtype=np.float64).reshape(-1))
    C = cov_from_H(H, Phi, pb.n)
    floor_H = float(np.abs(cov_from_H(gn.perturb_rel(H, tl.SEED_H), Phi, pb.n) - C).max())
    return C, tl.FLOOR_MULT * floor_H + 1e-12 * float(np.abs(C).max())


def query_times(cpm, T):
    """[0, 0.37 T, T] and one interior node time (the endpoints are nodes: phi is a unit row)."""
    nodes = cpm.tau2t(cpm.tau)
    return np.array([0.0, 0.37 * T, T, float(nodes[len(nodes) // 2])])


def check_blocks(name, C, Cref, bound):
    """Error, symmetry and definiteness of every block; prints each figure beside the bound."""
    tl.check(name, float(np.abs(C - Cref).max()), bound)
    tl.check(name + " symmetry", float(np.abs(C - np.swapaxes(C, -1, -2)).max()), bound)
    emin = float(np.linalg.eigvalsh(0.5 * (C + np.swapaxes(C, -1, -2))).min())
    print(f"{name}: smallest eigenvalue {emin:.3e}")
    assert emin > 0.0, name
