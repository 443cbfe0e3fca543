"""Covariance and arrival cost of mixed-row / bordered problems (ABI v11), the parts that need
no GPU: mhe_kkt_cov / mhe_kkt_arrival / mhe_kkt_cov_scratch_bytes refuse bad arguments before
any launch, in the order tests/test_cov_host.py pins for mhe_state_cov, and the reference
helper tests/kkt_cov_reference.py pinned against the definition on a small problem."""
import ctypes
import os

import numpy as np

from mhe import _lib
from oracle import gn_general as gg

import cov_reference as cr
import kkt_cov_reference as kr
from general_problems import multi_receiver_problem, two_receiver_problem

ERR_DIMS, ERR_UNSUPPORTED, ERR_NULL = -1, -4, -5
FAKE = ctypes.c_void_p(4096)  # a non-NULL pointer no check dereferences


def _c2_dims(N=100):
    d = _lib.MheDims()
    d.N, d.n, d.m, d.p, d.M, d.q, d.dyn_model, d.meas_model, d.T = N, 2, 1, 2, 101, 0, 5, 1, 10.0
    return d


def _mixed_dims(n_eq=0, n_extra=0):
    """gnss_two_receiver + mixed rows, N = 10 (tests/test_abi.py's general dims); the returned
    array keeps the equality table alive."""
    d = _lib.MheDims()
    d.N, d.n, d.m, d.p, d.M, d.q, d.dyn_model, d.meas_model, d.T = 10, 10, 6, 1, 30, 14, 8, 5, 5.0
    eq = np.array([[j * 10 + 2, j * 10 + 7] for j in range(n_eq)], dtype=np.int32).reshape(-1, 2)
    d.n_eq, d.n_extra = n_eq, n_extra
    if n_eq:
        d.eq_idx = eq.ctypes.data_as(ctypes.POINTER(ctypes.c_int32))
    return d, eq


def _args(batch=1, z=False):
    a = _lib.MheSolveArgs()
    a.batch = batch
    a.X0 = a.U = a.Y = a.PAR = a.x0 = FAKE
    if z:
        a.Z0 = FAKE
    return a


def _cov(lib, d, a, PhiQ=FAKE, nq=1, cov=FAKE, covz=None, status=FAKE):
    return lib.mhe_kkt_cov(d, FAKE, ctypes.byref(a) if a is not None else None, PhiQ, nq, cov, covz, status, None, 0,
                           None)


def _arr(lib, d, a, phi=FAKE, x=FAKE, Pw=FAKE, status=FAKE):
    return lib.mhe_kkt_arrival(d, FAKE, ctypes.byref(a) if a is not None else None, phi, x, Pw, None, status, None, 0,
                               None)


def test_symbols_exported():
    lib = ctypes.CDLL(_lib.LIB_PATH)
    names = {"mhe_kkt_cov", "mhe_kkt_arrival", "mhe_kkt_cov_scratch_bytes"}
    for name in names:
        assert hasattr(lib, name), name
    assert names <= set(_lib.SIGNATURES)
    src = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "mhe.h")).read()
    assert "#define MHE_ABI_VERSION 11" in src


def test_kkt_cov_host_checks_run_before_any_launch():
    lib = _lib.load()
    for d in (_c2_dims(), _mixed_dims(n_eq=11)[0]):  # the forwarded call and the general one alike
        assert _cov(lib, d, _args(), PhiQ=None) == ERR_NULL
        assert _cov(lib, d, _args(), cov=None) == ERR_NULL
        assert _cov(lib, d, _args(), status=None) == ERR_NULL
        assert _cov(lib, d, None) == ERR_NULL
        a = _args()
        a.struct_size -= 8  # a stale binding of mhe_solve_args
        assert _cov(lib, d, a) == ERR_DIMS
        assert _cov(lib, d, _args(), nq=0) == ERR_DIMS
        assert _cov(lib, d, _args(), nq=-3) == ERR_DIMS
        assert _cov(lib, d, _args(batch=-1)) == ERR_DIMS
        assert _cov(lib, d, _args(batch=0)) == 0  # nothing to do, nothing launched
        d.struct_size -= 4  # a stale binding of mhe_dims
        assert _cov(lib, d, _args()) == ERR_DIMS
    a = _args()
    a.Rw = FAKE  # per-solve weights with a linear measurement model, as mhe_solve
    assert _cov(lib, _c2_dims(), a) == ERR_UNSUPPORTED


def test_general_dims_are_accepted_up_to_the_workspace():
    """What mhe_state_cov refuses (tests/test_cov_host.py) passes every check here until the
    missing workspace / scratch: MHE_ERR_NULL, not MHE_ERR_UNSUPPORTED."""
    lib = _lib.load()
    for n_eq, n_extra in ((0, 0), (11, 0), (0, 3), (11, 2)):
        d, _eq = _mixed_dims(n_eq, n_extra)
        assert lib.mhe_padded_dim(d) == 160
        a = _args(z=True)
        assert lib.mhe_state_cov(d, FAKE, ctypes.byref(a), FAKE, 1, FAKE, FAKE, None, 0, None) == ERR_UNSUPPORTED
        assert _cov(lib, d, a) == ERR_NULL  # no workspace
    d, _eq = _mixed_dims(0, 3)
    assert _cov(lib, d, _args(z=False)) == ERR_NULL  # Z0 missing with n_extra > 0
    ws = lib.mhe_workspace_bytes(d, 2)
    a = _args(batch=2, z=True)
    a.workspace, a.workspace_bytes = FAKE, ws
    need = lib.mhe_kkt_cov_scratch_bytes(d, 2, 4)
    assert need > 0
    # a scratch smaller than the query's answer is refused on the host
    assert lib.mhe_kkt_cov(d, FAKE, ctypes.byref(a), FAKE, 4, FAKE, None, FAKE, FAKE, need - 8, None) == ERR_NULL
    assert lib.mhe_kkt_cov(d, FAKE, ctypes.byref(a), FAKE, 4, FAKE, None, FAKE, None, need, None) == ERR_NULL


def test_kkt_arrival_refusals():
    lib = _lib.load()
    d, _eq = _mixed_dims(n_eq=11)
    assert _arr(lib, d, _args()) == ERR_UNSUPPORTED  # rank-deficient block: no inverse
    d, _eq = _mixed_dims(n_eq=1, n_extra=2)
    assert _arr(lib, d, _args(z=True)) == ERR_UNSUPPORTED
    d, _eq = _mixed_dims()
    assert _arr(lib, d, _args(), phi=None) == ERR_NULL
    assert _arr(lib, d, _args(), x=None) == ERR_NULL
    assert _arr(lib, d, _args(), Pw=None) == ERR_NULL
    assert _arr(lib, d, _args(), status=None) == ERR_NULL
    assert _arr(lib, d, None) == ERR_NULL
    a = _args()
    a.struct_size -= 8
    assert _arr(lib, d, a) == ERR_DIMS
    assert _arr(lib, d, _args(batch=-1)) == ERR_DIMS
    assert _arr(lib, d, _args(batch=0)) == 0
    assert _arr(lib, d, _args()) == ERR_NULL  # no workspace
    d, _eq = _mixed_dims(n_extra=3)
    assert _arr(lib, d, _args(z=False)) == ERR_NULL  # Z0 missing


def test_scratch_query():
    lib = _lib.load()
    assert lib.mhe_kkt_cov_scratch_bytes(_c2_dims(), 1024, 8) == 0  # forwarded: the register path
    for n_eq, n_extra in ((0, 0), (11, 0), (0, 3)):
        d, _eq = _mixed_dims(n_eq, n_extra)
        dp = lib.mhe_padded_dim(d)
        assert dp == 160
        for B, nq in ((1, 1), (2, 4), (3, 5)):
            cols = -(-nq * 10 // 16) * 16  # ceil(n_query n / 16) 16-column panels
            assert lib.mhe_kkt_cov_scratch_bytes(d, B, nq) >= 8 * B * cols * dp
        assert lib.mhe_kkt_cov_scratch_bytes(d, 4, 0) == 0
        assert lib.mhe_kkt_cov_scratch_bytes(d, -1, 1) == 0


# ---------------------------------------------------------------- the reference helper
def test_reference_matches_the_definition_and_the_elimination():
    """kkt_cov_reference on the two-receiver problem: symmetric, positive semi-definite with
    an exact null direction per equality row, equal to the unconstrained covariance's
    projection  P - P C^T (C P C^T)^-1 C P  (the textbook constrained-estimate covariance),
    and to cov_reference's formula without rows."""
    pb, X0, U, Y, PAR, x0, _ = two_receiver_problem(N=6)
    X, _, _, _, st = gg.gauss_newton_general(pb, X0, None, U, Y, PAR, x0, max_iter=30)
    assert np.all(st == 0)
    Phi = kr.query_rows(pb.N, pb.T)
    cov, covz, bx, bz = kr.kkt_cov_reference(pb, Phi, X, None, U, Y, PAR, x0)
    assert cov.shape == (2, 4, 10, 10) and covz.shape == (2, 0, 0) and 0.0 < bx < 1e-10 and bz == 0.0
    assert np.abs(cov - np.swapaxes(cov, -1, -2)).max() <= bx
    assert np.linalg.eigvalsh(0.5 * (cov + np.swapaxes(cov, -1, -2))).min() >= -bx
    var = cov[:, :, 2, 2] + cov[:, :, 7, 7] - 2 * cov[:, :, 2, 7]
    assert np.abs(var).max() <= 4 * bx
    d = pb.P * pb.n
    H, _, _ = gg.normal_equations_full(pb, X, None, U, Y, PAR, x0)
    C = gg.constraint_rows(pb, d, 0)
    S = cr.selector(Phi, pb.n)
    for b in range(2):
        Pm = np.linalg.inv(H[b])
        proj = Pm - Pm @ C.T @ np.linalg.solve(C @ Pm @ C.T, C @ Pm)
        full = S @ proj @ S.T
        for q in range(4):
            assert np.abs(full[q * 10:(q + 1) * 10, q * 10:(q + 1) * 10] - cov[b, q]).max() <= bx
    # without the rows: cov_reference's S inv(H) S^T, and a larger covariance
    pb0, *_ = two_receiver_problem(N=6, with_eq=False)
    cov0, _, b0, _ = kr.kkt_cov_reference(pb0, Phi, X, None, U, Y, PAR, x0)
    assert np.abs(cov0 - cr.cov_from_H(H, Phi, pb.n)).max() <= b0
    assert np.abs(cov0 - cov).max() > 100 * (bx + b0)


def test_reference_holds_an_unobserved_extra_variable():
    pb, X0, Z0, U, Y, PAR, _, _ = multi_receiver_problem(N=7)
    X, Z, _, _, st = gg.gauss_newton_general(pb, X0, Z0, U, Y, PAR, None, max_iter=30)
    assert np.all(st == 0)
    Phi = kr.query_rows(pb.N, pb.T)
    cov, covz, bx, bz = kr.kkt_cov_reference(pb, Phi, X, Z, U, Y, PAR, None)
    assert np.all(np.isfinite(cov)) and bx > 0.0 and bz > 0.0
    assert np.all(np.isnan(covz[:, 2, :])) and np.all(np.isnan(covz[:, :, 2]))
    zz = covz[:, :2, :2]
    assert np.all(np.isfinite(zz)) and np.linalg.eigvalsh(zz).min() > 0.0  # a covariance: positive definite
    # the z block is the Schur complement's inverse of the observed unknowns
    d = pb.P * pb.n
    H, _, _ = gg.normal_equations_full(pb, X, Z, U, Y, PAR, None)
    for b in range(2):
        Hf = H[b][:d + 2, :d + 2]
        assert np.abs(np.linalg.inv(Hf)[d:, d:] - zz[b]).max() <= bz
