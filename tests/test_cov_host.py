"""Posterior covariance at query times, the parts that need no GPU: the C entry points'
host-side checks (mhe_state_cov / mhe_cov_scratch_bytes refuse bad arguments before any
launch) and the reference helper tests/cov_reference.py pinned on a linear problem."""
import ctypes

import numpy as np

from mhe import _lib
from nlp.collocation import ChebyshevPseudospectralMethod
from oracle import gn

import cov_reference as cr

ERR_DIMS, ERR_UNSUPPORTED, ERR_NULL = -1, -4, -5
FAKE = ctypes.c_void_p(4096)  # a non-NULL pointer no check dereferences


def _c2_dims(N=100):
    d = _lib.MheDims()
    d.N, d.n, d.m, d.p, d.M, d.q, d.dyn_model, d.meas_model, d.T = N, 2, 1, 2, 101, 0, 5, 1, 10.0
    return d


def _c3_dims():
    d = _lib.MheDims()  # gnss_pos_and_bias + pseudorange, N = 200: the large-system path
    d.N, d.n, d.m, d.p, d.M, d.q, d.dyn_model, d.meas_model, d.T = 200, 5, 3, 1, 2412, 3, 6, 2, 200.0
    for i in range(4):
        d.meas_idx[i] = i
    return d


def _args(batch=1):
    a = _lib.MheSolveArgs()
    a.batch = batch
    a.X0 = a.U = a.Y = a.PAR = a.x0 = FAKE
    return a


def _call(lib, d, a, PhiQ=FAKE, nq=1, cov=FAKE, status=FAKE):
    return lib.mhe_state_cov(d, FAKE, ctypes.byref(a) if a is not None else None, PhiQ, nq, cov, status, None, 0, None)


def test_symbols_exported():
    lib = ctypes.CDLL(_lib.LIB_PATH)
    assert hasattr(lib, "mhe_state_cov") and hasattr(lib, "mhe_cov_scratch_bytes")
    assert {"mhe_state_cov", "mhe_cov_scratch_bytes"} <= set(_lib.SIGNATURES)


def test_state_cov_host_checks_run_before_any_launch():
    lib = _lib.load()
    d = _c2_dims()
    assert _call(lib, d, _args(), PhiQ=None) == ERR_NULL
    assert _call(lib, d, _args(), cov=None) == ERR_NULL
    assert _call(lib, d, _args(), status=None) == ERR_NULL
    assert _call(lib, d, None) == ERR_NULL
    a = _args()
    a.struct_size -= 8  # a stale binding of mhe_solve_args
    assert _call(lib, d, a) == ERR_DIMS
    d.struct_size -= 4  # ... or of mhe_dims
    assert _call(lib, d, _args()) == ERR_DIMS
    d = _c2_dims()
    assert _call(lib, d, _args(), nq=0) == ERR_DIMS
    assert _call(lib, d, _args(), nq=-3) == ERR_DIMS
    assert _call(lib, d, _args(batch=-1)) == ERR_DIMS
    assert _call(lib, d, _args(batch=0)) == 0  # nothing to do, nothing launched
    a = _args()
    a.Rw = FAKE  # per-solve weights with a linear measurement model, as mhe_solve
    assert _call(lib, d, a) == ERR_UNSUPPORTED


def test_state_cov_refuses_bordered_and_mixed_problems():
    lib = _lib.load()
    eq = np.array([[0, 1]], dtype=np.int32)
    d = _c2_dims()
    d.n_eq, d.eq_idx = 1, eq.ctypes.data_as(ctypes.POINTER(ctypes.c_int32))
    assert lib.mhe_padded_dim(d) > 0  # valid dims, only not for this call
    assert _call(lib, d, _args()) == ERR_UNSUPPORTED
    m = _lib.MheDims()
    m.N, m.n, m.m, m.p, m.M, m.q, m.dyn_model, m.meas_model, m.T = 10, 10, 6, 1, 30, 14, 8, 5, 5.0  # mixed rows
    assert lib.mhe_padded_dim(m) > 0
    assert _call(lib, m, _args()) == ERR_UNSUPPORTED
    m.n_extra = 2
    assert lib.mhe_padded_dim(m) > 0
    assert _call(lib, m, _args()) == ERR_UNSUPPORTED


def test_scratch_query():
    lib = _lib.load()
    assert lib.mhe_cov_scratch_bytes(_c2_dims(), 1024, 8) == 0  # register path: the panel lives in LDS
    d = _c3_dims()
    dp = lib.mhe_padded_dim(d)
    assert dp == 5 * 208
    one = lib.mhe_cov_scratch_bytes(d, 1, 1)
    assert one >= 8 * 16 * dp  # one 16-column panel of dp rows
    # 8 queries x 5 components = 40 columns -> three panels per trajectory
    assert lib.mhe_cov_scratch_bytes(d, 4, 8) >= 4 * 8 * 48 * dp
    assert lib.mhe_cov_scratch_bytes(d, 4, 0) == 0
    # the large-system path needs its workspace and the scratch before anything is enqueued
    assert _call(lib, d, _args(batch=2)) == ERR_NULL


def _linear_problem(r_scale=1.0):
    N, T, M = 12, 4.0, 9
    cpm = ChebyshevPseudospectralMethod(N, 0, T)
    t_meas = np.linspace(0.0, T, M)
    Rw = np.broadcast_to(np.array([[25.0]]), (M, 1, 1)).copy()
    Rw[3] *= r_scale
    pb = gn.Problem(N, T, 1, 1, "single_integrator", "full_state", cpm.D, (T / 2) * cpm.w,
                    cpm.lagrange_matrix(t_meas), np.array([[1e3]]), Rw, Pw=np.array([[4.0]]))
    rng = np.random.default_rng(4)
    X = rng.normal(size=(2, N + 1, 1))
    U = rng.normal(size=(2, N + 1, 1))
    Y = rng.normal(size=(2, M, 1))
    x0 = rng.normal(size=(2, 1))
    return pb, cpm, X, U, Y, x0


def test_reference_is_symmetric_spd_and_shrinks_with_information():
    pb, cpm, X, U, Y, x0 = _linear_problem()
    t = cr.query_times(cpm, pb.T)
    C, bound = cr.cov_reference(pb, cpm, t, X, U, Y, None, x0)
    assert C.shape == (2, 4, 1, 1) and 0.0 < bound < 1e-12
    assert np.array_equal(C, np.swapaxes(C, -1, -2))
    assert np.linalg.eigvalsh(C).min() > 0.0
    # linear model: H does not depend on the point or the data
    C2, _ = cr.cov_reference(pb, cpm, t, X + 1.0, U, Y - 2.0, None, x0)
    assert np.abs(C2 - C).max() <= bound
    # against the definition, all query times at once (cross blocks dropped)
    H, _, _ = gn.normal_equations(pb, X, U, Y, None, x0)
    S = cr.selector(cpm.lagrange_matrix(t), pb.n)
    full = S @ np.linalg.solve(H[0], S.T)
    assert np.abs(np.diag(full) - C[0, :, 0, 0]).max() <= bound
    # raising one measurement row's weight shrinks the covariance in the Loewner order
    pb_hi, *_ = _linear_problem(r_scale=10.0)
    H_hi, _, _ = gn.normal_equations(pb_hi, X, U, Y, None, x0)
    diff = S @ (np.linalg.inv(H[0]) - np.linalg.inv(H_hi[0])) @ S.T
    ev = np.linalg.eigvalsh(0.5 * (diff + diff.T))
    print(f"Loewner difference eigenvalues: min {ev.min():.3e} max {ev.max():.3e}")
    assert ev.min() >= -1e-12 * np.abs(full).max() and ev.max() > 0.0
    C_hi, _ = cr.cov_reference(pb_hi, cpm, t, X, U, Y, None, x0)
    assert np.all(C_hi <= C + bound) and np.any(C_hi < C - bound)
