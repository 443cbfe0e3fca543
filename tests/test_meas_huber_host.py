"""Pseudo-Huber measurement rows (ABI v9), the parts that need no GPU: the C entry points'
host-side checks (a stale v8 mhe_solve_args, meas_delta on a linear model), the host
wrapper's and the facade's validation, and the reference helper
tests/meas_huber_reference.py pinned against a finite-difference gradient and against the
oracle's quadratic Gauss-Newton."""
import ctypes

import numpy as np
import pytest
import torch

import nlp.cost_functions as cost_functions
import nlp.dynamics as dynamics
import nlp.measurements as measurements
import nlp.nlp as nlp
from mhe import _lib, configs, solver
from oracle import gn

import meas_huber_reference as mh

ERR_DIMS, ERR_UNSUPPORTED = -1, -4
FAKE = ctypes.c_void_p(4096)  # a non-NULL pointer no check dereferences


def _full_state_dims(N=100):
    d = _lib.MheDims()  # van der Pol + full_state (C2): linear measurement model, p = 2
    d.N, d.n, d.m, d.p, d.M, d.q, d.dyn_model, d.meas_model, d.T = N, 2, 1, 2, 101, 0, 5, 1, 10.0
    return d


def _pseudorange_dims():
    d = _lib.MheDims()  # gnss_pos_and_bias + pseudorange, N = 10: the register path
    d.N, d.n, d.m, d.p, d.M, d.q, d.dyn_model, d.meas_model, d.T = 10, 5, 3, 1, 408, 3, 6, 2, 50.0
    for i in range(4):
        d.meas_idx[i] = i
    return d


def _args(batch=1):
    a = _lib.MheSolveArgs()
    a.batch = batch
    a.X0 = a.X_out = a.U = a.Y = a.PAR = a.x0 = a.cost_out = a.iters_out = a.status_out = FAKE
    a.max_iter = 1
    return a


def _calls(lib, d, a):
    r = ctypes.byref(a)
    return {"mhe_solve": lib.mhe_solve(d, FAKE, r, None),
            "mhe_state_cov": lib.mhe_state_cov(d, FAKE, r, FAKE, 1, FAKE, FAKE, None, 0, None),
            "mhe_assemble_at": lib.mhe_assemble_at(d, FAKE, r, FAKE, FAKE, FAKE, FAKE, None)}


def test_abi_v9_fields_and_entry_point():
    lib = ctypes.CDLL(_lib.LIB_PATH)
    assert hasattr(lib, "mhe_assemble_at") and "mhe_assemble_at" in _lib.SIGNATURES
    names = [f[0] for f in _lib.MheSolveArgs._fields_]
    assert names[-3:] == ["lambda_out", "meas_delta", "md_bstride"]
    a = _lib.MheSolveArgs()
    assert a.struct_size == ctypes.sizeof(a) and not a.meas_delta and a.md_bstride == 0


def test_stale_v8_solve_args_are_refused():
    """A binding that declares the v8 struct (without meas_delta / md_bstride: 16 bytes
    shorter) is refused before any later field is read, by every call that takes it."""
    lib = _lib.load()
    for d in (_full_state_dims(), _pseudorange_dims()):
        a = _args()
        a.struct_size -= 16
        assert _calls(lib, d, a) == {"mhe_solve": ERR_DIMS, "mhe_state_cov": ERR_DIMS, "mhe_assemble_at": ERR_DIMS}
    assert lib.mhe_assemble_at(_pseudorange_dims(), FAKE, None, FAKE, FAKE, FAKE, FAKE, None) == -5  # MHE_ERR_NULL


def test_linear_model_refuses_meas_delta():
    """full_state folds R into the constants (k_build_cc): no per-row reweighting, as for Rw."""
    lib = _lib.load()
    a = _args()
    a.meas_delta = FAKE
    assert _calls(lib, _full_state_dims(), a) == {"mhe_solve": ERR_UNSUPPORTED, "mhe_state_cov": ERR_UNSUPPORTED,
                                                  "mhe_assemble_at": ERR_UNSUPPORTED}
    a = _args()
    a.Rw = FAKE  # the kernel-level view of per-solve Rw follows the same rule
    assert lib.mhe_assemble_at(_full_state_dims(), FAKE, ctypes.byref(a), FAKE, FAKE, FAKE, FAKE, None) == ERR_UNSUPPORTED


def _shell(M=6, p=1, linear=False):
    """A BatchSolver with only what the argument checks read (no device)."""
    s = solver.BatchSolver.__new__(solver.BatchSolver)
    s.device, s.M, s.p, s.linear_meas, s.meas_name = torch.device("cpu"), M, p, linear, "pseudorange"
    return s


def test_host_wrapper_validates_meas_delta():
    s = _shell()
    ok = np.array([15.0, np.inf, 1e-3, 2.0, 3.0, 4.0])
    t, stride = s._md(ok, 4)
    assert t.shape == (1, 6) and stride == 0 and t.dtype == torch.float64
    t, stride = s._md(np.broadcast_to(ok, (4, 6)).copy(), 4)
    assert t.shape == (4, 6) and stride == 6
    assert s._md(None, 4) == (None, 0)
    for bad in (0.0, -1.0, np.nan, -np.inf):
        v = ok.copy()
        v[2] = bad
        with pytest.raises(ValueError):
            s._md(v, 4)
    with pytest.raises(ValueError):
        s._md(ok.astype(np.float32), 4)          # float64 only
    with pytest.raises(ValueError):
        s._md(ok[:5], 4)                         # (M,)
    with pytest.raises(ValueError):
        s._md(np.broadcast_to(ok, (3, 6)).copy(), 4)  # (B|1, M)
    with pytest.raises(ValueError):
        _shell(linear=True, p=2)._md(ok, 4)      # full_state, as _rw
    with pytest.raises(ValueError):
        _shell(linear=True, p=2)._rw(np.ones((6, 2, 2)), 4)


def _gnss_problem(w, cost_function=None, cost_params=None):
    problem = nlp.fixedTimeOptimalEstimationNLP(w.N, w.T, 5, 3)
    X = problem.addVariables(w.N + 1, 5, name="x")
    _, W = problem.addDynamics(dynamics.gnss_pos_and_bias, X, np.array([0.0, w.T]), np.zeros((3, 2)))
    problem.addDynamicsCost(cost_functions.weighted_l2_norm, W, {"Q": w.Qw})
    kw = {} if cost_function is None else dict(cost_function=cost_function, cost_params=cost_params)
    for i, t in enumerate(w.t_meas[:3]):
        problem.addResidualCost(measurements.pseudorange, X, np.array([[t]]), np.array([[w.Y[0, i, 0]]]),
                                np.array([[w.Rw[i, 0, 0]]]), {"sat_pos": w.PAR[0, i]}, **kw)
    return problem


def test_facade_validation():
    w = configs.make_gnss_small(B=1, N=6, epochs=9, n_sat=6)
    p = _gnss_problem(w, cost_functions.pseudo_huber_loss, {"delta": 15.0})
    assert [g["delta"] for g in p._meas] == [15.0] * 3
    assert [g["delta"] for g in _gnss_problem(w)._meas] == [np.inf] * 3
    with pytest.raises(nlp.UnsupportedFeature):   # R is the weight
        _gnss_problem(w, cost_functions.pseudo_huber_loss, {"Q": np.eye(1), "delta": 15.0})
    with pytest.raises(nlp.UnsupportedFeature):   # no other cost on the rows
        _gnss_problem(w, cost_functions.weighted_l2_norm, {"Q": np.eye(1)})
    with pytest.raises(ValueError):
        _gnss_problem(w, cost_functions.pseudo_huber_loss, {"delta": 0.0})
    with pytest.raises(TypeError):                # keyword-only: the positional signature is the reference's
        p.addResidualCost(measurements.pseudorange, None, np.array([[0.0]]), np.array([[1.0]]), np.eye(1),
                          {"sat_pos": w.PAR[0, 0]}, cost_functions.pseudo_huber_loss)


def test_facade_refuses_pure_full_state():
    w = configs.make_c1()
    problem = nlp.fixedTimeOptimalEstimationNLP(w.N, w.T, w.n, w.m)
    X = problem.addVariables(w.N + 1, w.n, name="x")
    _, W = problem.addDynamics(dynamics.single_integrator, X, w.t_meas, np.sin(w.t_meas)[None, :])
    problem.addDynamicsCost(cost_functions.weighted_l2_norm, W, {"Q": w.Qw})
    problem.addResidualCost(measurements.full_state, X, w.t_meas, w.Y[0].T, w.Rw[0],
                            cost_function=cost_functions.pseudo_huber_loss, cost_params={"delta": 0.5})
    with pytest.raises(nlp.UnsupportedFeature, match="COMPONENT"):
        problem.build()


# ---------------------------------------------------------------- the reference helper
def _small():
    w = configs.make_gnss_small(B=4, N=6, epochs=9, n_sat=6)
    pb = gn.Problem(w.N, w.T, w.n, w.m, w.dyn, w.meas, w.cpm.D, (w.T / 2) * w.cpm.w,
                    w.cpm.lagrange_matrix(w.t_meas), w.Qw, w.Rw, meas_static=w.meas_static)
    U = np.broadcast_to(w.U, (w.B,) + w.U.shape[1:])
    PAR = np.broadcast_to(w.PAR, (w.B,) + w.PAR.shape[1:])
    Y, out = mh.with_outliers(w.Y)
    assert 0 < out.sum() < out.size // 4
    return w, pb, U, PAR, Y


def test_reference_gradient_is_half_the_finite_difference_of_the_robust_cost():
    w, pb, U, PAR, Y = _small()
    X = w.X_init
    _, g, c = mh.normal_equations(pb, X, U, Y, PAR, mh.DELTA)
    assert np.array_equal(c, mh.cost(pb, X, U, Y, PAR, mh.DELTA))
    # five-point central differences: truncation O(h^4); the cost's rounding (eps |y| |R e| ~ 1e-8,
    # pseudoranges of 2e7 m) enters as ~1.5 * 1e-8 / h, ~1e-7 of max|g| ~ 3 at h = 4 cm
    h = 4e-2
    fd = np.zeros_like(g)
    for k in range(g.shape[1]):
        E = np.zeros(g.shape[1])
        E[k] = h
        E = E.reshape(1, w.P, w.n)
        f = lambda a: mh.cost(pb, X + a * E, U, Y, PAR, mh.DELTA)  # noqa: E731
        fd[:, k] = (-f(2.0) + 8.0 * f(1.0) - 8.0 * f(-1.0) + f(-2.0)) / (12.0 * h)
    err = np.abs(0.5 * fd - g).max(axis=1) / np.abs(g).max(axis=1)
    print(f"finite-difference gradient: relative error {err}")
    assert np.all(err <= 1e-6)


def test_reference_with_huge_delta_is_the_quadratic_gauss_newton():
    w, pb, U, PAR, Y = _small()
    Xq, cq, iq, sq = gn.gauss_newton(pb, w.X_init, U, Y, PAR, max_iter=40, tol=1e-10)
    for dl in (1e12, np.inf):
        X, c, it, st = mh.gauss_newton(pb, w.X_init, U, Y, PAR, dl, max_iter=40, tol=1e-10)
        assert it.tolist() == iq.tolist() and st.tolist() == sq.tolist() == [0] * w.B
        err = np.abs(X - Xq).max()
        print(f"delta {dl:g}: max |X - X_quadratic| {err:.3e}, cost {np.abs(c - cq).max():.3e}")
        assert err <= 1e-9 * (1.0 + np.abs(Xq).max()) and np.allclose(c, cq, rtol=1e-12)
    # the robust fit is not the quadratic one, and IRLS decreases the robust cost monotonically
    costs = [mh.cost(pb, w.X_init, U, Y, PAR, mh.DELTA)]
    for it in range(1, 8):
        costs.append(mh.gauss_newton(pb, w.X_init, U, Y, PAR, mh.DELTA, max_iter=it, tol=0.0)[1])
    assert np.all(np.diff(np.stack(costs), axis=0) <= 1e-12 * np.abs(costs[0]))
    Xr = mh.gauss_newton(pb, w.X_init, U, Y, PAR, mh.DELTA, max_iter=40, tol=1e-10)[0]
    assert np.all(mh.position_error(w, Xr) < mh.position_error(w, Xq))
