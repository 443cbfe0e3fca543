"""Per-solve prior weight and arrival cost (ABI v10), the parts that need no GPU: the new
fields and symbols, the entry points' host-side refusals (all before any launch), the host
wrapper's validation of ``Pw`` and the facade's engine key."""
import ctypes

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from mhe import _lib, solver  # noqa: E402

ERR_DIMS, ERR_UNSUPPORTED, ERR_NULL = -1, -4, -5
FAKE = ctypes.c_void_p(4096)  # a non-NULL pointer no check dereferences


def _c2_dims(N=100, has_prior=1):
    d = _lib.MheDims()
    d.N, d.n, d.m, d.p, d.M, d.q, d.dyn_model, d.meas_model, d.T = N, 2, 1, 2, 101, 0, 5, 1, 10.0
    d.has_prior = has_prior
    return d


def _gnss_dims(has_prior=1):
    d = _lib.MheDims()  # gnss_pos_and_bias + pseudorange, N = 10 (gnss_small)
    d.N, d.n, d.m, d.p, d.M, d.q, d.dyn_model, d.meas_model, d.T = 10, 5, 3, 1, 408, 3, 6, 2, 50.0
    for i in range(4):
        d.meas_idx[i] = i
    d.has_prior = has_prior
    return d


def _args(batch=1):
    a = _lib.MheSolveArgs()
    a.batch = batch
    a.X0 = a.X_out = a.U = a.Y = a.PAR = a.x0 = a.cost_out = a.iters_out = a.status_out = FAKE
    a.max_iter = 1
    return a


def _arrival(lib, d, a, phi=FAKE, x_arr=FAKE, Pw_arr=FAKE, cov=None, status=FAKE, scratch=None, sb=0):
    return lib.mhe_arrival(d, FAKE, ctypes.byref(a) if a is not None else None, phi, x_arr, Pw_arr, cov, status,
                           scratch, sb, None)


def _calls(lib, d, a):
    r = ctypes.byref(a)
    return {"mhe_solve": lib.mhe_solve(d, FAKE, r, None),
            "mhe_state_cov": lib.mhe_state_cov(d, FAKE, r, FAKE, 1, FAKE, FAKE, None, 0, None),
            "mhe_assemble_at": lib.mhe_assemble_at(d, FAKE, r, FAKE, FAKE, FAKE, FAKE, None),
            "mhe_arrival": _arrival(lib, d, a)}


def test_symbols_and_fields():
    lib = ctypes.CDLL(_lib.LIB_PATH)
    assert hasattr(lib, "mhe_arrival") and hasattr(lib, "mhe_arrival_scratch_bytes")
    assert {"mhe_arrival", "mhe_arrival_scratch_bytes"} <= set(_lib.SIGNATURES)
    names = [f[0] for f in _lib.MheSolveArgs._fields_]
    i = names.index("Rw")  # beside the other per-solve weight, each pointer followed by its stride
    assert names[i:i + 4] == ["Rw", "rw_bstride", "Pw", "pw_bstride"] and names.count("Pw") == 1
    assert _lib.MheSolveArgs.Pw.size == 8 and _lib.MheSolveArgs.pw_bstride.size == 8
    a = _lib.MheSolveArgs()
    assert a.struct_size == ctypes.sizeof(a) and not a.Pw and a.pw_bstride == 0
    # the library's own sizeof: a struct of this size passes the check, and only this size
    assert _calls(_lib.load(), _c2_dims(), _args(batch=0)) == dict.fromkeys(
        ("mhe_solve", "mhe_state_cov", "mhe_assemble_at", "mhe_arrival"), 0)


def test_stale_v9_solve_args_are_refused():
    """A binding that declares the v9 struct (without Pw / pw_bstride: 16 bytes shorter) is
    refused before any later field is read, by every call that takes it."""
    lib = _lib.load()
    for d in (_c2_dims(), _gnss_dims()):
        a = _args()
        a.struct_size -= 16
        assert _calls(lib, d, a) == dict.fromkeys(("mhe_solve", "mhe_state_cov", "mhe_assemble_at", "mhe_arrival"),
                                                  ERR_DIMS)


def test_pw_needs_a_prior():
    lib = _lib.load()
    for d in (_c2_dims(has_prior=0), _gnss_dims(has_prior=0)):
        a = _args()
        a.Pw, a.pw_bstride = FAKE, d.n * d.n
        assert _calls(lib, d, a) == dict.fromkeys(("mhe_solve", "mhe_state_cov", "mhe_assemble_at", "mhe_arrival"),
                                                  ERR_UNSUPPORTED)


def test_arrival_refusals_and_scratch():
    lib = _lib.load()
    d = _c2_dims()
    assert _arrival(lib, d, _args(), phi=None) == ERR_NULL
    assert _arrival(lib, d, _args(), x_arr=None) == ERR_NULL
    assert _arrival(lib, d, _args(), Pw_arr=None) == ERR_NULL
    assert _arrival(lib, d, _args(), status=None) == ERR_NULL
    assert _arrival(lib, d, None) == ERR_NULL
    assert _arrival(lib, d, _args(batch=-1)) == ERR_DIMS
    assert _arrival(lib, d, _args(batch=0)) == 0  # nothing to do, nothing launched
    # bordered and mixed problems
    eq = np.array([[0, 1]], dtype=np.int32)
    e = _c2_dims()
    e.n_eq, e.eq_idx = 1, eq.ctypes.data_as(ctypes.POINTER(ctypes.c_int32))
    assert lib.mhe_padded_dim(e) > 0 and _arrival(lib, e, _args()) == ERR_UNSUPPORTED
    m = _lib.MheDims()
    m.N, m.n, m.m, m.p, m.M, m.q, m.dyn_model, m.meas_model, m.T = 10, 10, 6, 1, 30, 14, 8, 5, 5.0  # mixed rows
    m.has_prior = 1
    assert lib.mhe_padded_dim(m) > 0 and _arrival(lib, m, _args()) == ERR_UNSUPPORTED
    m.n_extra = 2
    assert lib.mhe_padded_dim(m) > 0 and _arrival(lib, m, _args()) == ERR_UNSUPPORTED
    # register-resident path with n > 16: gnss_8_receivers (n = 40), N = 3 -> d = 160 <= 208
    r = _lib.MheDims()
    r.N, r.n, r.m, r.p, r.M, r.q, r.dyn_model, r.meas_model, r.T = 3, 40, 24, 40, 4, 0, 11, 1, 2.0
    r.has_prior = 1
    if lib.mhe_padded_dim(r) > 0 and lib.mhe_workspace_bytes(r, 1) == 0:  # this build has the pair, on that path
        assert _arrival(lib, r, _args()) == ERR_UNSUPPORTED
    # scratch: none on the register path, the single query's panel on the large-system path
    assert lib.mhe_arrival_scratch_bytes(d, 1024) == 0
    big = _c2_dims()
    big.force_large = 1
    sb = lib.mhe_arrival_scratch_bytes(big, 3)
    assert sb > 0 and sb == lib.mhe_cov_scratch_bytes(big, 3, 1)
    a = _args(batch=3)
    assert _arrival(lib, big, a, scratch=FAKE, sb=sb) == ERR_NULL  # no workspace
    a.workspace, a.workspace_bytes = FAKE, lib.mhe_workspace_bytes(big, 3)
    assert _arrival(lib, big, a, scratch=FAKE, sb=sb - 8) == ERR_NULL  # short scratch
    assert _arrival(lib, big, a, scratch=None, sb=sb) == ERR_NULL


def _shell(n=2, has_prior=1):
    """A BatchSolver with only what the argument checks read (no device)."""
    s = solver.BatchSolver.__new__(solver.BatchSolver)
    s.device, s.n = torch.device("cpu"), n
    s.dims = _lib.MheDims()
    s.dims.has_prior = has_prior
    return s


def test_host_wrapper_validates_pw():
    s = _shell()
    ok = np.array([[2.0, 0.5], [0.5, 3.0]])
    t, stride = s._pw(ok, 4)
    assert t.shape == (1, 2, 2) and stride == 0 and t.dtype == torch.float64
    t, stride = s._pw(np.broadcast_to(ok, (4, 2, 2)).copy(), 4)
    assert t.shape == (4, 2, 2) and stride == 4
    t, stride = s._pw(torch.as_tensor(ok)[None], 4)
    assert t.shape == (1, 2, 2) and stride == 0
    assert s._pw(None, 4) == (None, 0)
    with pytest.raises(ValueError):
        s._pw(np.array([[2.0, 0.5], [0.5000000001, 3.0]]), 4)   # asymmetric
    bad = np.broadcast_to(ok, (4, 2, 2)).copy()
    bad[2, 0, 1] += 1e-15
    with pytest.raises(ValueError):
        s._pw(bad, 4)                                            # one asymmetric block of a batch
    with pytest.raises(ValueError):
        s._pw(ok.astype(np.float32), 4)                          # float64 only
    with pytest.raises(ValueError):
        s._pw(np.eye(3), 4)                                      # (n, n)
    with pytest.raises(ValueError):
        s._pw(np.broadcast_to(ok, (3, 2, 2)).copy(), 4)          # (B|1, n, n)
    with pytest.raises(ValueError):
        s._pw(ok.ravel(), 4)
    with pytest.raises(ValueError):
        _shell(has_prior=0)._pw(ok, 4)                           # needs a prior
    # the NaN block of a failed arrival passes (that trajectory stays NaN), as the kernels expect
    nanb = np.broadcast_to(ok, (4, 2, 2)).copy()
    nanb[1] = np.nan
    assert s._pw(nanb, 4)[1] == 4


def test_facade_parameter_prior_weight_is_not_in_the_engine_key(monkeypatch):
    """A Parameter-valued "Q" of addInitialCost travels per solve: re-setting it builds no new
    engine, the engine's constants carry a zero prior weight, and the resolved value is what
    the solve passes.  An ndarray "Q" stays in the constants (and in the key)."""
    import nlp.cost_functions as cost_functions
    import nlp.dynamics as dynamics
    import nlp.measurements as measurements
    import nlp.nlp as nlp
    built = []

    class Stub:
        def __init__(self, *a, Pw=None, **kw):
            built.append(None if Pw is None else np.array(Pw, copy=True))

    monkeypatch.setattr(solver, "BatchSolver", Stub)

    def make(q):
        N, T, n, m = 8, 2.0, 2, 1
        problem = nlp.fixedTimeOptimalEstimationNLP(N, T, n, m)
        X = problem.addVariables(N + 1, n, name="x")
        problem.addDynamics(dynamics.van_der_pol, X, None, None)
        problem.addDynamicsCost(cost_functions.weighted_l2_norm, None, {"Q": np.eye(n)})
        par = problem.addParameter(1, n * n)[0] if q is None else None
        problem.addInitialCost(cost_functions.weighted_l2_norm, X[0], {"Q": par if q is None else q}, x0=np.zeros(n))
        t_meas = np.linspace(0.0, T, 9)
        problem.addResidualCost(measurements.full_state, X, t_meas, np.zeros((n, 9)), np.eye(n))
        return problem, par

    problem, par = make(None)
    A = np.array([[2.0, 0.5], [0.5, 3.0]])
    problem.setParameter(par, A)
    problem._build()
    problem.setParameter(par, 7.0 * A)
    problem._build()
    assert problem.engine_builds == 1 and len(built) == 1
    assert built[0].shape == (2, 2) and not built[0].any()
    assert np.array_equal(problem._Pw_solve, 7.0 * A)
    problem.setParameter(par, np.array([[2.0, 0.5], [0.25, 3.0]]))
    with pytest.raises(ValueError):
        problem._build()  # asymmetric
    # an ndarray weight keeps today's route
    problem, _ = make(A)
    problem._build()
    assert problem.engine_builds == 1 and np.array_equal(np.asarray(built[-1]).reshape(2, 2), A)
    assert problem._Pw_solve is None
