"""mhe_dims.force_large = MHE_PATH_FUSED_GENERAL (2): the host-side answers that follow from
dims alone -- path selection, sizes, the kernel's name and the refusals -- without a GPU.

Fused-general dims: mixed rows (with or without extra variables / equality rows), L2 dynamics
cost, no bounds, n <= 16, node-major padded system <= 208 and an LDS layout that fits.  For
every other dims the value 2 must answer as 0 does, and 0 / 1 as they always did."""
import ctypes
import os

import pytest

from mhe import _lib, registry

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MIXED = registry.MEAS["mixed"][0]
UNSUPPORTED = -4


def _dims(dyn, N, M, meas="mixed", n_eq=0, n_extra=0, path=0, keep=None):
    did, n, m = registry.DYN[dyn]
    mid, p, q, _ = registry.MEAS[meas]
    d = _lib.MheDims()
    d.N, d.n, d.m, d.p, d.M, d.q = N, n, m, (n if p is None else p), M, q
    d.dyn_model, d.meas_model, d.T = did, mid, 5.0
    d.n_extra, d.force_large = n_extra, path
    if n_eq:
        pairs = (ctypes.c_int32 * (2 * n_eq))(*[v for j in range(n_eq) for v in (j * n + 2, j * n + 7)])
        d.n_eq, d.eq_idx = n_eq, ctypes.cast(pairs, ctypes.POINTER(ctypes.c_int32))
        keep.append(pairs)
    return d


def _answers(lib, d):
    buf = ctypes.create_string_buffer(256)
    rc = lib.mhe_solve_kernel_name(d, 1024, None, buf, 256)
    return (lib.mhe_padded_dim(d), lib.mhe_kkt_dim(d), lib.mhe_workspace_bytes(d, 3), lib.mhe_const_bytes(d),
            rc, buf.value.decode())


def _two_rx(path, keep):
    return _dims("gnss_two_receiver", 10, 222, n_eq=11, path=path, keep=keep)  # gnss-multi-receiver.py's window


def test_header_names_the_path_values():
    src = open(os.path.join(ROOT, "include", "mhe.h")).read()
    for line in ("#define MHE_PATH_AUTO 0", "#define MHE_PATH_LARGE 1", "#define MHE_PATH_FUSED_GENERAL 2",
                 "#define MHE_HAS_FUSED_GENERAL 1"):
        assert line in src
    assert (_lib.PATH_AUTO, _lib.PATH_LARGE, _lib.PATH_FUSED_GENERAL) == (0, 1, 2)


def test_two_receiver_dims_take_the_fused_kernel():
    lib, keep = _lib.load(), []
    d = _two_rx(2, keep)
    dp, dk, ws, cb, rc, name = _answers(lib, d)
    assert dp == 112            # 16 ceil(11 * 10 / 16), node-major (the large path pads to 10 * 16)
    assert dk == 123            # + K = 11 equality rows
    assert ws == 0
    assert cb > 0
    assert rc == 0 and name.startswith("k_gn_general")
    # refused before any launch (no pointer is looked at, no device touched)
    assert lib.mhe_kkt_cov(d, None, None, None, 1, None, None, None, None, 0, None) == UNSUPPORTED
    assert lib.mhe_kkt_arrival(d, None, None, None, None, None, None, None, None, 0, None) == UNSUPPORTED
    assert lib.mhe_chol_solve_ws(d, None, 1, None, None, None, None, None, 0, None) == UNSUPPORTED
    assert lib.mhe_resjac(d, None, 1, None, None, 0, None, None, 0, None, None, None, None, None) == UNSUPPORTED
    g = _lib.MheSolveArgs()
    g.batch, g.meas_delta = 1, ctypes.c_void_p(256)   # never dereferenced: refused on the host
    g.X0 = g.X_out = g.cost_out = g.iters_out = g.status_out = g.Y = g.U = g.PAR = ctypes.c_void_p(256)
    assert lib.mhe_solve(d, ctypes.c_void_p(256), ctypes.byref(g), None) == UNSUPPORTED


def test_two_receiver_dims_with_0_or_1_answer_as_before():
    lib, keep = _lib.load(), []
    a0, a1 = _answers(lib, _two_rx(0, keep)), _answers(lib, _two_rx(1, keep))
    assert a0 == a1                                   # a general problem is on the large path either way
    dp, dk, ws, cb, rc, name = a0
    assert dp == 160 and dk == 171 and ws > 0 and rc == 0
    assert name.startswith("large-system path")
    assert cb != _answers(lib, _two_rx(2, keep))[3]   # another constants layout


def test_extra_variables_without_equality_rows_are_fused_general_too():
    lib = _lib.load()
    d = _dims("multi_receiver", 7, 91, n_extra=3, path=2)
    dp, dk, ws, _, rc, name = _answers(lib, d)
    assert (dp, dk, ws, rc) == (64, 67, 0, 0) and name.startswith("k_gn_general")
    assert lib.mhe_kkt_arrival(d, None, None, None, None, None, None, None, None, 0, None) == UNSUPPORTED


@pytest.mark.parametrize("case", ["n40", "N40_n8", "huber", "bounds", "typed_c2", "typed_eq"])
def test_fallback_dims_answer_as_value_0(case):
    """Dims the fused kernel does not take: the preference is ignored."""
    lib, keep = _lib.load(), []

    def make(path):
        if case == "n40":           # beyond the 16-column panel
            return _dims("gnss_eight_receivers", 10, 120, path=path)
        if case == "N40_n8":        # P n = 328 > 208
            return _dims("multi_receiver", 40, 91, n_extra=3, path=path)
        if case == "huber":
            d = _two_rx(path, keep)
            d.dyn_cost, d.huber_delta = 1, 0.5
            return d
        if case == "bounds":
            d = _dims("gnss_two_receiver", 10, 222, path=path)
            d.n_bounds, d.bound_idx[0], d.bound_lb[0], d.bound_ub[0] = 1, 0, -1.0, 1.0
            return d
        if case == "typed_c2":      # C2: the register-resident kernel, typed rows
            return _dims("van_der_pol", 100, 101, meas="full_state", path=path)
        d = _dims("van_der_pol", 12, 13, meas="full_state", path=path)   # typed rows under equality rows
        pairs = (ctypes.c_int32 * 4)(0, 1, 4, 5)
        keep.append(pairs)
        d.n_eq, d.eq_idx = 2, ctypes.cast(pairs, ctypes.POINTER(ctypes.c_int32))
        return d

    a0, a2 = _answers(lib, make(0)), _answers(lib, make(2))
    assert a0[0] > 0 and a0 == a2
    assert not a2[5].startswith("k_gn_general")
    if case == "typed_c2":
        assert a2[0] == 208 and a2[2] == 0 and "k_gn<" in a2[5]
    else:
        assert a2[2] > 0 and a2[5].startswith("large-system path")


def test_solver_refuses_both_preferences():
    """fused_general and force_large are one field: exclusive (checked before any device use).
    (On the parent the keyword is unknown: TypeError.)"""
    from mhe import solver
    with pytest.raises(ValueError, match="exclusive"):
        solver.BatchSolver(10, 5.0, "gnss_two_receiver", "mixed", None, None, None, None, None,
                           fused_general=True, force_large=True)


def test_facade_attribute_defaults_off():
    from nlp import nlp as nlpmod
    problem = nlpmod.fixedTimeOptimalEstimationNLP(4, 1.0, 2, 1)
    assert problem.fused_general is False and problem.max_iter == 50
