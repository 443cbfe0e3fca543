"""Device parity of the compiled (dynamics, measurement) pairs no other test launches
(registry.COMPILED_PAIRS), against the CPU oracle with the bounds of
tests/tolerance.py.  Every comparison prints the observed error beside its bound.

  (single_integrator_2D, full_state)        n = 2, m = 2: the n == 2 linear L2 instances of k_gn
                                            (build_slots_n2, the trimmed / chained factorization)
                                            with two control columns
  (double_integrator, full_state)           n = 4: the generic table reads of build_tiles' FAST
                                            branch with n dividing 16 and a nonzero Jacobian
  (gnss_pos_and_bias, full_state)           n = 5: the FAST branch with 16 % n != 0, node blocks
                                            across tile edges (the E terms and the clamped index
                                            arithmetic there; this pair's F^T E has the (4, 4)
                                            entry only, a diagonal element of H, so the F^T E
                                            term of off-diagonal tiles reads zeros for it)
  (kinematic_bycicle_and_bias, pseudorange) n = 6 on the register-resident path (C4 itself runs
                                            the large-system path only)
  (kinematic_bycicle_and_bias, mixed), (vehicle_dynamics_and_gnss, mixed): the large-system path
                                            and k_gn_general

Inputs.  Every workload has full (non-diagonal) SPD Q, R and prior weights: a kernel that read
only their diagonals fails.  The linear pairs have linear dynamics and measurements, so a
Gauss-Newton iteration with a wrong H and a right gradient still converges to the optimum: for
them the assembled system and the SINGLE step (max_iter = 1) are the checks that see H.  The
CPU tests at the end of the module show the inputs are not vacuous: with the oracle's own
Jacobian zeroed its single step moves by 1e7 .. 1e9 bounds for n = 4, 5, 6.

The kinematic pair without a prior is singular (x[5] enters no pseudorange and no other
state's dynamics), so every kinematic case carries a prior on node 0.

Bounds: resjac 64 / 16 / 8 / 16 eps per entry (tests/test_gpu_resjac.py); assembled H
<= 1e-12 max|H|, g and cost with the floors (tests/test_gpu_parity.py); iterates after the same
number of iterations at tol 0 <= tolerance.bound, counts and status exact; the Huber instances
as tests/test_gpu_robust.py; covariance blocks with tests/cov_reference.py's bound; the mixed
pairs as tests/test_gpu_general.py / test_gpu_fused_general.py.  The oracle runs on 4
trajectories per case; the two-workgroups-per-CU instance is reached by tiling those four.
"""
import ctypes
import functools
import os
import re

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from mhe import configs, registry, solver  # noqa: E402
from nlp.collocation import ChebyshevPseudospectralMethod  # noqa: E402
from oracle import gn, models  # noqa: E402
from oracle import gn_general as gg  # noqa: E402

import cov_reference as cr  # noqa: E402
import general_problems as gp  # noqa: E402
import tolerance as tl  # noqa: E402

gpu = pytest.mark.gpu
EPS = np.finfo(np.float64).eps
B = 4


# ---------------------------------------------------------------- the pairs and their device tests
_NEW = "tests/test_gpu_pairs.py::"
COVERAGE = {
    ("single_integrator", "full_state"): ["tests/test_gpu_parity.py::test_gn_iterates_match_oracle"],       # c1
    ("single_integrator_2D", "full_state"): [_NEW + "test_solve_matches_oracle", _NEW + "test_assemble_matches_oracle"],
    ("van_der_pol", "full_state"): ["tests/test_gpu_gn_chain.py::test_chain_factorization_matches_oracle"],
    ("gnss_pos_and_bias", "pseudorange"): ["tests/test_gpu_parity.py::test_gn_iterates_match_oracle"],      # gnss_small
    ("gnss_pos_and_bias", "full_state"): [_NEW + "test_solve_matches_oracle", _NEW + "test_assemble_matches_oracle"],
    ("kinematic_bycicle_and_bias", "pseudorange"): [_NEW + "test_solve_matches_oracle",                     # register path
                                                    "tests/test_gpu_configs.py::test_c4_full_shape_matches_oracle"],
    ("double_integrator", "full_state"): [_NEW + "test_solve_matches_oracle", _NEW + "test_assemble_matches_oracle"],
    ("vehicle_dynamics_and_gnss", "vehicle_pseudorange"): ["tests/test_gpu_autocar.py::test_autonomous_car_mhe_matches_oracle"],
    ("van_der_pol", "mixed"): ["tests/test_gpu_general.py::test_mixed_component_rows_equal_fused_full_state_path"],
    ("multi_receiver", "mixed"): ["tests/test_gpu_general.py::test_extra_variables_match_oracle_and_hold_unobservable"],
    ("gnss_two_receiver", "mixed"): ["tests/test_gpu_general.py::test_two_receiver_one_step_matches_kkt_oracle"],
    ("gnss_pos_and_bias", "mixed"): ["tests/test_gpu_meas_huber.py::test_mixed_pseudorange_rows_match_reference"],
    ("kinematic_bycicle_and_bias", "mixed"): [_NEW + "test_mixed_pairs_match_kkt_oracle"],
    ("vehicle_dynamics_and_gnss", "mixed"): [_NEW + "test_mixed_pairs_match_kkt_oracle"],
    ("gnss_eight_receivers", "mixed"): ["tests/test_gpu_configs.py::test_c5_eight_receivers_reduced_matches_oracle"],
}


def test_every_compiled_pair_has_a_device_test():
    """A pair added to registry.COMPILED_PAIRS without a GPU test that launches it fails here,
    on the CPU suite.  Every listed id must name a test function that exists."""
    assert set(COVERAGE) == set(registry.COMPILED_PAIRS)
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    for pair, ids in COVERAGE.items():
        assert ids, pair
        for tid in ids:
            path, name = tid.split("::")
            with open(os.path.join(root, path)) as f:
                src = f.read()
            assert re.search(rf"^def {re.escape(name)}\(", src, re.M), tid
            assert "pytest.mark.gpu" in src, tid


# ---------------------------------------------------------------- workloads
def _controls(m, t):
    """(len(t), m): smooth, nonzero, a different curve per column."""
    t = np.asarray(t, dtype=np.float64)
    return np.stack([0.6 * np.sin(0.5 * t + 0.9 * c) + 0.25 * (c + 1) for c in range(m)], axis=-1)


def make_linear(dyn, P, M, seed=21):
    """A linear pair (dyn, full_state) with P nodes and M measurement times over T = 10: truth by
    RK4 under the controls above, full SPD Q and R (R scaled per row, so a wrong row index in the
    constants' measurement term shows)."""
    _, n, m = registry.DYN[dyn]
    T, N = 10.0, P - 1
    rng = np.random.default_rng(seed)
    x0 = rng.normal(size=(B, n))
    t = np.linspace(0, T, M)
    rhs = lambda tt, x: models.dyn_eval(dyn, x, np.broadcast_to(_controls(m, [tt])[0], (x.shape[0], m)))[0]  # noqa: E731
    xt = configs._rk4(rhs, x0, t)
    R = gp.spd(rng, 0.01 * (1.0 + 0.5 * np.arange(n)))
    Q = gp.spd(rng, 1e-4 * (1.0 + 0.5 * np.arange(n)[::-1]))
    Y = xt + rng.normal(size=(B, M, n)) * np.sqrt(np.diag(R))[None, None, :]
    cpm = ChebyshevPseudospectralMethod(N, 0, T)
    Rw = np.linalg.inv(R)[None] * (1.0 + 0.3 * np.sin(1.3 * np.arange(M)))[:, None, None]
    return configs.Workload(name=f"{dyn}_P{P}_M{M}", N=N, T=T, n=n, m=m, p=n, M=M, B=B, dyn=dyn, meas="full_state",
                            meas_static={}, t_meas=t, Y=Y, U=_controls(m, cpm.tau2t(cpm.tau))[None], PAR=None,
                            Qw=np.linalg.inv(Q), Rw=Rw, Pw=None, x0=None,
                            X_init=configs._init_from_measurements(cpm, t, Y), X_true=xt, cpm=cpm)


def make_kinematic(N, slots, seed=23):
    """configs.make_c4 cut to T = 10 s (11 epochs) with N + 1 nodes, the first ``slots`` of the
    12 satellite slots of every epoch, and a full SPD prior on node 0 with a perturbed mean."""
    w = configs.make_c4(B=B, N=N, T=10.0)
    keep = np.arange(w.M) % 12 < slots
    w.t_meas, w.Y, w.PAR, w.Rw = w.t_meas[keep], w.Y[:, keep], w.PAR[:, keep], w.Rw[keep]
    w.M = int(keep.sum())
    rng = np.random.default_rng(seed)
    w.Qw = np.linalg.inv(gp.spd(rng, [1, 1, 0.001, .01, .01, 1]))
    w.Pw = np.linalg.inv(gp.spd(rng, [4, 4, 0.01, 4, 0.01, 0.04]))
    w.x0 = w.X_true[:, 0] + rng.normal(size=(B, 6)) * np.array([1.0, 1.0, 0.05, 1.0, 0.05, 0.1])
    w.name = f"kinematic_N{N}_M{w.M}"
    return w


SI2, DI, GPB = "single_integrator_2D", "double_integrator", "gnss_pos_and_bias"
WORKLOADS = {
    # name: (builder, padded system size 16 NT)
    "si2d_P17_M16": (lambda: make_linear(SI2, 17, 16), 48),
    "si2d_P104_M101": (lambda: make_linear(SI2, 104, 101), 208),     # NT 13, no padding
    "di_P5_M7": (lambda: make_linear(DI, 5, 7), 32),                 # one tile edge, padding
    "di_P17_M16": (lambda: make_linear(DI, 17, 16), 80),             # d = 68: a node block ends on every tile edge
    "di_P52_M40": (lambda: make_linear(DI, 52, 40), 208),
    "gpb_P4_M6": (lambda: make_linear(GPB, 4, 6), 32),               # d = 20: the first straddling block
    "gpb_P7_M9": (lambda: make_linear(GPB, 7, 9), 48),               # d = 35
    "gpb_P16_M16": (lambda: make_linear(GPB, 16, 16), 80),           # d = 80 = 5 tiles, blocks still straddle
    "gpb_P41_M33": (lambda: make_linear(GPB, 41, 33), 208),          # d = 205
    "kin_N4_M132": (lambda: make_kinematic(4, 12), 32),              # M > 128: the un-fused row pass
    "kin_N10_M88": (lambda: make_kinematic(10, 8), 80),              # M <= 128: node and row pass fused
    "kin_N10_M132": (lambda: make_kinematic(10, 12), 80),
    "kin_N33_M132": (lambda: make_kinematic(33, 12), 208),           # d = 204
}
# the small-batch instance's LDS layout (U block rows double-buffered) does not hold NT = 13 tiles
# beside 132 per-row 6 x 6 blocks: launch_gn then runs the two-workgroups-per-CU instance at any batch
NO_SMALL_BATCH_INSTANCE = {"kin_N33_M132"}
LINEAR = [k for k in WORKLOADS if not k.startswith("kin")]
ONE_PER_PAIR = ["si2d_P17_M16", "di_P17_M16", "gpb_P7_M9", "kin_N10_M88"]


class Case:
    def __init__(self, name):
        build, self.dp = WORKLOADS[name]
        self.name, self.w = name, build()
        self._solvers, self._refs = {}, {}

    def pb(self, **kw):
        w = self.w
        return gn.Problem(w.N, w.T, w.n, w.m, w.dyn, w.meas, w.cpm.D, (w.T / 2) * w.cpm.w,
                          w.cpm.lagrange_matrix(w.t_meas), w.Qw, w.Rw, Pw=w.Pw, meas_static=w.meas_static, **kw)

    @property
    def U(self):
        return np.broadcast_to(self.w.U, (B,) + self.w.U.shape[1:])

    @property
    def PAR(self):
        return None if self.w.PAR is None else np.broadcast_to(self.w.PAR, (B,) + self.w.PAR.shape[1:])

    def solver(self, **kw):
        key = tuple(sorted(kw.items()))
        if key not in self._solvers:
            self._solvers[key] = solver.from_workload(self.w, **kw)
        return self._solvers[key]

    def ref(self, iters, **kw):
        """The oracle's iterate after ``iters`` iterations at tol 0 with its floors:
        (X, cost, iters, status, floor_X, floor_cost) -- computed once per case."""
        key = (iters,) + tuple(sorted(kw.items()))
        if key not in self._refs:
            w, pb = self.w, self.pb(**kw)
            run = lambda Y, pt=None: gn.gauss_newton(pb, w.X_init, self.U, Y, self.PAR, w.x0, max_iter=iters,  # noqa: E731
                                                     tol=0.0, perturb=pt)
            fx, fc = tl.floor(lambda Y, pt: run(Y, pt)[:2], w.Y)
            self._refs[key] = run(w.Y) + (fx, fc)
        return self._refs[key]


@functools.lru_cache(maxsize=None)
def case(name):
    return Case(name)


def _np(out):
    return [t.cpu().numpy() for t in out]


def _kernel_name(s, batch):
    buf = ctypes.create_string_buffer(256)
    st = torch.cuda.current_stream()
    assert s.lib.mhe_solve_kernel_name(s.dims, batch, ctypes.c_void_p(st.cuda_stream), buf, 256) == 0
    return buf.value.decode()


# ---------------------------------------------------------------- residuals and Jacobians
@gpu
@pytest.mark.parametrize("name", sorted(WORKLOADS))
def test_resjac_matches_oracle(name):
    c = case(name)
    w, pb, s = c.w, c.pb(), c.solver()
    assert not s.large_system and s.dp == c.dp
    W, F, E, Hm = _np(s.resjac(w.X_init, w.U, w.Y, w.PAR))
    f, Fr = models.dyn_eval(w.dyn, w.X_init, c.U)
    Wr = pb.alpha * np.einsum("kj,bja->bka", pb.D, w.X_init) - f
    scale_W = pb.alpha * np.einsum("kj,bja->bka", np.abs(pb.D), np.abs(w.X_init)) + np.abs(f)
    xi = np.einsum("ij,bja->bia", pb.Phi, w.X_init)
    h, Hr = models.meas_eval(w.meas, xi, c.PAR, w.meas_static)
    live = ~gn.masked_rows(pb.Rw[None])[0]      # R = 0 slots: h undefined there
    Er = w.Y - h
    dW = (np.abs(W - Wr) / scale_W.clip(1e-300)).max()
    dF = np.abs(F - Fr).max() / max(1.0, np.abs(Fr).max())
    dE = (np.abs(E - Er) / (np.abs(w.Y) + np.abs(h)).clip(1e-300))[:, live].max()
    dH = np.abs(Hm - Hr)[:, live].max() / max(1.0, np.abs(Hr).max())
    print(f"{name}: W {dW / EPS:.1f} eps, F {dF / EPS:.1f} eps, e {dE / EPS:.1f} eps, "
          f"H {dH / EPS:.1f} eps (relative to each entry's scale)")
    assert dW <= 64 * EPS and dF <= 16 * EPS and dE <= 8 * EPS and dH <= 16 * EPS


# ---------------------------------------------------------------- the assembled system
@gpu
@pytest.mark.parametrize("name", sorted(WORKLOADS))
def test_assemble_matches_oracle(name):
    c = case(name)
    w, pb, s = c.w, c.pb(), c.solver()
    H, g, cost = _np(s.assemble(w.X_init, w.U, w.Y, w.PAR, w.x0))
    run = lambda Y: gn.normal_equations(pb, w.X_init, c.U, Y, c.PAR, w.x0)  # noqa: E731
    Hr, gr, cr_ = run(w.Y)
    _, fg, fc = tl.floor(lambda Y, pt: run(Y), w.Y, conditioning=False)
    d = pb.d
    assert np.abs(Hr - np.swapaxes(Hr, 1, 2)).max() <= 1e-12 * np.abs(Hr).max()
    tl.check(f"{name} H", np.abs(H[:, :d, :d] - Hr).max(), 1e-12 * np.abs(Hr).max())
    tl.check(f"{name} g", np.abs(g[:, :d] - gr).max(), tl.FLOOR_MULT * fg + 1e-12 * np.abs(gr).max())
    tl.check(f"{name} cost", np.abs(cost - cr_).max(), tl.FLOOR_MULT * fc + 1e-12 * np.abs(cr_).max())
    assert s.dp == c.dp
    if s.dp > d:  # padding: identity block, zero coupling, zero gradient
        assert np.array_equal(H[:, d:, d:], np.broadcast_to(np.eye(s.dp - d), H[:, d:, d:].shape))
        assert not H[:, :d, d:].any() and not H[:, d:, :d].any() and not g[:, d:].any()


# ---------------------------------------------------------------- Gauss-Newton iterates
@gpu
@pytest.mark.parametrize("batch", ["small_batch", "two_per_cu"])
@pytest.mark.parametrize("iters", [1, 3])
@pytest.mark.parametrize("name", sorted(WORKLOADS))
def test_solve_matches_oracle(name, iters, batch):
    """One step (the only solve of a linear pair that depends on H) and three, in a batch of 4
    (the small-batch instance where its LDS layout fits) and tiled to CUs + 8 (the
    two-workgroups-per-CU instance; every copy bitwise its source)."""
    c = case(name)
    w, s = c.w, c.solver()
    assert not s.large_system
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    rep = np.arange(B) if batch == "small_batch" else np.arange(cus + 8) % B
    kname = _kernel_name(s, rep.size)
    print(kname)
    assert kname.startswith("mhe::k_gn<")
    if batch == "small_batch" and name not in NO_SMALL_BATCH_INSTANCE:
        assert "SB=true" in kname
    else:
        assert "two workgroups per CU" in kname and "SB=true" not in kname
    x0 = None if w.x0 is None else w.x0[rep]
    X, cost, it, status = _np(s.solve(w.X_init[rep], w.U, w.Y[rep], w.PAR, x0=x0, max_iter=iters, tol=0.0))
    for a in (X, cost, it, status):
        assert np.array_equal(a, a[:B][rep])
    Xr, cr_, ir, sr, fx, fc = c.ref(iters)
    assert it[:B].tolist() == ir.tolist() == [iters] * B
    assert status[:B].tolist() == sr.tolist() == [1] * B
    unit = " m" if name.startswith("kin") else ""
    tl.check(f"{name} {iters} it {batch} X", np.abs(X[:B] - Xr).max(), tl.bound(fx, Xr), unit)
    tl.check(f"{name} {iters} it {batch} cost", np.abs(cost[:B] - cr_).max(), tl.FLOOR_MULT * fc + 1e-10 * np.abs(cr_).max())


@gpu
@pytest.mark.parametrize("name", ONE_PER_PAIR)
def test_large_system_path_matches_oracle(name):
    """k_big_* of these pairs (force_large) on the same workload and bound."""
    c = case(name)
    w, s = c.w, c.solver(force_large=True)
    assert s.large_system
    assert _kernel_name(s, B).startswith("large-system path")
    X, cost, it, status = _np(s.solve(w.X_init, w.U, w.Y, w.PAR, x0=w.x0, max_iter=3, tol=0.0))
    Xr, cr_, ir, sr, fx, fc = c.ref(3)
    assert it.tolist() == ir.tolist() == [3] * B and status.tolist() == sr.tolist() == [1] * B
    tl.check(f"{name} large path X", np.abs(X - Xr).max(), tl.bound(fx, Xr))
    tl.check(f"{name} large path cost", np.abs(cost - cr_).max(), tl.FLOOR_MULT * fc + 1e-10 * np.abs(cr_).max())


# ---------------------------------------------------------------- pseudo-Huber dynamics cost
# scale of the pseudo-Huber dynamics cost per case: between the node residuals of X_init (the
# measurement interpolant's defects), so that some weights are in the linear regime and some
# are not -- asserted on the oracle's weights below
HUBER = {"di_P17_M16": 0.15, "gpb_P16_M16": 0.15}


def _huber_weights(c, delta):
    pb = c.pb(dyn_cost="huber", delta=delta)
    W = gn.residuals(pb, c.w.X_init, c.U, c.w.Y, c.PAR, c.w.x0)[0]
    lam, _ = gn.huber_weights(pb, W)
    return lam / np.diag(pb.Qw)            # 1 / sqrt(1 + W^2 / delta^2): < 1 / sqrt 2 beyond delta


@pytest.mark.parametrize("name", sorted(HUBER))
def test_huber_scale_splits_the_node_residuals(name):
    rel = _huber_weights(case(name), HUBER[name])
    beyond = (rel < np.sqrt(0.5)).mean()
    print(f"{name}: {beyond:.2f} of the node residuals beyond delta, weights {rel.min():.3f} .. {rel.max():.3f}")
    assert 0.1 <= beyond <= 0.9


@gpu
@pytest.mark.parametrize("name", sorted(HUBER))
def test_huber_instances_match_oracle(name):
    """dyn_cost = huber: the linear pairs leave the FAST branch for h_element (n = 4, n = 5)."""
    c = case(name)
    w, delta = c.w, HUBER[name]
    s = c.solver(dyn_cost="huber", huber_delta=delta)
    assert not s.large_system and "HUBER=1" in _kernel_name(s, B)
    pb = c.pb(dyn_cost="huber", delta=delta)
    H, g, cost = _np(s.assemble(w.X_init, w.U, w.Y))
    Hr, gr, cr_ = gn.normal_equations(pb, w.X_init, c.U, w.Y)
    d = pb.d
    tl.check(f"{name} huber H", np.abs(H[:, :d, :d] - Hr).max(), 1e-12 * np.abs(Hr).max())
    tl.check(f"{name} huber g", np.abs(g[:, :d] - gr).max(), 1e-12 * np.abs(gr).max())
    tl.check(f"{name} huber cost", np.abs(cost / cr_ - 1.0).max(), 1e-12)
    X, cost, it, status = _np(s.solve(w.X_init, w.U, w.Y, max_iter=5, tol=0.0))
    Xr, cr_, ir, sr = gn.gauss_newton(pb, w.X_init, c.U, w.Y, max_iter=5, tol=0.0)
    assert status.tolist() == sr.tolist() and it.tolist() == ir.tolist() == [5] * B
    tl.check(f"{name} huber X", np.abs(X - Xr).max(), 1e-9 * (1 + np.abs(Xr).max()))
    tl.check(f"{name} huber cost after 5", np.abs(cost / cr_ - 1.0).max(), 1e-9)
    # not the L2 iterate: the weights are read
    assert np.abs(Xr - c.ref(3)[0]).max() > 1e-6


# ---------------------------------------------------------------- covariance
@gpu
@pytest.mark.parametrize("name", ONE_PER_PAIR + ["gpb_P41_M33"])   # d = 205: three queries per 16-column panel
def test_covariance_matches_oracle(name):
    c = case(name)
    w, s = c.w, c.solver()
    X = c.ref(3)[0]
    t = np.array([0.0, 0.37 * w.T])     # node 0 and an interior time that is no node
    assert np.abs(w.cpm.tau2t(w.cpm.tau) - t[1]).min() > 1e-3
    Cr, bound = cr.cov_reference(c.pb(), w.cpm, t, X, c.U, w.Y, c.PAR, w.x0)
    cov, status = s.covariance(X, w.U, w.Y, w.PAR, w.x0, t=t)
    assert np.all(status.cpu().numpy() == 0)
    cr.check_blocks(f"cov {name}", cov.cpu().numpy(), Cr, bound)


# ---------------------------------------------------------------- the two mixed pairs
MIXED = {"kinematic": gp.kinematic_mixed_problem, "vehicle": gp.vehicle_mixed_problem}
MIXED_ITERS = 2


@functools.lru_cache(maxsize=None)
def mixed_case(name, with_eq):
    pb, X0, U, Y, PAR, x0, _ = MIXED[name](B=B, with_eq=with_eq)
    run = lambda Yv, pt=None: gg.gauss_newton_general(pb, X0, None, U, Yv, PAR, x0, max_iter=MIXED_ITERS, tol=0.0,  # noqa: E731
                                                      perturb=pt)
    Xr, _, cr_, ir, sr = run(Y)
    fx, fc = tl.floor(lambda Yv, pt: (lambda r: (r[0], r[2]))(run(Yv, pt)), Y)
    return (pb, X0, U, Y, PAR, x0), (Xr, cr_, ir, sr, fx, fc)


@pytest.mark.parametrize("with_eq", [False, True], ids=["free", "eq"])
@pytest.mark.parametrize("name", sorted(MIXED))
def test_mixed_inputs_are_well_posed(name, with_eq):
    """The conditions the comparison below rests on, on the oracle alone: it reaches status 1,
    cond(H) <= 1e8 at the initial iterate and its bound is below 1e-6."""
    (pb, X0, U, Y, PAR, x0), (Xr, cr_, ir, sr, fx, fc) = mixed_case(name, with_eq)
    H = gg.normal_equations_full(pb, X0, None, U, Y, PAR, x0)[0]
    cond = max(np.linalg.cond(h) for h in H)
    print(f"{name} eq={with_eq}: cond(H) {cond:.2e}, bound {tl.bound(fx, Xr):.2e}")
    assert sr.tolist() == [1] * B and ir.tolist() == [MIXED_ITERS] * B
    assert cond <= 1e8 and tl.bound(fx, Xr) < 1e-6
    if name == "vehicle":
        assert X0[:, :, 3].min() > 5.0 and Xr[:, :, 3].min() > 5.0     # far from the pole at vx = -0.001


@gpu
@pytest.mark.parametrize("path", ["large", "fused"])
@pytest.mark.parametrize("with_eq", [False, True], ids=["free", "eq"])
@pytest.mark.parametrize("name", sorted(MIXED))
def test_mixed_pairs_match_kkt_oracle(name, with_eq, path):
    (pb, X0, U, Y, PAR, x0), (Xr, cr_, ir, sr, fx, fc) = mixed_case(name, with_eq)
    dyn_par = None if pb.dyn_par is None else registry.dyn_params(pb.dyn, {"car_params": pb.dyn_par})
    s = solver.BatchSolver(pb.N, pb.T, pb.dyn, "mixed", pb.D, pb.c, pb.Phi, pb.Qw, pb.Rw, Pw=pb.Pw,
                           eq=pb.eq if pb.eq.size else None, dyn_par=dyn_par, fused_general=path == "fused")
    kname = _kernel_name(s, B)
    print(kname)
    if path == "fused":
        assert s.fused_general and not s.large_system and kname.startswith("k_gn_general")
    else:
        assert s.large_system and kname.startswith("large-system path")
    X, cost, it, status = _np(s.solve(X0, U, Y, PAR, x0, max_iter=MIXED_ITERS, tol=0.0))
    assert it.tolist() == ir.tolist() == [MIXED_ITERS] * B and status.tolist() == sr.tolist()
    tag = f"{name} {'eq' if with_eq else 'free'} {path}"
    tl.check(f"{tag} X", np.abs(X - Xr).max(), tl.bound(fx, Xr), " m")
    tl.check(f"{tag} cost", np.abs(cost - cr_).max(), tl.FLOOR_MULT * fc + 1e-10 * np.abs(cr_).max())
    v = X.reshape(B, -1)
    for a, b in pb.eq:
        assert np.abs(v[:, a] - v[:, b]).max() <= 1e-9 * (1 + np.abs(X).max())
    if with_eq:  # the rows bind: the free problem's iterate does not satisfy them
        vf = mixed_case(name, False)[1][0].reshape(B, -1)
        assert max(np.abs(vf[:, a] - vf[:, b]).max() for a, b in pb.eq) > 1e-6


# ---------------------------------------------------------------- the inputs see the Jacobian
SENSITIVITY = {"si2d_P17_M16": False, "di_P17_M16": True, "gpb_P7_M9": True, "gpb_P41_M33": True, "kin_N10_M88": True}


@pytest.mark.parametrize("name", sorted(SENSITIVITY))
def test_single_step_depends_on_the_dynamics_jacobian(name, monkeypatch):
    """With the oracle's F = df/dx zeroed (f kept: the gradient loses its F^T term too) its
    single step moves by many bounds for n = 4, 5, 6, and not at all for single_integrator_2D,
    whose F is zero: the one-step comparison above is not vacuous."""
    c = case(name)
    w, pb = c.w, c.pb()
    Xr, _, _, _, fx, _ = c.ref(1)
    real = models.dyn_eval
    monkeypatch.setattr(models, "dyn_eval", lambda *a, **k: (lambda f, F: (f, np.zeros_like(F)))(*real(*a, **k)))
    X0 = gn.gauss_newton(pb, w.X_init, c.U, w.Y, c.PAR, w.x0, max_iter=1, tol=0.0)[0]
    change, bound = np.abs(X0 - Xr).max(), tl.bound(fx, Xr)
    print(f"{name}: single step with F = 0 moves by {change:.3e}, bound {bound:.3e}")
    if SENSITIVITY[name]:
        assert change > 1e3 * bound     # an error a thousandth of a dropped Jacobian still fails the comparison
    else:
        assert change == 0.0
