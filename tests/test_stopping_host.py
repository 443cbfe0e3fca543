"""The oracle side of the stopping-rule tests (no GPU): every batch of tests/stopping_cases.py
meets its guard -- the band of 2 around every decision, the rounding floor a hundredth of the
threshold, the spread of iteration counts, step length 1 on the bounded traces -- and the
expected counts can fail: restatements of the rule that leave out an entry, a component or the
extra variables, or that take max|X| before the update, give other counts on the same inputs.
"""
import numpy as np
import pytest

import stopping_cases as sc

# distinct iteration counts a batch must hold; DESIGN.md §8 says why two cases hold fewer than 4
SPREAD = {"c2": 4, "c2_large20": 4, "c2_pw": 4, "c2_huber": 2, "gnss_small": 2, "c2_bounded": 2,
          "two_receiver": 3, "multi_receiver": 3}


def _report(c):
    margin, share = c.guard()
    print(f"{c.name}: iterations {c.ref[3].tolist()}, nearest ratio a factor {2.0 ** margin:.2f} from 1, "
          f"8 floor = {share:.1e} of the threshold")


@pytest.mark.parametrize("name", sc.BLENDED)
def test_blended_batch_meets_its_guard(name):
    c = sc.blended(name)
    assert c.min_counts == SPREAD[name] and c.tol == sc.TOL
    _report(c)
    assert len(set(c.ref[3].tolist())) >= SPREAD[name]
    assert c.ref[3].max() < c.max_iter


def test_large_path_batch_has_early_and_late_stoppers_in_both_halves():
    it = sc.blended("c2_large20").ref[3]
    assert it.size == 20
    for half in (it[:16], it[16:]):  # the two streams of the split factorization
        assert half.min() == 1 and half.max() >= 5, half


@pytest.mark.parametrize("name", [n for n in sc.BLENDED if n != "c2_bounded"])
def test_trace_restates_the_oracle(name):
    c = sc.blended(name)
    X, Z, it, st, ratios = c.trace()
    Xr, Zr, _, ir, sr = c.ref
    assert it.tolist() == ir.tolist() and st.tolist() == sr.tolist()
    assert np.abs(X - Xr).max() <= 1e-12 * (1.0 + np.abs(Xr).max())
    if Z is not None:
        assert np.abs(Z - Zr).max() <= 1e-12 * (1.0 + np.abs(Zr).max())


def test_bounded_trace_has_unit_steps_only():
    c = sc.blended("c2_bounded")
    assert len(c.alphas) == int(c.ref[3].sum()) and set(c.alphas) == {1.0}
    X = c.ref[0]
    assert (X[:, :, 1] == 0.5).any(), "the bound should be active at the solution"


@pytest.mark.parametrize("name", sorted(sc.ENTRY_SHAPES))
def test_displaced_entry_batch_meets_its_guard(name):
    c, ent = sc.displaced(name)
    _report(c)
    assert c.tol == sc.TOL_ENTRY and c.ref[3].tolist() == sc.displaced_counts(ent)
    d = c.X0[0].size
    assert {0, d - 1} <= set(ent) and all(e in ent for e in (63, 64, 127, 128, 191, 192, 255, 256) if e < d)
    # the first step of a displaced trajectory is the displacement and nothing else
    s = 10.0 * c.tol * (1.0 + np.abs(c.X0[-1]).max())
    X1 = c.oracle(max_iter=1, tol=0.0)[0]
    for k, e in enumerate(ent):
        step = (X1[2 * k] - c.X0[2 * k]).ravel()
        assert abs(step[e] + s) <= 1e-6 * s and np.abs(np.delete(step, e)).max() <= 1e-6 * s


@pytest.mark.parametrize("name", sorted(sc.ENTRY_SHAPES))
def test_a_rule_that_misses_an_entry_or_its_component_changes_the_count(name):
    c, ent = sc.displaced(name)
    n = c.w.n
    d = c.X0[0].size
    for k, e in enumerate(ent):
        for mask in (np.arange(d) == e, np.arange(d) % n == e % n):
            it = c.trace(sc.rule_skipping(mask), only=[2 * k])[2]
            assert it[2 * k] == 1 and c.ref[3][2 * k] == 2, (name, e)


def test_scale_batch_and_the_rules_that_misjudge_it():
    c, star = sc.scale_case()
    _report(c)
    assert c.ref[3].tolist() == [1] * c.B
    assert np.abs(star[:, 0]).min() > 0.9 * sc.SCALE_C and np.abs(star[:, 1:]).max() < 0.1 * sc.SCALE_C
    for rs in c.ratios:
        assert abs(rs[0] - 0.25) <= 1e-6
    # max|X| without the position component: every ratio above 2, every count 2
    mask = np.arange(star.size) % c.w.n == 0
    _, _, it, _, ratios = c.trace(sc.rule_skipping(mask))
    assert it.tolist() == [2] * c.B and min(rs[0] for rs in ratios) > sc.BAND
    # max|X| before the update: indistinguishable at tol = 1e-7 (the two maxima differ by the step) ...
    assert c.trace(sc.rule_before_update)[2].tolist() == [1] * c.B
    # ... and a different count at a tolerance of order 1
    a = sc.scale_after_update_case()
    _report(a)
    assert a.ref[3].tolist() == [1]
    _, _, it, _, ratios = a.trace(sc.rule_before_update)
    assert it.tolist() == [2] and ratios[0][0] > sc.BAND


def test_extra_variable_batch_and_a_rule_that_ignores_them():
    c = sc.extra_variable_case()
    _report(c)
    nz = c.Z0.shape[1]
    assert c.ref[3].tolist() == [2, 2]
    for rs in c.ratios:
        assert 5.0 <= rs[0] <= 20.0
    mask = np.arange(c.X0[0].size + nz) >= c.X0[0].size
    _, _, it, _, ratios = c.trace(sc.rule_skipping(mask))
    assert it.tolist() == [1, 1] and max(rs[0] for rs in ratios) < 1.0 / sc.BAND


def test_start_at_the_optimum_converges_within_one_permitted_iteration():
    c = sc.at_optimum()
    assert c.max_iter == 1
    _report(c)
    assert c.ref[3].tolist() == [1, 1] and c.ref[4].tolist() == [0, 0]
