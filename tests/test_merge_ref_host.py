"""The reference of the pair merges (tests/merge_ref.py) on the CPU: the formulas against brute
force, f's log1p form against 60-digit decimals, the stall case with its numbers, and the gap
condition that lets tests/test_gpu_merge.py demand the reference's best pair everywhere."""
import decimal
import math

import numpy as np
import pytest

import merge_ref as MR
import refine_ref as R


@pytest.mark.parametrize("seed", range(30))
def test_formula_against_brute_force(seed):
    rng = np.random.default_rng(seed)
    N, M = int(rng.integers(2, 25)), int(rng.integers(1, 8))
    Ka, Kz = int(rng.integers(1, 7)), int(rng.integers(1, 6))
    c = rng.integers(0, Ka, N)
    tr = rng.integers(0, Kz, (M, N))
    n = np.bincount(c, minlength=Ka)
    for loss in ("VI", "Binder"):
        g = MR.merge_gains_formula(c, tr, Ka, loss)
        assert np.array_equal(g, g.T) and not g.diagonal().any()
        assert not g[n == 0].any() and not g[:, n == 0].any()
        for (a, b), want in MR.merge_gains_brute(c, tr, Ka, loss).items():
            if loss == "Binder":
                assert int(g[a, b]) == want
            else:
                assert abs(g[a, b] - want) <= 1e-12


def f_decimal(s, t):
    with decimal.localcontext() as ctx:
        ctx.prec = 60
        s, t, ln2 = decimal.Decimal(s), decimal.Decimal(t), decimal.Decimal(2).ln()
        return ((s + t) * (s + t).ln() - s * s.ln() - t * t.ln()) / ln2


@pytest.mark.parametrize("s,t", [(10 ** 6, 1), (999983, 17), (3, 10 ** 6)])
def test_f_log1p_form(s, t):
    want = f_decimal(s, t)
    rel = abs((decimal.Decimal(float(MR.f(s, t))) - want) / want)
    assert rel <= decimal.Decimal("1e-14")
    assert float(MR.f(s, t)) == float(MR.f(t, s))


def test_f_difference_of_products_fails_the_bound():
    want = f_decimal(10 ** 6, 1)
    rel = abs((decimal.Decimal(MR.f_products(10 ** 6, 1)) - want) / want)
    assert rel > decimal.Decimal("1e-14")


def test_stall_case():
    c, tr, merged = MR.stall_case()
    for loss, before, after, other in (("Binder", 216, 144, 480), ("VI", 0.36, 0.24, 0.6897)):
        r = R.refine_ref(c, tr, loss)
        assert r["rounds"] == 0 and r["converged"]
        g = R.gains_formula(c, tr, 3, loss)
        assert not (g < 0).any()
        mg = MR.merge_gains_formula(c, tr, 3, loss)
        best, bg = MR.best_pair(mg, np.bincount(c))
        assert best == (0, 1)
        if loss == "Binder":
            assert R.loss_of(c, tr, loss) == before and R.loss_of(merged, tr, loss) == after
            assert bg == after - before and mg[0, 2] == other and mg[1, 2] == other
        else:
            assert abs(R.loss_of(c, tr, loss) - before) < 1e-12 and abs(R.loss_of(merged, tr, loss) - after) < 1e-12
            assert abs(bg - (after - before)) < 1e-12
            assert abs(mg[0, 2] - other) < 5e-5 and abs(mg[1, 2] - other) < 5e-5
        rm = MR.refine_merge_ref(c, tr, loss, 100, 5)
        assert rm["merges"] == 1 and rm["converged"] and rm["K"] == 2
        assert np.array_equal(rm["cl"], merged)
        assert len(rm["history"]) == 2


@pytest.mark.parametrize("loss", ("VI", "Binder"))
def test_alternation_case(loss):
    truth, tr, start = MR.alternation_case()
    plain = R.refine_ref(start, tr, loss)
    assert plain["converged"] and plain["K"] == 5 and plain["rounds"] == 1
    # the first merge decision stands clear of VI's rounding
    g = MR.merge_gains_formula(plain["cl"], tr, 5, loss)
    assert MR.gap(g, np.bincount(plain["cl"])) > 2 * MR.vi_atol(truth.size)
    r = MR.refine_merge_ref(start, tr, loss, 100, 20)
    assert (r["rounds"], r["merges"], r["converged"], r["K"]) == (1, 2, True, 3)
    assert np.array_equal(r["cl"], R.relabel(truth)) and len(r["history"]) == 4
    assert all(x > y for x, y in zip(r["history"], r["history"][1:]))
    r1 = MR.refine_merge_ref(start, tr, loss, 100, 1)
    assert (r1["merges"], r1["converged"], r1["K"]) == (1, False, 4)


def clear(g, n, N, loss):
    """the best pair stands clear: VI by more than twice the tolerance; Binder's integers differ
    or the tie rule decides, which the exact device value obeys either way"""
    return loss == "Binder" or MR.gap(g, n) > 2 * MR.vi_atol(N)


@pytest.mark.parametrize("shape", MR.SHAPES)
def test_gap_condition_shapes(shape):
    N, M, Ka = shape[:3]
    c, tr = MR.gains_case(*shape)
    assert c.max() < Ka and tr.max() + 1 == shape[3]          # the device's Kz is the shape's
    n = np.bincount(c, minlength=Ka)
    for loss in ("VI", "Binder"):
        assert clear(MR.merge_gains_formula(c, tr, Ka, loss), n, N, loss)


def test_gap_condition_paths():
    truth, tr, start = MR.path_case()
    for loss in ("VI", "Binder"):
        p = MR.merge_path_ref(start, tr, 12, loss)
        assert len(p["merge"]) == 11
        if loss == "VI":
            assert min(p["gap"]) > 2 * MR.vi_atol(truth.size)
        v = p["value"]
        assert int(np.argmin(np.asarray(v, np.float64))) == 9           # the level of 3 classes
        assert np.array_equal(MR.coarsen_ref(start, p["merge"], 9), R.relabel(truth))
        # the gains telescope to the values
        for s in range(11):
            if loss == "Binder":
                assert v[s + 1] - v[s] == p["step_gain"][s]
            else:
                assert abs(v[s + 1] - v[s] - p["step_gain"][s]) < 1e-12
    c, tr, _ = MR.stall_case()
    p = MR.merge_path_ref(c, tr, 3, "VI")
    assert p["merge"] == [(0, 1), (0, 2)] and min(p["gap"][:1]) > 2 * MR.vi_atol(20)
