"""The numpy reference of the single-point moves (tests/refine_ref.py) against itself: the
formulas against brute force (moving the point and recomputing the whole loss), and the two
constructions of tests/test_gpu_refine.py under the reference's own round rule, so that they
are known to hold before a GPU sees them.  No GPU."""
import numpy as np
import pytest

import refine_ref as R


def random_case(seed, N, M, K, Ka_used):
    rng = np.random.default_rng(seed)
    tr = np.stack([R.relabel(rng.integers(0, K, N)) for _ in range(M)])
    c = np.sort(R.relabel(rng.integers(0, Ka_used, N)))      # dense 0..k-1
    return rng.permutation(c), tr


@pytest.mark.parametrize("N,M,K,Ka_used,extra", [(1, 3, 1, 1, 0), (12, 5, 3, 4, 0), (25, 4, 6, 3, 2), (40, 7, 5, 8, 1)])
def test_formula_against_brute_force(N, M, K, Ka_used, extra):
    c, tr = random_case(N * 100 + M, N, M, K, Ka_used)
    if N > 3:
        c[0] = c.max() + 1                                    # a singleton class
    Ka = int(c.max()) + 1 + extra                             # `extra` empty classes
    gb = R.gains_formula(c, tr, Ka, "Binder")
    assert gb.dtype == np.int64
    assert np.array_equal(gb.astype(object), R.gains_brute(c, tr, Ka, "Binder"))
    gv = R.gains_formula(c, tr, Ka, "VI")
    np.testing.assert_allclose(gv, R.gains_brute(c, tr, Ka, "VI"), rtol=0, atol=1e-12)
    # the own class is 0; a singleton's new class is exactly 0 too, and "stay" wins the tie
    me = np.arange(N)
    assert np.all(gb[me, c] == 0) and np.all(gv[me, c] == 0.0)
    if N > 3:
        assert gb[0, Ka] == 0 and gv[0, Ka] == 0.0
        for g in (gb, gv):
            best, bg = R.best_of(g, c)
            assert bg[0] < 0 or best[0] == c[0]


def test_h_keeps_its_digits():
    # the difference of the two products loses eight digits at t = 1e6; the sum does not
    from fractions import Fraction
    import math
    t = 10 ** 6
    exact = math.log2(t + 1) + t * math.log1p(Fraction(1, t)) / math.log(2)
    assert abs(float(R.h(t)) - exact) < 1e-13 * exact
    assert R.h(0) == 0.0 and R.h(1) == 2.0


def test_tie_rules():
    g = np.array([[0.0, -1.0, -1.0, 5.0], [0.0, 0.0, 0.0, 0.0], [-2.0, 0.0, -2.0, -2.0]])
    best, bg = R.best_of(g, np.array([0, 1, 1]))
    assert best.tolist() == [1, 1, 0] and bg.tolist() == [-1.0, 0.0, -2.0]


def test_select_keeps_one_new_class():
    best = np.array([3, 3, 1, 0, 3, 2])
    gain = np.array([-1.0, -2.0, -2.0, 0.0, -2.0, -0.5])
    mv = R.select(best, gain, 3)
    assert [(i, to) for i, to, _ in mv] == [(1, 3), (2, 1), (5, 2)]


@pytest.mark.parametrize("loss", ["VI", "Binder"])
def test_planted_partition(loss):
    truth, tr, start = R.planted()
    r = R.refine_ref(start, tr, loss)
    assert r["converged"] and r["rounds"] >= 1
    assert np.array_equal(r["cl"], R.relabel(truth))
    assert r["value"] == R.loss_of(R.relabel(truth), tr, loss)
    assert all(a > b for a, b in zip(r["history"], r["history"][1:]))
    # the end state is a minimum under single moves
    g = R.gains_formula(r["cl"], tr, r["K"], loss)
    assert (g >= 0).all()


@pytest.mark.parametrize("loss", ["VI", "Binder"])
def test_halving(loss):
    tr, start = R.halving()
    g = R.gains_formula(start, tr, 3, loss)
    if loss == "Binder":
        assert g[0, 1] == -5 and g[1, 0] == -5
    both = start.copy()
    both[0], both[1] = 1, 0
    assert R.loss_of(R.relabel(both), tr, loss) == R.loss_of(start, tr, loss)     # moving both gains nothing
    r = R.refine_ref(start, tr, loss)
    assert (r["trials"], r["rounds"], r["moved"], r["converged"]) == (2, 1, 1, True)
    assert r["cl"].tolist() == [0, 0] + [1] * 10
    assert r["value"] == 0 if loss == "Binder" else abs(r["value"]) < 1e-14


@pytest.mark.parametrize("loss", ["VI", "Binder"])
def test_minimum_and_no_rounds(loss):
    truth, tr, start = R.planted()
    r = R.refine_ref(truth, tr, loss)
    assert (r["rounds"], r["trials"], r["converged"]) == (0, 0, True)
    r = R.refine_ref(start + 5, tr, loss, max_rounds=0)
    assert (r["rounds"], r["trials"], r["converged"]) == (0, 0, False)
    assert np.array_equal(r["cl"], R.relabel(start)) and r["history"] == [r["start"]]
