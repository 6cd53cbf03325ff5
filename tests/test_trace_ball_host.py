"""The host selection behind credible_ball (posterior._ball) on hand-made distances and
cluster counts: mcclust.ext::credibleball's ball and its three bounds, every tie kept.  R is
absent, so the expectations are worked out by hand from the rule in the docstring."""
import numpy as np
import pytest

from split_and_merge_gibbs_sampling_amd.posterior import _ball


def idx(x):
    return np.asarray(x).tolist()


def test_ties_at_the_radius_are_all_in_the_ball():
    # M = 10, alpha = 0.5: the 5th smallest distance is 3, and three draws sit at 3
    d = np.array([1, 3, 2, 3, 9, 0, 3, 7, 2, 8])
    k = np.array([4, 4, 4, 4, 4, 4, 4, 4, 4, 4])
    b = _ball(d, k, 0.5)
    assert b["radius"] == 3
    assert idx(b["ball"]) == [0, 1, 2, 3, 5, 6, 8]
    assert idx(b["horizontal"]) == [1, 3, 6]
    # one cluster count: both vertical bounds are the horizontal one
    assert idx(b["upper_vertical"]) == [1, 3, 6] and idx(b["lower_vertical"]) == [1, 3, 6]
    assert b["horizontal_distance"] == 3 and b["upper_vertical_distance"] == 3 and b["lower_vertical_distance"] == 3


def test_ties_inside_a_bound_and_distinct_bounds():
    #            0    1    2    3    4    5    6    7
    d = np.array([0.5, 2.0, 2.0, 1.0, 3.0, 2.5, 2.5, 9.0])
    k = np.array([4,   3,   3,   3,   4,   5,   5,   2])
    b = _ball(d, k, 0.1)                  # ceil(0.9 * 8) = 8 -> everything
    assert idx(b["ball"]) == list(range(8)) and b["radius"] == 9.0
    assert idx(b["horizontal"]) == [7]
    assert idx(b["upper_vertical"]) == [7] and idx(b["lower_vertical"]) == [5, 6]
    b = _ball(d, k, 0.2)                  # ceil(0.8 * 8) = 7 -> the draw at 9.0 drops out
    assert idx(b["ball"]) == list(range(7)) and b["radius"] == 3.0
    assert idx(b["horizontal"]) == [4]
    assert idx(b["upper_vertical"]) == [1, 2] and b["upper_vertical_distance"] == 2.0     # K = 3: a tie of two
    assert idx(b["lower_vertical"]) == [5, 6] and b["lower_vertical_distance"] == 2.5     # K = 5: a tie of two
    assert b["horizontal_distance"] == 3.0


def test_alpha_zero_takes_every_draw():
    d = np.array([4.0, 1.0, 6.0, 2.0])
    k = np.array([2, 3, 3, 1])
    b = _ball(d, k, 0.0)
    assert idx(b["ball"]) == [0, 1, 2, 3] and b["radius"] == 6.0
    assert idx(b["horizontal"]) == [2] and idx(b["upper_vertical"]) == [3] and idx(b["lower_vertical"]) == [2]


def test_large_alpha_clamps_the_index_to_one():
    d = np.array([4.0, 1.0, 6.0, 1.0])
    k = np.array([2, 3, 3, 1])
    for alpha in (1.0, 0.99):
        b = _ball(d, k, alpha)            # ceil(0) = 0 -> 1; ceil(0.04) = 1
        assert b["radius"] == 1.0
        assert idx(b["ball"]) == [1, 3]   # the smallest distance, with its tie
        assert idx(b["horizontal"]) == [1, 3]
        assert idx(b["upper_vertical"]) == [3] and idx(b["lower_vertical"]) == [1]


def test_a_single_draw():
    for d in (np.array([0.75]), np.array([12], np.uint64)):
        for alpha in (0.0, 0.05, 1.0):
            b = _ball(d, np.array([7]), alpha)
            assert idx(b["ball"]) == [0] and idx(b["horizontal"]) == [0]
            assert idx(b["upper_vertical"]) == [0] and idx(b["lower_vertical"]) == [0]
            assert b["radius"] == d[0]


def test_integer_and_float_distances_select_alike():
    rng = np.random.default_rng(3)
    di = rng.integers(0, 12, 40).astype(np.uint64)      # many ties
    k = rng.integers(2, 6, 40)
    for alpha in (0.05, 0.3, 0.5):
        bi, bf = _ball(di, k, alpha), _ball(di.astype(np.float64) / 8, k, alpha)
        for name in ("ball", "horizontal", "upper_vertical", "lower_vertical"):
            assert idx(bi[name]) == idx(bf[name]), name
        assert isinstance(bi["radius"], int) and isinstance(bf["radius"], float)
        assert bi["radius"] == bf["radius"] * 8
    # uint64 distances beyond 2^53 are compared as integers
    big = np.array([2 ** 60 + 1, 2 ** 60, 2 ** 60 + 2], np.uint64)
    b = _ball(big, np.array([1, 1, 1]), 0.5)            # ceil(1.5) = 2 -> the 2nd smallest
    assert b["radius"] == 2 ** 60 + 1 and idx(b["ball"]) == [0, 1] and idx(b["horizontal"]) == [0]


def test_bad_arguments():
    with pytest.raises(ValueError):
        _ball(np.zeros(0), np.zeros(0), 0.05)
    with pytest.raises(ValueError):
        _ball(np.zeros(3), np.zeros(2), 0.05)
    with pytest.raises(ValueError):
        _ball(np.zeros(3), np.zeros(3), 1.5)
