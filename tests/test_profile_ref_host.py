"""The restatement of the cluster profiles (tests/profile_ref.py) checked against itself, without
a GPU: center_cnt from the definition over the points equals center_cnt from the tables (the
restatement asserts it; here it is asserted again from outside), sum_l center_cnt = M n_a,
sum_l code_pmf = 1 within 1e-12 for a non-empty class (the exps of an attribute's pair sum to 1
to rounding, and M K_s <= 200 positive terms are added), an empty class is all zero, and the
profile does not depend on how a draw numbers its clusters."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import profile_ref as pref  # noqa: E402


@pytest.fixture(scope="module")
def small():
    p = pref.problem(seed=31, N=40, d=9, Ks=[3, 1, 5, 4], att=[2, 3, 4, 6, 16, 17, 100, 255, 2])
    p["cl"] = np.where(np.arange(40) % 4 == 1, 3, np.arange(40) % 4).astype(np.int32)      # class 1 is empty
    p["Ka"], p["ld"] = 4, 255
    p["out"] = pref.profile(p["c_trace"], p["centers"], p["sigmas"], p["att"], p["cl"], 4, 255)
    return p


def test_two_routes_to_center_cnt_agree(small):
    p = small
    pts = pref.center_cnt_points(p["c_trace"], p["centers"], p["cl"], 4, 9, 255)
    assert np.array_equal(p["out"]["center_cnt"].astype(np.int64), pts)


def test_sums(small):
    p, o = small, small["out"]
    M = p["c_trace"].shape[0]
    n = o["sizes"]
    assert n.tolist() == np.bincount(p["cl"], minlength=4).tolist() and n[1] == 0
    assert np.array_equal(o["center_cnt"].sum(axis=2), np.broadcast_to((M * n)[:, None], (4, 9)).astype(np.uint64))
    tot = o["code_pmf"].sum(axis=2)
    assert np.all(np.abs(tot[n > 0] - 1.0) <= 1e-12), float(np.abs(tot[n > 0] - 1.0).max())
    for j, m in enumerate(p["att"]):
        assert np.all(o["center_cnt"][:, j, m:] == 0) and np.all(o["code_pmf"][:, j, m:] == 0.0)
        assert np.all(o["code_pmf"][n > 0, j, :m] > 0.0)
    for key in ("center_cnt", "code_pmf", "sigma_mean", "sigma_var", "sigma_trace"):
        a = o[key][:, 1] if key == "sigma_trace" else o[key][1]
        assert np.all(a == 0), key
    assert np.all(o["sigma_mean"][n > 0] > 0) and np.all(o["sigma_var"] >= 0)
    # the mean of the trace, and its variance, by the two-pass formulas
    np.testing.assert_allclose(o["sigma_mean"], o["sigma_trace"].mean(axis=0), rtol=1e-13)
    np.testing.assert_allclose(o["sigma_var"], o["sigma_trace"].var(axis=0, ddof=1), rtol=1e-10, atol=1e-18)


def test_mode_is_the_first_arg_max(small):
    o = small["out"]
    mode = pref.mode_of(o["center_cnt"], o["sizes"])
    assert np.all(mode[1] == 0)
    assert np.array_equal(mode[o["sizes"] > 0], (np.argmax(o["center_cnt"], axis=2) + 1)[o["sizes"] > 0])
    tie = np.zeros((1, 1, 4), np.uint64)
    tie[0, 0] = [2, 5, 5, 1]
    assert pref.mode_of(tie, np.array([3]))[0, 0] == 2


def test_one_draw_own_labels_is_the_draw(small):
    p = small
    z, cen, sig = p["c_trace"][2], p["centers"][2], p["sigmas"][2]
    o = pref.profile(z[None, :], [cen], [sig], p["att"], z, 5, 255)
    n = np.bincount(z, minlength=5)
    for a in range(5):
        for j in range(9):
            row = o["center_cnt"][a, j]
            assert row[int(cen[a, j]) - 1] == n[a] and row.sum() == n[a]
    assert np.all(np.abs(o["sigma_trace"][0] - sig) <= 2 * np.spacing(sig))
    assert np.all(o["sigma_var"] == 0.0)


def test_label_switching_changes_nothing_but_rounding(small):
    p = small
    rng = np.random.default_rng(4)
    tr, cens, sigs = [], [], []
    for s, z in enumerate(p["c_trace"]):
        K = p["centers"][s].shape[0]
        perm = rng.permutation(K)                     # old label k becomes perm[k]
        inv = np.argsort(perm)
        tr.append(perm[z])
        cens.append(p["centers"][s][inv])
        sigs.append(p["sigmas"][s][inv])
    o2 = pref.profile(np.stack(tr), cens, sigs, p["att"], p["cl"], 4, 255)
    o = p["out"]
    assert np.array_equal(o["center_cnt"], o2["center_cnt"])
    np.testing.assert_allclose(o2["sigma_trace"], o["sigma_trace"], rtol=1e-12)
    np.testing.assert_allclose(o2["sigma_mean"], o["sigma_mean"], rtol=1e-12)
    assert np.all(np.abs(o2["sigma_var"] - o["sigma_var"]) <= 1e-10 * (1 + o["sigma_var"]))
    assert np.all(np.abs(o2["code_pmf"] - o["code_pmf"]) <= 1e-10)
