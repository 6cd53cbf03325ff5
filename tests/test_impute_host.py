"""Rows with missing attributes, without a GPU: the host helpers of csrc/predict_host.hpp
(tests/cpp/impute_host_test.cpp: the code check, the per-row ll_0 against pr_ll0 by bits, the
missing entries and their offsets across block edges, the ld check) and the restatement the
GPU tests compare against (tests/impute_ref.py) checked against itself and against
tests/predict_ref.py."""
import math
import os
import subprocess
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import impute_ref as iref  # noqa: E402
import predict_ref as ref  # noqa: E402

GAMMA = 0.7


def test_impute_host_helpers(tmp_path):
    exe = tmp_path / "impute_host_test"
    src = os.path.join(HERE, "cpp", "impute_host_test.cpp")
    # -ffp-contract=off as in csrc/Makefile: the doubles are compared by bytes
    r = subprocess.run(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-Wall", "-o", str(exe), src],
                       capture_output=True, text=True)
    if r.returncode != 0:
        pytest.fail(r.stderr)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "impute host ok" in r.stdout


@pytest.fixture(scope="module")
def small():
    p = ref.problem(seed=12, N=40, d=9, Ks=[3, 1, 5, 4], att=[2, 3, 4, 6, 16, 17, 100, 255, 2])
    p["Y"] = ref.rows_near(p["rng"], p["centers"][2][p["rng"].integers(0, 5, size=7)], p["att"], 0.3)
    return p


def args(p):
    return p["c_trace"], p["centers"], p["sigmas"], p["att"], GAMMA


def test_ref_complete_rows_are_predict_ref(small):
    p = small
    assert iref.ll0_row(p["Y"][0], p["att"]) == ref.ll0(p["att"])
    assert np.float64(iref.ll0_row(p["Y"][0], p["att"])).tobytes() == np.float64(ref.ll0(p["att"])).tobytes()
    for s in range(4):
        a = iref.ll_matrix(p["Y"], p["centers"][s], p["sigmas"][s], p["att"])
        assert a.tobytes() == ref.ll_matrix(p["Y"], p["centers"][s], p["sigmas"][s], p["att"]).tobytes()
    cl = np.arange(40) % 3
    lpd, pn, co = iref.partial(p["Y"], *args(p), cl, 3)
    lpd_w, pn_w, co_w, _ = ref.new_rows(p["Y"], *args(p), cl, 3)
    assert lpd.tobytes() == lpd_w.tobytes()
    np.testing.assert_allclose(pn, pn_w, rtol=0, atol=1e-15)
    np.testing.assert_allclose(co, co_w, rtol=0, atol=1e-14)


def test_ref_all_missing_row(small):
    p = small
    Y = iref.mask(p["Y"], "all")
    assert iref.ll0_row(Y[0], p["att"]) == 0.0
    lpd, pn, _ = iref.partial(Y, *args(p))
    assert np.all(np.abs(lpd) <= 1e-14)
    np.testing.assert_allclose(pn, GAMMA / (40 + GAMMA), rtol=1e-14)


@pytest.mark.parametrize("pattern", ["all", "first", "last", "alternate", "one", "row"])
def test_ref_pmf_rows_sum_to_one(small, pattern):
    p = small
    Y = iref.mask(p["Y"], pattern, np.random.default_rng(3))
    rows, attrs, pmf, mode, lpd = iref.impute(Y, *args(p))
    assert rows.size == int((Y == 0).sum()) and pmf.shape[1] == p["att"][attrs].max()
    assert np.all(np.diff(rows * 9 + attrs) > 0)          # row-major order
    np.testing.assert_allclose(pmf.sum(axis=1), 1.0, rtol=0, atol=1e-14)
    for e in range(rows.size):
        m = p["att"][attrs[e]]
        assert np.all(pmf[e, :m] > 0) and np.all(pmf[e, m:] == 0.0)
        assert mode[e] == 1 + int(np.argmax(pmf[e]))
    assert lpd.tobytes() == iref.partial(Y, *args(p))[0].tobytes()


def test_ref_bayes_identity(small):
    """p(y_j = l | y_O) = p(y_O, y_j = l) / p(y_O): the pmf of a single gap against the
    densities of the filled-in rows, all within the restatements."""
    p = small
    for j in (0, 4, 8):
        Y = p["Y"].copy()
        Y[:, j] = 0
        _, _, pmf, _, lpd = iref.impute(Y, *args(p))
        for l in range(1, p["att"][j] + 1):
            F = p["Y"].copy()
            F[:, j] = l
            full = ref.new_rows(F, *args(p))[0]
            np.testing.assert_allclose(pmf[:, l - 1], np.exp(full - lpd), rtol=1e-12)


def test_ref_marginal_is_the_sum_over_the_gap(small):
    """exp(lpd) of a row with one gap is the sum over the gap's levels of the filled-in rows'."""
    p = small
    j = 3
    Y = p["Y"].copy()
    Y[:, j] = 0
    lpd = iref.partial(Y, *args(p))[0]
    tot = np.zeros(len(Y))
    for l in range(1, p["att"][j] + 1):
        F = p["Y"].copy()
        F[:, j] = l
        tot += np.exp(ref.new_rows(F, *args(p))[0])
    np.testing.assert_allclose(np.exp(lpd), tot, rtol=1e-12)
    assert math.isfinite(float(lpd.sum()))
