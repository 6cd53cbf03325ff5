"""The host arithmetic of the posterior predictive (csrc/predict_host.hpp, plain C++): the
parameter tables against dhamming_pair, every refusal, the block rule and the packing,
checked by tests/cpp/predict_host_test.cpp; and the restatement the GPU tests compare
against (tests/predict_ref.py) checked against itself.  No GPU."""
import math
import os
import subprocess
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import predict_ref as ref  # noqa: E402


def test_predict_host_helpers(tmp_path):
    exe = tmp_path / "predict_host_test"
    src = os.path.join(HERE, "cpp", "predict_host_test.cpp")
    # -ffp-contract=off as in csrc/Makefile: the doubles are compared by bytes
    r = subprocess.run(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-Wall", "-o", str(exe), src],
                       capture_output=True, text=True)
    if r.returncode != 0:
        pytest.fail(r.stderr)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "predict host ok" in r.stdout


@pytest.fixture(scope="module")
def small():
    p = ref.problem(seed=11, N=40, d=9, Ks=[3, 1, 5, 4])
    p["Y"] = ref.rows_near(p["rng"], p["centers"][2][p["rng"].integers(0, 5, size=7)], p["att"], 0.3)
    p["cl"] = np.array([i % 4 if i % 4 != 2 else 0 for i in range(40)])      # class 2 of 0..3 is empty
    return p


def test_ref_matrix_form_has_the_scalar_loops_bits(small):
    p = small
    llm = ref.ll_matrix(p["Y"], p["centers"][2], p["sigmas"][2], p["att"])
    for y in range(len(p["Y"])):
        for k in range(5):
            assert llm[y, k].tobytes() == np.float64(
                ref.ll_scalar(p["Y"][y], p["centers"][2][k], p["sigmas"][2][k], p["att"])).tobytes()


def test_ref_responsibilities_sum_to_one(small):
    p = small
    for s in range(4):
        llm = ref.ll_matrix(p["Y"], p["centers"][s], p["sigmas"][s], p["att"])
        for w in ref.draw_weights(llm, p["c_trace"][s], 0.7, p["att"]):
            l, r = ref.responsibilities(w)
            assert math.isfinite(l)
            assert abs(math.fsum(r) - 1.0) <= 1e-14


def test_ref_coclass_table_form_equals_the_definition(small):
    p = small
    a = ref.new_rows(p["Y"], p["c_trace"], p["centers"], p["sigmas"], p["att"], 0.7, p["cl"], 4)
    b = ref.new_rows(p["Y"], p["c_trace"], p["centers"], p["sigmas"], p["att"], 0.7, p["cl"], 4, table_form=True)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
    np.testing.assert_allclose(a[2], b[2], rtol=0, atol=1e-14)
    assert np.all(a[2][:, 2] == 0.0)                     # the empty class
    # sum_a n_a coclass[a] = (1/M) sum_s sum_k r_k n_k, the expected number of training points
    # in y's cluster: between 0 and N
    tot = (a[2] * np.bincount(p["cl"], minlength=4)[None, :]).sum(axis=1)
    assert np.all(tot >= 0) and np.all(tot <= 40 + 1e-9)


@pytest.mark.parametrize("m", [2, 3, 6, 255])
@pytest.mark.parametrize("sigma", [0.05, 0.3, 1.0, 7.0])
def test_prior_predictive_identity(m, sigma):
    """exp(match) + (m - 1) exp(mismatch) = 1 for every sigma: dhamming is a density over the
    m codes, so under the uniform prior center a row's prior predictive is prod_j 1 / m_j."""
    ma, mi = ref.dhamming_pair(sigma, m)
    assert abs(math.exp(ma) + (m - 1) * math.exp(mi) - 1.0) <= 1e-15
    # and so the mean over centers c of exp(dhamming(x, c)) is 1 / m for any code x
    mean = (math.exp(ma) + (m - 1) * math.exp(mi)) / m
    assert abs(mean * m - 1.0) <= 2e-15
    assert ref.ll0([m, m]) == -(math.log(float(m)) + math.log(float(m)))


def test_ref_pointwise_bounds(small):
    p = small
    lppd, var, cpo = ref.pointwise(p["X"], p["c_trace"], p["centers"], p["sigmas"], p["att"])
    # the harmonic mean of the likelihoods is at most their arithmetic mean
    assert np.all(cpo <= lppd + 1e-12) and np.all(var >= 0)
    one = ref.pointwise(p["X"], p["c_trace"][:1], p["centers"][:1], p["sigmas"][:1], p["att"])
    assert np.all(one[1] == 0.0)
    np.testing.assert_allclose(one[0], one[2], rtol=1e-15)
    assert abs(ref.waic(lppd, var) + 2.0 * (math.fsum(lppd) - math.fsum(var))) < 1e-9
    assert ref.lpml(cpo) == math.fsum(cpo)
