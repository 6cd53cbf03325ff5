"""The oracle's record of a split-merge move's acceptance addends (oracle.h orc_sm_terms) and the
plain restatement of logprobgs_c_i that the GPU tests use as a second reference (CPU only)."""
import math

import numpy as np
import pytest

import sm_terms_ref as R


def _records(oracle, ds, c, pseed, rseed, moves, t, r, fast):
    ost, rng, _, _ = R.oracle_start(oracle, ds, c, pseed, rseed)
    out = []
    for k in range(moves):
        out.append(R.oracle_move(oracle, ds, ost, rng, t, r, k, fast))
    return out, ost, rng


@pytest.mark.parametrize("shape", ["zoo", "300x16", "1200x160"])
def test_oracle_records_agree_between_per_term_and_table_modes(oracle, zoo, shape):
    """fast=1 (dhamming per term) and fast=2 (cluster tables) follow the same chain and record
    the same addends: integers equal, addends within RTOL, each record consistent with itself."""
    if shape == "zoo":
        ds, c, moves, t = zoo, zoo.truth, 12, 5
    elif shape == "300x16":
        ds = R.synth(300, 16, 3, (2, 6), seed=5)
        c, moves, t = ds.truth, 12, 5
    else:
        ds = R.synth(1200, 160, 4, 5, seed=40)
        c, moves, t = ds.truth, 6, 3
    a, osta, rnga = _records(oracle, ds, c, 3, 11, moves, t, t, 1)
    b, ostb, rngb = _records(oracle, ds, c, 3, 11, moves, t, t, 2)
    assert np.array_equal(osta.c_i, ostb.c_i) and np.array_equal(rnga, rngb)
    kinds = set()
    for k, (ra, rb) in enumerate(zip(a, b)):
        R.check_self(ra, f"move {k} fast=1")
        R.check_self(rb, f"move {k} fast=2")
        for key in ("kind", "accepted", "i1", "i2", "nS", "size"):
            assert ra[key] == rb[key], (k, key)
        assert R.same_bits(ra["log_u"], rb["log_u"])
        for q in range(14):
            assert R.close(rb["term"][q], ra["term"][q]), (k, q, ra["term"][q], rb["term"][q])
        kinds.add(ra["kind"])
    assert kinds == {1, 2}, kinds


def test_oracle_record_is_cleared_by_a_failed_move(oracle):
    """A move that returns an error leaves kind 0 (here: the 2F1 series of clusters of ~1.5k
    members diverges, ORC_E_GSL)."""
    ds = R.synth(3000, 16, 2, 2, seed=3)
    ost, rng, _, _ = R.oracle_start(oracle, ds, ds.truth, 3, 11)
    st, _ = oracle.split_and_merge(ds.codes, ds.attrisize, ds.gamma, ds.v, ds.w, ost, 2, 2, 0, rng, fast=2)
    assert st == 2
    assert oracle.sm_last_terms()["kind"] == 0


@pytest.mark.parametrize("nS,d", R.LPGS_SIZES)
def test_lpgs_restatement_matches_oracle(oracle, nS, d):
    ds, c, cen, sig, g, S, i1, i2 = R.lpgs_case(nS, d, (2, 6), 100 + nS + d, stray=(nS == 257))
    ref = oracle.logprobgs_c_i(ds.codes, ds.attrisize, oracle.OracleState(c, 3, cen, sig), g, S, i1, i2)
    mine = R.lpgs_fsum(ds.codes, ds.attrisize, c, cen, sig, g, S, i1, i2)
    assert math.isfinite(ref)
    assert R.close(mine, ref), (mine, ref)


@pytest.mark.parametrize("nS,q", [(300, 64), (600, 256 + 70)])
def test_lpgs_underflow_is_minus_infinity_in_both_references(oracle, nS, q):
    ds, c, cen, sig, g, S, i1, i2, p = R.lpgs_underflow_case(nS, q)
    L, _ = oracle.loglik_matrix(ds.codes, ds.attrisize, cen, sig)
    # exp(x) is exactly 0 below -745.14; the sizes' logs move the difference by < log(n) < 7
    assert L[p, 1 - c[p]] - L[p, c[p]] > 745.2 + 7.0, L[p]
    ref = oracle.logprobgs_c_i(ds.codes, ds.attrisize, oracle.OracleState(c, 3, cen, sig), g, S, i1, i2)
    mine = R.lpgs_fsum(ds.codes, ds.attrisize, c, cen, sig, g, S, i1, i2)
    assert ref == -math.inf and mine == -math.inf, (ref, mine)
