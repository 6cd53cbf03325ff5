"""MI355X: the addends of the split-merge log acceptance ratio (sm:438-540) against the oracle's,
move by move.  The accepted flag alone says little: log(u) is rarely below -20 while the ratios
of the suite's moves lie hundreds to hundreds of thousands of nats below 0, so an error of that
size in any addend flips no flag.  Here every addend of every move is compared (include/hdpm.h
hdpm_sm_terms, Engine.sm_last_terms), on top of the state and the stream after the move, and
logprobgs_c_i (k_sm_ll_lds / k_sm_ll, k_sm_lpgs, the host merge of the block partials) directly
against the oracle and a plain math.fsum restatement."""
import math
import os

import numpy as np
import pytest

import sm_terms_ref as R
from split_and_merge_gibbs_sampling_amd import Debug

pytestmark = pytest.mark.gpu

G = os.path.join(os.path.dirname(__file__), "golden")


@pytest.fixture(scope="module")
def hd():
    import split_and_merge_gibbs_sampling_amd as hd
    hd.build()
    return hd


def same(eng, ost, rng, what):
    c, cen, sig = eng.get_state()
    assert cen.shape[0] == ost.K, what
    assert np.array_equal(c, ost.c_i), what
    assert np.array_equal(cen, ost.centers[:ost.K]), what
    assert np.array_equal(sig, ost.sigma[:ost.K]), what
    assert np.array_equal(eng.rng_state, rng), what


def report(name, worst, kinds):
    print(f"\n[sm terms] {name}: kinds {sorted(kinds)} largest relative difference " +
          ", ".join(f"{k} {v:.3g}" for k, v in sorted(worst.items())))


def sm_term_step(eng, oracle, ds, ost, rng, t, r, k, fast, worst, what):
    """One move on both sides: flag, state, stream, and the record of its addends."""
    acc = eng.split_and_merge(t, r, k)
    ref = R.oracle_move(oracle, ds, ost, rng, t, r, k, fast)
    got = eng.sm_last_terms()
    assert acc == ref["accepted"], what
    same(eng, ost, rng, what)
    R.compare(got, ref, what, worst)
    return got, ref


def engine_start(hd, oracle, cfg, setup=None):
    ds = cfg["ds"]
    eng = hd.Engine(0)
    eng.set_data(ds.codes, ds.attrisize, ds.gamma, ds.v, ds.w)
    if cfg["logspace"]:
        eng.set_hig_logspace(True)
    if setup:
        setup(eng)
    cen, sig = R.random_params(ds, int(cfg["c"].max()) + 1, cfg["pseed"])
    eng.set_state(cfg["c"], cen, sig)
    eng.rng_state = oracle.seed_state(cfg["rseed"])
    eng.update_phi()
    return eng


def run_moves(hd, oracle, name, setup=None):
    """The configuration's moves stepwise from its start (truth labels, random_params, one
    update_phi on both sides); returns the engine's records."""
    cfg = R.move_config(name)
    ds = cfg["ds"]
    worst, kinds, recs = {}, set(), []
    eng = engine_start(hd, oracle, cfg, setup)
    try:
        oracle.set_hig_logspace(cfg["logspace"])
        ost, rng, _, _ = R.oracle_start(oracle, ds, cfg["c"], cfg["pseed"], cfg["rseed"])
        same(eng, ost, rng, "start")
        assert eng.sm_last_terms()["kind"] == 0
        for k in range(cfg["moves"]):
            got, ref = sm_term_step(eng, oracle, ds, ost, rng, cfg["t"], cfg["t"], k, cfg["fast"], worst,
                                    f"{name} move {k}")
            kinds.add(ref["kind"])
            recs.append(got)
    finally:
        oracle.set_hig_logspace(False)
        eng.close()
    report(name, worst, kinds)
    assert kinds == {1, 2}, kinds
    return recs


def chain_steps(eng, oracle, ds, iters, m, t, r, fast, name):
    """`iters` passes of the chain's loop body (la:85-132) after Engine.init_chain, step by step
    on both sides: Neal-8 sweep, update_phi, the split-merge move with its record, the latent
    pool's regeneration at iteration 0.  Returns (accepted flags, labels after every pass)."""
    c, cen, sig = eng.get_state()
    P = ds.n * m
    pc, ps = eng.get_pool(P)
    ost = oracle.OracleState(c, cen.shape[0], cen, sig)
    rng = eng.rng_state.copy()
    worst, kinds, acc, labels = {}, set(), [], []
    for it in range(iters):
        eng.neal8_sweep(m)
        assert oracle.neal8_sweep(ds.codes, ds.attrisize, ds.gamma, ds.v, ds.w, ost, m, pc, ps, rng, fast=fast) == 0
        eng.update_phi()
        assert oracle.update_phi(ds.codes, ds.attrisize, ds.v, ds.w, ost, rng) == 0
        same(eng, ost, rng, f"{name} sweep {it}")
        got, ref = sm_term_step(eng, oracle, ds, ost, rng, t, r, it, fast, worst, f"{name} move {it}")
        kinds.add(ref["kind"])
        acc.append(got["accepted"])
        if it % 1000 == 0:
            eng.generate_pool(P)
            pc, ps, st = oracle.pool_generate(ds.attrisize, ds.v, ds.w, P, rng)
            assert st == 0
            assert np.array_equal(eng.rng_state, rng)
        labels.append(ost.c_i.copy())
    report(name, worst, kinds)
    assert kinds == {1, 2}, kinds
    return np.array(acc), np.array(labels)


def test_zoo_golden_chain_moves(hd, oracle, zoo):
    """The golden split-merge configuration (N = 101, seed 7, t = r = 10), its 30 moves one by
    one: four of them have ratios within 10 nats of 0, where the flag does discriminate."""
    g = np.load(os.path.join(G, "zoo_sm_seed7.npz"))
    eng = hd.Engine(0)
    try:
        eng.set_data(zoo.codes, zoo.attrisize, zoo.gamma, zoo.v, zoo.w)
        eng.set_seed(7)
        params = eng.chain_params(m=3, iterations=30, L=1, burnin=0, t=10, r=10, neal8=True, split_merge=True)
        eng.init_chain(params, c_i=np.zeros(zoo.n, np.int32))
        acc, labels = chain_steps(eng, oracle, zoo, 30, 3, 10, 10, 1, "zoo")
    finally:
        eng.close()
    assert np.array_equal(acc, g["accepted"])
    assert np.array_equal(labels, g["c_i"])


@pytest.mark.parametrize("name", ["tiny-2x1", "tiny-3x2"])
def test_tiny_shapes(hd, oracle, name):
    """|S| is 0 or 1: logprobgs_c_i of an empty S is 0.0 on both sides."""
    recs = run_moves(hd, oracle, name)
    assert any(r["nS"] == 0 for r in recs)
    for r in recs:
        if r["nS"] == 0:
            assert r["term"][13 if r["kind"] == 1 else 12] == 0.0


@pytest.mark.parametrize("name", ["mixed-300x16", "mixed-400x8"])
def test_mixed_levels(hd, oracle, name):
    run_moves(hd, oracle, name)


def test_wide_rows(hd, oracle):
    """d = 160: priors and logprobgs_phi per attribute on the host pool."""
    run_moves(hd, oracle, "wide-1200x160")


@pytest.mark.parametrize("name", ["lds-1927", "lds-1928"])
def test_lds_boundary(hd, oracle, name):
    """d = 1927: k_sm_ll_lds with exactly 64 KiB and an odd tail chunk; d = 1928: the unfused
    path (k_sm_ll, k_sm_cert on its own, no wide scan, k_sm_freq zeroing its table itself)."""
    run_moves(hd, oracle, name)


LARGE = {}


def large_default(hd, oracle):
    if "default" not in LARGE:
        LARGE["default"] = run_moves(hd, oracle, "large-6000x64")
    return LARGE["default"]


def test_large_moves(hd, oracle):
    """|S| = 5998 (merges: device draws, 24 k_sm_lpgs blocks, the wide scan) and 2998 (splits)."""
    recs = large_default(hd, oracle)
    assert {r["nS"] for r in recs} == {5998, 2998}


@pytest.mark.parametrize("variant", ["sm_chain", "phi_device", "wide_wait_0", "host_draws"])
def test_large_moves_same_records_on_every_path(hd, oracle, variant):
    """The device chain, the device update_phi, a wide scan that gives up and host draws change
    where the work runs, not one bit of any addend."""
    setup = {"sm_chain": lambda e: e.set_sm_chain(1), "phi_device": lambda e: e.set_phi_device(True),
             "wide_wait_0": lambda e: e.set_sm_wide_wait_us(0),
             "host_draws": lambda e: e.set_debug(Debug.SM_HOST_DRAWS)}[variant]
    base = large_default(hd, oracle)
    recs = run_moves(hd, oracle, "large-6000x64", setup)
    assert len(recs) == len(base)
    for k, (a, b) in enumerate(zip(recs, base)):
        for key in ("kind", "accepted", "i1", "i2", "nS", "size"):
            assert a[key] == b[key], (variant, k, key)
        for key in ("log_prior", "log_likelihood", "log_proposal", "log_ratio", "log_u"):
            assert R.same_bits(a[key], b[key]), (variant, k, key, a[key], b[key])
        for q in range(14):
            assert R.same_bits(a["term"][q], b["term"][q]), (variant, k, q, a["term"][q], b["term"][q])


def test_second_dataset_other_attrisize_moves(hd, oracle):
    """The sequence of test_split_merge_second_dataset_other_attrisize (test_gpu_parity.py), the
    second data set's chain step by step: the priors addends show constants norm_const2(w_j,
    v_j, m_j) kept from the first data set's m_j, which the flags (ratios near -2771) cannot."""
    kw = dict(m=3, iterations=4, L=1, burnin=0, t=3, r=3, neal8=True, split_merge=True)
    da = R.synth(900, 16, 3, 2, seed=61)
    db = R.synth(900, 16, 3, 5, seed=62)
    assert np.array_equal(da.v, db.v) and np.array_equal(da.w, db.w)
    st, ref = oracle.run_markov_chain(db.codes, db.attrisize, db.gamma, db.v, db.w, seed=10, c_i=db.truth,
                                      fast=1, **kw)
    assert st == 0
    eng = hd.Engine(0)
    try:
        eng.set_data(da.codes, da.attrisize, da.gamma, da.v, da.w)
        eng.set_seed(9)
        eng.run_markov_chain(c_i=da.truth, **kw)
        assert eng.stats()["sm_moves"] > 0
        R.check_self(eng.sm_last_terms(), "first data set, last move of run_markov_chain")
        eng.set_data(db.codes, db.attrisize, db.gamma, db.v, db.w)
        eng.set_seed(10)
        eng.init_chain(eng.chain_params(**kw), c_i=db.truth)
        acc, labels = chain_steps(eng, oracle, db, 4, 3, 3, 3, 1, "second data set")
    finally:
        eng.close()
    assert np.array_equal(acc, ref["accepted"])
    assert np.array_equal(labels, ref["c_i"])


def test_failed_move_clears_the_record(hd, oracle):
    """A move that returns an error leaves kind 0: two clusters of ~1.5k members, whose 2F1
    series diverges (HDPM_E_GSL) unless it is summed in log space."""
    ds = R.synth(3000, 16, 2, 2, seed=3)
    cfg = dict(ds=ds, c=np.ascontiguousarray(ds.truth, np.int32), pseed=3, rseed=1, logspace=True)
    eng = engine_start(hd, oracle, cfg)
    try:
        eng.split_and_merge(2, 2, 0)
        R.check_self(eng.sm_last_terms(), "log-space move")
        eng.set_hig_logspace(False)
        with pytest.raises(hd.HdpmError) as e:
            eng.split_and_merge(2, 2, 1)
        assert e.value.status == 2
        assert eng.sm_last_terms()["kind"] == 0
    finally:
        eng.close()


# ------------------------------------------------------------------ logprobgs_c_i directly
def lpgs_three_ways(hd, oracle, case):
    ds, c, cen, sig, g, S, i1, i2 = case
    eng = hd.Engine(0)
    try:
        eng.set_data(ds.codes, ds.attrisize, ds.gamma, ds.v, ds.w)
        eng.set_state(c, cen, sig)
        got = eng.logprobgs_c_i(g, S, i1, i2)
    finally:
        eng.close()
    ref = oracle.logprobgs_c_i(ds.codes, ds.attrisize, oracle.OracleState(c, 3, cen, sig), g, S, i1, i2)
    mine = R.lpgs_fsum(ds.codes, ds.attrisize, c, cen, sig, g, S, i1, i2)
    return got, ref, mine


@pytest.mark.parametrize("nS,d", R.LPGS_SIZES)
def test_logprobgs_c_i_sizes(hd, oracle, nS, d):
    """|S| across wave, workgroup and block-partial boundaries; d across the tail chunk, the
    8-deep prefetch and the 64 KiB limit of k_sm_ll_lds (1928: k_sm_ll)."""
    got, ref, mine = lpgs_three_ways(hd, oracle, R.lpgs_case(nS, d, (2, 6), 100 + nS + d, stray=(nS == 257)))
    print(f"\n[lpgs] |S| {nS} d {d}: engine {got!r} oracle {ref!r} fsum {mine!r} "
          f"rel {abs(got - ref) / max(1.0, abs(ref)):.3g} / {abs(got - mine) / max(1.0, abs(mine)):.3g}")
    assert math.isfinite(ref) and math.isfinite(mine)
    assert R.close(got, ref), (got, ref)
    assert R.close(got, mine), (got, mine)


def test_logprobgs_c_i_launch_label_outside_both_clusters(hd, oracle):
    """One S point whose launch label is neither c(i1) nor c(i2) (side_ref 2): both sizes count
    in full for it.  Reachable through the C ABI only."""
    case = R.lpgs_case(300, 16, (2, 6), 77, stray=True)
    g, S = case[4], case[5]
    assert sum(int(g[s]) == 2 for s in S) == 1
    got, ref, mine = lpgs_three_ways(hd, oracle, case)
    assert R.close(got, ref), (got, ref)
    assert R.close(got, mine), (got, mine)


@pytest.mark.parametrize("nS,q", [(300, 64), (600, 256 + 70)])
def test_logprobgs_c_i_underflow_is_minus_infinity(hd, oracle, nS, q):
    """A point on the side whose probability underflows to exactly 0 contributes log(0) = -inf,
    and the sum is -inf as the reference's (which rejects a merge), not the NaN a compensated
    sum makes of inf - inf (min(0, NaN) = 0 would accept it).  The -inf lane is the first of a
    wave of block 0 (the kernel's sums) or lies in block 1 of 3 (the host merge of the blocks).
    Before the sums were made infinity-safe this returned NaN."""
    ds, c, cen, sig, g, S, i1, i2, p = R.lpgs_underflow_case(nS, q)
    L, _ = oracle.loglik_matrix(ds.codes, ds.attrisize, cen, sig)
    assert L[p, 1 - c[p]] - L[p, c[p]] > 745.2 + 7.0, L[p]
    got, ref, mine = lpgs_three_ways(hd, oracle, (ds, c, cen, sig, g, S, i1, i2))
    print(f"\n[lpgs underflow] |S| {nS} q {q}: engine {got!r} oracle {ref!r} fsum {mine!r}")
    assert ref == -math.inf and mine == -math.inf, (ref, mine)
    assert got == -math.inf, got
