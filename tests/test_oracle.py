"""CPU tests of the oracle: pinned against R's RNG outputs, cross-checked against the
independent Python restatement (tests/pyref.py) and the committed golden traces."""
import json
import os

import numpy as np
import pytest

import pyref as P

G = os.path.join(os.path.dirname(__file__), "golden")


def test_r_runif_known_answers(oracle):
    kat = json.load(open(os.path.join(G, "r_runif_kat.json")))
    for seed, vals in kat["seeds"].items():
        got = oracle.runif(oracle.seed_state(int(seed)), 5)
        np.testing.assert_allclose(got, vals, atol=5e-8)          # R prints 7 digits
        r = P.RRng(int(seed))
        assert np.array_equal(got, [r.unif() for _ in range(5)])


def test_rng_state_roundtrip_matches_numpy_mt(oracle):
    st = oracle.seed_state(2024)
    a = oracle.runif(st, 3000)          # crosses several 624-word twists
    r = P.RRng(2024)
    b = np.array([r.unif() for _ in range(3000)])
    assert np.array_equal(a, b)
    assert np.array_equal(st, r.export())


@pytest.mark.parametrize("a,b", [(2.5, 7.0), (1.25, 5.0), (0.5, 3.0), (0.7, 0.4), (40.0, 900.0)])
def test_rbeta_matches_pyref(oracle, a, b):
    st = oracle.seed_state(11)
    got = oracle.rbeta(st, a, b, 400)
    r = P.RRng(11)
    exp = np.array([P.rbeta(r, a, b) for _ in range(400)])
    assert np.array_equal(got, exp)
    assert np.array_equal(st, r.export())
    assert abs(got.mean() - a / (a + b)) < 0.05


@pytest.mark.parametrize("v,w,m", [(6, 0.25, 2), (3, 0.5, 6), (6.0, 40.25, 2.0), (8.0, 30.25, 4.0),
                                   (2.5, 60.0, 2.0), (106.0, 3.25, 2.0)])
def test_rhig_both_branches_match_pyref(oracle, v, w, m):
    st = oracle.seed_state(5)
    got, err = oracle.rhig(st, v, w, m, 25)
    assert err == 0
    r = P.RRng(5)
    exp = np.array([P.rhig1(r, v, w, m) for _ in range(25)])
    assert np.array_equal(got, exp)
    assert np.all(got > 0)


def test_qbeta_branch_against_scipy(oracle):
    from scipy.special import betaincinv
    rng = np.random.default_rng(0)
    for _ in range(300):
        a, b = rng.uniform(1.01, 80), rng.uniform(1.01, 80)
        x = rng.uniform(0.3, 0.99)
        q = betaincinv(a, b, 0.1)
        if abs(q - x) < 1e-9:
            continue
        assert oracle.lib().orc_ffi_qbeta01_lt(a, b, x) == int(q < x)


def test_norm_const2_throws_from_200_levels(oracle):
    """The split-merge prior's constant norm_const2(w, v, m) (sm:419-436) at the usual priors:
    defined up to 100 levels, the reference throws at 200 and 255 (GSL's 2F1 at z = (m - 1) / m),
    with and without the log-space extension -- so a split-merge move is undefined on such an
    attribute (tests/test_gpu_phi_edges.py keeps its split-merge data at 64 levels)."""
    for logspace in (False, True):
        oracle.set_hig_logspace(logspace)
        try:
            for m in (2.0, 17.0, 64.0, 100.0):
                v, err = oracle.norm_const2(0.25, 6.0, m)
                assert err == 0 and np.isfinite(v), (logspace, m)
            for m in (200.0, 255.0):
                assert oracle.norm_const2(0.25, 6.0, m)[1] == 2, (logspace, m)
        finally:
            oracle.set_hig_logspace(False)


def test_norm_const2_against_mpmath(oracle):
    mp = pytest.importorskip("mpmath")
    for d, c, m in [(0.25, 6.0, 2.0), (3.5, 40.0, 4.0), (10.25, 200.0, 6.0)]:
        v, err = oracle.norm_const2(d, c, m)
        assert err == 0
        ref = float(mp.log(d + 1) + (d + c) * mp.log(m) - mp.log(mp.hyp2f1(d + c, 1, d + 2, (m - 1) / m)))
        assert abs(v - ref) < 1e-9 * max(1, abs(ref))
    # overflow of the series -> the reference throws (norm_const2 hg:43-45)
    _, err = oracle.norm_const2(0.25, 3000.0, 2.0)
    assert err == 2


def test_revsort_ties_and_order():
    a, ib = [0.2, 0.5, 0.5, 0.1], [1, 2, 3, 4]
    P.revsort(a, ib)
    assert a == sorted(a, reverse=True)
    a2, ib2 = [0.5, 0.5], [1, 2]
    P.revsort(a2, ib2)
    assert ib2 == [2, 1]        # equal pair: second index first


def test_sample_prob1_matches_pyref(oracle):
    rng = np.random.default_rng(3)
    st = oracle.seed_state(9)
    r = P.RRng(9)
    for n in (1, 2, 3, 7, 23, 64):
        for _ in range(20):
            p = rng.random(n) ** 3
            p[rng.random(n) < 0.2] = 0.0
            if p.sum() == 0:
                p[0] = 1.0
            p = p / p.sum()
            got, s = oracle.sample_prob1(st, p)
            assert s == 0 and got == P.sample_prob1(r, list(p))


def test_walker_alias_matches_pyref(oracle):
    """> 200 entries with n p > 0.1 after FixupProb: Rcpp's sample() switches to Walker's
    alias method (R random.c walker_ProbSampleReplace); C oracle vs the Python restatement,
    and the draw frequencies against p (a loose statistical check of the alias table)."""
    rng = np.random.default_rng(31)
    st = oracle.seed_state(5)
    r = P.RRng(5)
    for n in (230, 300, 403, 1000):
        for trial in range(15):
            p = rng.random(n) + (0.3 if trial % 2 else 1.0)
            if n >= 400:
                p[rng.random(n) < 0.1] = 0.0        # zero-probability entries
            if trial % 5 == 0:
                p[:3] *= 20.0                       # a few heavy entries
            assert (n * p / p.sum() > 0.1).sum() > 200
            for _ in range(4):
                got, s = oracle.sample_prob1(st, p)
                assert s == 0 and got == P.sample_prob1(r, list(p)), (n, trial)
    assert np.array_equal(st, r.export())
    # frequencies: 20000 draws over n = 300 entries with 3 heavy ones
    n = 300
    p = np.ones(n)
    p[:3] = 30.0
    p /= p.sum()
    st = oracle.seed_state(6)
    cnt = np.zeros(n)
    for _ in range(20000):
        got, s = oracle.sample_prob1(st, p)
        cnt[got] += 1
    assert abs(cnt[:3].sum() / 20000 - p[:3].sum()) < 0.02
    assert abs(cnt[3:].sum() / 20000 - p[3:].sum()) < 0.02


def test_dhamming_matches_pyref(oracle):
    for x, c, s, m in [(1, 1, 0.5, 2), (1, 2, 0.5, 2), (3, 3, 1.7, 6), (2, 5, 0.05, 6)]:
        assert oracle.lib().orc_ffi_dhamming(x, c, s, m) == P.dhamming(x, c, s, m)


def test_zoo_neal8_trace_oracle_vs_pyref_vs_golden(oracle, zoo):
    g = np.load(os.path.join(G, "zoo_neal8_seed1.npz"))
    c0 = np.zeros(zoo.n, np.int32)
    for fast in (0, 1, 2):
        st, res = oracle.run_markov_chain(zoo.codes, zoo.attrisize, zoo.gamma, zoo.v, zoo.w, m=3, iterations=40,
                                          L=1, c_i=c0, burnin=0, neal8=True, split_merge=False, seed=1, fast=fast)
        assert st == 0
        assert np.array_equal(res["c_i"], g["c_i"])
        assert np.array_equal(res["loglikelihood"], g["loglikelihood"])
    tr, lls = P.Model(zoo.codes, zoo.attrisize, zoo.gamma, zoo.v, zoo.w).run_neal8(P.RRng(1), list(c0), 3, 10)
    assert np.array_equal(np.array(tr), g["c_i"][:10])


def test_zoo_split_merge_faithful_equals_fast_and_golden(oracle, zoo):
    g = np.load(os.path.join(G, "zoo_sm_seed7.npz"))
    c0 = np.zeros(zoo.n, np.int32)
    for fast in (0, 1, 2):
        st, res = oracle.run_markov_chain(zoo.codes, zoo.attrisize, zoo.gamma, zoo.v, zoo.w, m=3, iterations=30,
                                          L=1, c_i=c0, burnin=0, t=10, r=10, neal8=True, split_merge=True,
                                          seed=7, fast=fast)
        assert st == 0
        for k in ("c_i", "total_cls", "loglikelihood", "accepted"):
            assert np.array_equal(res[k], g[k]), k
    assert g["accepted"].sum() > 0


@pytest.mark.parametrize("which", ["zoo_sm", "synth_thin3", "synth_fast2"])
def test_traced_chain_equals_untraced_and_is_consistent(oracle, zoo, which):
    """orc_run_markov_chain_trace: the trace only reads the state (every untraced result and the
    random stream position keep their bits); moves / k_all cover every iteration, the saved
    centers / sigmas are the state the saved labels and log-likelihood belong to."""
    from split_and_merge_gibbs_sampling_amd.data import hamming_mixture
    if which == "zoo_sm":
        ds, c0 = zoo, np.zeros(zoo.n, np.int32)
        kw = dict(m=3, iterations=20, L=1, c_i=c0, burnin=0, t=5, r=5, neal8=True, split_merge=True, fast=1)
    else:
        ds = hamming_mixture(1500, 16, 5, 3, seed=3)
        c0 = ds.truth
        kw = dict(m=3, iterations=8, L=1, c_i=c0, burnin=2, neal8=True, split_merge=False, thinning=3,
                  fast=1 if which == "synth_thin3" else 2)
    args = (ds.codes, ds.attrisize, ds.gamma, ds.v, ds.w)
    s0, s1 = oracle.seed_state(5), oracle.seed_state(5)
    st, ref = oracle.run_markov_chain(*args, rng=s0, **kw)
    assert st == 0
    st, res = oracle.run_markov_chain(*args, rng=s1, trace=True, **kw)
    assert st == 0
    for k in ("c_i", "total_cls", "loglikelihood", "accepted", "final_ass"):
        assert np.array_equal(res[k], ref[k]), k
    assert np.array_equal(s0, s1)
    iters, burnin, thin = kw["iterations"], kw["burnin"], kw.get("thinning", 1)
    total = (iters + burnin) * thin
    assert res["moves"].shape == res["k_all"].shape == (total,)
    assert np.all(res["moves"] >= 0) and np.all(res["moves"] <= ds.n)
    saved = [it for it in range(total) if it >= thin * burnin and it % thin == 0]
    assert np.array_equal(res["k_all"][saved], ref["total_cls"])
    assert len(res["centers"]) == len(res["sigmas"]) == iters
    for q in range(iters):
        K = int(ref["total_cls"][q])
        assert res["centers"][q].shape == res["sigmas"][q].shape == (K, ds.d)
        # the traced parameters with the saved labels reproduce the saved log-likelihood
        state = oracle.OracleState(ref["c_i"][q], K, res["centers"][q], res["sigmas"][q])
        assert oracle.compute_loglikelihood(ds.codes, ds.attrisize, state, fast=kw["fast"]) == ref["loglikelihood"][q]
    assert res["centers"][-1].shape == (ref["total_cls"][-1], ds.d)
    if thin == 1:
        prev = np.concatenate([(c0 - c0.min())[None], ref["c_i"][:-1]])
        assert np.array_equal(res["moves"], (ref["c_i"] != prev).sum(axis=1))
        assert res["moves"].sum() > 0
    # a capacity one row short of what the saved iterations need is an error, not an overrun
    st, _ = oracle.run_markov_chain(*args, seed=5, trace=True, trace_rows=int(ref["total_cls"].sum()) - 1, **kw)
    assert st == 5
    st, res2 = oracle.run_markov_chain(*args, seed=5, trace=True, trace_rows=int(ref["total_cls"].sum()), **kw)
    assert st == 0 and all(np.array_equal(a, b) for a, b in zip(res2["centers"], res["centers"]))


def test_random_init_with_unused_label_fails_validation(oracle, zoo):
    # la:28 + cf:146-172: L labels drawn at random; an unused label stops the chain.
    bad = None
    for seed in range(1, 60):
        st0 = oracle.seed_state(seed)
        u = oracle.runif(st0, zoo.n)
        if len(np.unique((20 * u + 1).astype(int) - 1)) < 20:
            bad = seed
            break
    assert bad is not None
    st, _ = oracle.run_markov_chain(zoo.codes, zoo.attrisize, zoo.gamma, zoo.v, zoo.w, m=3, iterations=2, L=20,
                                    burnin=0, neal8=True, split_merge=False, seed=bad, fast=0)
    assert st == 1


def _bits(x):
    return np.float64(x).view(np.uint64)


def test_hig_logspace_extension(oracle):
    """HDPM_OPT_HIG_LOGSPACE (an extension, not the reference): where the reference's 2F1
    series (hg:11-48) is finite within 30000 terms the log-space value has the same bits;
    where it overflows (the reference throws, hg:43-45) the value is finite and agrees with
    mpmath at 50 digits to double precision on the cancelling terms."""
    mp = pytest.importorskip("mpmath")
    try:
        for d in (0.25, 0.5, 3.5, 40.25):
            for c in (2.0, 3.0, 6.0, 57.0, 400.0, 900.0):
                for m in (2.0, 4.0, 6.0):
                    oracle.set_hig_logspace(False)
                    a, ea = oracle.norm_const2(d, c, m)
                    oracle.set_hig_logspace(True)
                    b, eb = oracle.norm_const2(d, c, m)
                    if ea == 0:
                        assert eb == 0 and _bits(a) == _bits(b), (d, c, m, a, b)
        mp.mp.dps = 50
        for d, c, m in [(0.25, 3000.0, 2.0), (0.25, 20000.0, 2.0), (5.25, 8000.0, 4.0), (2.5, 2500.0, 6.0)]:
            oracle.set_hig_logspace(False)
            _, ea = oracle.norm_const2(d, c, m)
            assert ea == 2                          # the reference throws here
            oracle.set_hig_logspace(True)
            b, eb = oracle.norm_const2(d, c, m)
            assert eb == 0 and np.isfinite(b)
            ref = float(mp.log(d + 1) + (d + c) * mp.log(m) - mp.log(mp.hyp2f1(d + c, 1, d + 2, mp.mpf(m - 1) / m, maxterms=10**6)))
            # norm_const2 = log(d + 1) + (d + c) log m - log 2F1 cancels terms of size
            # (d + c) log m; agreement to 1e-14 of that scale is double precision on them
            assert abs(b - ref) <= 1e-14 * (d + c) * np.log(m), (d, c, m, b, ref)
    finally:
        oracle.set_hig_logspace(False)


@pytest.mark.parametrize("init", ["one", "truth", "singletons"])
def test_optimised_oracle_sweep_is_bit_identical(oracle, init):
    """fast=2 (src/fast.c: tables, uniforms drawn ahead, parallel log-likelihoods) against
    fast=1 (model.c, per-term dhamming): labels, K, parameters, stream and loglik."""
    from split_and_merge_gibbs_sampling_amd.data import hamming_mixture
    ds = hamming_mixture(1500, 24, 6, (2, 5), seed=3)
    rng = np.random.default_rng(4)
    if init == "one":
        c = np.zeros(ds.n, np.int32)
    elif init == "truth":
        c = ds.truth.astype(np.int32)
    else:
        c = (np.arange(ds.n) % 300).astype(np.int32)
    K = int(c.max()) + 1
    cen = np.stack([rng.integers(1, ds.attrisize + 1) for _ in range(K)]).astype(np.float64)
    sig = rng.uniform(0.2, 2.0, size=(K, ds.d))
    st = oracle.seed_state(11)
    pc, ps, _ = oracle.pool_generate(ds.attrisize, ds.v, ds.w, ds.n * 3, st)
    a, b = oracle.OracleState(c, K, cen, sig), oracle.OracleState(c, K, cen, sig)
    ra, rb = st.copy(), st.copy()
    for sweep in range(4):
        assert oracle.neal8_sweep(ds.codes, ds.attrisize, ds.gamma, ds.v, ds.w, a, 3, pc, ps, ra, fast=1) == 0
        assert oracle.neal8_sweep(ds.codes, ds.attrisize, ds.gamma, ds.v, ds.w, b, 3, pc, ps, rb, fast=2) == 0
        assert a.K == b.K and np.array_equal(a.c_i, b.c_i) and np.array_equal(ra, rb), sweep
        assert np.array_equal(a.centers[:a.K], b.centers[:b.K]) and np.array_equal(a.sigma[:a.K], b.sigma[:b.K])
        assert oracle.update_phi(ds.codes, ds.attrisize, ds.v, ds.w, a, ra) == 0
        assert oracle.update_phi(ds.codes, ds.attrisize, ds.v, ds.w, b, rb) == 0
        l1 = oracle.compute_loglikelihood(ds.codes, ds.attrisize, a)
        l2 = oracle.compute_loglikelihood(ds.codes, ds.attrisize, b, fast=2)
        assert _bits(l1) == _bits(l2)


def test_optimised_oracle_split_merge_chain_is_bit_identical(oracle):
    from split_and_merge_gibbs_sampling_amd.data import hamming_mixture
    ds = hamming_mixture(600, 20, 4, (2, 4), seed=8)
    out = []
    for fast in (1, 2):
        st, res = oracle.run_markov_chain(ds.codes, ds.attrisize, ds.gamma, ds.v, ds.w, m=3, iterations=12, L=1,
                                          c_i=np.zeros(ds.n, np.int32), burnin=0, t=4, r=4, neal8=True,
                                          split_merge=True, seed=21, fast=fast)
        assert st == 0
        out.append(res)
    for k in ("c_i", "total_cls", "loglikelihood", "accepted"):
        assert np.array_equal(out[0][k], out[1][k]), k


@pytest.mark.parametrize("shape", [(1, 1, 1, 2), (2, 1, 1, 2), (3, 2, 2, 2), (7, 5, 3, 4), (65, 1, 2, 3)])
@pytest.mark.parametrize("m", [1, 3])
def test_tiny_shapes_oracle_vs_pyref(oracle, shape, m):
    # Edge shapes of the GPU tiny-shape parity test: the three oracle variants agree, and the
    # Neal-8 trace equals the independent Python restatement's.
    from split_and_merge_gibbs_sampling_amd.data import hamming_mixture
    n, d, k, levels = shape
    ds = hamming_mixture(n, d, k, levels, seed=40 + n + d)
    c0 = np.asarray(ds.truth, np.int32)
    outs = []
    for fast in (0, 1, 2):
        st, res = oracle.run_markov_chain(ds.codes, ds.attrisize, ds.gamma, ds.v, ds.w, m=m, iterations=5, L=1,
                                          c_i=c0, burnin=0, neal8=True, split_merge=False, seed=5, fast=fast)
        assert st == 0
        outs.append(res)
    for r in outs[1:]:
        assert np.array_equal(r["c_i"], outs[0]["c_i"])
        assert np.array_equal(r["loglikelihood"], outs[0]["loglikelihood"])
    tr, _ = P.Model(ds.codes, ds.attrisize, ds.gamma, ds.v, ds.w).run_neal8(P.RRng(5), list(c0), m, 5)
    assert np.array_equal(np.array(tr), outs[0]["c_i"])
