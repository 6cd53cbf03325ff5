"""MI355X: posterior point estimates from the saved labels with no N x N matrix
(csrc/trace_summary.hip through LabelTrace) against numpy: the contingency tables as
bincounts, the integer sums exactly, and the losses against the dense definitions of
tests/test_gpu_posterior.py restated (psm_ref / vi_lb_ref) and mcclust.ext's VI double loop."""
import math

import numpy as np
import pytest

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def hd():
    import split_and_merge_gibbs_sampling_amd as hd
    hd.build()
    return hd


# ------------------------------------------------------------------ numpy references

def dense(rows):
    """each row relabelled 0..K-1, as LabelTrace does"""
    rows = np.atleast_2d(np.asarray(rows))
    return np.stack([np.unique(r, return_inverse=True)[1] for r in rows]).astype(np.int64)


def tables_ref(c, tr):
    """T^m[a][b] of one candidate against every draw: M x 256 x 256"""
    return np.stack([np.bincount(c * 256 + z, minlength=65536).reshape(256, 256) for z in tr])


def terms_ref(cands, tr):
    M, N = tr.shape
    all_ = np.zeros(N, np.int64)
    for z in tr:
        all_ += np.bincount(z, minlength=256)[z]
    same = np.zeros((len(cands), N), np.int64)
    for k, c in enumerate(cands):
        for z in tr:
            same[k] += np.bincount(c * 256 + z, minlength=65536)[c * 256 + z]
    return all_, same


def c2(x):
    return x * (x - 1) // 2


def q_ref(c, tr):
    return sum(int(c2(np.bincount(c * 256 + z, minlength=65536).astype(object)).sum()) for z in tr)


def psm_ref(tr):
    M, N = tr.shape
    cnt = np.zeros((N, N), np.int64)
    for m in range(M):
        cnt += tr[m][:, None] == tr[m][None, :]
    return cnt / M


def vi_lb_ref(cl, psm):
    n = psm.shape[0]
    f = 0.0
    for i in range(n):
        ind = cl == cl[i]
        f += (math.log2(ind.sum()) + math.log2(psm[i].sum()) - 2 * math.log2((ind * psm[i]).sum())) / n
    return f


def vi_ref(cl, tr):
    """mcclust.ext VI(cls, cls.draw): the double loop over points and draws"""
    M, n = tr.shape
    f = 0.0
    for i in range(n):
        ind = cl == cl[i]
        f += math.log2(ind.sum())
        for m in range(M):
            indm = tr[m] == tr[m][i]
            f += (math.log2(indm.sum()) - 2 * math.log2((ind * indm).sum())) / M
    return f / n


def binder_ref(c, psm):
    N = psm.shape[0]
    return np.abs((c[:, None] == c[None, :]) - psm)[np.triu_indices(N, 1)].sum()


def check_exact(t, cands, tr, with_tables=True):
    """tables, all and same of LabelTrace `t` against numpy, for relabelled inputs"""
    all_, same = t.terms(cands)
    want_all, want_same = terms_ref(cands, tr)
    assert all_.dtype == np.uint64 and same.dtype == np.uint64
    assert np.array_equal(all_.astype(np.int64), want_all)
    assert np.array_equal(same.astype(np.int64), want_same)
    if with_tables:
        got = t.tables(cands, 0, tr.shape[0])
        for k, c in enumerate(cands):
            assert np.array_equal(got[k], tables_ref(c, tr)), k
    return all_, same


# ------------------------------------------------------------------ 1. exact integers

@pytest.mark.parametrize("N,M,K", [(1000, 37, 12), (129, 1, 254), (1, 3, 1)])
def test_exact_integers_awkward_sizes(hd, N, M, K):
    from split_and_merge_gibbs_sampling_amd.posterior import LabelTrace
    rng = np.random.default_rng(N + M)
    tr = dense(rng.integers(0, K, size=(M, N)))
    cands = [tr[0], tr[-1], np.zeros(N, np.int64), rng.integers(0, 7, N)]
    if N <= 255:
        cands.append(np.arange(N))
    cands = dense(np.stack(cands))
    t = LabelTrace(tr)
    all_, _ = check_exact(t, cands, tr)
    # the dense definition: M * psm is the matrix of co-clustering counts (rounded back to
    # the integers it was divided from), and all[i] is its row sum
    cnt = np.rint(psm_ref(tr) * M).astype(np.int64)
    assert np.array_equal(all_.astype(np.int64), cnt.sum(1))
    # a window of draws
    m0 = M // 2
    assert np.array_equal(t.tables(cands[:2], m0, M - m0)[1], tables_ref(cands[1], tr)[m0:])
    t.close()


def test_terms_with_one_output_null(hd):
    """the C call with same = NULL (only `all`: no table pass at all) and with all = NULL,
    several candidate blocks in the second; the buffers start as 0xFF.. so an output that is
    never written cannot pass"""
    from split_and_merge_gibbs_sampling_amd import Engine
    from split_and_merge_gibbs_sampling_amd._lib import ptr
    from split_and_merge_gibbs_sampling_amd.posterior import LabelTrace
    N, M, K = 1000, 37, 12
    rng = np.random.default_rng(N + M)
    tr = dense(rng.integers(0, K, size=(M, N)))
    cands = dense(np.stack([tr[0], rng.integers(0, 7, N), np.zeros(N, np.int64), tr[-1], rng.integers(0, 30, N)]))
    want_all, want_same = terms_ref(cands, tr)
    per = M * (int(cands.max()) + 1) * (int(tr.max()) + 1) * 4
    eng = Engine(0)
    t = LabelTrace(tr, engine=eng, table_budget=2 * per)     # 5 candidates: 3 blocks
    c32 = np.ascontiguousarray(cands, dtype=np.int32)
    # `all` first, on a context that has run no table pass and no gather yet
    all_ = np.full(N, np.uint64(2 ** 64 - 1))
    eng._check(eng._L.hdpm_trace_terms(eng._h, ptr(c32), len(c32), ptr(all_), None))
    assert np.array_equal(all_.astype(np.int64), want_all)
    same = np.full(cands.shape, np.uint64(2 ** 64 - 1))
    eng._check(eng._L.hdpm_trace_terms(eng._h, ptr(c32), len(c32), None, ptr(same)))
    assert np.array_equal(same.astype(np.int64), want_same)
    # and again after the other calls have left their results in the device buffers
    all_[:] = np.uint64(2 ** 64 - 1)
    eng._check(eng._L.hdpm_trace_terms(eng._h, ptr(c32[1:2]), 1, ptr(all_), None))
    assert np.array_equal(all_.astype(np.int64), want_all)
    eng._check(eng._L.hdpm_trace_terms(eng._h, ptr(c32), len(c32), None, None))
    t.close()
    eng.close()


# ------------------------------------------------------------------ 2. both table cases

def test_hot_cell_table(hd):
    """two clusters, 95% of the points in one, the candidate equal to a draw: nearly every
    add of a workgroup goes to one cell of a 2 x 2 table"""
    from split_and_merge_gibbs_sampling_amd.posterior import LabelTrace
    N, M = 4097, 16
    rng = np.random.default_rng(4097)
    tr = (rng.random((M, N)) < 0.05).astype(np.int64)
    tr = dense(tr)
    assert all(np.bincount(z).tolist()[0] > 0.93 * N and z.max() == 1 for z in tr)
    t = LabelTrace(tr)
    check_exact(t, tr[3:4], tr)
    t.close()


def test_banded_table_255_by_255(hd):
    """a draw and a candidate of 255 clusters each: 65,025 cells do not fit the LDS of a
    workgroup, so the table is counted in bands of candidate labels"""
    from split_and_merge_gibbs_sampling_amd.posterior import LabelTrace
    N = 300
    rng = np.random.default_rng(300)
    tr = dense(np.stack([rng.permutation(np.arange(N) % 255), rng.permutation(np.arange(N) % 255)]))
    cand = dense(rng.permutation(np.arange(N) % 255))
    assert tr.max() == 254 and cand.max() == 254
    t = LabelTrace(tr)
    check_exact(t, cand, tr)
    tab = t.tables(cand, 0, 2)[0]
    off = tab.sum() - sum(np.trace(x) for x in tab)
    assert off > 0          # the 45 points beyond one per cluster land off the diagonal too
    t.close()


# ------------------------------------------------------------------ 3. candidate blocks

def test_candidate_blocks_change_nothing(hd):
    from split_and_merge_gibbs_sampling_amd.posterior import LabelTrace
    N, M, K = 1000, 37, 12
    rng = np.random.default_rng(N + M)
    tr = dense(rng.integers(0, K, size=(M, N)))
    cands = dense(np.stack([tr[0], tr[5], tr[-1], np.zeros(N, np.int64), np.arange(N) % 200,
                            rng.integers(0, 7, N), rng.integers(0, 3, N), tr[7], rng.integers(0, 40, N)]))
    assert len(cands) == 9
    # one candidate's tables: M x Ka x Kz uint32; room for 3 of the 9 candidates: 3 blocks
    per = M * (int(cands.max()) + 1) * (int(tr.max()) + 1) * 4
    budget = 3 * per
    assert budget // per * 3 <= len(cands)
    whole = LabelTrace(tr)
    split = LabelTrace(tr, table_budget=budget)
    a0, s0 = whole.terms(cands)
    a1, s1 = split.terms(cands)
    assert np.array_equal(a0, a1) and np.array_equal(s0, s1)
    assert np.array_equal(whole.tables(cands, 3, 4), split.tables(cands, 3, 4))
    # the doubles bit for bit: the reduction order does not depend on the blocking
    assert whole.vi_lb(cands).tobytes() == split.vi_lb(cands).tobytes()
    assert whole.vi(cands).tobytes() == split.vi(cands).tobytes()
    assert whole.binder_terms(cands) == split.binder_terms(cands)
    assert whole.binder(cands).tobytes() == split.binder(cands).tobytes()
    # and the blocked results are right, not merely equal
    want_all, want_same = terms_ref(cands, tr)
    assert np.array_equal(a1.astype(np.int64), want_all) and np.array_equal(s1.astype(np.int64), want_same)
    assert split.binder_terms(cands)[2] == [q_ref(c, tr) for c in cands]
    whole.close()
    split.close()


# ------------------------------------------------------------------ 4. 64-bit sums

def test_sums_beyond_32_bits(hd):
    from split_and_merge_gibbs_sampling_amd.posterior import LabelTrace
    N, M = 100_000, 2
    tr = np.zeros((M, N), np.int32)
    c = np.zeros(N, np.int32)
    t = LabelTrace(tr)
    A, P, Q = t.binder_terms(c)
    assert Q == [2 * (N * (N - 1) // 2)] and Q[0] > 2 ** 32
    assert P == 2 * (N * (N - 1) // 2) and A == [N * (N - 1) // 2]
    assert t.binder(c)[0] == 0.0
    assert abs(t.vi(c)[0]) <= 1e-12 * 3 * math.log2(N)
    all_, same = t.terms(c)
    assert np.all(all_ == np.uint64(M * N)) and np.all(same == np.uint64(M * N))
    t.close()


# ------------------------------------------------------------------ 5. losses vs the dense path

@pytest.fixture(scope="module")
def zoo_chain(hd, zoo):
    res = hd.run_markov_chain(zoo.codes, zoo.attrisize, zoo.gamma, zoo.v, zoo.w, m=3, iterations=200, L=1,
                              c_i=np.zeros(zoo.n, np.int32), burnin=100, t=10, r=10, neal8=True, split_merge=True,
                              seed=3)
    tr = res["c_i"]
    psm = psm_ref(tr)
    return tr, psm


def test_losses_against_the_dense_path(hd, zoo, zoo_chain):
    from split_and_merge_gibbs_sampling_amd import posterior as P
    tr, psm = zoo_chain
    N = zoo.n
    cand = np.stack([tr[0], tr[-1], zoo.truth, np.zeros(N, np.int32), np.arange(N)])
    t = P.LabelTrace(tr)
    p = P.PSM(tr)
    got = t.vi_lb(cand)
    np.testing.assert_allclose(got, p.vi_lb(cand), rtol=1e-12, atol=0)
    np.testing.assert_allclose(got, [vi_lb_ref(c, psm) for c in cand], rtol=1e-12, atol=0)
    np.testing.assert_allclose(t.vi(cand), [vi_ref(c, tr) for c in cand], rtol=1e-12,
                               atol=1e-12 * 3 * math.log2(N))
    np.testing.assert_allclose(t.binder(cand), [binder_ref(c, psm) for c in cand], rtol=1e-12, atol=0)
    # minVI over the draws: the value of the dense path, attained by the partition returned
    cl_t, v_t = P.minvi(t, cls_draw=tr, method="draws")
    cl_p, v_p = P.minvi(p, cls_draw=tr, method="draws")
    assert v_t == pytest.approx(v_p, rel=1e-12)
    assert v_t == pytest.approx(min(vi_lb_ref(c, psm) for c in tr), rel=1e-12)
    assert t.vi_lb(cl_t)[0] == v_t
    assert cl_t.min() == 1
    # the expected VI as the loss: the smallest of the draws' reference values
    cl_v, v_v = P.minvi(t, cls_draw=tr, method="draws", loss="VI")
    assert v_v == pytest.approx(float(t.vi(tr).min()), rel=1e-12)
    assert v_v == pytest.approx(vi_ref(cl_v, tr), rel=1e-12, abs=1e-12 * 3 * math.log2(N))
    # minbinder: the draw with the smallest reference loss
    ref = np.array([binder_ref(c, psm) for c in tr])
    cl_b, v_b = P.minbinder(t, cls_draw=tr, method="draws")
    assert binder_ref(cl_b, psm) == pytest.approx(ref.min(), rel=1e-12)
    assert v_b == pytest.approx(ref.min(), rel=1e-12)
    best = np.flatnonzero(np.isclose(ref, ref.min(), rtol=1e-12, atol=0))
    assert any(np.array_equal(cl_b - 1, dense(tr[b])[0]) for b in best)
    with pytest.raises(ValueError):
        P.minvi(t, method="avg")
    with pytest.raises(ValueError):
        P.minvi(p, cls_draw=tr, method="draws", loss="VI")
    t.close()
    p.close()


# ------------------------------------------------------------------ 6. headline size

def test_headline_size(hd):
    """N = 1,000,000: the size the dense path cannot reach (4 TB of counts)"""
    from split_and_merge_gibbs_sampling_amd.posterior import LabelTrace
    N, M, K = 1_000_000, 8, 10
    rng = np.random.default_rng(5)
    truth = rng.integers(0, K, N)
    tr = np.where(rng.random((M, N)) < 0.9, truth[None, :], rng.integers(0, K, (M, N))).astype(np.int32)
    cands = np.stack([truth, rng.integers(0, K, N)]).astype(np.int32)
    assert all(np.unique(r).size == K for r in tr) and all(np.unique(r).size == K for r in cands)
    tr64, c64 = tr.astype(np.int64), cands.astype(np.int64)      # already 0..K-1: relabelling is the identity
    t = LabelTrace(tr)
    check_exact(t, c64, tr64, with_tables=False)
    A, Pn, Q = t.binder_terms(cands)
    assert Q == [q_ref(c, tr64) for c in c64]
    assert Pn == sum(int(c2(np.bincount(z).astype(object)).sum()) for z in tr64)
    v = t.vi_lb(cands)
    assert np.all(np.isfinite(v))
    assert v[0] < v[1]
    t.close()


# ------------------------------------------------------------------ 7. refusals

def test_refusals(hd):
    from split_and_merge_gibbs_sampling_amd import Engine, HdpmError
    from split_and_merge_gibbs_sampling_amd._lib import ptr
    from split_and_merge_gibbs_sampling_amd.posterior import PSM, LabelTrace
    with pytest.raises(ValueError):
        LabelTrace(np.arange(256, dtype=np.int32)[None, :])
    rng = np.random.default_rng(11)
    tr = rng.integers(0, 9, size=(11, 400)).astype(np.int32)
    eng = Engine(0)
    # no trace yet: the C call refuses with HDPM_E_ARG
    c = np.zeros((1, 400), np.int32)
    out = np.zeros(400, np.uint64)
    with pytest.raises(HdpmError) as e:
        eng._check(eng._L.hdpm_trace_terms(eng._h, ptr(c), 1, ptr(out), None))
    assert e.value.status == 5
    # a PSM and a LabelTrace in one context: the matrix is untouched by the trace calls
    p = PSM(tr, engine=eng)
    before = p.matrix()
    t = LabelTrace(tr * 1000 + 300, engine=eng)      # any label values, as PSM
    with pytest.raises(ValueError):
        t.vi_lb(np.arange(400) % 256)                # 256 clusters in a candidate
    with pytest.raises(ValueError):
        t.vi_lb(np.zeros(399, np.int32))             # wrong length
    with pytest.raises(ValueError):
        t.tables(tr[0], 5, 7)                        # m0 + nm > M
    with pytest.raises(HdpmError) as e:
        eng._check(eng._L.hdpm_trace_terms(eng._h, ptr(np.full((1, 400), 255, np.int32)), 1, ptr(out), None))
    assert e.value.status == 5
    cands = dense(np.stack([tr[0], tr[4]]))
    check_exact(t, cands, dense(tr))
    np.testing.assert_allclose(t.vi_lb(cands), p.vi_lb(cands), rtol=1e-12, atol=0)
    assert np.array_equal(p.matrix(), before) and np.array_equal(before, psm_ref(tr))
    t.close()
    p.close()
    eng.close()
