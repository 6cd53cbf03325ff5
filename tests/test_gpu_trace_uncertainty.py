"""MI355X: credible balls and point-to-cluster affinities from the saved labels with no
N x N matrix (csrc/trace_uncertainty.hip through LabelTrace.distances / affinity /
membership / cluster_similarity and credible_ball) against numpy on the saved labels: the
contingency tables as bincounts of c * Kz + z, aff as the sum over m of T^m[:, z_m].T, cross
as the sum over m of T^m @ T^m.T, and the distances from the same tables with Python
integers for Binder.  The small helpers of tests/test_gpu_trace_summary.py are restated."""
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


def tables_ref(c, tr, Ka, Kz):
    """T^m[a][b] of one partition against every draw: M x Ka x Kz"""
    return np.stack([np.bincount(c * Kz + z, minlength=Ka * Kz).reshape(Ka, Kz) for z in tr])


def aff_cross_ref(c, tr, Ka=None):
    Ka = int(c.max()) + 1 if Ka is None else Ka
    Kz = int(tr.max()) + 1
    aff = np.zeros((tr.shape[1], Ka), np.int64)
    cross = np.zeros((Ka, Ka), np.int64)
    for z in tr:
        T = np.bincount(c * Kz + z, minlength=Ka * Kz).reshape(Ka, Kz)
        aff += T[:, z].T
        cross += T @ T.T
    return aff, cross


def c2(x):
    return x * (x - 1) // 2


def xlog2x(x):
    x = np.asarray(x, np.float64)
    return np.where(x > 0, x * np.log2(np.maximum(x, 1.0)), 0.0)


def distances_ref(c, tr):
    """(vi[M], binder[M] as Python ints, draw_k[M]) of one partition against every draw"""
    M, N = tr.shape
    Ka, Kz = int(c.max()) + 1, int(tr.max()) + 1
    na = np.bincount(c, minlength=Ka)
    A = int(c2(na.astype(object)).sum())
    vi, binder, k = [], [], []
    for z in tr:
        nz = np.bincount(z, minlength=Kz)
        T = np.bincount(c * Kz + z, minlength=Ka * Kz)
        binder.append(A + int(c2(nz.astype(object)).sum()) - 2 * int(c2(T.astype(object)).sum()))
        vi.append((xlog2x(na).sum() + xlog2x(nz).sum() - 2 * xlog2x(T).sum()) / N)
        k.append(int((nz > 0).sum()))
    return np.array(vi), binder, k


def vi_atol(N):
    return 1e-12 * 3 * math.log2(N)


def check_affinity(t, c, tr, Ka=None):
    """aff and cross of LabelTrace `t` for the relabelled partition c against numpy, and the
    identities that tie them to each other and to `terms`"""
    from split_and_merge_gibbs_sampling_amd._lib import ptr
    N = tr.shape[1]
    if Ka is None:
        aff, cross = t.affinity(c)
        Ka = int(c.max()) + 1
    else:
        aff = np.full((N, Ka), np.uint64(2 ** 64 - 1))
        cross = np.full((Ka, Ka), np.uint64(2 ** 64 - 1))
        c32 = np.ascontiguousarray(c, dtype=np.int32)
        t.eng._check(t.eng._L.hdpm_trace_affinity(t.eng._h, ptr(c32), Ka, ptr(aff), ptr(cross)))
    assert aff.dtype == np.uint64 and cross.dtype == np.uint64
    assert aff.shape == (N, Ka) and cross.shape == (Ka, Ka)
    want_aff, want_cross = aff_cross_ref(c, tr, Ka)
    aff, cross = aff.astype(np.int64), cross.astype(np.int64)
    assert np.array_equal(aff, want_aff)
    assert np.array_equal(cross, want_cross)
    assert np.array_equal(cross, cross.T)
    onehot = np.zeros((N, Ka), np.int64)
    onehot[np.arange(N), c] = 1
    assert np.array_equal(cross, onehot.T @ aff)
    all_, same = t.terms(c)
    assert np.array_equal(aff.sum(1), all_.astype(np.int64))
    assert np.array_equal(aff[np.arange(N), c], same[0].astype(np.int64))
    return aff, cross


# ------------------------------------------------------------------ 1. exact integers

@pytest.mark.parametrize("N,M,K", [(1000, 37, 12), (129, 1, 254), (1, 3, 1), (257, 40, 5)])
def test_exact_integers_awkward_sizes(hd, N, M, K):
    from split_and_merge_gibbs_sampling_amd.posterior import LabelTrace
    rng = np.random.default_rng(N + M)
    tr = dense(rng.integers(0, K, size=(M, N)))
    cands = dense(np.stack([tr[M // 2], np.zeros(N, np.int64), rng.integers(0, 7, N)]))
    t = LabelTrace(tr)
    for c in cands:
        check_affinity(t, c, tr)
    vi, binder, draw_k = t.distances(cands)
    assert vi.shape == (3, M) and binder.shape == (3, M) and binder.dtype == np.uint64
    for q, c in enumerate(cands):
        want_vi, want_b, want_k = distances_ref(c, tr)
        assert [int(x) for x in binder[q]] == want_b
        assert draw_k.tolist() == want_k
        np.testing.assert_allclose(vi[q], want_vi, rtol=1e-12, atol=vi_atol(N))
    if N <= 300:
        # per-draw Binder is the brute-force count of pairs on which the partitions disagree
        iu = np.triu_indices(N, 1)
        for q, c in enumerate(cands):
            for m in (0, M - 1):
                dis = (c[:, None] == c[None, :]) != (tr[m][:, None] == tr[m][None, :])
                assert int(binder[q][m]) == int(dis[iu].sum())
    t.close()


def test_outputs_may_be_null(hd):
    """each output alone through the C call; buffers start as 0xFF.. so that an output never
    written cannot pass"""
    from split_and_merge_gibbs_sampling_amd._lib import ptr
    from split_and_merge_gibbs_sampling_amd.posterior import LabelTrace
    N, M, K = 257, 40, 5
    rng = np.random.default_rng(N + M)
    tr = dense(rng.integers(0, K, size=(M, N)))
    c = dense(rng.integers(0, 7, N))
    c32 = np.ascontiguousarray(c, dtype=np.int32)
    Ka = int(c.max()) + 1
    want_aff, want_cross = aff_cross_ref(c[0], tr)
    want_vi, want_b, want_k = distances_ref(c[0], tr)
    t = LabelTrace(tr)
    L, h = t.eng._L, t.eng._h
    k = np.full(M, -1, np.int32)
    t.eng._check(L.hdpm_trace_distances(h, ptr(c32), 1, None, None, ptr(k)))
    assert k.tolist() == want_k
    b = np.full((1, M), np.uint64(2 ** 64 - 1))
    t.eng._check(L.hdpm_trace_distances(h, ptr(c32), 1, None, ptr(b), None))
    assert [int(x) for x in b[0]] == want_b
    v = np.full((1, M), -1.0)
    t.eng._check(L.hdpm_trace_distances(h, ptr(c32), 1, ptr(v), None, None))
    np.testing.assert_allclose(v[0], want_vi, rtol=1e-12, atol=vi_atol(N))
    t.eng._check(L.hdpm_trace_distances(h, ptr(c32), 1, None, None, None))
    aff = np.full((N, Ka), np.uint64(2 ** 64 - 1))
    t.eng._check(L.hdpm_trace_affinity(h, ptr(c32), Ka, ptr(aff), None))
    assert np.array_equal(aff.astype(np.int64), want_aff)
    cross = np.full((Ka, Ka), np.uint64(2 ** 64 - 1))
    t.eng._check(L.hdpm_trace_affinity(h, ptr(c32), Ka, None, ptr(cross)))
    assert np.array_equal(cross.astype(np.int64), want_cross)
    t.eng._check(L.hdpm_trace_affinity(h, ptr(c32), Ka, None, None))
    t.close()


# ------------------------------------------------------------------ 2. widest tables

def test_widest_tables(hd):
    """255 clusters in the partition and in the draws: the banded path of k_tr_tables; and
    Ka = 255 passed for a 3-cluster partition: 252 zero columns of aff, zero rows of cross"""
    from split_and_merge_gibbs_sampling_amd.posterior import LabelTrace
    N, M = 4096, 3
    rng = np.random.default_rng(4096)
    tr = dense(np.stack([rng.permutation(np.arange(N) % 255) for _ in range(M)]))
    wide = dense(rng.permutation(np.arange(N) % 255))[0]
    assert tr.max() == 254 and wide.max() == 254
    t = LabelTrace(tr)
    check_affinity(t, wide, tr)
    three = dense(rng.integers(0, 3, N))[0]
    aff, cross = check_affinity(t, three, tr, Ka=255)
    assert not aff[:, 3:].any() and not cross[3:].any() and not cross[:, 3:].any()
    t.close()


# ------------------------------------------------------------------ 3. 64-bit sums

def test_sums_beyond_32_bits(hd):
    """cross[0][0] = M N^2 = 9.8e9 needs 64 bits.  aff cannot exceed 32 bits at a size a test
    can afford (it needs M N > 4.29e9); its accumulators are 64-bit by construction."""
    from split_and_merge_gibbs_sampling_amd.posterior import LabelTrace
    N, M = 70000, 2
    t = LabelTrace(np.zeros((M, N), np.int32))
    aff, cross = t.affinity(np.zeros(N, np.int32))
    assert cross.shape == (1, 1) and int(cross[0, 0]) == M * N * N and int(cross[0, 0]) > 2 ** 32
    assert aff.shape == (N, 1) and np.all(aff == np.uint64(M * N))
    vi, binder, k = t.distances(np.zeros(N, np.int32))
    assert not binder.any() and k.tolist() == [1, 1]
    assert np.all(vi >= 0) and np.all(vi <= vi_atol(N))
    t.close()


# ------------------------------------------------------------------ 4. blocks change nothing

def test_blocks_change_nothing(hd):
    from split_and_merge_gibbs_sampling_amd.posterior import LabelTrace
    N, M, K = 1000, 37, 12
    rng = np.random.default_rng(N + M)
    tr = dense(rng.integers(0, K, size=(M, N)))
    c = dense(rng.integers(0, 7, N))[0]
    # 4096 bytes: 73 points of aff per block at Ka = 7 -> 64 (groups of 16): 16 blocks of
    # points; and one candidate per block of tables (37 x 7 x 12 x 4 bytes > 4096)
    whole = LabelTrace(tr)
    split = LabelTrace(tr, table_budget=4096)
    a0, x0 = whole.affinity(c)
    a1, x1 = split.affinity(c)
    assert np.array_equal(a0, a1) and np.array_equal(x0, x1)
    want_aff, want_cross = aff_cross_ref(c, tr)
    assert np.array_equal(a1.astype(np.int64), want_aff) and np.array_equal(x1.astype(np.int64), want_cross)
    # 70 candidates: more than one block of 64 at the default budget, 70 blocks at 4096 bytes
    cands = dense(np.stack([tr[m % M] if m % 3 else rng.integers(0, 2 + m % 9, N) for m in range(70)]))
    v0, b0, k0 = whole.distances(cands)
    v1, b1, k1 = split.distances(cands)
    assert v0.tobytes() == v1.tobytes() and np.array_equal(b0, b1) and np.array_equal(k0, k1)
    for q in range(70):
        v, b, _ = whole.distances(cands[q])
        assert v.tobytes() == v0[q].tobytes() and np.array_equal(b[0], b0[q]), q
    for q in (0, 1, 69):
        want_vi, want_b, _ = distances_ref(cands[q], tr)
        assert [int(x) for x in b0[q]] == want_b
        np.testing.assert_allclose(v0[q], want_vi, rtol=1e-12, atol=vi_atol(N))
    whole.close()
    split.close()


# ------------------------------------------------------------------ 5. distances vs the losses

def test_distances_against_the_existing_losses(hd):
    from split_and_merge_gibbs_sampling_amd.posterior import LabelTrace
    N, M, K = 1000, 37, 12
    rng = np.random.default_rng(N + M)
    truth = rng.integers(0, K, N)
    tr = dense(np.where(rng.random((M, N)) < 0.8, truth[None, :], rng.integers(0, K, (M, N))))
    tr[9] = tr[4]                                  # two draws with equal labels
    cands = dense(np.stack([tr[4], truth, np.zeros(N, np.int64), rng.integers(0, 7, N)]))
    t = LabelTrace(tr)
    vi, binder, _ = t.distances(cands)
    A, P, Q = t.binder_terms(cands)
    atol = vi_atol(N)
    for q, c in enumerate(cands):
        assert sum(int(x) for x in binder[q]) == M * A[q] + P - 2 * Q[q]
        want_vi, want_b, _ = distances_ref(c, tr)
        np.testing.assert_allclose(vi[q], want_vi, rtol=1e-12, atol=atol)
        assert [int(x) for x in binder[q]] == want_b
    np.testing.assert_allclose(vi.mean(1), t.vi(cands), rtol=1e-12, atol=atol)
    # the candidate that is draw 4 (and draw 9)
    for m in (4, 9):
        assert int(binder[0][m]) == 0
        assert 0.0 <= vi[0][m] <= atol
    assert vi[:, 4].tobytes() == vi[:, 9].tobytes()          # equal draws: bit-equal distances
    assert np.all(vi >= 0)
    t.close()


# ------------------------------------------------------------------ 6. credible ball

def ball_ref(d, k, alpha):
    """the rule of posterior._ball restated"""
    d, k = np.asarray(d), np.asarray(k)
    M = d.size
    r = np.sort(d)[min(max(math.ceil((1 - alpha) * M), 1), M) - 1]
    ball = [m for m in range(M) if d[m] <= r]
    hor = [m for m in ball if d[m] == max(d[j] for j in ball)]
    few = [m for m in ball if k[m] == min(k[j] for j in ball)]
    most = [m for m in ball if k[m] == max(k[j] for j in ball)]
    up = [m for m in few if d[m] == max(d[j] for j in few)]
    lo = [m for m in most if d[m] == max(d[j] for j in most)]
    return r, ball, hor, up, lo


def constructed_trace():
    """N = 96, M = 60: a base of 4 x 24 points; draws with m % 6 == 1 merge two clusters
    (K = 3), those with m % 6 == 2 split one (K = 5), the others move a few points (draw 3
    moves 14 and keeps K = 4); the last six draws are uniform random 6-cluster partitions"""
    N, M = 96, 60
    rng = np.random.default_rng(96)
    base = np.repeat(np.arange(4), 24)
    tr = np.tile(base, (M, 1))
    for m in range(M - 6):
        if m % 6 == 1:
            tr[m][tr[m] == 3] = 2
        elif m % 6 == 2:
            tr[m][36:48] = 4
        else:
            pts = rng.choice(N, 14 if m == 3 else 1 + m % 3, replace=False)      # draw 3: the farthest of the ball
            tr[m][pts] = (tr[m][pts] + 1 + rng.integers(0, 3, pts.size)) % 4
    for m in range(M - 6, M):
        tr[m] = rng.permutation(np.arange(N) % 6)
    return base, tr


def test_credible_ball_on_a_constructed_trace(hd):
    from split_and_merge_gibbs_sampling_amd import credible_ball
    from split_and_merge_gibbs_sampling_amd.posterior import LabelTrace
    base, tr = constructed_trace()
    M = tr.shape[0]
    t = LabelTrace(tr)
    vi, binder, k = t.distances(base)
    want_vi, want_b, want_k = distances_ref(base, dense(tr))
    assert k.tolist() == want_k and [int(x) for x in binder[0]] == want_b
    for dist, d in (("VI", vi[0]), ("Binder", binder[0])):
        for alpha in (0.05, 0.1, 0.5):
            got = credible_ball(t, base, dist=dist, alpha=alpha)
            assert got["distances"].tobytes() == d.tobytes()
            r, ball, hor, up, lo = ball_ref(d, k, alpha)
            assert got["radius"] == r
            assert got["ball"].tolist() == ball
            assert got["horizontal"].tolist() == hor
            assert got["upper_vertical"].tolist() == up
            assert got["lower_vertical"].tolist() == lo
            assert got["horizontal_distance"] == d[hor[0]]
            assert got["upper_vertical_distance"] == d[up[0]]
            assert got["lower_vertical_distance"] == d[lo[0]]
    # the shape this trace was built for, at alpha = 0.1 in VI: the six random draws fall
    # outside, the vertical bounds are the tie sets of the merged and of the split draws, and
    # the horizontal bound is apart from both
    got = credible_ball(t, base, dist="VI", alpha=0.1)
    merged = [m for m in range(M - 6) if m % 6 == 1]
    split = [m for m in range(M - 6) if m % 6 == 2]
    assert got["ball"].tolist() == list(range(M - 6))
    assert got["upper_vertical"].tolist() == merged and len(merged) == 9
    assert got["lower_vertical"].tolist() == split and len(split) == 9
    assert got["horizontal"].tolist() == [3]
    with pytest.raises(ValueError):
        credible_ball(t, base, dist="L2")
    t.close()


# ------------------------------------------------------------------ 7. against the dense path

def test_membership_and_similarity_against_the_dense_path(hd, zoo):
    from split_and_merge_gibbs_sampling_amd import posterior as P
    res = hd.run_markov_chain(zoo.codes, zoo.attrisize, zoo.gamma, zoo.v, zoo.w, m=3, iterations=200, L=1,
                              c_i=np.zeros(zoo.n, np.int32), burnin=100, t=10, r=10, neal8=True, split_merge=True,
                              seed=3)
    tr = res["c_i"]
    M, N = tr.shape
    t = P.LabelTrace(tr)
    cl, _ = P.minvi_avg(t)
    c = dense(cl)[0]
    Ka = int(c.max()) + 1
    p = P.PSM(tr)
    psm = p.matrix()
    p.close()
    # psm = count / M: the counts back as integers, combined as integers, one division each
    cnt = np.rint(psm * M).astype(np.int64)
    onehot = np.zeros((N, Ka), np.int64)
    onehot[np.arange(N), c] = 1
    n = onehot.sum(0)
    # the mean psm of i with the members of a, the point itself (psm_ii = 1) excluded
    num = cnt @ onehot - M * onehot
    den = M * (n[None, :] - onehot)
    want = np.where(den > 0, num / np.maximum(den, 1), 1.0)
    got = t.membership(cl)
    assert got.shape == (N, Ka) and got.min() >= 0.0 and got.max() <= 1.0
    np.testing.assert_allclose(got, want, rtol=1e-12, atol=0)
    blk = (onehot.T @ cnt @ onehot).tolist()
    n = n.tolist()
    want = np.ones((Ka, Ka))
    for a in range(Ka):
        for b in range(Ka):
            if a != b:
                want[a, b] = blk[a][b] / (M * n[a] * n[b])
            elif n[a] > 1:
                want[a, a] = (blk[a][a] - M * n[a]) / (M * n[a] * (n[a] - 1))
    np.testing.assert_allclose(t.cluster_similarity(cl), want, rtol=1e-12, atol=0)
    # aff == (M psm) @ onehot, in integers
    aff, _ = t.affinity(cl)
    assert np.array_equal(aff.astype(np.int64), cnt @ onehot)
    t.close()


# ------------------------------------------------------------------ 8. a larger shape

def test_larger_shape(hd):
    from split_and_merge_gibbs_sampling_amd.posterior import LabelTrace
    N, M, K = 100_000, 16, 20
    rng = np.random.default_rng(8)
    truth = rng.integers(0, K, N)
    tr = np.where(rng.random((M, N)) < 0.9, truth[None, :], rng.integers(0, K, (M, N)))
    assert all(np.unique(r).size == K for r in tr)       # already 0..K-1: relabelling is the identity
    t = LabelTrace(tr)
    aff, cross = t.affinity(truth)
    want_aff, want_cross = aff_cross_ref(truth, tr)
    assert np.array_equal(aff.astype(np.int64), want_aff)
    assert np.array_equal(cross.astype(np.int64), want_cross)
    t.close()


# ------------------------------------------------------------------ 9. refusals

def test_refusals(hd):
    from split_and_merge_gibbs_sampling_amd import Engine, HdpmError
    from split_and_merge_gibbs_sampling_amd._lib import ptr
    from split_and_merge_gibbs_sampling_amd.posterior import LabelTrace
    N, M = 400, 11
    rng = np.random.default_rng(11)
    tr = rng.integers(0, 9, size=(M, N)).astype(np.int32)
    eng = Engine(0)
    L, h = eng._L, eng._h
    c = np.ascontiguousarray(rng.integers(0, 5, size=(1, N)), dtype=np.int32)
    c[0, :5] = np.arange(5)
    aff, cross = np.zeros((N, 5), np.uint64), np.zeros((5, 5), np.uint64)
    vi, b, k = np.zeros((1, M)), np.zeros((1, M), np.uint64), np.zeros(M, np.int32)

    def refused(status):
        with pytest.raises(HdpmError) as e:
            eng._check(status())
        assert e.value.status == 5
        return str(e.value)

    # no trace yet
    assert "hdpm_trace_build" in refused(lambda: L.hdpm_trace_distances(h, ptr(c), 1, ptr(vi), ptr(b), ptr(k)))
    assert "hdpm_trace_build" in refused(lambda: L.hdpm_trace_affinity(h, ptr(c), 5, ptr(aff), ptr(cross)))
    t = LabelTrace(tr, engine=eng)
    for Ka in (0, 256):
        assert "Ka" in refused(lambda: L.hdpm_trace_affinity(h, ptr(c), Ka, ptr(aff), ptr(cross)))
    assert "Ka" in refused(lambda: L.hdpm_trace_affinity(h, ptr(c), 4, ptr(aff), ptr(cross)))      # a label >= Ka
    bad = c.copy()
    bad[0, 7] = 255
    refused(lambda: L.hdpm_trace_affinity(h, ptr(bad), 255, ptr(aff), ptr(cross)))
    refused(lambda: L.hdpm_trace_distances(h, ptr(bad), 1, ptr(vi), ptr(b), ptr(k)))
    bad[0, 7] = -1
    refused(lambda: L.hdpm_trace_affinity(h, ptr(bad), 5, ptr(aff), ptr(cross)))
    refused(lambda: L.hdpm_trace_distances(h, ptr(c), 0, ptr(vi), ptr(b), ptr(k)))                  # ncand = 0
    refused(lambda: L.hdpm_trace_distances(h, None, 1, ptr(vi), ptr(b), ptr(k)))
    with pytest.raises(ValueError):
        t.affinity(np.zeros((2, N), np.int32))           # one partition only
    with pytest.raises(ValueError):
        t.membership(np.zeros(N - 1, np.int32))
    # and the calls still work after the refusals
    check_affinity(t, c[0].astype(np.int64), dense(tr))
    t.close()
    eng.close()
