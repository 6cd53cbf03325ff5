"""MI355X: minVI(method = "avg") / minbinder(method = "avgl") from the saved labels with no
N x N matrix (csrc/trace_summary.hip k_tg_*, csrc/trace_tree.hpp through LabelTrace.groups /
avg_tree / cut and minvi_avg / minbinder_avg) against numpy and fractions.Fraction: the
groups by np.unique of the label columns, S by broadcasting, the greedy merge loop with the
tie rule of include/hdpm.h, the losses by the trace's own dense-checked entry points, and
the whole search against scipy's average linkage on the dense matrix."""
import math
from fractions import Fraction

import numpy as np
import pytest

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def hd():
    import split_and_merge_gibbs_sampling_amd as hd
    hd.build()
    return hd


@pytest.fixture(scope="module")
def eng(hd):
    e = hd.Engine(0)
    yield e
    e.close()


# ------------------------------------------------------------------ numpy references

def dense(rows):
    """each row relabelled 0..K-1, as LabelTrace does"""
    rows = np.atleast_2d(np.asarray(rows))
    return np.stack([np.unique(r, return_inverse=True)[1] for r in rows]).astype(np.int64)


def first_appearance(cl):
    """labels 0..k-1 in order of first appearance"""
    _, idx, inv = np.unique(cl, return_index=True, return_inverse=True)
    rank = np.empty(idx.size, np.int64)
    rank[np.argsort(idx)] = np.arange(idx.size)
    return rank[inv.ravel()]


def groups_ref(tr):
    """(first, weight, group_of, sig): the distinct columns ordered by first index"""
    cols = np.ascontiguousarray(tr.T)
    _, idx, inv, cnt = np.unique(cols, axis=0, return_index=True, return_inverse=True, return_counts=True)
    order = np.argsort(idx)
    rank = np.empty(order.size, np.int64)
    rank[order] = np.arange(order.size)
    return idx[order], cnt[order], rank[inv.ravel()], cols[idx[order]]


def counts_ref(sig):
    U, M = sig.shape
    S = np.zeros((U, U), np.int64)
    for m in range(M):
        S += sig[:, m][:, None] == sig[:, m][None, :]
    return S


def tree_ref(w, S):
    """The greedy merge list.  Groups are numbered by ascending `first`, so the tie rule reads:
    among the pairs with the largest Q_AB / (w_A w_B), the smallest (min index, max index).
    The float ratio only shortlists the pairs within 1e-9 of the largest; Fractions decide."""
    U = len(w)
    w = [int(x) for x in w]
    Q = (S.astype(object) * np.outer(np.array(w, object), np.array(w, object)))
    Q = Q.astype(np.int64)               # N^2 M < 2^53 at the test sizes
    wf = np.array(w, np.float64)
    R = Q / np.outer(wf, wf)
    R[np.tril_indices(U)] = -1.0
    merge = []
    for _ in range(U - 1):
        top = R.max()
        cand = np.argwhere(R >= top * (1 - 1e-9))
        best = None
        for a, b in cand:
            key = (-Fraction(int(Q[a, b]), w[a] * w[b]), int(a), int(b))
            if best is None or key < best:
                best = key
        _, A, B = best
        merge.append((A, B))
        Q[A, :] += Q[B, :]
        Q[:, A] = Q[A, :]
        w[A] += w[B]
        wf[A] = w[A]
        R[B, :] = -1.0
        R[:, B] = -1.0
        live = R[A, :] >= 0
        live |= R[:, A] >= 0
        live[A] = False
        r = Q[A] / (wf[A] * wf)
        hi = np.flatnonzero(live & (np.arange(U) > A))
        lo = np.flatnonzero(live & (np.arange(U) < A))
        R[A, hi] = r[hi]
        R[lo, A] = r[lo]
    return np.array(merge, np.int64).reshape(-1, 2)


def cuts_ref(merge, group_of, U, ks):
    """{k: labels per point of the state after U - k merges, by first appearance}"""
    g = np.arange(U)
    out = {}
    if U in ks:
        out[U] = first_appearance(g[group_of])
    for s, (A, B) in enumerate(merge):
        g[g == B] = A
        k = U - s - 1
        if k in ks:
            out[k] = first_appearance(g[group_of])
    return out


_cache = {}


def case(N, M, K):
    """the trace and its reference structure, computed once per module"""
    key = (N, M, K)
    if key not in _cache:
        rng = np.random.default_rng(N * 1000 + M)
        tr = dense(np.zeros((M, N), np.int64) if K == 1 else rng.integers(0, K, size=(M, N)))
        first, weight, group_of, sig = groups_ref(tr)
        S = counts_ref(sig)
        merge = tree_ref(weight, S)
        _cache[key] = (tr, first, weight, group_of, S, merge)
    return _cache[key]


def structure(t, hash_bits=0):
    g = t.groups(hash_bits=hash_bits)
    merge, height = t.avg_tree()
    return g, merge, height


def check_structure(t, N, M, K, hash_bits=0, every_cut=True):
    tr, first, weight, group_of, S, merge = case(N, M, K)
    U = len(first)
    g, got_merge, height = structure(t, hash_bits)
    assert g["U"] == U
    assert np.array_equal(g["first"], first)
    assert np.array_equal(g["weight"], weight)
    assert np.array_equal(g["group_of"], group_of)
    assert np.array_equal(g["counts"].astype(np.int64), S)
    assert np.array_equal(got_merge.astype(np.int64), merge)
    assert np.all((height >= 0) & (height <= 1))
    ks = set(range(1, U + 1)) if every_cut else {1, 2, min(U, 7), min(U, 255), U}
    want = cuts_ref(merge, group_of, U, ks)
    for k in sorted(ks):
        assert np.array_equal(t.cut(k).astype(np.int64), want[k]), k
    return g, got_merge


# ------------------------------------------------------------------ 1. exact structure

SIZES = [(1, 3, 5), (2, 1, 2), (129, 1, 3), (130, 5, 1), (1000, 37, 12), (4099, 7, 2)]


@pytest.mark.parametrize("N,M,K", SIZES)
def test_exact_structure_awkward_sizes(hd, eng, N, M, K):
    from split_and_merge_gibbs_sampling_amd.posterior import LabelTrace
    tr = case(N, M, K)[0]
    U = len(case(N, M, K)[1])
    if (N, M) == (130, 5):
        assert U == 1
    if (N, M) == (1000, 37):
        assert U > 255
    if (N, M) == (4099, 7):
        assert 2 < U <= 128 and case(N, M, K)[2].max() > 16
    t = LabelTrace(tr, engine=eng)
    check_structure(t, N, M, K)
    t.close()


# ------------------------------------------------------------------ 2. hash independence

@pytest.mark.parametrize("N,M,K", [(1000, 37, 12), (4099, 7, 2)])
def test_hash_independence(hd, eng, N, M, K):
    """one and four hash bits put every column in 2 / 16 home slots: grouping then rests on
    the byte-for-byte comparison and the probe sequence alone"""
    from split_and_merge_gibbs_sampling_amd.posterior import LabelTrace
    tr = case(N, M, K)[0]
    t = LabelTrace(tr, engine=eng)
    outs = []
    for bits in (1, 4, 0):
        g, merge = check_structure(t, N, M, K, hash_bits=bits, every_cut=False)
        outs.append((g, merge))
    for g, merge in outs[1:]:
        for k in ("first", "weight", "group_of", "counts"):
            assert np.array_equal(g[k], outs[0][0][k]), k
        assert np.array_equal(merge, outs[0][1])
    t.close()


# ------------------------------------------------------------------ 3. losses of the cuts

@pytest.mark.parametrize("N,M,K", [(1000, 37, 12), (4099, 7, 2), (130, 5, 1)])
def test_cut_losses_equal_the_expanded_partitions(hd, eng, N, M, K):
    from split_and_merge_gibbs_sampling_amd.posterior import LabelTrace
    tr = case(N, M, K)[0]
    t = LabelTrace(tr, engine=eng)
    U = t.groups()["U"]
    t.avg_tree()
    kmax = min(U, 255)
    cuts = np.stack([t.cut(k) for k in range(1, kmax + 1)])
    lb, vi, A, Q = t.cut_losses(1, kmax)
    want_lb, want_vi = t.vi_lb(cuts), t.vi(cuts)
    wA, _, wQ = t.binder_terms(cuts)
    print("max rel diff vi_lb", np.max(np.abs(lb - want_lb) / np.maximum(np.abs(want_lb), 1e-300)),
          "vi", np.max(np.abs(vi - want_vi) / np.maximum(np.abs(want_vi), 1e-300)))
    np.testing.assert_allclose(lb, want_lb, rtol=1e-12, atol=0)
    np.testing.assert_allclose(vi, want_vi, rtol=1e-12, atol=0)
    assert [int(x) for x in A] == wA
    assert [int(x) for x in Q] == wQ
    # a window of cuts, and the whole range again with one cut per block
    lb2, vi2, A2, Q2 = t.cut_losses(2, min(3, kmax - 1)) if kmax > 1 else (lb[1:], vi[1:], A[1:], Q[1:])
    n2 = len(lb2)
    assert lb2.tobytes() == lb[1:1 + n2].tobytes() and np.array_equal(Q2, Q[1:1 + n2]) and np.array_equal(A2, A[1:1 + n2])
    np.testing.assert_allclose(vi2, vi[1:1 + n2], rtol=1e-12, atol=0)
    t.close()
    t1 = LabelTrace(tr, engine=eng, table_budget=1)
    assert t1.groups()["U"] == U
    t1.avg_tree()
    lb1, vi1, A1, Q1 = t1.cut_losses(1, kmax)
    assert lb1.tobytes() == lb.tobytes() and vi1.tobytes() == vi.tobytes()
    assert np.array_equal(A1, A) and np.array_equal(Q1, Q)
    t1.close()


# ------------------------------------------------------------------ 4. against the dense path

def converged_like(N, M, K, flip, seed):
    r = np.random.default_rng(seed)
    base = r.integers(0, K, N)
    tr = np.tile(base, (M, 1))
    mask = r.random((M, N)) < flip
    tr[mask] = r.integers(0, K, mask.sum())
    return tr


def same_partition(a, b):
    return np.array_equal(first_appearance(np.asarray(a)), first_appearance(np.asarray(b)))


@pytest.mark.parametrize("seed", range(8))
@pytest.mark.parametrize("N,M,K,flip", [(96, 12, 3, 0.006), (120, 16, 3, 0.004), (160, 24, 4, 0.003),
                                        (200, 16, 4, 0.004)])
def test_minvi_avg_against_the_dense_path(hd, eng, N, M, K, flip, seed):
    from split_and_merge_gibbs_sampling_amd import posterior as P
    tr = converged_like(N, M, K, flip, seed)
    t = P.LabelTrace(tr, engine=eng)
    p = P.PSM(tr, engine=eng)
    cl_t, v_t = P.minvi_avg(t)
    cl_p, v_p = P.minvi(p, method="avg")
    print("k", cl_t.max(), cl_p.max(), "values", v_t, v_p)
    assert cl_t.min() == 1
    assert same_partition(cl_t, cl_p)
    assert v_t == pytest.approx(v_p, rel=1e-12)
    # minbinder_avg: the smallest Binder loss among the same cuts, on exact integers
    cl_b, v_b = P.minbinder_avg(t)
    kmax = min(math.ceil(N / 8), t.U)
    cuts = np.stack([t.cut(k) for k in range(1, kmax + 1)])
    A, Pn, Q = t.binder_terms(cuts)
    num = [M * a + Pn - 2 * q for a, q in zip(A, Q)]
    best = min(range(kmax), key=num.__getitem__)
    assert same_partition(cl_b, cuts[best])
    assert v_b == t.binder(cuts[best])[0]
    t.close()
    p.close()


# ------------------------------------------------------------------ 5. refusals

def test_refusals(hd, eng):
    from split_and_merge_gibbs_sampling_amd import HdpmError
    from split_and_merge_gibbs_sampling_amd import posterior as P
    tr = case(1000, 37, 12)[0]
    t = P.LabelTrace(tr, engine=eng)
    with pytest.raises(HdpmError) as e:
        t.avg_tree()                                   # before groups
    assert e.value.status == 5 and "hdpm_trace_groups" in str(e.value)
    with pytest.raises(HdpmError) as e:
        t.groups(max_groups=10)
    assert e.value.status == 5
    assert "max_groups = 10" in str(e.value) and "too unsettled" in str(e.value)
    with pytest.raises(HdpmError):
        t.avg_tree()                                   # the refused grouping left no groups
    with pytest.raises(HdpmError):
        t.groups(max_groups=16385)
    U = t.groups()["U"]
    with pytest.raises(HdpmError) as e:
        t.cut(3)                                       # before avg_tree
    assert "hdpm_trace_avg_tree" in str(e.value)
    with pytest.raises(HdpmError):
        t.cut_losses(1, 2)
    t.avg_tree()
    with pytest.raises(HdpmError):
        t.cut_losses(1, 256)                           # beyond the 255 clusters of the tables
    with pytest.raises(HdpmError):
        t.cut(U + 1)
    with pytest.raises(ValueError):
        P.minvi(t, method="avg")                       # the dense entry point is unchanged
    with pytest.raises(ValueError):
        P.minvi_avg(tr)
    t.close()
    # a new trace in the context discards the groups of the old one
    t2 = P.LabelTrace(tr[:3], engine=eng)
    with pytest.raises(HdpmError):
        t2.avg_tree()
    t2.close()


# ------------------------------------------------------------------ 6. headline size

def test_headline_size(hd):
    """N = 1,000,000, M = 16: a base partition with a few thousand moved labels"""
    from split_and_merge_gibbs_sampling_amd import posterior as P
    N, M, K = 1_000_000, 16, 10
    rng = np.random.default_rng(6)
    base = rng.integers(0, K, N)
    tr = np.tile(base, (M, 1)).astype(np.int32)
    moved = rng.choice(M * N, 4000, replace=False)
    tr.reshape(-1)[moved] = rng.integers(0, K, moved.size)
    assert all(np.unique(r).size == K for r in tr)
    # N^2 counts would be 4 TB, more than the device holds: completing at all shows that no
    # allocation scales with N^2
    t = P.LabelTrace(tr)
    cl, v = P.minvi_avg(t)
    print("U", t.U, "k", cl.max(), "VI.lb", v)
    assert 1000 < t.U <= 8192
    assert cl.min() == 1 and cl.shape == (N,)
    assert v == pytest.approx(float(t.vi_lb(cl)[0]), rel=1e-12)
    # the settled structure is found: the best cut is the base partition up to the moved points
    assert cl.max() == K
    assert np.mean(first_appearance(cl) == first_appearance(base)) > 0.99
    t.close()
