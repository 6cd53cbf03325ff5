"""MI355X: the single-point moves of a partition and the descent built on them
(csrc/trace_refine.hip and csrc/trace_refine.hpp through LabelTrace.move_gains, refine and
hdpm_trace_move_gains / hdpm_trace_refine) against the numpy reference of tests/refine_ref.py,
which tests/test_refine_ref_host.py checks against brute force on the CPU."""
import itertools
import math

import numpy as np
import pytest

import refine_ref as R

pytestmark = pytest.mark.gpu

LOSSES = ("VI", "Binder")
CODE = {"VI": 0, "Binder": 1}


@pytest.fixture(scope="module")
def hd():
    import split_and_merge_gibbs_sampling_amd as hd
    hd.build()
    return hd


def vi_atol(N):
    """tests/test_gpu_trace_uncertainty.py's atol of a VI value"""
    return 1e-12 * 3 * math.log2(max(N, 2))


def dense(rows):
    """each row relabelled 0..K-1 by value, as LabelTrace does"""
    return np.stack([np.unique(r, return_inverse=True)[1] for r in np.atleast_2d(rows)]).astype(np.int64)


def noisy_case(seed, N, M, Ka, Kz, used, wide_draw=False):
    """(c, trace): a truth of `used` classes, draws equal to it with a tenth of their labels
    (more where N is small) redrawn from Kz labels, and the partition c = the truth with a tenth of the points shifted
    to the next class and, where Ka > used, point 0 alone in class `used`; the classes above
    it are empty.  wide_draw: draw 0 has 255 clusters."""
    rng = np.random.default_rng(seed)
    truth = rng.integers(0, used, N)
    tr = np.tile(truth, (M, 1))
    for z in tr:
        idx = rng.choice(N, size=max(N // 10, min(N // 3, Kz), 1), replace=False)
        z[idx] = rng.integers(0, Kz, idx.size)
    if wide_draw:
        tr[0] = rng.permutation(np.arange(N) % 255)
    c = truth.copy()
    idx = rng.choice(N, size=N // 10, replace=False)
    c[idx] = (c[idx] + 1) % used
    if used < Ka:
        c[0] = used
    return c.astype(np.int64), dense(tr)


def device_gains(t, c, Ka, loss, want=(True, True, True)):
    """hdpm_trace_move_gains with labels as they stand; outputs start as sentinels so that
    one never written cannot pass"""
    from split_and_merge_gibbs_sampling_amd._lib import ptr
    N = t.N
    c32 = np.ascontiguousarray(c, dtype=np.int32)
    best = np.full(N, -7, np.int32) if want[0] else None
    gain = np.full(N, np.nan) if want[1] else None
    full = np.full((N, Ka + 1), np.nan) if want[2] else None
    t.eng._check(t.eng._L.hdpm_trace_move_gains(t.eng._h, ptr(c32), Ka, CODE[loss], ptr(best), ptr(gain), ptr(full)))
    return best, gain, full


# ------------------------------------------------------------------ 1. gains at awkward shapes

# N, M, Ka, Kz, occupied classes of the truth (one more holds point 0 alone, the rest of the Ka
# are empty), a draw of 255 clusters.  The truth's classes are few and large: among many tiny
# classes the smallest gain of a point is tied between classes that look alike, and the
# comparison of `best` would leave out more than 1 % of the points.
SHAPES = [
    (1, 1, 1, 1, 1, False),
    (15, 3, 2, 4, 1, False),           # Kz > Ka
    (17, 5, 20, 3, 3, False),          # M = the unroll + 1
    (63, 4, 63, 5, 4, False),          # Ka + 1 = one wave, Kz < Ka, M = the unroll
    (65, 37, 64, 12, 5, False),        # Ka + 1 = a wave and a lane
    (257, 37, 254, 40, 6, True),       # the new class still offered; a draw of 255 clusters: Kz > Ka
    (1000, 37, 255, 255, 40, True),    # the new class refused
    (1000, 5, 20, 12, 18, False),
]


@pytest.mark.parametrize("N,M,Ka,Kz,used,wide", SHAPES)
def test_gains_awkward_shapes(hd, N, M, Ka, Kz, used, wide):
    from split_and_merge_gibbs_sampling_amd._lib import ptr
    from split_and_merge_gibbs_sampling_amd.posterior import LabelTrace
    c, tr = noisy_case(1000 * N + M, N, M, Ka, Kz, used, wide)
    assert c.max() < Ka and (not wide or tr[0].max() == 254)
    t = LabelTrace(tr)
    me = np.arange(N)

    # Binder: exact, and the expression in affinity's output
    best, gain, full = device_gains(t, c, Ka, "Binder")
    want = R.gains_formula(c, tr, Ka, "Binder")
    wbest, wgain = R.best_of(want, c)
    assert np.array_equal(full, want.astype(np.float64))
    assert np.array_equal(best, wbest) and np.array_equal(gain, wgain.astype(np.float64))
    assert gain.tobytes() == full[me, best].tobytes()
    aff = np.zeros((N, Ka), np.uint64)
    t.eng._check(t.eng._L.hdpm_trace_affinity(t.eng._h, ptr(c.astype(np.int32)), Ka, ptr(aff), None))
    aff = np.concatenate([aff.astype(np.int64), np.zeros((N, 1), np.int64)], axis=1)
    na = np.bincount(c, minlength=Ka + 1).astype(np.int64)
    expr = (M * (na[None, :] - na[c][:, None] - 1) - 2 * (aff - aff[me, c][:, None])).astype(np.float64)
    expr[me, c] = 0.0
    if Ka == 255:
        expr[:, 255] = np.inf
    assert np.array_equal(full, expr)

    # VI: a gain is the difference of two VI values
    atol = vi_atol(N)
    best, gain, full = device_gains(t, c, Ka, "VI")
    want = R.gains_formula(c, tr, Ka, "VI")
    wbest, wgain = R.best_of(want, c)
    np.testing.assert_allclose(full, want, rtol=1e-12, atol=atol)
    np.testing.assert_allclose(gain, wgain, rtol=1e-12, atol=atol)
    assert np.all(full[me, c] == 0.0)
    assert gain.tobytes() == full[me, best].tobytes()
    # best is compared where the reference's smallest gain stands clear of the next by more
    # than atol, and where everything within atol of it is exactly 0: then the own class is
    # among them (a point alone in its class against the new and the empty classes), those
    # gains must be exactly 0 on the device too, and the tie rule says "stay"
    near = want <= want.min(axis=1)[:, None] + atol
    tied0 = (near.sum(axis=1) > 1) & np.all(~near | (want == 0.0), axis=1)
    assert np.all(full[tied0][near[tied0]] == 0.0) and np.array_equal(best[tied0], c[tied0])
    clear = (near.sum(axis=1) == 1) | tied0
    print(f"N={N} M={M} Ka={Ka}: best compared at {int(clear.sum())} of {N} points, {int(tied0.sum())} tied at 0")
    assert (~clear).sum() <= N // 100
    assert np.array_equal(best[clear], wbest[clear])
    if Ka == 255:
        assert np.all(np.isposinf(full[:, 255])) and np.all(best < 255)
    if N > 1:
        # point 0 is alone in its class: its new class is exactly 0 and loses to "stay"
        assert full[0, Ka] == 0.0 or Ka == 255
        assert best[0] != Ka
    t.close()


# ------------------------------------------------------------------ 2. ties

@pytest.mark.parametrize("loss", LOSSES)
def test_ties(hd, loss):
    from split_and_merge_gibbs_sampling_amd.posterior import LabelTrace
    # every draw one cluster, three classes of three: the other two classes tie, the lower wins
    t = LabelTrace(np.zeros((4, 9), np.int64))
    c = np.repeat(np.arange(3), 3)
    best, gain, full = t.move_gains(c, loss, full=True)
    assert best.tolist() == [1, 1, 1, 0, 0, 0, 0, 0, 0]
    assert np.all(gain < 0) and full[8, 0] == full[8, 1] and full[0, 1] == full[0, 2]
    t.close()
    # the draws equal the partition, which has a singleton: its new class ties with "stay" at 0
    c = np.array([0, 0, 0, 1, 1, 2, 1])
    t = LabelTrace(np.tile(c, (3, 1)))
    best, gain, full = t.move_gains(c, loss, full=True)
    assert full[5, 3] == 0.0 and best.tolist() == c.tolist() and np.all(gain == 0.0)
    assert np.all(full >= 0.0)
    t.close()


# ------------------------------------------------------------------ 3. blocks change nothing

def test_blocks_change_nothing(hd):
    from split_and_merge_gibbs_sampling_amd.posterior import LabelTrace, refine
    N, M, Ka = 1000, 7, 20
    c, tr = noisy_case(3, N, M, Ka, 12, 18)
    a, b = LabelTrace(tr), LabelTrace(tr, table_budget=4096)       # 16 points per block
    for loss in LOSSES:
        for x, y in zip(device_gains(a, c, Ka, loss), device_gains(b, c, Ka, loss)):
            assert x.tobytes() == y.tobytes()
        ra, rb = refine(a, c, loss), refine(b, c, loss)
        assert ra["rounds"] >= 1
        assert ra["cl"].tobytes() == rb["cl"].tobytes() and ra["history"].tobytes() == rb["history"].tobytes()
        assert (ra["rounds"], ra["trials"], ra["moved"]) == (rb["rounds"], rb["trials"], rb["moved"])
    a.close()
    b.close()


# ------------------------------------------------------------------ 4. null outputs, refusals

@pytest.mark.parametrize("loss", LOSSES)
def test_outputs_may_be_null(hd, loss):
    from split_and_merge_gibbs_sampling_amd.posterior import LabelTrace
    N, M, Ka = 257, 5, 7
    c, tr = noisy_case(5, N, M, Ka, 9, 5)
    t = LabelTrace(tr)
    ref = device_gains(t, c, Ka, loss)
    for want in itertools.product((False, True), repeat=3):
        got = device_gains(t, c, Ka, loss, want)
        for w, g, r in zip(want, got, ref):
            assert (g is None) if not w else g.tobytes() == r.tobytes()
    t.close()


def test_refusals(hd):
    from split_and_merge_gibbs_sampling_amd import Engine, HdpmError
    from split_and_merge_gibbs_sampling_amd._lib import RefineInfo, ptr
    from split_and_merge_gibbs_sampling_amd.posterior import LabelTrace, refine
    import ctypes as C
    N, M = 400, 11
    rng = np.random.default_rng(11)
    tr = rng.integers(0, 9, size=(M, N)).astype(np.int32)
    eng = Engine(0)
    L, h = eng._L, eng._h
    c = np.ascontiguousarray(rng.integers(0, 5, size=N), dtype=np.int32)
    c[:5] = np.arange(5)
    best, gain, out = np.zeros(N, np.int32), np.zeros(N), np.zeros(N, np.int32)
    info, hist = RefineInfo(), np.zeros(4)

    def refused(status):
        with pytest.raises(HdpmError) as e:
            eng._check(status())
        assert e.value.status == 5
        return str(e.value)

    def gains(cl, Ka, loss=0):
        return lambda: L.hdpm_trace_move_gains(h, ptr(cl), Ka, loss, ptr(best), ptr(gain), None)

    def run(cl, loss=0, rounds=3):
        return lambda: L.hdpm_trace_refine(h, ptr(cl), loss, rounds, ptr(out), C.byref(info), ptr(hist))

    assert "hdpm_trace_build" in refused(gains(c, 5))
    assert "hdpm_trace_build" in refused(run(c))
    t = LabelTrace(tr, engine=eng)
    for Ka in (0, 256):
        assert "Ka" in refused(gains(c, Ka))
    assert "Ka" in refused(gains(c, 4))                      # a label >= Ka
    for loss in (-1, 2):
        assert "loss" in refused(gains(c, 5, loss))
        assert "loss" in refused(run(c, loss))
    assert "max_rounds" in refused(run(c, 0, -1))
    bad = c.copy()
    bad[7] = 255
    refused(gains(bad, 255))
    refused(run(bad))
    bad[7] = -1
    refused(gains(bad, 5))
    refused(run(bad))
    refused(lambda: L.hdpm_trace_move_gains(h, None, 5, 0, ptr(best), ptr(gain), None))
    with pytest.raises(ValueError):
        t.move_gains(c, "VI.lb")
    with pytest.raises(ValueError):
        refine(t, c, "Binder", max_rounds=-1)
    with pytest.raises(ValueError):
        refine(t, c[:-1])
    # and the calls still work after the refusals
    b2, g2 = t.move_gains(c, "Binder")
    want = R.best_of(R.gains_formula(c.astype(np.int64), dense(tr), 5, "Binder"), c)
    assert np.array_equal(b2, want[0]) and np.array_equal(g2, want[1].astype(np.float64))
    t.close()


# ------------------------------------------------------------------ 5. the planted partition

@pytest.mark.parametrize("loss", LOSSES)
def test_planted_partition(hd, loss):
    from split_and_merge_gibbs_sampling_amd.posterior import LabelTrace, refine
    truth, tr, start = R.planted()
    want = R.refine_ref(start, tr, loss)
    assert want["converged"] and np.array_equal(want["cl"], R.relabel(truth))     # the reference alone ends there
    t = LabelTrace(tr)
    r = refine(t, start, loss)
    assert np.array_equal(r["cl"] - 1, R.relabel(truth))
    assert r["converged"] is True and r["moved"] == want["moved"]
    assert (r["rounds"], r["trials"]) == (want["rounds"], want["trials"])
    hist = r["history"]
    assert hist.shape == (r["rounds"] + 1,) and np.all(np.diff(hist) < 0)
    assert hist[0] == r["start"] and hist[-1] == r["value"]
    if loss == "VI":
        np.testing.assert_allclose(hist, want["history"], rtol=1e-12, atol=vi_atol(truth.size))
        assert r["value"] == t.vi(truth)[0] and r["start"] == t.vi(R.relabel(start))[0]
    else:
        assert [int(round(x * t.M)) for x in hist] == want["history"]
        assert r["value"] == t.binder(truth)[0] and r["start"] == t.binder(start)[0]
    t.close()


# ------------------------------------------------------------------ 6. the halving

@pytest.mark.parametrize("loss", LOSSES)
def test_halving(hd, loss):
    from split_and_merge_gibbs_sampling_amd.posterior import LabelTrace, refine
    tr, start = R.halving()
    t = LabelTrace(tr)
    best, gain = t.move_gains(start, loss)
    assert best[:2].tolist() == [1, 0] and gain[0] == gain[1] < 0
    if loss == "Binder":
        assert gain[0] == -5.0
    r = refine(t, start, loss)
    assert (r["trials"], r["rounds"], r["moved"], r["converged"]) == (2, 1, 1, True)
    assert r["cl"].tolist() == [1, 1] + [2] * 10
    assert r["value"] == 0.0 if loss == "Binder" else abs(r["value"]) <= vi_atol(12)
    t.close()


# ------------------------------------------------------------------ 7. nothing to do

@pytest.mark.parametrize("loss", LOSSES)
def test_minimum_and_no_rounds(hd, loss):
    from split_and_merge_gibbs_sampling_amd.posterior import LabelTrace, refine
    truth, tr, start = R.planted()
    t = LabelTrace(tr)
    r = refine(t, truth + 3, loss)
    assert (r["rounds"], r["trials"], r["moved"], r["converged"]) == (0, 0, 0, True)
    assert np.array_equal(r["cl"] - 1, R.relabel(truth)) and r["start"] == r["value"]
    assert r["history"].tolist() == [r["value"]]
    r = refine(t, start[::-1], loss, max_rounds=0)
    assert (r["rounds"], r["trials"], r["moved"], r["converged"]) == (0, 0, 0, False)
    assert np.array_equal(r["cl"] - 1, R.relabel(start[::-1])) and r["history"].tolist() == [r["start"]]
    r = refine(t, truth, loss, max_rounds=0)                      # no candidate: converged without a round
    assert r["converged"] is True and r["rounds"] == 0
    t.close()


# ------------------------------------------------------------------ 8. one larger shape

@pytest.mark.parametrize("loss", LOSSES)
def test_larger_shape(hd, loss):
    from split_and_merge_gibbs_sampling_amd.posterior import LabelTrace, refine
    N, M, K = 100_000, 16, 12
    rng = np.random.default_rng(100_000)
    truth = rng.integers(0, K, N)
    tr = np.tile(truth, (M, 1))
    for z in tr:
        idx = rng.choice(N, size=N // 10, replace=False)
        z[idx] = rng.integers(0, K, idx.size)
    t = LabelTrace(tr)
    r = refine(t, tr[0], loss)
    print(f"{loss}: rounds {r['rounds']} trials {r['trials']} moved {r['moved']} {r['start']} -> {r['value']}")
    assert r["converged"] and r["rounds"] >= 1 and r["value"] < r["start"]
    best, gain = t.move_gains(r["cl"], loss)
    assert np.all(gain >= 0.0) and np.array_equal(best, r["cl"] - 1)
    assert r["value"] == (t.vi(r["cl"]) if loss == "VI" else t.binder(r["cl"]))[0]
    t.close()
