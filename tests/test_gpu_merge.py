"""MI355X: the merge gains of all pairs of classes, the greedy merge path and the descent that
alternates single moves with merges (csrc/trace_merge.hip and csrc/trace_merge.hpp through
LabelTrace.merge_gains, LabelTrace.merge_path, coarsen, refine(..., merges=) and
hdpm_trace_merge_gains / hdpm_trace_merge_path / hdpm_trace_refine_merge) against the numpy
reference of tests/merge_ref.py, which tests/test_merge_ref_host.py checks against brute force
on the CPU, together with the gap condition that lets every comparison of a best pair here be
exact."""
import ctypes as C
import itertools

import numpy as np
import pytest

import merge_ref as MR
import refine_ref as R

pytestmark = pytest.mark.gpu

LOSSES = ("VI", "Binder")
CODE = {"VI": 0, "Binder": 1}


@pytest.fixture(scope="module")
def hd():
    import split_and_merge_gibbs_sampling_amd as hd
    hd.build()
    return hd


def device_gains(t, c, Ka, loss, want=(True, True, True)):
    """hdpm_trace_merge_gains with labels as they stand; outputs start as sentinels so that
    one never written cannot pass"""
    from split_and_merge_gibbs_sampling_amd._lib import ptr
    c32 = np.ascontiguousarray(c, dtype=np.int32)
    gain = np.full((Ka, Ka), np.nan) if want[0] else None
    best = np.full(2, -7, np.int32) if want[1] else None
    bg = np.full(1, np.nan) if want[2] else None
    t.eng._check(t.eng._L.hdpm_trace_merge_gains(t.eng._h, ptr(c32), Ka, CODE[loss], ptr(gain), ptr(best), ptr(bg)))
    return gain, best, bg


def device_path(t, c, Ka, loss, k_min):
    from split_and_merge_gibbs_sampling_amd._lib import ptr
    c32 = np.ascontiguousarray(c, dtype=np.int32)
    merge, sg, val = np.full((Ka, 2), -7, np.int32), np.full(Ka, np.nan), np.full(Ka + 1, np.nan)
    steps = C.c_int32(-7)
    t.eng._check(t.eng._L.hdpm_trace_merge_path(t.eng._h, ptr(c32), Ka, CODE[loss], k_min, ptr(merge), ptr(sg),
                                                ptr(val), C.byref(steps)))
    s = steps.value
    # nothing is written past the steps
    assert np.all(merge[s:] == -7) and np.all(np.isnan(sg[s:])) and np.all(np.isnan(val[s + 1:]))
    return merge[:s], sg[:s], val[:s + 1]


# ------------------------------------------------------------------ 1. gains at awkward shapes

@pytest.mark.parametrize("shape", MR.SHAPES)
def test_gains_awkward_shapes(hd, shape):
    from split_and_merge_gibbs_sampling_amd.posterior import LabelTrace
    N, M, Ka, Kz, used, wide, hole, _ = shape
    c, tr = MR.gains_case(*shape)
    assert c.max() < Ka and tr.max() + 1 == Kz and (not wide or tr[0].max() == 254)
    n = np.bincount(c, minlength=Ka)
    if hole:
        assert n[2] == 0 and n[used + 1] > 0 and n[Ka - 1] == 0
    t = LabelTrace(tr)
    zero = np.zeros(Ka).tobytes()
    for loss in LOSSES:
        gain, best, bg = device_gains(t, c, Ka, loss)
        want = MR.merge_gains_formula(c, tr, Ka, loss)
        wbest, wbg = MR.best_pair(want, n)
        if loss == "Binder":
            assert np.array_equal(gain, want.astype(np.float64))
            assert bg[0] == float(wbg)
        else:
            err = np.abs(gain - want).max()
            print(f"N={N} M={M} Ka={Ka} Kz={Kz}: VI max |gain - ref| = {err:.3e}, atol {MR.vi_atol(N):.3e}, "
                  f"gap {MR.gap(want, n):.3e}")
            assert err <= MR.vi_atol(N)
            assert abs(bg[0] - wbg) <= MR.vi_atol(N)
        assert tuple(best) == wbest
        if wbest[0] >= 0:
            assert bg.tobytes() == gain[wbest].tobytes()
        else:
            assert bg[0] == 0.0
        # symmetric with a zero diagonal, bitwise; empty classes exactly 0.0
        assert gain.tobytes() == np.ascontiguousarray(gain.T).tobytes()
        assert np.ascontiguousarray(gain.diagonal()).tobytes() == zero
        for a in np.flatnonzero(n == 0):
            assert gain[a].tobytes() == zero and np.ascontiguousarray(gain[:, a]).tobytes() == zero
    t.close()


@pytest.mark.parametrize("loss", LOSSES)
def test_outputs_may_be_null(hd, loss):
    from split_and_merge_gibbs_sampling_amd.posterior import LabelTrace
    shape = MR.SHAPES[3]
    c, tr = MR.gains_case(*shape)
    t = LabelTrace(tr)
    ref = device_gains(t, c, shape[2], loss)
    for want in itertools.product((False, True), repeat=3):
        got = device_gains(t, c, shape[2], loss, want)
        for w, g, r in zip(want, got, ref):
            assert (g is None) if not w else g.tobytes() == r.tobytes()
    # the Python method: labels relabelled as the candidates are
    gain, best, bg = t.merge_gains(c + 5, loss)
    assert gain.tobytes() == ref[0].tobytes() and best == tuple(ref[1]) and bg == ref[2][0]
    t.close()


# ------------------------------------------------------------------ 2. the budget changes nothing

def test_bytes_do_not_depend_on_the_budget(hd):
    from split_and_merge_gibbs_sampling_amd.posterior import LabelTrace
    shape = MR.SHAPES[5]
    c, tr = MR.gains_case(*shape)
    a, b = LabelTrace(tr), LabelTrace(tr, table_budget=4096)
    for loss in LOSSES:
        for x, y in zip(device_gains(a, c, shape[2], loss), device_gains(b, c, shape[2], loss)):
            assert x.tobytes() == y.tobytes()
        for x, y in zip(device_path(a, c, shape[2], loss, 40), device_path(b, c, shape[2], loss, 40)):
            assert x.tobytes() == y.tobytes()
    a.close()
    b.close()


# ------------------------------------------------------------------ 3. the stall case

@pytest.mark.parametrize("loss", LOSSES)
def test_stall_case(hd, loss):
    from split_and_merge_gibbs_sampling_amd._lib import RefineInfo, ptr
    from split_and_merge_gibbs_sampling_amd.posterior import LabelTrace, refine
    c, tr, merged = MR.stall_case()
    t = LabelTrace(tr)
    best, gain = t.move_gains(c, loss)
    assert not np.any(gain < 0.0) and np.array_equal(best, c)
    r = refine(t, c, loss)
    assert r["rounds"] == 0 and r["converged"] is True and r["cl"].max() == 3 and "merges" not in r
    g, pair, bg = t.merge_gains(c, loss)
    assert pair == (0, 1) and bg < 0
    r = refine(t, c, loss, merges=5)
    assert r["merges"] == 1 and r["rounds"] == 0 and r["trials"] == 1 and r["converged"] is True
    assert np.array_equal(r["cl"] - 1, merged) and r["history"].shape == (2,)
    # the C call: Binder's value is the integer M A + P - 2 Q
    out, info, nm, hist = np.full(20, -7, np.int32), RefineInfo(), C.c_int32(-7), np.full(106, np.nan)
    t.eng._check(t.eng._L.hdpm_trace_refine_merge(t.eng._h, ptr(c.astype(np.int32)), CODE[loss], 100, 5, ptr(out),
                                                  C.byref(info), C.byref(nm), ptr(hist)))
    assert nm.value == 1 and info.K == 2 and info.converged == 1 and np.array_equal(out, merged)
    assert np.all(np.isnan(hist[2:]))
    if loss == "Binder":
        assert info.start == 216.0 and info.value == 144.0 and hist[:2].tolist() == [216.0, 144.0]
        assert g[0, 1] == -72.0 and g[0, 2] == 480.0 and g[1, 2] == 480.0
        # refine's dict keeps LabelTrace.binder's scale: the integer over M
        assert r["value"] == t.binder(merged)[0] and r["start"] == t.binder(c)[0]
        assert abs(r["value"] - 14.4) < 1e-12 and abs(r["start"] - 21.6) < 1e-12
    else:
        atol = MR.vi_atol(20)
        assert abs(info.value - 0.24) <= atol and abs(info.start - 0.36) <= atol
        assert abs(r["value"] - 0.24) <= atol and r["value"] == t.vi(merged)[0] == info.value
        assert abs(g[0, 1] + 0.12) <= atol and abs(g[0, 2] - 0.6897) <= 5e-5
    # no merge allowed: the negative pair is left and reported
    t.eng._check(t.eng._L.hdpm_trace_refine_merge(t.eng._h, ptr(c.astype(np.int32)), CODE[loss], 100, 0, ptr(out),
                                                  C.byref(info), C.byref(nm), ptr(hist)))
    assert nm.value == 0 and info.K == 3 and info.converged == 0 and np.array_equal(out, c)
    t.close()


# ------------------------------------------------------------------ 4. a path

@pytest.fixture(scope="module")
def path_refs():
    truth, tr, start = MR.path_case()
    return truth, tr, start, {loss: MR.merge_path_ref(start, tr, 12, loss) for loss in LOSSES}


@pytest.mark.parametrize("loss", LOSSES)
def test_path(hd, path_refs, loss):
    from split_and_merge_gibbs_sampling_amd.posterior import LabelTrace, coarsen
    truth, tr, start, refs = path_refs
    want = refs[loss]
    N = truth.size
    t = LabelTrace(tr)
    p = t.merge_path(start, loss)
    assert p["merge"].shape == (11, 2) and p["step_gain"].shape == (11,) and p["value"].shape == (12,)
    assert [tuple(x) for x in p["merge"].tolist()] == want["merge"]
    levels = [coarsen(start, p["merge"], k) for k in range(12, 0, -1)]
    for s, lv in enumerate(levels):
        assert np.array_equal(lv, MR.coarsen_ref(start, want["merge"], s)) and lv.max() == 11 - s
    if loss == "Binder":
        A, P, Q = t.binder_terms(np.stack(levels))
        assert p["value"].tolist() == [float(t.M * a + P - 2 * q) for a, q in zip(A, Q)]
        assert p["value"].tolist() == [float(v) for v in want["value"]]
        assert p["step_gain"].tolist() == [float(g) for g in want["step_gain"]]
        assert np.array_equal(np.diff(p["value"]), p["step_gain"])
    else:
        atol = MR.vi_atol(N)
        vi = t.vi(np.stack(levels))
        print("VI path: max |value - vi| =", np.abs(p["value"] - vi).max(), "atol", atol)
        assert np.abs(p["value"] - vi).max() <= atol
        assert np.abs(p["value"] - np.array(want["value"])).max() <= atol
        assert np.abs(p["step_gain"] - np.array(want["step_gain"])).max() <= atol
        assert p["value"][0] == t.vi(start)[0]        # the start: the same tables, the same sums
    assert int(np.argmin(p["value"])) == 9 and np.array_equal(coarsen(start, p["merge"], 3), R.relabel(truth))
    # a shorter path is a prefix; at or above the classes there is nothing to do
    q = t.merge_path(start, loss, k_min=3)
    assert q["merge"].tobytes() == p["merge"][:9].tobytes() and q["value"].tobytes() == p["value"][:10].tobytes()
    assert q["step_gain"].tobytes() == p["step_gain"][:9].tobytes()
    for k_min in (12, 13, 500):
        q = t.merge_path(start, loss, k_min=k_min)
        assert q["merge"].shape == (0, 2) and q["value"].tolist() == [p["value"][0]]
    # labels as they stand, with empty classes between them: the caller's labels are named
    m2, _, v2 = device_path(t, start * 3 + 1, 36, loss, 1)
    assert np.array_equal(m2, p["merge"] * 3 + 1)
    if loss == "Binder":
        assert v2.tobytes() == p["value"].tobytes()
    else:
        assert np.abs(v2 - p["value"]).max() <= MR.vi_atol(N)
    t.close()


@pytest.mark.parametrize("loss", LOSSES)
def test_refine_alternates_moves_and_merges(hd, loss):
    """single moves put the misplaced points back, merges join the halves: the truth's three"""
    from split_and_merge_gibbs_sampling_amd.posterior import LabelTrace, refine
    truth, tr, start = MR.alternation_case()
    t = LabelTrace(tr)
    plain = refine(t, start, loss)
    assert plain["converged"] is True and plain["cl"].max() == 5       # single moves alone keep the halves
    r = refine(t, start, loss, merges=20)
    K = int(r["cl"].max())
    print(f"{loss}: rounds {r['rounds']} merges {r['merges']} trials {r['trials']} K {K} {r['start']} -> {r['value']}")
    assert r["converged"] is True and r["history"].shape == (r["rounds"] + r["merges"] + 1,)
    assert np.all(np.diff(r["history"]) < 0) and r["history"][0] == r["start"] and r["history"][-1] == r["value"]
    assert r["value"] == (t.vi(r["cl"]) if loss == "VI" else t.binder(r["cl"]))[0]
    best, gain = t.move_gains(r["cl"], loss)
    assert np.all(gain >= 0.0)
    g, pair, bg = t.merge_gains(r["cl"], loss)
    assert not bg < 0
    # the run is the reference's, step for step (its decisions stand clear of VI's rounding)
    want = MR.refine_merge_ref(start, tr, loss, 100, 20)
    assert (want["rounds"], want["merges"]) == (1, 2)
    assert (r["rounds"], r["merges"], r["trials"], r["moved"]) == (want["rounds"], want["merges"], want["trials"],
                                                                   want["moved"])
    assert np.array_equal(r["cl"] - 1, want["cl"])
    if loss == "Binder":
        assert [int(round(x * t.M)) for x in r["history"]] == want["history"]
    else:
        assert np.abs(r["history"] - np.array(want["history"])).max() <= MR.vi_atol(truth.size)
    assert np.array_equal(r["cl"] - 1, R.relabel(truth))
    # bounded merges: one merge, and one still to be had
    r1 = refine(t, start, loss, merges=1)
    assert r1["merges"] == 1 and r1["converged"] is False
    t.close()


# ------------------------------------------------------------------ 5. refusals

def test_refusals(hd):
    from split_and_merge_gibbs_sampling_amd import Engine, HdpmError
    from split_and_merge_gibbs_sampling_amd._lib import RefineInfo, ptr
    from split_and_merge_gibbs_sampling_amd.posterior import LabelTrace, coarsen, refine
    N, M = 400, 11
    rng = np.random.default_rng(11)
    tr = rng.integers(0, 9, size=(M, N)).astype(np.int32)
    eng = Engine(0)
    L, h = eng._L, eng._h
    c = np.ascontiguousarray(rng.integers(0, 5, size=N), dtype=np.int32)
    c[:5] = np.arange(5)
    gain, best, bg = np.zeros((5, 5)), np.zeros(2, np.int32), np.zeros(1)
    merge, sg, val, steps = np.zeros((5, 2), np.int32), np.zeros(5), np.zeros(6), C.c_int32(0)
    out, info, nm, hist = np.zeros(N, np.int32), RefineInfo(), C.c_int32(0), np.zeros(8)

    def refused(status):
        with pytest.raises(HdpmError) as e:
            eng._check(status())
        assert e.value.status == 5 and str(e.value)
        return str(e.value)

    def gains(cl, Ka, loss=0):
        return lambda: L.hdpm_trace_merge_gains(h, ptr(cl), Ka, loss, ptr(gain), ptr(best), ptr(bg))

    def path(cl, Ka, loss=0, k_min=1):
        return lambda: L.hdpm_trace_merge_path(h, ptr(cl), Ka, loss, k_min, ptr(merge), ptr(sg), ptr(val),
                                               C.byref(steps))

    def run(cl, loss=0, rounds=3, merges=3):
        return lambda: L.hdpm_trace_refine_merge(h, ptr(cl), loss, rounds, merges, ptr(out), C.byref(info),
                                                 C.byref(nm), ptr(hist))

    for call in (gains(c, 5), path(c, 5), run(c)):
        assert "hdpm_trace_build" in refused(call)
    t = LabelTrace(tr, engine=eng)
    for Ka in (0, 256):
        assert "Ka" in refused(gains(c, Ka))
        assert "Ka" in refused(path(c, Ka))
    assert "Ka" in refused(gains(c, 4))                      # a label >= Ka
    assert "Ka" in refused(path(c, 4))
    for loss in (-1, 2):
        assert "loss" in refused(gains(c, 5, loss))
        assert "loss" in refused(path(c, 5, loss))
        assert "loss" in refused(run(c, loss))
    for k_min in (0, -3):
        assert "k_min" in refused(path(c, 5, 0, k_min))
    assert "max_rounds" in refused(run(c, 0, -1, 3))
    assert "max_merges" in refused(run(c, 0, 3, -1))
    bad = c.copy()
    bad[7] = 255
    for call in (gains(bad, 255), path(bad, 255), run(bad)):
        refused(call)
    bad[7] = -1
    for call in (gains(bad, 5), path(bad, 5), run(bad)):
        refused(call)
    refused(lambda: L.hdpm_trace_merge_gains(h, None, 5, 0, ptr(gain), ptr(best), ptr(bg)))
    with pytest.raises(ValueError):
        t.merge_gains(c, "VI.lb")
    with pytest.raises(ValueError):
        t.merge_path(c[:-1])
    with pytest.raises(ValueError):
        refine(t, c, "Binder", merges=-1)
    with pytest.raises(ValueError):
        coarsen(c, np.zeros((2, 2), np.int32), 1)            # 5 classes and two merges: k >= 3
    # and the calls still work after the refusals
    g2, b2, bg2 = t.merge_gains(c, "Binder")
    want = MR.merge_gains_formula(c.astype(np.int64), MR.dense(tr), 5, "Binder")
    assert np.array_equal(g2, want.astype(np.float64))
    assert (b2, bg2) == MR.best_pair(want, np.bincount(c))
    t.close()


# ------------------------------------------------------------------ 6. merges = 0 is today's call

@pytest.mark.parametrize("loss", LOSSES)
def test_merges_zero_is_refine(hd, loss):
    from split_and_merge_gibbs_sampling_amd.posterior import LabelTrace, refine
    truth, tr, start = R.planted()
    t = LabelTrace(tr)
    a, b = refine(t, start, loss), refine(t, start, loss, merges=0)
    assert a.keys() == b.keys() and "merges" not in a
    for k in a:
        if isinstance(a[k], np.ndarray):
            assert a[k].dtype == b[k].dtype and a[k].tobytes() == b[k].tobytes()
        else:
            assert type(a[k]) is type(b[k]) and a[k] == b[k]
    # with merges allowed but none to be had, the end state is the same
    m = refine(t, start, loss, merges=3)
    assert m["merges"] == 0 and np.array_equal(m["cl"], a["cl"]) and m["value"] == a["value"]
    assert (m["rounds"], m["trials"], m["moved"], m["converged"]) == (a["rounds"], a["trials"], a["moved"], True)
    assert m["history"].tobytes() == a["history"].tobytes()
    t.close()
