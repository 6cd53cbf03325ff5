"""MI355X: the profiles of an estimate's classes (csrc/profile.hip through Predictive.profile /
hdpm_predict_profile) against the plain restatement of tests/profile_ref.py.

center_cnt is compared as integers; sigma_trace, sigma_mean and sigma_var by bytes (every sum
has one order, k within s, and the build does not fuse multiply and add); code_pmf within 1e-10
absolute, the project's tolerance downstream of an exp (the device adds the same M K_s positive
terms regrouped as base + sum (em - ei): at most 37 x 255 terms of at most 1, about 1e-12).

The shapes: d in {1, 63, 64, 65, 130}, the edges of a wave's 64 attribute lanes, each with the
three (M, Ka) shapes of test_gpu_predict.py's case_values (M = 1 with Ka = 1; M = 2 with Ka = 3,
class 1 empty; M = 37 with Ka = 255), and K_s in {1, 2, 20, 255} spread over them so that every
(M, Ka) shape meets every K_s: the 37 draws cycle through all four, the one- and two-draw chains
take them in turn over the five d.  N <= 300; attrisize is predict_ref.problem's mix of 2..255,
so ld = 255 (2 at d = 1).  A restatement is computed once per case and shared."""
import functools

import numpy as np
import pytest

import profile_ref as pref

pytestmark = pytest.mark.gpu

GAMMA = 0.68
DS = (1, 63, 64, 65, 130)
KS = (1, 2, 20, 255)
ONE = {1: [1], 63: [2], 64: [20], 65: [255], 130: [20]}
TWO = {1: [1, 255], 63: [2, 20], 64: [255, 1], 65: [20, 2], 130: [255, 20]}


@pytest.fixture(scope="module")
def hd():
    import split_and_merge_gibbs_sampling_amd as hd
    hd.build()
    return hd


def fitted(hd, p, budget=None):
    tr = hd.LabelTrace(p["c_trace"], table_budget=budget)
    return tr, hd.Predictive(tr, p["centers"], p["sigmas"], p["att"], GAMMA)


@functools.lru_cache(maxsize=None)
def case(name, d):
    """(problem, cl, Ka, ld, restatement)"""
    i = DS.index(d)
    if name == "M1_Ka1":
        Ks = ONE[d]
        N = 300 if max(Ks) > 50 else 50
        cl, Ka = np.zeros(N, np.int32), 1
    elif name == "M2_Ka3_empty":
        Ks = TWO[d]
        N = 300
        cl, Ka = np.where(np.arange(N) % 3 == 0, 0, 2).astype(np.int32), 3          # class 1 is empty
    else:
        Ks = [KS[(s + i) % 4] for s in range(37)]
        N = 300
        cl, Ka = (np.arange(N) * 7 % 255).astype(np.int32), 255
    p = pref.problem(seed=900 + 10 * i + len(Ks), N=N, d=d, Ks=Ks)
    ld = int(p["att"].max())
    assert p["att"].min() == 2 and (d == 1 or ld == 255)
    want = pref.profile(p["c_trace"], p["centers"], p["sigmas"], p["att"], cl, Ka, ld)
    return p, cl, Ka, ld, want


def same_bytes(got, want, what):
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want, dtype=got.dtype)
    assert got.shape == want.shape, what
    if got.tobytes() != want.tobytes():
        bad = np.flatnonzero(got.ravel() != want.ravel())
        raise AssertionError((what, bad.size, got.ravel()[bad[:3]], want.ravel()[bad[:3]]))


def check_against(out, want, M):
    assert out["center_cnt"].dtype == np.uint64
    assert np.array_equal(out["center_cnt"], want["center_cnt"])
    same_bytes(out["sigma_trace"], want["sigma_trace"], "sigma_trace")
    same_bytes(out["sigma_mean"], want["sigma_mean"], "sigma_mean")
    same_bytes(out["sigma_sd"], np.sqrt(want["sigma_var"]), "sigma_sd")
    err = np.abs(out["code_pmf"] - want["code_pmf"])
    print("code_pmf max abs err", float(err.max()))
    assert np.all(np.isfinite(out["code_pmf"])) and np.all(err <= 1e-10), float(err.max())
    assert np.array_equal(out["sizes"], want["sizes"])


def invariants(out, att, M, cl, Ka):
    n = np.bincount(cl, minlength=Ka)
    cnt = out["center_cnt"]
    assert np.array_equal(out["sizes"], n)
    assert np.array_equal(cnt.sum(axis=2), np.broadcast_to((M * n)[:, None], cnt.shape[:2]).astype(np.uint64))
    for j, m in enumerate(att):
        assert np.all(cnt[:, j, m:] == 0) and np.all(out["code_pmf"][:, j, m:] == 0.0)
    tot = out["code_pmf"].sum(axis=2)
    assert np.all(np.abs(tot[n > 0] - 1.0) <= 1e-10)
    empty = n == 0
    for key in ("center_cnt", "center_pmf", "code_pmf", "sigma_mean", "sigma_sd", "mode", "mode_prob"):
        assert np.all(out[key][empty] == 0), key
    if "sigma_trace" in out:
        assert np.all(out["sigma_trace"][:, empty] == 0.0)
    assert np.array_equal(out["mode"], pref.mode_of(cnt, n))
    live = ~empty
    assert np.array_equal(out["mode_prob"][live], np.take_along_axis(out["center_pmf"], out["mode"][:, :, None].clip(1) - 1,
                                                                    axis=2)[:, :, 0][live])
    den = (M * n).astype(np.float64)[:, None, None]
    assert np.array_equal(out["center_pmf"][live], (cnt / np.where(den > 0, den, 1.0))[live])
    assert np.all(out["sigma_mean"][live] > 0) and np.all(out["sigma_sd"] >= 0)


# ------------------------------------------------------------------ 1. against the restatement

@pytest.mark.parametrize("d", DS)
@pytest.mark.parametrize("name", ["M1_Ka1", "M2_Ka3_empty", "M37_Ka255"])
def test_against_the_restatement(hd, name, d):
    p, cl, Ka, ld, want = case(name, d)
    M = p["c_trace"].shape[0]
    tr, pr = fitted(hd, p)
    try:
        out = pr.profile(cl, Ka, trace=True)
    finally:
        tr.close()
    assert out["center_cnt"].shape == (Ka, d, ld) and out["sigma_trace"].shape == (M, Ka, d)
    check_against(out, want, M)
    invariants(out, p["att"], M, cl, Ka)
    if name == "M2_Ka3_empty":
        assert out["sizes"][1] == 0
    if M == 1:
        assert np.all(out["sigma_sd"] == 0.0)


# The level rows of a wave's lanes live in 64 KB of LDS: with both level outputs all 64 lanes work up
# to ld = 64 and 63 at ld = 65 (16 at ld = 255, the shapes above), so the lanes' edge moves with ld.
@pytest.mark.parametrize("d,top", [(63, 6), (64, 6), (65, 6), (130, 6), (130, 64), (130, 65)])
def test_few_levels(hd, d, top):
    rng = np.random.default_rng(d + top)
    att = rng.choice([2, 3, 4, 6], size=d)
    att[d // 2] = top
    Ks = [3, 20, 1, 7, 2]
    p = pref.problem(seed=300 + d + top, N=60, d=d, Ks=Ks, att=att)
    cl, Ka = np.where(np.arange(60) % 4 == 2, 3, np.arange(60) % 4).astype(np.int32), 4       # class 2 is empty
    want = pref.profile(p["c_trace"], p["centers"], p["sigmas"], p["att"], cl, Ka, top)
    tr, pr = fitted(hd, p)
    try:
        out = pr.profile(cl, Ka, trace=True)
    finally:
        tr.close()
    assert out["center_cnt"].shape == (Ka, d, top)
    check_against(out, want, len(Ks))
    invariants(out, p["att"], len(Ks), cl, Ka)


# ------------------------------------------------------------------ 2. no result depends on the budget

def test_budget_independence(hd):
    p, cl, Ka, ld, want = case("M37_Ka255", 130)
    assert ld == 255
    # 1 byte: one attribute per block of level rows, one draw per chunk; 5 draws of u_s (255 x 130 x 8
    # bytes each) hold one attribute's level rows (255 x 255 x 16 bytes) and not two: chunks of 5 draws
    got = []
    for budget in (1, 5 * 255 * 130 * 8, None):
        tr, pr = fitted(hd, p, budget=budget)
        try:
            got.append(pr.profile(cl, Ka, trace=True))
        finally:
            tr.close()
    for other in got[:2]:
        for key, a in got[2].items():
            same_bytes(other[key], a, key)
    check_against(got[0], want, 37)


# ------------------------------------------------------------------ 3. label switching

def test_label_switching(hd):
    p, cl, Ka, ld, _ = case("M37_Ka255", 65)
    rng = np.random.default_rng(8)
    tr2, cens, sigs = [], [], []
    for s, z in enumerate(p["c_trace"]):
        K = p["centers"][s].shape[0]
        perm = rng.permutation(K)                     # old label k becomes perm[k]
        inv = np.argsort(perm)
        tr2.append(perm[z])
        cens.append(p["centers"][s][inv])
        sigs.append(p["sigmas"][s][inv])
    q = {**p, "c_trace": np.stack(tr2).astype(np.int32), "centers": cens, "sigmas": sigs}
    assert not np.array_equal(q["c_trace"], p["c_trace"])
    outs = []
    for prob in (p, q):
        tr, pr = fitted(hd, prob)
        try:
            outs.append(pr.profile(cl, Ka, trace=True))
        finally:
            tr.close()
    a, b = outs
    assert np.array_equal(a["center_cnt"], b["center_cnt"])
    # at most 255 positive terms in another order: 255 eps is about 6e-14
    assert np.all(np.abs(b["sigma_trace"] - a["sigma_trace"]) <= 1e-12 * np.abs(a["sigma_trace"]))
    assert np.all(np.abs(b["sigma_mean"] - a["sigma_mean"]) <= 1e-12 * np.abs(a["sigma_mean"]))
    va, vb = a["sigma_sd"] ** 2, b["sigma_sd"] ** 2
    assert np.all(np.abs(vb - va) <= 1e-10 * (1 + va))
    assert np.all(np.abs(b["code_pmf"] - a["code_pmf"]) <= 1e-10)


# ------------------------------------------------------------------ 4. one draw, its own labels

@pytest.mark.parametrize("d,K", [(65, 20), (130, 255)])
def test_identity(hd, d, K):
    p = pref.problem(seed=400 + d, N=300, d=d, Ks=[K])
    z, cen, sig, att = p["c_trace"][0], p["centers"][0], p["sigmas"][0], p["att"]
    tr, pr = fitted(hd, p)
    try:
        out = pr.profile(z, K, trace=True)
    finally:
        tr.close()
    n = np.bincount(z, minlength=K)
    assert n.min() >= 1
    want = np.zeros(out["center_cnt"].shape, np.uint64)
    a, j = np.meshgrid(np.arange(K), np.arange(d), indexing="ij")
    want[a, j, cen.astype(np.int64) - 1] = n[:, None]
    assert np.array_equal(out["center_cnt"], want)
    assert np.array_equal(out["mode"], cen.astype(np.int64)) and np.all(out["mode_prob"] == 1.0)
    # (n x) / n takes two roundings
    assert np.all(np.abs(out["sigma_trace"][0] - sig) <= 2 * np.spacing(sig))
    assert np.all(np.abs(out["sigma_mean"] - sig) <= 2 * np.spacing(sig))
    assert np.all(out["sigma_sd"] == 0.0)
    lev = np.arange(1, out["code_pmf"].shape[2] + 1)
    for k in range(K):
        em, ei = pref.exp_pairs(sig[k:k + 1], att)
        row = np.where(lev[None, :] == cen[k].astype(np.int64)[:, None], em[0][:, None], ei[0][:, None])
        row[lev[None, :] > att[:, None]] = 0.0
        assert np.all(np.abs(out["code_pmf"][k] - row) <= 1e-10)


# ------------------------------------------------------------------ 5. outputs on request, refusals

def test_outputs_on_request_and_refusals(hd):
    from split_and_merge_gibbs_sampling_amd._lib import ptr
    p, cl, Ka, ld, want = case("M2_Ka3_empty", 63)
    d, M = 63, 2
    eng = hd.Engine(0)
    L, h = eng._L, eng._h

    def refused(status, *parts):
        assert status == 5
        msg = L.hdpm_last_error(h).decode()
        for part in parts:
            assert part in msg, msg

    mean = np.full(Ka * d + 8, -7.0)              # 8 doubles of guard behind the Ka x d results

    def only_mean(ld_=ld, Ka_=Ka, cl_=cl):
        return L.hdpm_predict_profile(h, ptr(np.ascontiguousarray(cl_, np.int32)), Ka_, ld_, None, None, ptr(mean),
                                      None, None)

    try:
        refused(only_mean(), "hdpm_trace_build has not been called")
        trace = hd.LabelTrace(p["c_trace"], engine=eng)
        refused(only_mean(), "hdpm_predict_build has not been called")
        pr = hd.Predictive(trace, p["centers"], p["sigmas"], p["att"], GAMMA)
        # only sigma_mean asked for: its bytes, nothing behind them written
        assert only_mean() == 0
        same_bytes(mean[:Ka * d].reshape(Ka, d), want["sigma_mean"], "sigma_mean alone")
        assert np.all(mean[Ka * d:] == -7.0)
        # each output alone has the bytes it has beside the others; nothing asked for is accepted
        full = pr.profile(cl, Ka, trace=True)
        cnt, pmf = np.zeros((Ka, d, ld), np.uint64), np.zeros((Ka, d, ld))
        var, trc = np.zeros((Ka, d)), np.zeros((M, Ka, d))
        for k, buf in enumerate((cnt, pmf, None, var, trc)):
            if buf is None:
                continue
            args = [None] * 5
            args[k] = ptr(buf)
            assert L.hdpm_predict_profile(h, ptr(cl), Ka, ld, *args) == 0
        same_bytes(cnt, full["center_cnt"], "center_cnt alone")
        same_bytes(pmf, full["code_pmf"], "code_pmf alone")
        same_bytes(np.sqrt(var), full["sigma_sd"], "sigma_var alone")
        same_bytes(trc, full["sigma_trace"], "sigma_trace alone")
        assert L.hdpm_predict_profile(h, ptr(cl), Ka, ld, None, None, None, None, None) == 0
        # Ka above the labels: further empty classes; Ka = None relabels the labels present (0, 2 -> 0, 1)
        wide = pr.profile(cl, 5)
        assert np.array_equal(wide["sizes"], [100, 0, 200, 0, 0])
        same_bytes(wide["sigma_mean"][:3], full["sigma_mean"], "sigma_mean at Ka = 5")
        assert np.all(wide["center_cnt"][3:] == 0) and "sigma_trace" not in wide
        dense = pr.profile(cl)
        assert dense["sizes"].tolist() == [100, 200]
        same_bytes(dense["sigma_mean"], full["sigma_mean"][[0, 2]], "sigma_mean relabelled")
        # the refusals
        refused(only_mean(ld_=int(p["att"].max()) - 1), "ld is 254", "attrisize 255", "attribute 0")
        refused(only_mean(ld_=256), "ld must be in 1..255")
        refused(only_mean(ld_=0), "ld must be in 1..255")
        refused(only_mean(Ka_=2), "0..Ka-1", "point 1")
        refused(only_mean(Ka_=0), "Ka must be in 1..255")
        refused(only_mean(Ka_=256), "Ka must be in 1..255")
        with pytest.raises(hd.HdpmError, match="ld is 100"):
            pr.profile(cl, Ka, ld=100)
        with pytest.raises(ValueError, match="N labels"):
            pr.profile(cl[:-1], Ka)
        # a later hdpm_trace_build discards the parameters
        hd.LabelTrace(p["c_trace"], engine=eng)
        refused(only_mean(), "hdpm_predict_build has not been called")
    finally:
        eng.close()


def test_padding_levels(hd):
    """ld above the largest attrisize pads every level row with zeros and changes nothing else."""
    p = pref.problem(seed=77, N=40, d=5, Ks=[3, 2], att=[2, 3, 4, 5, 6])
    cl = (np.arange(40) % 3).astype(np.int32)
    want = pref.profile(p["c_trace"], p["centers"], p["sigmas"], p["att"], cl, 3, 6)
    tr, pr = fitted(hd, p)
    try:
        a, b = pr.profile(cl, 3, trace=True), pr.profile(cl, 3, ld=9, trace=True)
    finally:
        tr.close()
    check_against(a, want, 2)
    assert b["center_cnt"].shape == (3, 5, 9) and np.all(b["center_cnt"][:, :, 6:] == 0)
    same_bytes(b["center_cnt"][:, :, :6], a["center_cnt"], "center_cnt")
    same_bytes(b["code_pmf"][:, :, :6], a["code_pmf"], "code_pmf")
    assert np.all(b["code_pmf"][:, :, 6:] == 0.0)
    same_bytes(b["sigma_trace"], a["sigma_trace"], "sigma_trace")


# ------------------------------------------------------------------ 6. a real chain

def test_zoo_chain(hd, zoo):
    from split_and_merge_gibbs_sampling_amd import posterior as P
    res = hd.run_markov_chain(zoo.codes, zoo.attrisize, zoo.gamma, zoo.v, zoo.w, m=3, iterations=40, L=1,
                              c_i=np.zeros(zoo.n, np.int32), burnin=20, t=10, r=10, neal8=True, split_merge=True,
                              seed=7, keep_params=True)
    tr_lab, cens, sigs = res["c_i"], res["centers"], res["sigmas"]
    M = tr_lab.shape[0]
    trace = hd.LabelTrace(tr_lab)
    try:
        cl = np.ascontiguousarray(P.minvi_avg(trace)[0] - 1, dtype=np.int32)
        Ka = int(cl.max()) + 1
        pr = hd.Predictive(trace, cens, sigs, zoo.attrisize, zoo.gamma)
        out = pr.profile(cl, trace=True)
    finally:
        trace.close()
    ld = int(np.max(zoo.attrisize))
    assert out["center_cnt"].shape == (Ka, zoo.d, ld)
    want = pref.profile(tr_lab, cens, sigs, zoo.attrisize, cl, Ka, ld)
    check_against(out, want, M)
    invariants(out, np.asarray(zoo.attrisize), M, cl, Ka)
