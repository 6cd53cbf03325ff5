"""MI355X: the posterior predictive from the recorded draws (csrc/predict.hip through
Predictive / hdpm_predict_*) against the plain restatement of tests/predict_ref.py.

The per-cluster log-densities are compared by bytes (with the restatement and with
Engine.set_state + loglik_matrix on the same rows); everything downstream of an exp or a log
within 1e-10 relative (absolute for probabilities), the project's tolerance for
log-likelihood sums; the one-pass variance within 1e-9 (1 + var) (M <= 37 draws, |l| < ~1e3:
a one-pass update's error is about M eps sqrt(1 + mean^2 / var) <= 1e-10 there)."""
import math

import numpy as np
import pytest

import predict_ref as ref

pytestmark = pytest.mark.gpu

REL = 1e-10
GAMMA = 0.68


@pytest.fixture(scope="module")
def hd():
    import split_and_merge_gibbs_sampling_amd as hd
    hd.build()
    return hd


def fitted(hd, p, gamma=GAMMA, budget=None):
    tr = hd.LabelTrace(p["c_trace"], table_budget=budget)
    return tr, hd.Predictive(tr, p["centers"], p["sigmas"], p["att"], gamma)


def rel_close(got, want, rel=REL):
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    assert got.shape == want.shape
    assert np.all(np.isfinite(got)), got
    err = np.abs(got - want)
    assert np.all(err <= rel * np.abs(want)), (float(err.max()), got.ravel()[int(err.argmax())],
                                               want.ravel()[int(err.argmax())])


def abs_close(got, want, tol=REL):
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    assert got.shape == want.shape
    assert np.all(np.isfinite(got)), got
    assert np.all(np.abs(got - want) <= tol), float(np.abs(got - want).max())


def rows_for(p, s, ny, noise=0.3):
    K = p["centers"][s].shape[0]
    return ref.rows_near(p["rng"], p["centers"][s][p["rng"].integers(0, K, size=ny)], p["att"], noise)


# ------------------------------------------------------------------ 1. the bits of ll

# d: 1, the 16-byte tile edge (16, 17), the 64-attribute word edge (64, 65), past one word pair
# (130), one past C4's width (785: four staged chunks of 256).  K: 1, 2, 20 (groups of 8, 8,
# 4), 255 (the most).  ny: one row, the wave edge (63, 64, 65), more than one tile (257).
@pytest.mark.parametrize("d,ny,K", [(1, 1, 1), (16, 63, 2), (17, 64, 20), (64, 65, 255), (65, 257, 2),
                                    (130, 1, 20), (785, 65, 255), (785, 257, 1), (130, 257, 20)])
def test_loglik_bits(hd, d, ny, K):
    p = ref.problem(seed=1000 + d + K, N=K + 5, d=d, Ks=[K])
    assert p["att"].min() == 2 and (d == 1 or p["att"].max() == 255)
    Y = rows_for(p, 0, ny)
    want = ref.ll_matrix(Y, p["centers"][0], p["sigmas"][0], p["att"])
    tr, pr = fitted(hd, p)
    try:
        ll, resp = pr.loglik(0, Y)
    finally:
        tr.close()
    assert ll.shape == (ny, K) and resp.shape == (ny, K + 1)
    assert ll.tobytes() == want.tobytes()
    # the diagnostic route on the same rows: the draw as a chain state
    eng = hd.Engine(0)
    try:
        eng.set_data(Y, p["att"], GAMMA, np.full(d, 0.5), np.full(d, 0.5))
        eng.set_state(np.arange(ny) % K, p["centers"][0], p["sigmas"][0])
        Lm, _ = eng.loglik_matrix(K)
    finally:
        eng.close()
    assert ll.tobytes() == Lm.tobytes()


# ------------------------------------------------------------------ 2. lse, lpd, resp, p_new, coclass

def case_values(name):
    if name == "M1_Ka1":
        p = ref.problem(seed=21, N=50, d=17, Ks=[4])
        return p, rows_for(p, 0, 65), np.zeros(50, np.int32), 1
    if name == "M2_Ka3_empty":
        p = ref.problem(seed=22, N=60, d=64, Ks=[3, 6])
        return p, rows_for(p, 1, 63), np.where(np.arange(60) % 3 == 0, 0, 2).astype(np.int32), 3    # class 1 is empty
    p = ref.problem(seed=23, N=300, d=65, Ks=[1 + (5 * s) % 9 for s in range(37)])
    return p, rows_for(p, 3, 33), (np.arange(300) * 7 % 255).astype(np.int32), 255


@pytest.mark.parametrize("name", ["M1_Ka1", "M2_Ka3_empty", "M37_Ka255"])
def test_new_rows_against_the_restatement(hd, name):
    p, Y, cl, Ka = case_values(name)
    M, N = p["c_trace"].shape
    lpd_w, pn_w, co_w, lse_w = ref.new_rows(Y, p["c_trace"], p["centers"], p["sigmas"], p["att"], GAMMA, cl, Ka)
    tr, pr = fitted(hd, p)
    try:
        lpd = pr.density(Y)
        cls, co, pn = pr.classify(Y, cl, Ka)
        resp = [pr.loglik(s, Y)[1] for s in range(min(M, 3))]
    finally:
        tr.close()
    rel_close(lpd, lpd_w)
    abs_close(pn, pn_w)
    assert co.shape == (len(Y), Ka)
    abs_close(co, co_w)
    assert np.array_equal(cls, np.argmax(co, axis=1))
    if name == "M2_Ka3_empty":
        assert np.all(co[:, 1] == 0.0)
    for s, r in enumerate(resp):
        llm = ref.ll_matrix(Y, p["centers"][s], p["sigmas"][s], p["att"])
        W = ref.draw_weights(llm, p["c_trace"][s], GAMMA, p["att"])
        abs_close(r, np.array([ref.responsibilities(w)[1] for w in W]))
        abs_close(r.sum(axis=1), np.ones(len(Y)))
    if M <= 2:
        # lse of each draw: the density of that draw alone is lse - log(N + gamma)
        for s in range(M):
            one = {**p, "c_trace": p["c_trace"][s:s + 1], "centers": p["centers"][s:s + 1],
                   "sigmas": p["sigmas"][s:s + 1]}
            tr, pr = fitted(hd, one)
            try:
                lse = pr.density(Y) + math.log(N + GAMMA)
            finally:
                tr.close()
            rel_close(lse, lse_w[s])


# ------------------------------------------------------------------ 3. extremes

def extreme_problem():
    d, N = 16, 40
    att = np.full(d, 5, np.int32)
    cens = [np.stack([np.full(d, k + 1.0) for k in range(3)]) for _ in range(2)]
    sigs = [np.full((3, d), 0.02) for _ in range(2)]
    z = np.array([0] * 30 + [1] * 6 + [2] * 4)
    c_trace = np.stack([z, z[::-1].copy()]).astype(np.int32)
    Y = np.stack([np.full(d, 1), np.full(d, 2), np.full(d, 5)]).astype(np.uint8)    # center 0, center 1, nobody's
    return {"att": att, "centers": cens, "sigmas": sigs, "c_trace": c_trace}, Y


def test_extremes(hd):
    p, Y = extreme_problem()
    lpd_w, pn_w, _, lse_w = ref.new_rows(Y, p["c_trace"], p["centers"], p["sigmas"], p["att"], GAMMA)
    llm = ref.ll_matrix(Y, p["centers"][0], p["sigmas"][0], p["att"])
    resp_w = np.array([ref.responsibilities(w)[1] for w in ref.draw_weights(llm, p["c_trace"][0], GAMMA, p["att"])])
    # the restatement itself meets the bounds
    assert llm[0, 0] - llm[0, 1] > 745 and llm[1, 1] - llm[1, 0] > 745
    assert np.all(resp_w[0, 2:] == 0.0) and resp_w[1, 1] == 0.0 and resp_w[1, 3] == 0.0
    assert np.all(np.isfinite(lse_w)) and np.all(np.isfinite(lpd_w))
    assert pn_w[2] > 0.99 and pn_w[0] < 1e-6
    tr, pr = fitted(hd, p)
    try:
        lpd = pr.density(Y)
        cls, co, pn = pr.classify(Y, p["c_trace"][0])
        ll, resp = pr.loglik(0, Y)
        lppd, var, cpo = pr.pointwise(np.full((40, 16), 3, np.uint8))      # every row far from its cluster
    finally:
        tr.close()
    assert ll.tobytes() == llm.tobytes()
    for a in (lpd, co, pn, resp, lppd, var, cpo):
        assert np.all(np.isfinite(a))
    assert np.all(resp[0, 2:] == 0.0) and resp[1, 1] == 0.0 and resp[1, 3] == 0.0
    abs_close(resp, resp_w)
    rel_close(lpd, lpd_w)
    abs_close(pn, pn_w)
    assert pn[2] > 0.99 and pn[0] < 1e-6
    assert cls[0] == 0 and cls[1] == 1


# ------------------------------------------------------------------ 4. no result depends on the budget

def test_budget_independence(hd):
    p = ref.problem(seed=41, N=100, d=65, Ks=[3, 9, 1, 4, 12])
    Y = rows_for(p, 1, 257)
    cl = (np.arange(100) % 4).astype(np.int32)
    got = []
    for budget in (1, 64 << 10, None):
        tr, pr = fitted(hd, p, budget=budget)
        try:
            got.append((pr.density(Y),) + pr.classify(Y, cl) + pr.pointwise(p["X"]))
        finally:
            tr.close()
    for other in got[1:]:
        for a, b in zip(got[0], other):
            assert a.tobytes() == b.tobytes()
    assert got[0][0].shape == (257,) and got[0][2].shape == (257, 4) and got[0][4].shape == (100,)


# ------------------------------------------------------------------ 5. pointwise, WAIC, LPML

@pytest.mark.parametrize("M,d,N", [(37, 64, 130), (2, 17, 65), (1, 33, 64)])
def test_pointwise(hd, M, d, N):
    p = ref.problem(seed=50 + M, N=N, d=d, Ks=[2 + (3 * s) % 7 for s in range(M)])
    lppd_w, var_w, cpo_w = ref.pointwise(p["X"], p["c_trace"], p["centers"], p["sigmas"], p["att"])
    tr, pr = fitted(hd, p)
    try:
        pw = pr.pointwise(p["X"])
    finally:
        tr.close()
    lppd, var, cpo = pw
    rel_close(lppd, lppd_w)
    rel_close(cpo, cpo_w)
    assert np.all(np.abs(var - var_w) <= 1e-9 * (1 + var_w)), float(np.abs(var - var_w).max())
    if M == 1:
        assert np.all(var == 0.0)
    # the sums: each within what its terms' tolerances add up to
    w_tol = 2 * (REL * float(np.abs(lppd_w).sum()) + 1e-9 * float((1 + var_w).sum()))
    assert abs(hd.waic(pw) - ref.waic(lppd_w, var_w)) <= w_tol
    assert abs(hd.lpml(pw) - ref.lpml(cpo_w)) <= REL * float(np.abs(cpo_w).sum())
    assert hd.waic(pw) == -2.0 * math.fsum(float(a) - float(b) for a, b in zip(lppd, var))
    assert hd.lpml(pw) == math.fsum(cpo.tolist())


# ------------------------------------------------------------------ 6. end to end on Zoo

def test_zoo_end_to_end(hd, zoo):
    from split_and_merge_gibbs_sampling_amd import posterior as P
    held = np.arange(5, 101, 10)                     # 10 of the 101 animals
    train = np.setdiff1d(np.arange(zoo.n), held)
    X, Y = zoo.codes[train], zoo.codes[held]
    res = hd.run_markov_chain(X, zoo.attrisize, zoo.gamma, zoo.v, zoo.w, m=3, iterations=40, L=1,
                              c_i=np.zeros(len(train), np.int32), burnin=20, t=10, r=10, neal8=True,
                              split_merge=True, seed=7, keep_params=True)
    tr_lab, cens, sigs = res["c_i"], res["centers"], res["sigmas"]
    assert tr_lab.shape == (40, 91) and len(cens) == 40 and len(sigs) == 40
    trace = hd.LabelTrace(tr_lab)
    try:
        cl = P.minvi_avg(trace)[0] - 1
        Ka = int(cl.max()) + 1
        pr = hd.Predictive(trace, cens, sigs, zoo.attrisize, zoo.gamma)
        lpd = pr.density(Y)
        cls, co, pn = pr.classify(Y, cl)
        pw = pr.pointwise(X)
    finally:
        trace.close()
    lpd_w, pn_w, co_w, _ = ref.new_rows(Y, tr_lab, cens, sigs, zoo.attrisize, zoo.gamma, cl, Ka)
    rel_close(lpd, lpd_w)
    abs_close(pn, pn_w)
    abs_close(co, co_w)
    assert np.array_equal(cls, np.argmax(co_w, axis=1))
    lppd_w, var_w, cpo_w = ref.pointwise(X, tr_lab, cens, sigs, zoo.attrisize)
    rel_close(pw[0], lppd_w)
    rel_close(pw[2], cpo_w)
    assert np.all(np.abs(pw[1] - var_w) <= 1e-9 * (1 + var_w))
    assert abs(hd.lpml(pw) - ref.lpml(cpo_w)) <= REL * float(np.abs(cpo_w).sum())


# ------------------------------------------------------------------ 7. refusals

def test_refusals(hd):
    from split_and_merge_gibbs_sampling_amd._lib import ptr
    p = ref.problem(seed=71, N=20, d=5, Ks=[2, 3], att=[2, 3, 4, 5, 6])
    att, d = p["att"], 5
    K = np.array([2, 3], np.int32)
    cen, sig = np.concatenate(p["centers"]), np.concatenate(p["sigmas"])
    Y = np.ascontiguousarray(p["X"][:4])
    eng = hd.Engine(0)
    L, h = eng._L, eng._h

    def refused(status, *parts):
        assert status == 5
        msg = L.hdpm_last_error(h).decode()
        for part in parts:
            assert part in msg, msg

    def build(d_=d, att_=att, gamma=GAMMA, K_=K, cen_=cen, sig_=sig):
        att_ = np.ascontiguousarray(att_, np.int32)
        return L.hdpm_predict_build(h, d_, ptr(att_), gamma, ptr(K_), ptr(np.ascontiguousarray(cen_)),
                                    ptr(np.ascontiguousarray(sig_)))

    def changed(a, q, v):
        b = a.copy()
        b.ravel()[q] = v
        return b

    lpd = np.zeros(4)
    try:
        # before hdpm_trace_build, then before hdpm_predict_build
        refused(build(), "hdpm_trace_build has not been called")
        refused(L.hdpm_predict_new(h, ptr(Y), 4, None, 0, ptr(lpd), None, None), "hdpm_trace_build has not been called")
        trace = hd.LabelTrace(p["c_trace"], engine=eng)
        refused(L.hdpm_predict_new(h, ptr(Y), 4, None, 0, ptr(lpd), None, None),
                "hdpm_predict_build has not been called")
        refused(L.hdpm_predict_own(h, ptr(p["X"]), ptr(np.zeros(20)), None, None),
                "hdpm_predict_build has not been called")
        refused(L.hdpm_predict_loglik(h, 0, ptr(Y), 4, ptr(np.zeros((4, 2))), None),
                "hdpm_predict_build has not been called")
        # the model and the parameters
        refused(build(K_=np.array([2, 2], np.int32)), "draw 1", "total_cls is 2", "3 clusters")
        refused(build(d_=0), "d must be positive")
        refused(build(att_=[2, 3, 0, 5, 6]), "attrisize", "attribute 2")
        refused(build(att_=[2, 3, 4, 5, 256]), "attrisize", "attribute 4")
        refused(build(gamma=0.0), "gamma")
        refused(build(gamma=-1.0), "gamma")
        refused(build(cen_=changed(cen, 2 * d + 1, 4.0)), "center", "draw 1, cluster 0, attribute 1")
        refused(build(cen_=changed(cen, 0, 0.0)), "center", "draw 0, cluster 0, attribute 0")
        refused(build(cen_=changed(cen, d + 3, 1.5)), "center", "draw 0, cluster 1, attribute 3")
        refused(build(sig_=changed(sig, 4 * d + 4, 0.0)), "sigma", "draw 1, cluster 2, attribute 4")
        refused(build(sig_=changed(sig, 2, float("nan"))), "sigma", "draw 0, cluster 0, attribute 2")
        refused(build(sig_=changed(sig, 2, float("inf"))), "sigma", "draw 0, cluster 0, attribute 2")
        # a refused build leaves no parameters
        refused(L.hdpm_predict_new(h, ptr(Y), 4, None, 0, ptr(lpd), None, None),
                "hdpm_predict_build has not been called")
        assert build() == 0
        assert L.hdpm_predict_new(h, ptr(Y), 4, None, 0, ptr(lpd), None, None) == 0
        assert L.hdpm_predict_new(h, ptr(Y), 4, None, 0, None, None, None) == 0       # nothing asked for
        # rows, classes, draws
        refused(L.hdpm_predict_new(h, ptr(changed(Y, d + 2, 0)), 4, None, 0, ptr(lpd), None, None),
                "codes", "row 1, attribute 2")
        refused(L.hdpm_predict_new(h, ptr(changed(Y, 3 * d, 3)), 4, None, 0, ptr(lpd), None, None),
                "codes", "row 3, attribute 0")
        refused(L.hdpm_predict_own(h, ptr(changed(p["X"], 19 * d + 4, 7)), ptr(np.zeros(20)), None, None),
                "codes", "row 19, attribute 4")
        refused(L.hdpm_predict_loglik(h, 0, ptr(changed(Y, 1, 4)), 4, ptr(np.zeros((4, 2))), None),
                "codes", "row 0, attribute 1")
        cl, co = (np.arange(20) % 3).astype(np.int32), np.zeros((4, 3))
        assert L.hdpm_predict_new(h, ptr(Y), 4, ptr(cl), 3, None, None, ptr(co)) == 0
        refused(L.hdpm_predict_new(h, ptr(Y), 4, ptr(cl), 2, None, None, ptr(co)), "0..Ka-1", "point 2")
        refused(L.hdpm_predict_new(h, ptr(Y), 4, ptr(cl), 0, None, None, ptr(co)), "Ka must be in 1..255")
        refused(L.hdpm_predict_new(h, ptr(Y), 4, ptr(cl), 256, None, None, ptr(np.zeros((4, 256)))),
                "Ka must be in 1..255")
        refused(L.hdpm_predict_loglik(h, -1, ptr(Y), 4, ptr(np.zeros((4, 3))), None), "draw -1", "0..1")
        refused(L.hdpm_predict_loglik(h, 2, ptr(Y), 4, ptr(np.zeros((4, 3))), None), "draw 2", "0..1")
        # a later hdpm_trace_build discards the parameters
        trace2 = hd.LabelTrace(p["c_trace"], engine=eng)
        refused(L.hdpm_predict_new(h, ptr(Y), 4, None, 0, ptr(lpd), None, None),
                "hdpm_predict_build has not been called")
        # the Python layer: labels that are not exactly 0..K_s-1
        with pytest.raises(ValueError, match="exactly 0..1"):
            hd.Predictive(hd.LabelTrace(p["c_trace"] + 1, engine=eng), p["centers"], p["sigmas"], att, GAMMA)
        with pytest.raises(ValueError, match="draw 1"):
            hd.Predictive(trace2, p["centers"], [p["sigmas"][0], p["sigmas"][1][:2]], att, GAMMA)
        del trace
    finally:
        eng.close()
