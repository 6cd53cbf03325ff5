"""MI355X: the predictive of rows with missing attributes (code 0) and the imputation of the
missing codes (csrc/predict.hip k_pr_part / k_pr_impute through Predictive.partial /
Predictive.impute) against the restatement of tests/impute_ref.py.

Complete rows are compared with density / classify by bytes; everything else within the
tolerance of tests/test_gpu_predict.py for this path: 1e-10, relative for lpd and pmf
entries, absolute for p_new, coclass and the sums of pmf rows.  The identity that ties the
imputation to hdpm_predict_new (pmf_l = exp(density(filled_l) - partial.lpd)) is held to 1e-9
relative: two lpd of magnitude ~1e2, each good to ~1e-14 relative, enter an exp, so the
ratio carries ~1e-12."""
import math

import numpy as np
import pytest

import impute_ref as iref
import predict_ref as ref

pytestmark = pytest.mark.gpu

REL = 1e-10
BAYES = 1e-9
GAMMA = 0.68


@pytest.fixture(scope="module")
def hd():
    import split_and_merge_gibbs_sampling_amd as hd
    hd.build()
    return hd


def fitted(hd, p, gamma=GAMMA, budget=None):
    tr = hd.LabelTrace(p["c_trace"], table_budget=budget)
    return tr, hd.Predictive(tr, p["centers"], p["sigmas"], p["att"], gamma)


def args(p, gamma=GAMMA):
    return p["c_trace"], p["centers"], p["sigmas"], p["att"], gamma


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


def lpd_close(got, want):
    """lpd within REL relative; a row of all gaps has lpd = 0, held to 1e-12 absolute."""
    zero = np.abs(want) <= 1e-12
    assert np.all(np.abs(got[zero]) <= 1e-12), got[zero]
    rel_close(got[~zero], want[~zero])


def rows_for(p, s, ny, noise=0.3):
    K = p["centers"][s].shape[0]
    return ref.rows_near(p["rng"], p["centers"][s][p["rng"].integers(0, K, size=ny)], p["att"], noise)


def check_pmf(got, want, att):
    """Predictive.impute's result against the restatement's: entries in the same order, pmf
    entries within REL, rows summing to 1, slots past m_j exactly 0.0, the same mode."""
    rows, attrs, pmf, mode, lpd = got
    assert np.array_equal(rows, want[0]) and np.array_equal(attrs, want[1])
    rel_close(pmf, want[2])
    if rows.size:
        abs_close(pmf.sum(axis=1), np.ones(rows.size))
        past = np.arange(pmf.shape[1])[None, :] >= np.asarray(att)[attrs][:, None]
        assert np.all(pmf[past] == 0.0) and np.all(pmf[~past] > 0.0)
    assert np.array_equal(mode, want[3])
    lpd_close(lpd, want[4])


# ------------------------------------------------------------------ 1. complete rows: the old bytes

# 257 attributes: one past the staged chunk of 256; K = 8 / 9: the cluster-group edge
@pytest.mark.parametrize("d,ny,K,M", [(1, 1, 1, 1), (17, 64, 20, 2), (65, 257, 9, 3), (257, 65, 8, 2)])
def test_complete_rows_have_the_bytes_of_predict_new(hd, d, ny, K, M):
    p = ref.problem(seed=2000 + d + K, N=K + 5, d=d, Ks=[K] * M)
    Y = rows_for(p, 0, ny)
    cl = (np.arange(K + 5) % 3).astype(np.int32)
    tr, pr = fitted(hd, p)
    try:
        lpd = pr.density(Y)
        cls, co, pn = pr.classify(Y, cl)
        got = pr.partial(Y, cl)
        plain = pr.partial(Y)
        imp = pr.impute(Y)
    finally:
        tr.close()
    assert got[0].tobytes() == lpd.tobytes() and got[1].tobytes() == pn.tobytes()
    assert got[2].tobytes() == co.tobytes()
    assert plain[0].tobytes() == lpd.tobytes() and plain[1].tobytes() == pn.tobytes() and plain[2] is None
    # no gaps: no entries, and the density alone
    assert imp[0].size == 0 and imp[1].size == 0 and imp[2].shape == (0, 0) and imp[3].size == 0
    assert imp[4].tobytes() == lpd.tobytes()


# ------------------------------------------------------------------ 2. marginals against the restatement

# d: 1, the four-code word edge (4, 5), a padding word (17, 65), one past the staged chunk (257:
# its last attribute sits alone in a word)
@pytest.mark.parametrize("d", [1, 4, 5, 17, 65, 257])
def test_marginals_against_the_restatement(hd, d):
    p = ref.problem(seed=2100 + d, N=30, d=d, Ks=[3, 9])
    N = 30
    base = rows_for(p, 1, 65)
    cl = (np.arange(N) % 4).astype(np.int32)
    tr, pr = fitted(hd, p)
    try:
        for pattern in ("none", "all", "first", "last", "alternate", "one", "row"):
            Y = iref.mask(base, pattern, np.random.default_rng(d))
            lpd_w, pn_w, co_w = iref.partial(Y, *args(p), cl, 4)
            lpd, pn, co = pr.partial(Y, cl)
            lpd_close(lpd, lpd_w)
            abs_close(pn, pn_w)
            abs_close(co, co_w)
            gone = np.flatnonzero((Y == 0).all(axis=1))
            assert gone.size == {"all": 65, "row": 1}.get(pattern, 65 if d == 1 and pattern != "none" else 0)
            # a row of all gaps: the urn's prior weights alone
            assert np.all(np.abs(lpd[gone]) <= 1e-12)
            rel_close(pn[gone], np.full(gone.size, GAMMA / (N + GAMMA)))
    finally:
        tr.close()


def coclass_case(name):
    """The three shapes of test_gpu_predict.case_values."""
    if name == "M1_Ka1":
        p = ref.problem(seed=21, N=50, d=17, Ks=[4])
        return p, rows_for(p, 0, 65), np.zeros(50, np.int32), 1
    if name == "M2_Ka3_empty":
        p = ref.problem(seed=22, N=60, d=64, Ks=[3, 6])
        return p, rows_for(p, 1, 63), np.where(np.arange(60) % 3 == 0, 0, 2).astype(np.int32), 3    # class 1 is empty
    p = ref.problem(seed=23, N=300, d=65, Ks=[1 + (5 * s) % 9 for s in range(37)])
    return p, rows_for(p, 3, 33), (np.arange(300) * 7 % 255).astype(np.int32), 255


@pytest.mark.parametrize("name", ["M1_Ka1", "M2_Ka3_empty", "M37_Ka255"])
def test_coclass_with_gaps(hd, name):
    p, Y, cl, Ka = coclass_case(name)
    Y = iref.mask(Y, "alternate")
    Y[1] = 0
    lpd_w, pn_w, co_w = iref.partial(Y, *args(p), cl, Ka)
    tr, pr = fitted(hd, p)
    try:
        lpd, pn, co = pr.partial(Y, cl, Ka)
    finally:
        tr.close()
    assert co.shape == (len(Y), Ka)
    rel_close(np.delete(lpd, 1), np.delete(lpd_w, 1))
    assert abs(lpd[1]) <= 1e-12
    abs_close(pn, pn_w)
    abs_close(co, co_w)
    if name == "M2_Ka3_empty":
        assert np.all(co[:, 1] == 0.0)


# ------------------------------------------------------------------ 3. imputation against the restatement

LEVELS = [2, 3, 64, 65, 255]          # one pass of 64 lanes, its edge, and the fourth pass's last level

# (name, att, ny, Ks, pattern, ld)
IMPUTE_CASES = [
    ("every_m_K1", LEVELS, 65, [1], "all", None),
    ("two_tiles_K8_K9", LEVELS, 257, [8, 9], "alternate", None),
    ("first_m2_wide_ld", LEVELS, 64, [9, 20], "first", 255),
    ("last_m255", LEVELS, 64, [9, 20], "last", None),
    ("one_row", [3, 65, 64, 2], 1, [20], "all", None),
    ("M37_one_gap", None, 63, [1 + (7 * s) % 20 for s in range(37)], "one", None),
    ("one_row_among_64", None, 65, [8, 9], "row", None),
    ("m64_only", [64, 5, 64], 65, [3, 1], "alternate", None),
]


@pytest.mark.parametrize("name,att,ny,Ks,pattern,ld", IMPUTE_CASES, ids=[c[0] for c in IMPUTE_CASES])
def test_imputation_against_the_restatement(hd, name, att, ny, Ks, pattern, ld):
    d = len(att) if att is not None else 17
    p = ref.problem(seed=2300 + ny + len(Ks), N=max(Ks) + 7, d=d, Ks=Ks, att=att)
    Y = iref.mask(rows_for(p, 0, ny), pattern, np.random.default_rng(ny))
    want = iref.impute(Y, *args(p), ld=ld)
    tr, pr = fitted(hd, p)
    try:
        got = pr.impute(Y, ld=ld)
        lpd = pr.partial(Y)[0]
    finally:
        tr.close()
    assert got[2].shape == (int((Y == 0).sum()), ld or int(p["att"][got[1]].max()))
    check_pmf(got, want, p["att"])
    assert got[4].tobytes() == lpd.tobytes()


# ------------------------------------------------------------------ 4. Bayes' identity across entry points

@pytest.mark.parametrize("m", [2, 6, 255])
def test_bayes_identity_with_predict_new(hd, m):
    """Rows with exactly one gap (y, j): pmf_l = p(y_O, y_j = l) / p(y_O), the numerator from
    hdpm_predict_new on the row with level l filled in."""
    d, ny, j = 17, 65, 8
    att = np.array([255, 3, 4, 2, 16, 17, 100, 4, m, 6, 2, 3, 255, 4, 6, 17, 2], np.int32)
    p = ref.problem(seed=2400 + m, N=40, d=d, Ks=[3, 8, 9, 1, 5], att=att)
    full = rows_for(p, 1, ny)
    Y = full.copy()
    Y[:, j] = 0
    filled = np.repeat(full[None], m, axis=0)
    filled[:, :, j] = np.arange(1, m + 1)[:, None]
    tr, pr = fitted(hd, p)
    try:
        rows, attrs, pmf, mode, lpd = pr.impute(Y)
        marg = pr.partial(Y)[0]
        dens = pr.density(filled.reshape(m * ny, d)).reshape(m, ny)
    finally:
        tr.close()
    assert np.array_equal(rows, np.arange(ny)) and np.all(attrs == j) and pmf.shape == (ny, m)
    assert lpd.tobytes() == marg.tobytes()
    rel_close(pmf, np.exp(dens - marg[None, :]).T, BAYES)
    abs_close(pmf.sum(axis=1), np.ones(ny))


# ------------------------------------------------------------------ 5. both branches of the running maximum

def rising_problem():
    """Six draws with the same two clusters and a sigma that falls from draw to draw: rows
    that sit on a center get a strictly larger lse in every draw."""
    d, N = 9, 30
    att = np.array([4, 3, 6, 2, 17, 5, 64, 3, 4], np.int32)
    cen = np.stack([np.ones(d), np.array(att, np.float64)])
    sig = [np.full((2, d), s) for s in (1.5, 1.1, 0.8, 0.55, 0.35, 0.2)]
    z = np.array([0] * 18 + [1] * 12)
    p = {"att": att, "centers": [cen.copy() for _ in sig], "sigmas": sig,
         "c_trace": np.stack([z] * len(sig)).astype(np.int32)}
    Y = np.stack([cen[0], cen[1], cen[0], cen[1]]).astype(np.uint8)
    Y[0, 4] = 0
    Y[1, 6] = 0
    Y[2, ::2] = 0
    Y[3, 0] = 0
    return p, Y


def test_running_maximum_rising_and_falling(hd):
    p, Y = rising_problem()
    back = {**p, "centers": p["centers"][::-1], "sigmas": p["sigmas"][::-1], "c_trace": p["c_trace"][::-1].copy()}
    lses = iref.all_terms(Y, *args(p))[0]
    assert np.all(np.diff(lses, axis=0) > 0)                  # a new maximum at every draw
    assert np.all(np.diff(iref.all_terms(Y, *args(back))[0], axis=0) < 0)
    got = []
    for q in (p, back):
        want = iref.impute(Y, *args(q))
        tr, pr = fitted(hd, q)
        try:
            got.append(pr.impute(Y))
        finally:
            tr.close()
        check_pmf(got[-1], want, q["att"])
        # a budget of 1 byte cuts the draws into chunks of one: the sums carried between
        # chunks give the same bytes
        tr, pr = fitted(hd, q, budget=1)
        try:
            cut = pr.impute(Y)
        finally:
            tr.close()
        assert cut[2].tobytes() == got[-1][2].tobytes() and cut[4].tobytes() == got[-1][4].tobytes()
    rel_close(got[0][2], got[1][2])
    lpd_close(got[0][4], got[1][4])
    assert np.array_equal(got[0][3], got[1][3])


def extreme_problem():
    """The setting of test_gpu_predict.extreme_problem (sigma 0.02, three clusters on the
    constant rows 1, 2, 3), its three rows with attribute 7 missing."""
    d = 16
    att = np.full(d, 5, np.int32)
    cens = [np.stack([np.full(d, k + 1.0) for k in range(3)]) for _ in range(2)]
    sigs = [np.full((3, d), 0.02) for _ in range(2)]
    z = np.array([0] * 30 + [1] * 6 + [2] * 4)
    p = {"att": att, "centers": cens, "sigmas": sigs, "c_trace": np.stack([z, z[::-1].copy()]).astype(np.int32)}
    Y = np.stack([np.full(d, 1), np.full(d, 2), np.full(d, 5)]).astype(np.uint8)    # center 0, center 1, nobody's
    Y[:, 7] = 0
    return p, Y


# With a cluster k dominating (r_k = 1 to the last bit) the definition gives pmf_l = r_0 / m_j +
# exp(dhamming(l, c_kj)): the dominating cluster's own row plus the new cluster's share.  At the
# suite's gamma that share is r_0 / 5 = 1.5e-13 (w_0 - w_k = log 0.68 - 15 log 5 - log 30 = -27.9),
# far above exp(mismatch) = 1.9e-22, so only the match level can equal the cluster's row within
# REL there; at gamma = 1e-25 the share is 2e-38, below REL * exp(mismatch), and every level does.
@pytest.mark.parametrize("gamma", [GAMMA, 1e-25])
def test_extremes(hd, gamma):
    p, Y = extreme_problem()
    llm = iref.ll_matrix(Y, p["centers"][0], p["sigmas"][0], p["att"])
    assert llm[0, 0] - llm[0, 1] > 745 and llm[1, 1] - llm[1, 0] > 745 and llm[2, 0] < -740
    want = iref.impute(Y, *args(p, gamma))
    tr, pr = fitted(hd, p, gamma=gamma)
    try:
        got = pr.impute(Y)
    finally:
        tr.close()
    rows, attrs, pmf, mode, lpd = got
    assert np.all(np.isfinite(pmf)) and np.all(np.isfinite(lpd)) and pmf.shape == (3, 5)
    abs_close(pmf.sum(axis=1), np.ones(3))
    check_pmf(got, want, p["att"])
    ma, mi = ref.dhamming_pair(0.02, 5)
    own = np.full((2, 5), math.exp(mi))
    own[0, 0] = own[1, 1] = math.exp(ma)
    if gamma == GAMMA:
        rel_close(pmf[[0, 1], [0, 1]], own[[0, 1], [0, 1]])
        abs_close(pmf[:2], own)
    else:
        rel_close(pmf[:2], own)                               # the dominating cluster's own row
    rel_close(pmf[2], np.full(5, 1.0 / 5))                    # nobody's row: the new cluster, a uniform code
    assert list(mode) == [1, 2, 1]


# ------------------------------------------------------------------ 6. no result depends on the budget

def test_budget_independence(hd):
    p = ref.problem(seed=2600, N=100, d=17, Ks=[3, 9, 1, 4, 12])
    assert p["att"][0] == 255
    Y = rows_for(p, 1, 257)
    Y[::3, ::2] = 0                                           # 86 rows x 9 gaps, the widest attribute among them
    for r in (63, 64, 127, 128, 191, 192, 255, 256):          # both sides of every 64-row block edge
        Y[r, 5] = 0
    Y[130] = 0
    cl = (np.arange(100) % 4).astype(np.int32)
    got = []
    for budget in (1, 64 << 10, None):
        tr, pr = fitted(hd, p, budget=budget)
        try:
            got.append(pr.partial(Y, cl) + pr.impute(Y))
        finally:
            tr.close()
    for other in got[1:]:
        for a, b in zip(got[0], other):
            assert a.dtype == b.dtype and a.tobytes() == b.tobytes()
    rows, attrs = np.nonzero(Y == 0)
    assert np.array_equal(got[0][3], rows) and np.array_equal(got[0][4], attrs)
    assert got[0][5].shape == (rows.size, 255) and rows.size > 700
    abs_close(got[0][5].sum(axis=1), np.ones(rows.size))


def test_uneven_blocks_and_a_block_without_gaps(hd):
    """Gaps only in the first and the last 64 of 257 rows, few levels.  A budget of 25,000
    bytes cuts the rows into blocks of 1, 2, 1 and 1 quanta (a quantum of complete rows costs
    ~10 KB, one with three gaps per row ~21 KB): the block of two quanta has no entry at all,
    its records take what that block's budget leaves, and its draws go in chunks; 64 KiB and
    the default make one block."""
    p = ref.problem(seed=2650, N=12, d=5, Ks=[3, 4, 2, 5, 3], att=[2, 3, 4, 3, 2])
    Y = rows_for(p, 0, 257)
    Y[:64, ::2] = 0
    Y[-64:, ::2] = 0
    want = iref.impute(Y, *args(p))
    got = []
    for budget in (25_000, 64 << 10, None):
        tr, pr = fitted(hd, p, budget=budget)
        try:
            got.append(pr.impute(Y))
        finally:
            tr.close()
    check_pmf(got[0], want, p["att"])
    assert got[0][2].shape == (128 * 3, 4)
    for other in got[1:]:
        for a, b in zip(got[0], other):
            assert a.tobytes() == b.tobytes()


# ------------------------------------------------------------------ 7. refusals

def test_refusals(hd):
    from split_and_merge_gibbs_sampling_amd._lib import ptr
    p = ref.problem(seed=71, N=20, d=5, Ks=[2, 3], att=[2, 3, 4, 5, 6])
    att, d = p["att"], 5
    K = np.array([2, 3], np.int32)
    cen, sig = np.concatenate(p["centers"]), np.concatenate(p["sigmas"])
    full = p["X"][:4].copy()
    Y = full.copy()
    Y[1, 2] = 0
    Y[3, 4] = 0
    eng = hd.Engine(0)
    L, h = eng._L, eng._h

    def refused(status, *parts):
        assert status == 5
        msg = L.hdpm_last_error(h).decode()
        for part in parts:
            assert part in msg, msg

    def changed(a, q, v):
        b = a.copy()
        b.ravel()[q] = v
        return b

    lpd, pmf = np.zeros(4), np.zeros((2, 255))

    def impute(Y_=Y, n=2, ld=6, pmf_=pmf):
        return L.hdpm_predict_impute(h, ptr(Y_), 4, n, ld, ptr(pmf_), ptr(lpd))

    try:
        trace = hd.LabelTrace(p["c_trace"], engine=eng)
        refused(L.hdpm_predict_partial(h, ptr(Y), 4, None, 0, ptr(lpd), None, None),
                "hdpm_predict_build has not been called")
        refused(impute(), "hdpm_predict_build has not been called")
        assert L.hdpm_predict_build(h, d, ptr(att), GAMMA, ptr(K), ptr(cen), ptr(sig)) == 0
        assert L.hdpm_predict_partial(h, ptr(Y), 4, None, 0, ptr(lpd), None, None) == 0
        assert impute() == 0
        assert impute(ld=255) == 0
        # the count of missing codes
        refused(impute(n=1), "n_missing is 1", "hold 2 missing codes")
        refused(impute(n=3), "n_missing is 3", "hold 2 missing codes")
        refused(impute(n=0), "n_missing is 0")
        # ld: attribute 4 has 6 levels, attribute 2 has 4
        refused(impute(ld=5), "ld is 5", "attrisize 6", "row 3, attribute 4")
        refused(impute(ld=3), "ld is 3", "attrisize 4", "row 1, attribute 2")
        refused(impute(ld=256), "ld must be in 0..255")
        # a code above m_j
        refused(impute(Y_=changed(Y, d + 1, 4)), "codes", "row 1, attribute 1")
        refused(L.hdpm_predict_partial(h, ptr(changed(Y, 3 * d, 3)), 4, None, 0, ptr(lpd), None, None),
                "codes", "row 3, attribute 0")
        # the partition, as hdpm_predict_new
        cl, co = (np.arange(20) % 3).astype(np.int32), np.zeros((4, 3))
        assert L.hdpm_predict_partial(h, ptr(Y), 4, ptr(cl), 3, None, None, ptr(co)) == 0
        refused(L.hdpm_predict_partial(h, ptr(Y), 4, ptr(cl), 2, None, None, ptr(co)), "0..Ka-1", "point 2")
        refused(L.hdpm_predict_partial(h, ptr(Y), 4, ptr(cl), 0, None, None, ptr(co)), "Ka must be in 1..255")
        # no gaps: accepted, only lpd written
        want = np.zeros(4)
        assert L.hdpm_predict_new(h, ptr(full), 4, None, 0, ptr(want), None, None) == 0
        lpd[:] = 7.0
        assert L.hdpm_predict_impute(h, ptr(full), 4, 0, 0, None, ptr(lpd)) == 0
        assert lpd.tobytes() == want.tobytes()
        # no existing behaviour changes: the complete-row calls still refuse a 0
        refused(L.hdpm_predict_new(h, ptr(Y), 4, None, 0, ptr(lpd), None, None), "codes", "row 1, attribute 2")
        pr = hd.Predictive(trace, p["centers"], p["sigmas"], att, GAMMA)
        with pytest.raises(hd.HdpmError, match="row 1, attribute 2"):
            pr.density(Y)
        with pytest.raises(hd.HdpmError, match="row 1, attribute 2"):
            pr.loglik(0, Y)
        del trace
    finally:
        eng.close()


# ------------------------------------------------------------------ 8. end to end on Zoo

def test_zoo_end_to_end(hd, zoo):
    held = np.arange(5, 101, 10)                     # 10 of the 101 animals
    train = np.setdiff1d(np.arange(zoo.n), held)
    X, full = zoo.codes[train], zoo.codes[held]
    res = hd.run_markov_chain(X, zoo.attrisize, zoo.gamma, zoo.v, zoo.w, m=3, iterations=40, L=1,
                              c_i=np.zeros(len(train), np.int32), burnin=20, t=10, r=10, neal8=True,
                              split_merge=True, seed=7, keep_params=True)
    tr_lab, cens, sigs = res["c_i"], res["centers"], res["sigmas"]
    ny, d = full.shape
    trace = hd.LabelTrace(tr_lab)
    try:
        pr = hd.Predictive(trace, cens, sigs, zoo.attrisize, zoo.gamma)
        for j in range(d):                           # one attribute at a time, in every held-out animal
            m = int(zoo.attrisize[j])
            Y = full.copy()
            Y[:, j] = 0
            rows, attrs, pmf, mode, lpd = pr.impute(Y)
            assert np.array_equal(rows, np.arange(ny)) and np.all(attrs == j) and pmf.shape == (ny, m)
            abs_close(pmf.sum(axis=1), np.ones(ny))
            assert np.all((mode >= 1) & (mode <= m))
            filled = np.repeat(full[None], m, axis=0)
            filled[:, :, j] = np.arange(1, m + 1)[:, None]
            dens = pr.density(filled.reshape(m * ny, d)).reshape(m, ny)
            rel_close(pmf, np.exp(dens - lpd[None, :]).T, BAYES)
    finally:
        trace.close()
    p = {"c_trace": tr_lab, "centers": cens, "sigmas": sigs, "att": zoo.attrisize}
    check_pmf((rows, attrs, pmf, mode, lpd), iref.impute(Y, *args(p, zoo.gamma)), zoo.attrisize)
