"""Device update_phi (csrc/phi.hip) where the parity suite never took it: attributes with more
than kPhiLdsLevels = 16 levels (the global cum / perm scratch of phi_prep_item_in), up to the 255
a uint8 code holds, a one-level attribute, Rcpp sample's Walker threshold (nc > 200), rhig's
bisection branch, drifts that leave the windows, and the split-merge device chain on such data.

Every case runs a first sweep (it launches the window of the device's random stream that a
device update reads; the case's state is set again after it), then `UPDATES` rounds of update_phi
(from the state the case sets, then from what the sweeps make of it) and a Neal-8 sweep (m = 3),
on the oracle first (reference_chain, shared by
the three device paths, read-only) and then on the engine (replay), comparing after every step:
labels, centers, sigmas and the RNG state bit for bit, after every update loglik_matrix's L and
H bit for bit (the tables the update committed) and compute_loglikelihood within 1e-10; the
sweeps read the committed bound records and heads, the updates after them the speculated and
chained device updates.

What the device is expected to do -- commit, or hand back with which status -- comes from
tests/phi_predict.py: numpy restatements of the reference's decisions on the oracle's states,
never from the device's status word.  Each test asserts its own predicate on those first.

path: "fast" (launch_phi2 first), "trees" (the general kernels' composition trees), "walks"
(Debug.PHI_WALKS: the per-start-drift walks)."""
import numpy as np
import pytest

import phi_predict as PP
from split_and_merge_gibbs_sampling_amd import Debug

pytestmark = pytest.mark.gpu

RTOL = 1e-10
UPDATES = 3
PATHS = ["fast", "trees", "walks"]
MIXED = [2, 16, 17, 3, 40, 6, 255, 16, 17]          # both sides of 16 inside one group of 8


@pytest.fixture(scope="module")
def hd():
    import split_and_merge_gibbs_sampling_amd as hd
    hd.build()
    return hd


def make_engine(hd, ds):
    e = hd.Engine(0)
    e.set_data(ds.codes, ds.attrisize, ds.gamma, ds.v, ds.w)
    return e


def random_params(ds, K, seed, lo=0.15, hi=2.5):
    rng = np.random.default_rng(seed)
    cen = np.stack([rng.integers(1, ds.attrisize + 1) for _ in range(K)]).astype(np.float64)
    sig = rng.uniform(lo, hi, size=(K, ds.d))
    return cen, sig


def converged_params(ds, c, K, sigma=0.5):
    """Centers at each cluster's per-attribute mode, sigmas `sigma`."""
    cen = np.zeros((K, ds.d))
    for k in range(K):
        rows = ds.codes[c == k]
        for j in range(ds.d):
            cen[k, j] = np.bincount(rows[:, j], minlength=int(ds.attrisize[j]) + 1)[1:].argmax() + 1
    return cen, np.full((K, ds.d), sigma)


def mixture(n, attrisize, k, seed, sigma=0.25, v=6.0, w=0.25):
    """data.hamming_mixture's model (equal cluster sizes, P(x_j = c_j) = 1 / (1 + (m_j - 1)
    e^(-1/sigma)), else uniform over the other levels) with the level counts given per attribute."""
    from split_and_merge_gibbs_sampling_amd.data import Dataset
    mm = np.asarray(attrisize, np.int32)
    d = len(mm)
    rng = np.random.Generator(np.random.MT19937(seed))
    centers = (rng.random((k, d)) * mm[None, :]).astype(np.int64) + 1
    sizes = np.full(k, n // k, np.int64)
    sizes[: n - sizes.sum()] += 1
    truth = np.repeat(np.arange(k, dtype=np.int32), sizes)
    p_c = 1.0 / (1.0 + (mm - 1.0) * np.exp(-1.0 / sigma))
    cen = centers[truth]
    keep = rng.random((n, d)) < p_c[None, :]
    off = (rng.random((n, d)) * np.maximum(mm[None, :] - 1, 1)).astype(np.int64) + 1
    other = (cen - 1 + off) % mm[None, :] + 1
    codes = np.where(keep, cen, other).astype(np.uint8)
    return Dataset(codes, mm, np.full(d, v), np.full(d, w), 0.68, truth, "mixture")


def mixed_levels(d, one_level_at=None):
    mm = [MIXED[j % len(MIXED)] for j in range(d)]
    if one_level_at is not None:
        mm[one_level_at] = 1
    return mm


LADDER = ["m2", "m15", "m16", "m17", "m33", "m64", "m200", "m255", "mixed24", "mixed136"]


def ladder_dataset(key, n=2400, k=6):
    """Section 1 / 2 data: hamming_mixture's model, n points in k equal clusters, generator sigma
    0.25 (P(x_j = c_j) from 0.98 at 2 levels to 0.18 at 255: the center stays each cluster's mode)."""
    if key == "mixed24":
        return mixture(n, mixed_levels(24), k, seed=101)
    if key == "mixed136":
        return mixture(n, mixed_levels(136), k, seed=102)
    if key == "one24":
        return mixture(n, mixed_levels(24, one_level_at=11), k, seed=103)
    from split_and_merge_gibbs_sampling_amd.data import hamming_mixture
    m = int(key[1:])
    return hamming_mixture(n, 24, k, m, sigma=0.25, seed=100 + m)


# ------------------------------------------------------------------ the oracle's chain
_refs = {}


def _frozen(a):
    a = np.array(a, copy=True)
    a.setflags(write=False)
    return a


def reference_chain(oracle, key, make, updates=UPDATES, m=3):
    """The oracle's chain of a case, computed once per key and shared read-only by the paths.
    make() -> (ds, c, cen, sig, seed).  Steps: ("sweep" | "reset" | "phi", labels, K, centers,
    sigmas, rng[, L, H, ll, prediction])."""
    if key in _refs:
        return _refs[key]
    ds, c, cen, sig, seed = make()
    K = cen.shape[0]
    st = oracle.seed_state(seed)
    pc, ps, s0 = oracle.pool_generate(ds.attrisize, ds.v, ds.w, ds.n * 3, st)
    assert s0 == 0
    ref = dict(ds=ds, c=_frozen(np.asarray(c, np.int32)), cen=_frozen(cen), sig=_frozen(sig), pc=_frozen(pc),
               ps=_frozen(ps), rng0=_frozen(st), steps=[], preds=[])
    ost = oracle.OracleState(c, K, cen, sig)

    def snap(kind, *more):
        ref["steps"].append((kind, _frozen(ost.c_i), ost.K, _frozen(ost.centers[:ost.K]), _frozen(ost.sigma[:ost.K]),
                             _frozen(st)) + more)

    # a device update needs a window of the device's random stream, which a sweep launches: one
    # sweep first (both sides, compared), then the case's state set again for the first update
    assert oracle.neal8_sweep(ds.codes, ds.attrisize, ds.gamma, ds.v, ds.w, ost, m, pc, ps, st, fast=1) == 0
    snap("sweep")
    ost = oracle.OracleState(c, K, cen, sig)
    snap("reset")
    for u in range(updates):
        sig_before, st_before = ost.sigma[:ost.K].copy(), st.copy()
        assert oracle.update_phi(ds.codes, ds.attrisize, ds.v, ds.w, ost, st) == 0
        consumed = PP.stream_distance(oracle, st_before, st, 40 * ost.K * ds.d + 1000)
        pred = PP.UpdatePrediction(oracle, ds, ost.c_i, ost.K, sig_before, ost.centers[:ost.K], consumed)
        L, H = oracle.loglik_matrix(ds.codes, ds.attrisize, ost.centers[:ost.K], ost.sigma[:ost.K])
        snap("phi", _frozen(L), _frozen(H), oracle.compute_loglikelihood(ds.codes, ds.attrisize, ost), pred)
        ref["preds"].append(pred)
        assert oracle.neal8_sweep(ds.codes, ds.attrisize, ds.gamma, ds.v, ds.w, ost, m, pc, ps, st, fast=1) == 0
        snap("sweep")
    _refs[key] = ref
    return ref


def assert_ambiguity_cap(preds):
    """Branch tests within 1e-6 of the threshold are no predictions; under 5% of the items."""
    near = sum(p.n_near for p in preds)
    items = sum(p.items for p in preds)
    assert near < 0.05 * items, (near, items)


def replay(hd, ref, path, sd_scale=None, m=3):
    """The reference's steps on the engine with update_phi on the device by `path`; every step
    compared (module docstring).  Returns the final stats and, per update, the increments of
    phi_device_calls / phi_device_fallbacks / phi_tree_retries and the status mask so far."""
    ds = ref["ds"]
    eng = make_engine(hd, ds)
    try:
        eng.set_debug(Debug.PHI_WALKS if path == "walks" else 0)
        eng.set_phi_device(True, general=path != "fast")
        if sd_scale is not None:
            eng.set_phi_sd_scale(sd_scale)
        eng.set_state(ref["c"], ref["cen"], ref["sig"])
        eng.set_pool(ref["pc"], ref["ps"])
        eng.rng_state = ref["rng0"].copy()
        per, prev = [], eng.stats()
        for q, step in enumerate(ref["steps"]):
            kind, c_ref, K, cen_ref, sig_ref, rng_ref = step[:6]
            if kind == "sweep":
                eng.neal8_sweep(m)
            elif kind == "reset":
                eng.set_state(ref["c"], ref["cen"], ref["sig"])
            else:
                eng.update_phi()
            c, cen, sig = eng.get_state()
            assert cen.shape[0] == K, (q, kind)
            assert np.array_equal(c, c_ref), (q, kind, "labels")
            assert np.array_equal(cen, cen_ref), (q, kind, "centers")
            assert np.array_equal(sig, sig_ref), (q, kind, "sigmas")
            assert np.array_equal(eng.rng_state, rng_ref), (q, kind, "rng state")
            if kind == "phi":
                L_ref, H_ref, ll_ref = step[6:9]
                L, H = eng.loglik_matrix(K)
                assert np.array_equal(H, H_ref), (q, "H")
                assert np.array_equal(L, L_ref), (q, "L: the committed tables")
                ll = eng.compute_loglikelihood()
                assert abs(ll - ll_ref) <= RTOL * abs(ll_ref), (q, ll, ll_ref)
                s = eng.stats()
                per.append(dict(calls=s["phi_device_calls"] - prev["phi_device_calls"],
                                fallbacks=s["phi_device_fallbacks"] - prev["phi_device_fallbacks"],
                                retries=s["phi_tree_retries"] - prev["phi_tree_retries"],
                                mask=s["phi_fallback_status_mask"]))
                prev = s
        stats = eng.stats()
    finally:
        eng.close()
    phis = {k: v for k, v in stats.items() if k.startswith("phi_")}
    print(path, sd_scale, [(p["calls"], p["fallbacks"], p["retries"], bin(p["mask"])) for p in per], phis)
    return stats, per


def check_against_predictions(stats, per, preds):
    """Per update, unless it is excused (an ambiguous branch test, or an end drift beyond
    Z_INSIDE model standard deviations: the test then claims neither outcome): a prediction with
    a Walker item or a clear bisection item is handed back and counts as exactly one hand-back
    and no commit, showing its status unless a larger allowed one can hide it (atomicMax); any
    other is committed and counts as exactly one commit and no hand-back.  The statuses of the
    hand-backs are always among those the predictions allow.  Returns the number of updates
    held to their prediction."""
    assert len(per) == len(preds)
    allowed = held = 0
    for q, (p, got) in enumerate(zip(preds, per)):
        if got["calls"] == 0 or got["fallbacks"]:
            allowed |= p.allowed_mask()
        excused = p.may_leave_window or p.ambiguous
        assert got["calls"] + got["fallbacks"] == 1, (q, got, "one update, one count")
        if p.handed_back:
            assert got["calls"] == 0 and got["fallbacks"] == 1, (q, got, "committed an update it cannot draw")
        elif not excused:
            assert got["calls"] == 1 and got["fallbacks"] == 0, (q, got, p.z, "handed back an update the device can draw")
        assert got["mask"] & ~allowed == 0, (q, bin(got["mask"]), bin(allowed))
        if p.handed_back and not excused:
            top = PP.BISECT if p.bisect else PP.WALKER
            assert got["mask"] >> top & 1, (q, bin(got["mask"]), top)
        held += p.handed_back or not excused
    return held


def held(preds):
    """The updates check_against_predictions holds to their prediction (CPU side)."""
    return [p for p in preds if p.handed_back or not (p.may_leave_window or p.ambiguous)]


def path_counters(stats, path, updates=UPDATES):
    if path == "fast":
        assert stats["phi_fast_calls"] >= updates and stats["phi_fast_handbacks"] == 0, stats
    elif path == "trees":
        assert stats["phi_tree_calls"] >= updates and stats["phi_tree_retries"] == 0, stats
    else:
        assert stats["phi_tree_calls"] == 0 and stats["phi_fast_calls"] == 0, stats


# ------------------------------------------------------------------ 1. level ladder, converged
def _converged(key):
    def make():
        ds = ladder_dataset(key)
        cen, sig = converged_params(ds, ds.truth, 6)
        return ds, ds.truth, cen, sig, 61
    return make


@pytest.mark.parametrize("path", PATHS)
@pytest.mark.parametrize("key", LADDER)
def test_level_ladder_converged(hd, oracle, key, path):
    """Level counts on both sides of kPhiLdsLevels, up to 255, alone and mixed inside one
    workgroup (d = 24) and over two walk segments (d = 136), from a converged state: every pick
    fixed, no Walker table, no bisection -- every update commits on the path asked for."""
    ref = reference_chain(oracle, ("conv", key), _converged(key))
    preds = ref["preds"]
    assert all(p.all_fixed and not p.walker and not p.bis.any() and p.min_count >= 16 for p in preds)
    assert_ambiguity_cap(preds)
    stats, per = replay(hd, ref, path)
    check_against_predictions(stats, per, preds)
    assert stats["phi_device_calls"] == UPDATES and stats["phi_device_fallbacks"] == 0, stats
    path_counters(stats, path)


# ------------------------------------------------------------------ 2. level ladder, unsettled
def _unsettled(key, small):
    def make():
        ds = ladder_dataset(key, n=600, k=24) if small else ladder_dataset(key)
        K = 24 if small else 6
        cen, sig = random_params(ds, K, 13)
        return ds, ds.truth, cen, sig, 62
    return make


SETTLED_AT_400 = {"m2", "m15", "m16", "m17", "m33", "m64"}


@pytest.mark.parametrize("path", PATHS)
@pytest.mark.parametrize("small", [False, True], ids=["k6", "k24"])
@pytest.mark.parametrize("key", LADDER)
def test_level_ladder_unsettled(hd, oracle, key, small, path):
    """The same level counts from random parameters (sigma up to 2.5: many candidates per item,
    picks that depend on the uniform), 400 and 25 points per cluster."""
    ref = reference_chain(oracle, ("uns", key, small), _unsettled(key, small))
    preds = ref["preds"]
    # the first update's picks depend on the uniform, except where 400 members agree on a few levels
    assert preds[0].all_fixed == (not small and key in SETTLED_AT_400)
    assert_ambiguity_cap(preds)
    stats, per = replay(hd, ref, path)
    check_against_predictions(stats, per, preds)
    assert stats["phi_device_calls"] + stats["phi_device_fallbacks"] == UPDATES, stats
    if not any(p.handed_back or p.ambiguous for p in preds):
        assert stats["phi_device_fallbacks"] == 0, stats
    if key == "mixed136" and not small:
        assert not preds[0].walker and not preds[0].bis.any()      # the retry assert below applies
    if path == "trees" and not preds[0].walker and not preds[0].bis.any():
        # two walk segments (d > 128): the update is re-run by the walks (kPhiNonDet); one
        # segment: the cluster is walked inside the tree-mode update
        if ref["ds"].d > 128:
            assert per[0]["retries"] >= 1, per
        else:
            assert stats["phi_tree_retries"] == 0, stats


# ------------------------------------------------------------------ m_j = 1
# The reference defines an attribute with one level: sample(1:1, 1, TRUE, prob) takes one
# uniform and returns level 1 (SampleReplace with n = 1), dhamming's log(1 + (m - 1) / e^(1/s))
# is 0, and rhig's branch test fails on (m - 1) / m = 0 > 0, so every sigma comes from the
# bisection branch, where norm_const2 and lF_conK2 reduce to u^(w + 1) = Omega.  The device
# therefore hands every such update back (kPhiBisect) and the host draws it.
@pytest.mark.parametrize("path", PATHS)
@pytest.mark.parametrize("state", ["converged", "unsettled"])
def test_one_level_attribute(hd, oracle, state, path):
    ref = reference_chain(oracle, ("one", state), _converged("one24") if state == "converged" else _unsettled("one24", False))
    preds = ref["preds"]
    assert int(ref["ds"].attrisize[11]) == 1
    assert all(p.bis[:, 11].all() and not p.near[:, 11].any() for p in preds)    # a bisection item in every update
    assert_ambiguity_cap(preds)
    stats, per = replay(hd, ref, path)
    check_against_predictions(stats, per, preds)
    assert stats["phi_device_calls"] == 0 and stats["phi_device_fallbacks"] == UPDATES, stats
    assert stats["phi_fallback_status_mask"] >> PP.BISECT & 1, stats


# ------------------------------------------------------------------ 3. Walker boundary
def walker_dataset(levels, n=480, seed=17, clustered=False):
    """One attribute of `levels` levels beside three small ones: uniform codes, or (clustered) 24
    clusters of the mixture model."""
    from split_and_merge_gibbs_sampling_amd.data import Dataset
    if clustered:
        return mixture(n, [levels, 4, 2, 3], WALKER_K, seed=seed, sigma=0.15)
    rng = np.random.default_rng(seed)
    att = np.array([levels, 4, 2, 3], np.int32)
    codes = np.stack([rng.integers(1, a + 1, size=n) for a in att], axis=1).astype(np.uint8)
    return Dataset(codes, att, np.full(4, 6.0), np.full(4, 0.25), 0.68, np.zeros(n, np.int32), "walker")


WALKER_K = 24


def _walker(levels, state):
    def make():
        if state == "clustered":
            ds = walker_dataset(levels, clustered=True)
            cen, sig = converged_params(ds, ds.truth, WALKER_K, sigma=0.3)
            return ds, ds.truth, cen, sig, 65
        ds = walker_dataset(levels)
        c = (np.arange(ds.n) % WALKER_K).astype(np.int32)
        if state == "flat":
            cen, sig = random_params(ds, WALKER_K, 3, 2.0, 6.0)
        else:
            cen, sig = random_params(ds, WALKER_K, 3, 0.02, 0.05)
        return ds, c, cen, sig, 63
    return make


@pytest.mark.parametrize("path", PATHS)
@pytest.mark.parametrize("levels,state", [(200, "flat"), (201, "flat"), (250, "flat"), (250, "concentrated"),
                                          (250, "clustered")])
def test_walker_boundary(hd, oracle, levels, state, path):
    """Rcpp sample() takes Walker's alias method iff more than 200 levels have m_j p > 0.1: 24
    clusters of 20 points with sigmas in [2, 6] have near-flat level probabilities (every level
    counts), with sigmas near 0.03 only the most frequent levels do.  On the uniform codes that
    holds for the first update only (the sweeps dissolve the clusters and the sigmas drawn for
    them are flat again: Walker items from the second update on); on 24 clusters of the mixture
    model ("clustered") in all three."""
    ref = reference_chain(oracle, ("walker", levels, state), _walker(levels, state))
    preds = ref["preds"]
    first = preds[0]
    if state == "clustered":
        assert all((p.nc <= 200).all() and not p.handed_back for p in preds)
    elif state == "concentrated":
        assert (first.nc <= 200).all() and not first.handed_back and any(p.walker for p in preds[1:])
    elif levels == 200:
        assert (first.nc[:, 0] == 200).all() and not any(p.walker for p in preds)
        assert any(not p.handed_back for p in preds)                 # the device has something to commit
    else:
        assert (first.nc[:, 0] > 200).all()
        assert any(p.walker and not p.bis.any() for p in preds)      # a Walker status nothing hides
    assert_ambiguity_cap(preds)
    # the counters are compared per update: every predicted hand-back, and at 200 levels and in
    # the concentrated states a commit, is held to its prediction (not excused by its drift)
    if levels > 200 and state != "clustered":
        assert any(p.handed_back for p in held(preds))
    if levels == 200 or state != "flat":
        assert any(not p.handed_back for p in held(preds))
    stats, per = replay(hd, ref, path)
    assert check_against_predictions(stats, per, preds) == len(held(preds))
    marked = sum(p.handed_back for p in preds)
    assert stats["phi_device_fallbacks"] >= marked and stats["phi_device_calls"] + stats["phi_device_fallbacks"] == UPDATES
    if len(held(preds)) == UPDATES:
        assert stats["phi_device_fallbacks"] == marked, stats
    if levels > 200 and state != "clustered":
        assert stats["phi_fallback_status_mask"] >> PP.WALKER & 1, stats


# ------------------------------------------------------------------ 4. bisection hand-back
def small_cluster_labels(n, sizes):
    """Labels of consecutive clusters whose sizes cycle through `sizes`."""
    c, k, i = np.zeros(n, np.int32), 0, 0
    while i < n:
        s = sizes[k % len(sizes)]
        c[i:i + s] = k
        i += s
        k += 1
    return c, k


def _bisect_case(which, sizes, sig_lo, sig_hi, seed=23):
    def make():
        if which == "zoo":
            from split_and_merge_gibbs_sampling_amd.data import load_zoo
            ds = load_zoo()
        else:
            # priors v = 1.2, w = 20: a center no member shares (f = 0) sends rhig to the bisection
            # branch at 1 to 3 members, a shared one to the beta branch (under the usual v = 6,
            # w = 0.25, and under Zoo's priors below 9 members, no draw takes the bisection branch)
            ds = mixture(96, [17] * 8, 4, seed=104, v=1.2, w=20.0)
        c, K = small_cluster_labels(ds.n, sizes)
        cen, sig = random_params(ds, K, 5, sig_lo, sig_hi)
        return ds, c, cen, sig, seed
    return make


# Clusters of 1 to 3 members reject far more rbeta attempts than the window model expects (end
# drifts 5 to 180 model standard deviations out), so their updates are excused either way; the
# cases with 8 to 25 members are the ones held to their predictions (|z| <= Z_INSIDE), chosen on
# the CPU to hold, per data set, a clear bisection update and an update without one.
BISECT_CASES = {
    "zoo_singletons": ("zoo", [1], 0.15, 2.5),
    "zoo_pairs_triples": ("zoo", [2, 3], 0.15, 2.5),
    "zoo_dozens": ("zoo", [10, 13], 2.5, 6.0),
    "zoo_twenties": ("zoo", [20, 25], 0.15, 2.5, 24),
    "m17_singletons": ("m17", [1], 0.15, 2.5),
    "m17_pairs_triples": ("m17", [2, 3], 0.15, 2.5),
    "m17_singletons_tight": ("m17", [1], 0.01, 0.02),
    "m17_eights": ("m17", [8, 16], 0.15, 2.5),
    "m17_twelves": ("m17", [12], 0.15, 2.5),
}


@pytest.mark.parametrize("which", ["zoo", "m17"])
def test_bisection_cases_cover_both_outcomes(oracle, which):
    """Per data set, the cases of test_bisection_handback hold an update with a clear bisection
    item and an update without any that are held to their prediction: not ambiguous, the end
    drift within Z_INSIDE of the window model (CPU only)."""
    preds = [p for name, a in BISECT_CASES.items() if a[0] == which
             for p in held(reference_chain(oracle, ("bis", name), _bisect_case(*a))["preds"])]
    assert any(p.bisect and not p.may_leave_window and not p.ambiguous for p in preds)
    assert any(not p.bis.any() and not p.walker for p in preds)


@pytest.mark.parametrize("path", PATHS)
@pytest.mark.parametrize("name", list(BISECT_CASES))
def test_bisection_handback(hd, oracle, name, path):
    """Clusters of one, two and three members: an update whose drawn center sends rhig to its
    bisection branch is handed back (kPhiBisect, or kPhiAmbig beside an ambiguous test), every
    other one is committed; the chain is the oracle's either way."""
    ref = reference_chain(oracle, ("bis", name), _bisect_case(*BISECT_CASES[name]))
    preds = ref["preds"]
    assert not any(p.walker for p in preds)
    assert_ambiguity_cap(preds)
    stats, per = replay(hd, ref, path)
    assert check_against_predictions(stats, per, preds) == len(held(preds))
    window = (1 << PP.WINDOW | 1 << PP.SHORT) if any(p.may_leave_window for p in preds) else 0
    assert stats["phi_fallback_status_mask"] & ~(1 << PP.BISECT | 1 << PP.AMBIG | 1 << PP.NONDET | window) == 0, stats


# ------------------------------------------------------------------ 5. drift leaving the window
SCALE_SEEDS = [71, 72, 73, 74]


def _c5_like(seed, K=4):
    def make():
        from split_and_merge_gibbs_sampling_amd.data import hamming_mixture
        ds = hamming_mixture(4000, 128, K, 4, seed=5)
        cen, sig = converged_params(ds, ds.truth, K)
        return ds, ds.truth, cen, sig, seed
    return make


def test_phi_sd_scale_option(hd, zoo):
    eng = make_engine(hd, zoo)
    try:
        from split_and_merge_gibbs_sampling_amd._lib import OPT_PHI_SD_SCALE as opt
        assert opt == 11 and eng.get_option(opt) == 1.0
        for v in (0.0, 0.25, 1.0):
            eng.set_phi_sd_scale(v)
            assert eng.get_option(opt) == v
        for v in (-0.1, 1.5, float("nan")):
            with pytest.raises(hd.HdpmError) as e:
                eng.set_phi_sd_scale(v)
            assert e.value.status == 5
        assert eng.get_option(opt) == 1.0
    finally:
        eng.close()


@pytest.mark.parametrize("scale", [1.0, 0.25, 0.0])
@pytest.mark.parametrize("path", PATHS)
def test_drift_leaves_the_window(hd, oracle, path, scale):
    """HDPM_OPT_PHI_SD_SCALE narrows the drift windows (C5-like shape, converged state, four
    stream seeds): the chain is the oracle's at every scale; at 1 every update commits; with
    the standard-deviation term gone (0) the drift leaves the window in some updates, which are
    handed back (kPhiWindow / kPhiShort) -- and stays inside in others, which commit."""
    window_bits = 1 << PP.WINDOW | 1 << PP.SHORT
    left = committed = 0
    for seed in SCALE_SEEDS:
        ref = reference_chain(oracle, ("c5", seed), _c5_like(seed))
        preds = ref["preds"]
        assert all(p.all_fixed and not p.walker and not p.bis.any() for p in preds)
        assert_ambiguity_cap(preds)
        stats, per = replay(hd, ref, path, sd_scale=scale)
        assert stats["phi_fallback_status_mask"] & ~window_bits == 0, stats
        if scale == 1.0:
            assert stats["phi_device_calls"] == UPDATES and stats["phi_device_fallbacks"] == 0, stats
        left += bool(stats["phi_fallback_status_mask"] & window_bits)
        committed += stats["phi_device_calls"]
    if scale == 0.0:
        assert left >= 1 and committed >= 1, (left, committed)


# ------------------------------------------------------------------ 5 / 6. split-merge device chain
def _split_merge_case(hd, oracle, ds, c, cen, sig, t, seed, moves=2, sd_scale=None):
    """Split-merge moves (their restricted Gibbs samplers: t scans, each with update_phi of the two
    clusters) with HDPM_OPT_SM_CHAIN = 1 and update_phi on the device, against the oracle: labels,
    parameters, acceptance and RNG state after every move.  (The C ABI's restricted_gibbs takes
    any S and so never runs as a device chain; the move's own sampler does.)"""
    st = oracle.seed_state(seed)
    pc, ps, s0 = oracle.pool_generate(ds.attrisize, ds.v, ds.w, ds.n * 3, st)
    assert s0 == 0
    K = cen.shape[0]
    rng = st.copy()
    eng = make_engine(hd, ds)
    try:
        oracle.set_hig_logspace(True)
        eng.set_hig_logspace(True)
        eng.set_phi_device(True)
        eng.set_sm_chain(1)
        if sd_scale is not None:
            eng.set_phi_sd_scale(sd_scale)
        eng.set_state(c, cen, sig)
        eng.set_pool(pc, ps)
        eng.rng_state = st
        # (a sweep first: it launches the window of the device's random stream the chain reads)
        ost = oracle.OracleState(c, K, cen, sig)
        assert oracle.neal8_sweep(ds.codes, ds.attrisize, ds.gamma, ds.v, ds.w, ost, 3, pc, ps, rng, fast=1) == 0
        eng.neal8_sweep(3)
        ost = oracle.OracleState(c, K, cen, sig)
        eng.set_state(c, cen, sig)
        for k in range(moves):
            ost_st, oacc = oracle.split_and_merge(ds.codes, ds.attrisize, ds.gamma, ds.v, ds.w, ost, t, t, k, rng)
            assert ost_st == 0
            acc = eng.split_and_merge(t, t, k)
            c2, cen2, sig2 = eng.get_state()
            assert acc == oacc and cen2.shape[0] == ost.K, k
            assert np.array_equal(c2, ost.c_i), k
            assert np.array_equal(cen2, ost.centers[:ost.K]) and np.array_equal(sig2, ost.sigma[:ost.K]), k
            assert np.array_equal(eng.rng_state, rng), k
        stats = eng.stats()
    finally:
        oracle.set_hig_logspace(False)
        eng.close()
    print({k: v for k, v in stats.items() if k.startswith(("phi_", "sm_"))})
    return stats


def test_split_merge_chain_window_retry(hd, oracle):
    """The restricted Gibbs sampler as one device chain with the windows' standard-deviation
    term gone: an update whose drift leaves the window stops the chain (the host resumes,
    sm_chain_resumes) or is re-run with a wider window (phi_sm_window_retries)."""
    from split_and_merge_gibbs_sampling_amd.data import hamming_mixture
    ds = hamming_mixture(4000, 128, 2, 4, seed=6)
    cen, sig = converged_params(ds, ds.truth, 2)
    stats = _split_merge_case(hd, oracle, ds, ds.truth.astype(np.int32), cen, sig, 3, 45, sd_scale=0.0)
    assert stats["phi_sm_window_retries"] > 0 or stats["sm_chain_resumes"] > 0, stats


def test_split_merge_chain_many_levels(hd, oracle):
    """The device chain's one-cluster updates on mixed level counts, both sides of kPhiLdsLevels
    inside one fast-path group: two clusters of 600 points, t = 3.  (64 levels in place of the
    ladder's 255: the reference's norm_const2(w, v, m), the split-merge prior's constant, throws
    from 200 levels on -- GSL's 2F1 at z = (m - 1) / m -- so a move is undefined there.)"""
    ds = mixture(1200, [64 if m == 255 else m for m in mixed_levels(24)], 2, seed=105)
    cen, sig = converged_params(ds, ds.truth, 2)
    stats = _split_merge_case(hd, oracle, ds, ds.truth.astype(np.int32), cen, sig, 3, 46)
    assert stats["sm_chain_runs"] > 0 and stats["phi_sm_device_calls"] > 0, stats
