"""The early conditional go of the host update's pipeline (engine.cpp pipe_early_go, DESIGN.md
section 7): the host gives its go for the sweep enqueued ahead at the join of the speculated
update_phi, before the running sweep has ended, and k_pipe_wait makes the last part of the
decision from that sweep's control block -- it goes behind a quiet sweep (complete in its one
launch, no move) and gates the enqueued kernels off behind any other.

Chains through hdpm_iterations (two calls per chain) against the CPU oracle's traced chain
(run_markov_chain, la:6-174): labels, K, centers, sigmas and the 625-word stream bit for bit
after each call, the per-iteration log-likelihood within RTOL.  K * d is far below the automatic
placement's 4096 items, so update_phi runs as the host job.  The oracle's trace also gives the
sweeps that moved points, and so how many early goes the device can take and must decline.
"""
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

RTOL = 1e-10
ITERS = 48
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KW = dict(m=3, L=1, burnin=0, neal8=True, split_merge=False)
SHAPES = {"mixed": (3000, 32, 6, 3, 1), "quiet": (1000, 32, 4, 3, 5)}


def dataset(shape):
    from split_and_merge_gibbs_sampling_amd.data import hamming_mixture
    n, d, k, levels, seed = SHAPES[shape]
    return hamming_mixture(n, d, k, levels, seed=seed)


_refs = {}


def reference(oracle, shape, seed, split):
    """The oracle's traced chain (computed once per case, read-only) and the stream where the
    first call ends (the same chain stopped there)."""
    key = (shape, seed, split)
    if key not in _refs:
        ds = dataset(shape)
        rng = oracle.seed_state(seed)
        st, ref = oracle.run_markov_chain(ds.codes, ds.attrisize, ds.gamma, ds.v, ds.w, rng=rng, fast=2, trace=True,
                                          iterations=ITERS, c_i=ds.truth, **KW)
        assert st == 0
        ref["rng_end"] = rng
        if split:
            rng1 = oracle.seed_state(seed)
            st, _ = oracle.run_markov_chain(ds.codes, ds.attrisize, ds.gamma, ds.v, ds.w, rng=rng1, fast=2,
                                            iterations=split, c_i=ds.truth, **KW)
            assert st == 0
            ref["rng_split"] = rng1
        for v in ref.values():
            for x in (v if isinstance(v, list) else [v]):
                x.setflags(write=False)
        _refs[key] = (ds, ref)
    return _refs[key]


def events(ref):
    """Iterations whose sweep follows a quiet one (only behind a quiet sweep is the next one
    enqueued ahead): those that move points (the device must decline the early go given for
    them) and those that are quiet too (it can take it)."""
    mv = ref["moves"]
    moving = [i for i in range(1, ITERS) if mv[i - 1] == 0 and mv[i] > 0]
    quiet = [i for i in range(1, ITERS) if mv[i - 1] == 0 and mv[i] == 0]
    return moving, quiet


def run_chain(hd, ds, seed, split):
    """The chain on the device, two hdpm_iterations calls: the state after each and the
    log-likelihoods."""
    eng = hd.Engine(0)
    eng.set_data(ds.codes, ds.attrisize, ds.gamma, ds.v, ds.w)
    eng.set_seed(seed)
    eng.init_chain(eng.chain_params(iterations=ITERS, **KW), c_i=ds.truth)
    out = {}
    _, ll1 = eng.iterations(0, split)
    out["c1"], out["cen1"], out["sig1"] = eng.get_state()
    out["rng1"] = eng.rng_state.copy()
    _, ll2 = eng.iterations(split, ITERS - split)
    out["c2"], out["cen2"], out["sig2"] = eng.get_state()
    out["rng2"] = eng.rng_state.copy()
    out["ll"] = np.concatenate([ll1, ll2])
    stats = eng.stats()
    eng.close()
    return out, stats


def check_parity(out, ref, split):
    for tag, it, rng in (("1", split - 1, ref["rng_split"]), ("2", ITERS - 1, ref["rng_end"])):
        assert out["cen" + tag].shape[0] == ref["total_cls"][it], tag
        assert np.array_equal(out["c" + tag], ref["c_i"][it]), tag
        assert np.array_equal(out["cen" + tag], ref["centers"][it]), tag
        assert np.array_equal(out["sig" + tag], ref["sigmas"][it]), tag
        assert np.array_equal(out["rng" + tag], rng), tag
    np.testing.assert_allclose(out["ll"], ref["loglikelihood"], rtol=RTOL, atol=0)


PIPE_KEYS = ("pipe_enqueued", "pipe_runs", "pipe_early", "pipe_early_ran", "pipe_early_off", "pipe_recovered",
             "pipe_refused", "pipe_desync", "phi_device_calls")


@pytest.fixture(scope="module")
def hd():
    import split_and_merge_gibbs_sampling_amd as hd
    hd.build()
    return hd


@pytest.mark.parametrize("seed", [21, 23])
def test_mixed_chain_device_declines_and_takes_early_goes(hd, oracle, seed, tmp_path):
    """Sweeps that move points right after a quiet one, and quiet ones after quiet ones: the
    device declines the first kind's early go and takes the second's, and the chain is the
    oracle's.  With HDPM_PIPE_EARLY=0 (a fresh process: the switch is read once) the same chain
    gives the same outputs with no early go."""
    _, probe = reference(oracle, "mixed", seed, 0)
    moving, quiet = events(probe)
    # the last iteration of a call launches no next sweep: the calls split away from the events
    split = next(s for s in range(20, 30) if not ({s - 1, s, s + 1} & set(moving + quiet)))
    ds, ref = reference(oracle, "mixed", seed, split)
    assert set(ref["k_all"].tolist()) == {6}
    away = lambda ev: [i for i in ev if 2 <= i < ITERS - 1 and abs(i - split) > 1]
    print("seed", seed, "split", split, "moving after quiet", moving, "quiet after quiet", quiet)
    assert len(away(moving)) >= 4 and len(away(quiet)) >= 4      # a condition of the test
    out, stats = run_chain(hd, ds, seed, split)
    print({k: stats[k] for k in PIPE_KEYS})
    check_parity(out, ref, split)
    assert stats["phi_device_calls"] == 0, stats
    assert stats["pipe_early_ran"] >= 1, stats
    assert stats["pipe_early_off"] >= 1, stats
    assert stats["pipe_early"] == stats["pipe_early_ran"] + stats["pipe_early_off"], stats
    assert stats["pipe_early_off"] <= len(moving), stats
    assert stats["pipe_desync"] == 0, stats
    # the switch off, in a child process
    res = tmp_path / "off.npz"
    env = dict(os.environ, HDPM_PIPE_EARLY="0")
    subprocess.run([sys.executable, os.path.abspath(__file__), "mixed", str(seed), str(split), str(res)], env=env,
                   check=True, timeout=300)
    off = np.load(res)
    for k, v in out.items():
        assert np.array_equal(off[k], v), k
    assert off["pipe_early"] == 0 and off["pipe_early_ran"] == 0 and off["pipe_early_off"] == 0
    assert off["pipe_desync"] == 0


@pytest.mark.parametrize("seed", [21, 23])
def test_quiet_chain_every_enqueued_sweep_goes_early(hd, oracle, seed):
    """No sweep of the chain moves a point: every sweep that ran from the pipeline ran behind an
    early go, none was declined, none gated off."""
    split = 24
    ds, ref = reference(oracle, "quiet", seed, split)
    assert not ref["moves"].any() and set(ref["k_all"].tolist()) == {4}
    out, stats = run_chain(hd, ds, seed, split)
    print({k: stats[k] for k in PIPE_KEYS})
    check_parity(out, ref, split)
    assert stats["phi_device_calls"] == 0, stats
    assert stats["pipe_early_ran"] == stats["pipe_runs"] > 0, stats
    assert stats["pipe_early_off"] == 0, stats
    assert stats["pipe_recovered"] == 0, stats
    assert stats["pipe_desync"] == 0, stats


def test_recording_rows_with_early_go(hd, oracle):
    """hdpm_iterations_record on the mixed input, thinning 3, update_phi on the host: every
    saved row equals the oracle's.  Some recorded iterations download their labels (the host
    mirror is invalid after an unrecorded sweep that moved points): no early go is given behind
    those, so the download stays ahead of every sweep that writes the labels."""
    ds = dataset("mixed")
    iters, burnin, thinning, seed = 15, 1, 3, 21
    kw = dict(KW, burnin=burnin, thinning=thinning)
    ost = oracle.seed_state(seed)
    st, ref = oracle.run_markov_chain(ds.codes, ds.attrisize, ds.gamma, ds.v, ds.w, rng=ost, fast=2, trace=True,
                                      iterations=iters, c_i=ds.truth, **kw)
    assert st == 0
    total = (iters + burnin) * thinning
    eng = hd.Engine(0)
    eng.set_data(ds.codes, ds.attrisize, ds.gamma, ds.v, ds.w)
    eng.set_seed(seed)
    eng.init_chain(eng.chain_params(iterations=iters, **kw), c_i=ds.truth)
    split = 26
    _, ll, kk, cis, cens, sigs = eng.iterations_record(0, split)
    _, ll2, kk2, cis2, cens2, sigs2 = eng.iterations_record(split, total - split)
    kk, cis, cens, sigs, ll = np.concatenate([kk, kk2]), np.concatenate([cis, cis2]), cens + cens2, sigs + sigs2, \
        np.concatenate([ll, ll2])
    stats = eng.stats()
    rng = eng.rng_state.copy()
    eng.close()
    print({k: stats[k] for k in PIPE_KEYS + ("labels_downloaded", "labels_mirrored")})
    assert len(kk) == len(cens) == len(sigs) == iters
    assert np.array_equal(kk, ref["total_cls"]) and np.array_equal(cis, ref["c_i"])
    for q in range(iters):
        assert np.array_equal(cens[q], ref["centers"][q]), q
        assert np.array_equal(sigs[q], ref["sigmas"][q]), q
    saved = [it for it in range(total) if it >= thinning * burnin and it % thinning == 0]
    np.testing.assert_allclose(ll[saved], ref["loglikelihood"], rtol=RTOL, atol=0)
    assert stats["phi_device_calls"] == 0, stats
    assert stats["labels_downloaded"] > 0, stats
    assert stats["pipe_early"] == stats["pipe_early_ran"] + stats["pipe_early_off"], stats
    assert stats["pipe_desync"] == 0, stats
    assert np.array_equal(rng, ost)


if __name__ == "__main__":
    # the chain of test_mixed_chain_..., run by it in a process of its own: its outputs and
    # pipeline counters into an .npz
    sys.path.insert(0, ROOT)
    import split_and_merge_gibbs_sampling_amd as _hd
    _shape, _seed, _split, _path = sys.argv[1], int(sys.argv[2]), int(sys.argv[3]), sys.argv[4]
    _out, _stats = run_chain(_hd, dataset(_shape), _seed, _split)
    np.savez(_path, **_out, **{k: _stats[k] for k in PIPE_KEYS})
