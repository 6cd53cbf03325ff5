"""The end of a round enqueued ahead, as the host sees it (engine.cpp wait_resolved, DESIGN.md
section 7): the control block's sequence word (ResolveCtl::seq), published by the round's
resolver -- or by k_pipe_wait when it gates the round off -- behind the block and the summary,
instead of an event record behind the resolver.

Chains through hdpm_iterations (two calls per chain) against the CPU oracle's traced chain, as in
test_gpu_early_go.py: labels, K, centers, sigmas and the 625-word stream bit for bit after each
call, the per-iteration log-likelihood within RTOL.  The switch HDPM_RES_WORD is read once per
process, so the run with it off is a child process.
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
# (points, attributes, clusters, levels, data seed)
SHAPES = {"mixed": (3000, 32, 6, 3, 1), "quiet": (1000, 32, 4, 3, 5)}
TAIL_KEYS = ("resolved_by_word",)
PIPE_KEYS = ("pipe_enqueued", "pipe_runs", "pipe_early", "pipe_early_ran", "pipe_early_off", "pipe_recovered",
             "pipe_refused", "pipe_desync", "phi_device_calls", "rounds", "sweeps")


def dataset(shape):
    from split_and_merge_gibbs_sampling_amd.data import hamming_mixture
    n, d, k, levels, seed = SHAPES[shape]
    return hamming_mixture(n, d, k, levels, seed=seed)


_refs = {}


def reference(oracle, shape, seed, split, iters=ITERS):
    """The oracle's traced chain (computed once per case, read-only) and the stream where the
    first call ends (the same chain stopped there)."""
    key = (shape, seed, split, iters)
    if key not in _refs:
        ds = dataset(shape)
        c0 = ds.truth
        rng = oracle.seed_state(seed)
        st, ref = oracle.run_markov_chain(ds.codes, ds.attrisize, ds.gamma, ds.v, ds.w, rng=rng, fast=2, trace=True,
                                          iterations=iters, c_i=c0, **KW)
        assert st == 0
        ref["rng_end"] = rng
        if split:
            rng1 = oracle.seed_state(seed)
            st, _ = oracle.run_markov_chain(ds.codes, ds.attrisize, ds.gamma, ds.v, ds.w, rng=rng1, fast=2,
                                            iterations=split, c_i=c0, **KW)
            assert st == 0
            ref["rng_split"] = rng1
        for v in ref.values():
            for x in (v if isinstance(v, list) else [v]):
                x.setflags(write=False)
        _refs[key] = (ds, ref)
    return _refs[key]


def events(ref, iters=ITERS):
    """Iterations whose sweep follows a quiet one (only behind a quiet sweep is the next one
    enqueued ahead): those that move points (the device must decline the early go given for
    them) and those that are quiet too (it can take it)."""
    mv = ref["moves"]
    moving = [i for i in range(1, iters) if mv[i - 1] == 0 and mv[i] > 0]
    quiet = [i for i in range(1, iters) if mv[i - 1] == 0 and mv[i] == 0]
    return moving, quiet


def mixed_split(oracle, seed):
    """Where the mixed chain's two calls split: away from the events (the last iteration of a
    call launches no next sweep)."""
    _, probe = reference(oracle, "mixed", seed, 0)
    moving, quiet = events(probe)
    split = next(s for s in range(20, 30) if not ({s - 1, s, s + 1} & set(moving + quiet)))
    return split, moving, quiet


def run_chain(hd, ds, seed, split, iters=ITERS):
    """The chain on the device, two hdpm_iterations calls: the state after each and the
    log-likelihoods."""
    eng = hd.Engine(0)
    eng.set_data(ds.codes, ds.attrisize, ds.gamma, ds.v, ds.w)
    eng.set_seed(seed)
    eng.init_chain(eng.chain_params(iterations=iters, **KW), c_i=ds.truth)
    out = {}
    _, ll1 = eng.iterations(0, split)
    out["c1"], out["cen1"], out["sig1"] = eng.get_state()
    out["rng1"] = eng.rng_state.copy()
    _, ll2 = eng.iterations(split, iters - split)
    out["c2"], out["cen2"], out["sig2"] = eng.get_state()
    out["rng2"] = eng.rng_state.copy()
    out["ll"] = np.concatenate([ll1, ll2])
    stats = eng.stats()
    eng.close()
    return out, stats


_runs = {}


def default_run(hd, shape, seed, split):
    """The chain with the switch at its default (once per case, shared)."""
    key = (shape, seed, split)
    if key not in _runs:
        _runs[key] = run_chain(hd, dataset(shape), seed, split)
    return _runs[key]


def check_parity(out, ref, split, iters=ITERS):
    for tag, it, rng in (("1", split - 1, ref["rng_split"]), ("2", iters - 1, ref["rng_end"])):
        assert out["cen" + tag].shape[0] == ref["total_cls"][it], tag
        assert np.array_equal(out["c" + tag], ref["c_i"][it]), tag
        assert np.array_equal(out["cen" + tag], ref["centers"][it]), tag
        assert np.array_equal(out["sig" + tag], ref["sigmas"][it]), tag
        assert np.array_equal(out["rng" + tag], rng), tag
    np.testing.assert_allclose(out["ll"], ref["loglikelihood"], rtol=RTOL, atol=0)


@pytest.fixture(scope="module")
def hd():
    import split_and_merge_gibbs_sampling_amd as hd
    hd.build()
    return hd


def test_quiet_chain_every_piped_sweep_ends_by_its_word(hd, oracle):
    """No sweep moves a point: every sweep that ran from the pipeline went behind an early go and
    the host took its end from the sequence word."""
    seed, split = 21, 24
    ds, ref = reference(oracle, "quiet", seed, split)
    assert not ref["moves"].any() and set(ref["k_all"].tolist()) == {4}
    out, stats = default_run(hd, "quiet", seed, split)
    print({k: stats[k] for k in PIPE_KEYS + TAIL_KEYS})
    check_parity(out, ref, split)
    assert stats["resolved_by_word"] > 0, stats
    assert stats["pipe_early_ran"] == stats["pipe_runs"] > 0, stats
    assert stats["resolved_by_word"] == stats["pipe_runs"], stats
    assert stats["pipe_desync"] == 0, stats


@pytest.mark.parametrize("seed", [21, 23])
def test_mixed_chain_word_behind_declined_gos(hd, oracle, seed):
    """Sweeps that move points right after quiet ones: declined gos and rounds gated off behind
    them (k_pipe_wait publishes their word), between rounds the host waits for by the word.  The
    chain is the oracle's and the early-go counters are what its trace predicts."""
    split, moving, quiet = mixed_split(oracle, seed)
    ds, ref = reference(oracle, "mixed", seed, split)
    assert set(ref["k_all"].tolist()) == {6}
    away = lambda ev: [i for i in ev if 2 <= i < ITERS - 1 and abs(i - split) > 1]
    print("seed", seed, "split", split, "moving after quiet", moving, "quiet after quiet", quiet)
    assert len(away(moving)) >= 4 and len(away(quiet)) >= 4      # a condition of the test
    out, stats = default_run(hd, "mixed", seed, split)
    print({k: stats[k] for k in PIPE_KEYS + TAIL_KEYS})
    check_parity(out, ref, split)
    assert stats["phi_device_calls"] == 0, stats
    assert stats["pipe_early_ran"] >= 1, stats
    assert stats["pipe_early_off"] >= 1, stats
    assert stats["pipe_early"] == stats["pipe_early_ran"] + stats["pipe_early_off"], stats
    assert stats["pipe_early_off"] <= len(moving), stats
    assert stats["pipe_desync"] == 0, stats
    assert stats["resolved_by_word"] == stats["pipe_runs"] > 0, stats


def test_switch_off_same_chain(hd, oracle, tmp_path):
    """The mixed chain in a fresh process with HDPM_RES_WORD=0: the same outputs bit for bit, the
    same pipeline counters, and no round waited for by the word."""
    seed = 21
    split, _, _ = mixed_split(oracle, seed)
    out, stats = default_run(hd, "mixed", seed, split)
    res = tmp_path / "off.npz"
    env = dict(os.environ, HDPM_RES_WORD="0")
    subprocess.run([sys.executable, os.path.abspath(__file__), "mixed", str(seed), str(split), str(res)], env=env,
                   check=True, timeout=300)
    off = np.load(res)
    print({k: int(off[k]) for k in PIPE_KEYS + TAIL_KEYS})
    for k, v in out.items():
        assert np.array_equal(off[k], v), k
    for k in PIPE_KEYS:
        assert off[k] == stats[k], k
    assert stats["resolved_by_word"] > 0 and off["resolved_by_word"] == 0


def test_recording_rows(hd, oracle):
    """hdpm_iterations_record on the mixed input, thinning 3, update_phi on the host: every
    saved row equals the oracle's (as test_recording_rows_with_early_go), with the sequence
    word in use."""
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
    print({k: stats[k] for k in PIPE_KEYS + TAIL_KEYS + ("labels_downloaded", "labels_mirrored")})
    assert len(kk) == len(cens) == len(sigs) == iters
    assert np.array_equal(kk, ref["total_cls"]) and np.array_equal(cis, ref["c_i"])
    for q in range(iters):
        assert np.array_equal(cens[q], ref["centers"][q]), q
        assert np.array_equal(sigs[q], ref["sigmas"][q]), q
    saved = [it for it in range(total) if it >= thinning * burnin and it % thinning == 0]
    np.testing.assert_allclose(ll[saved], ref["loglikelihood"], rtol=RTOL, atol=0)
    assert stats["phi_device_calls"] == 0, stats
    assert stats["resolved_by_word"] > 0, stats
    assert stats["pipe_early"] == stats["pipe_early_ran"] + stats["pipe_early_off"], stats
    assert stats["pipe_desync"] == 0, stats
    assert np.array_equal(rng, ost)


if __name__ == "__main__":
    # the chain of test_switch_off_same_chain, run by it in a process of its own: its outputs
    # and counters into an .npz
    sys.path.insert(0, ROOT)
    import split_and_merge_gibbs_sampling_amd as _hd
    _shape, _seed, _split, _path = sys.argv[1], int(sys.argv[2]), int(sys.argv[3]), sys.argv[4]
    _out, _stats = run_chain(_hd, dataset(_shape), _seed, _split)
    np.savez(_path, **_out, **{k: _stats[k] for k in PIPE_KEYS + TAIL_KEYS})
