"""The device windows of the random stream, each stretch generated once (engine.cpp device_draws,
DESIGN.md sections 5 and 7): the next window starts `window_overlap` words before the current
one's end, it is initialised from a block of the current window's own outputs (untempered as
it is loaded; no state array is stored any more), and the host adopts its state the same way.

The stream is R's MT19937 continued from the seeded state, checked against the oracle's
generator word for word and, after every call, as the 625-word state.  The number of windows is
what `Schedule` below -- the same rules as device_draws, restated -- implies.
"""
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SCALE = 2.3283064365386963e-10          # MT_genrand's 2^-32 (no 0 or 1 fixup in these ranges)
KLEAD, CMAX, PREFETCH = 8, 1 << 16, 4096   # engine.cpp kLead, cmax, phi_prefetch at their initial values


def span(n, cmax=CMAX):
    return max(n + cmax, min(16 * (n + (1 << 18)), 1 << 27))


class Schedule:
    """device_draws' window rules on positions alone.  once=False: the earlier schedule (the
    next window starts where the current request ends)."""

    def __init__(self, once=True):
        self.once, self.pos, self.req_max, self.cmax = once, 0, 0, CMAX
        self.win = [None, None]         # (start, count)
        self.launched = self.fresh = 0
        self.starts = []                # (start of a window launched from another, that one's start)
        self.used = []                  # start of the window each request was served from

    def overlap(self, n):
        return min(span(n, self.cmax) // 2, max(n + self.cmax, self.req_max) + 2 * PREFETCH + 8 * 624)

    def draw(self, n):
        self.req_max = max(self.req_max, n)
        k = None
        for q in (0, 1):
            w = self.win[q]
            if w and w[0] <= self.pos and self.pos + n <= w[0] + w[1] and (k is None or w[0] < self.win[k][0]):
                k = q
        if k is None:
            if self.win[0] or self.win[1]:
                self.cmax = min(self.cmax * 2, 1 << 26)
            k = 0
            self.win[0] = (self.pos, span(n, self.cmax))
            self.launched += 1
            self.fresh += 1
        w, other = self.win[k], self.win[1 - k]
        self.used.append(w[0])
        target, wend = self.pos + n, w[0] + w[1]
        ahead = other is not None and other[0] > w[0]
        if not ahead and wend < target + KLEAD * (n + self.cmax):
            start = max(target, wend - self.overlap(n)) if self.once else target
            self.win[1 - k] = (start, span(n, self.cmax))
            self.launched += 1
            self.starts.append((start, w[0]))
            self.req_max = 0            # the longest request of a window's lifetime
        self.pos = target

    def run(self, counts):
        for n in counts:
            self.draw(int(n))
        return self


def mti_of(pos, mti0):
    """The index (1..624) in its block of stream position `pos`, the stream having started at
    index mti0 (624: at a block edge)."""
    k = (pos + mti0) % 624
    return 624 if k == 0 else k


@pytest.fixture(scope="module")
def hd():
    import split_and_merge_gibbs_sampling_amd as hd
    hd.build()
    return hd


def fill_and_check(hd, oracle, zoo, st, counts):
    """rng_fill_device for every count from stream state `st`: every word and the state after
    every call equal the oracle's generator continued from `st`.  Returns the engine's stats."""
    eng = hd.Engine(0)
    eng.set_data(zoo.codes, zoo.attrisize, zoo.gamma, zoo.v, zoo.w)
    eng.rng_state = st
    ref = st.copy()
    try:
        for q, n in enumerate(counts):
            got = eng.rng_fill_device(int(n))
            want = oracle.runif(ref, int(n))
            assert np.array_equal(got.astype(np.float64) * SCALE, want), (q, n)
            assert np.array_equal(eng.rng_state, ref), (q, n)
        return eng.stats()
    finally:
        eng.close()


def test_stream_identity_across_junctions(hd, oracle, zoo):
    """300 calls, 100,003 words with every third call a few thousand (the draws between sweeps):
    20.3M words, three junctions crossed.  One fresh window (the first), and as many windows as
    span and overlap imply: 4, where the earlier schedule launched 5 (these fills are small against
    the allowance between them, so it started a window 1.3M words before the end of one of 5.8M;
    at the bench's shape, a window 8 sweeps before the end of one of 16, it is 21 against 36)."""
    counts = [100_003 if q % 3 != 2 else 2_000 + 37 * (q % 50) for q in range(300)]
    new, old = Schedule(True).run(counts), Schedule(False).run(counts)
    crossed = len(set(new.used)) - 1
    print("words", sum(counts), "windows", new.launched, "earlier schedule", old.launched, "junctions crossed", crossed)
    assert sum(counts) > 20_000_000 and crossed >= 3 and new.fresh == 1          # conditions of the test
    assert new.launched < old.launched
    stats = fill_and_check(hd, oracle, zoo, oracle.seed_state(2024), counts)
    assert stats["rng_windows_fresh"] == 1, stats
    assert stats["rng_windows"] == new.launched, (stats["rng_windows"], new.launched, old.launched)


def edge_counts(mti0, first, want_mti):
    """A first fill of `first` words from index mti0 of a block, then equal fills whose size is
    chosen (by the schedule) so that the second window's start lands at index want_mti of its
    block; enough of them to cross into that window and into the third."""
    for extra in range(0, 3 * 624):
        n = 150_000 + extra
        counts = [first] + [n] * 100
        s = Schedule(True).run(counts)
        if len(s.starts) >= 2 and mti_of(s.starts[0][0], mti0) == want_mti and len(set(s.used)) >= 3 and s.fresh == 1:
            return counts, s
    raise AssertionError("no fill size puts the window start there")


@pytest.mark.parametrize("pre,first,want_mti", [(0, 624, 624), (0, 1, 1), (0, 623, 623), (100, 1, 624), (100, 524, 1),
                                                (311, 623, 312)])
def test_window_start_at_block_edges(hd, oracle, zoo, pre, first, want_mti):
    """The second window's start -- the block of the first window it is initialised from, and
    the block the host adopts when a request ends there -- at the last word of a block (index
    624), the first (1), the one before the last (623) and mid-block, after first fills of 624, 1
    and 623 words.  pre > 0: the stream is handed over mid-block (index `pre`), so the first
    window has a block 0 (the rest of the seeded array) and the first call's state is adopted
    from it: inside it (first = 1) and at its last word (first = 524).  A window *started* inside
    its source's block 0 cannot come about under this schedule: a window starts at least a
    request past its source's start."""
    st = oracle.seed_state(99 + first)
    assert st[0] == 624                      # seeded at a block edge
    oracle.runif(st, pre)
    mti0 = int(st[0])
    assert mti0 == (pre if pre else 624)
    counts, s = edge_counts(mti0, first, want_mti)
    print("mti0", mti0, "first", first, "fill", counts[1], "window starts", s.starts[:2], "windows", s.launched)
    stats = fill_and_check(hd, oracle, zoo, st, counts)
    assert stats["rng_windows_fresh"] == 1, stats
    assert stats["rng_windows"] == s.launched, (stats["rng_windows"], s.launched)


# ------------------------------------------------------------------ a chain through a junction
KW = dict(m=3, L=1, burnin=0, neal8=True, split_merge=False)
# (points, attributes, clusters, levels, sigma, data seed).  "quiet": tight clusters, no sweep of
# the oracle's chain moves a point, so every sweep is enqueued ahead (pre_enqueue's span must lie
# whole in one window, pipe_early_go's draws must be covered, the device's own go at the device
# update) and the pipelined sweeps cross the junctions.  "moving": points move in every sweep
# (46,000 moves, K between 4 and 7): sweeps in several rounds, updates of changing size, nothing
# enqueued ahead.
SHAPES = {"quiet": (20_000, 16, 4, 3, 0.2, 5), "moving": (20_000, 16, 4, 3, 0.5, 5)}
ITERS, SPLIT, SEED = 150, 70, 21
# (pipe_enqueued, pipe_enqueued - pipe_runs) of these chains on the commit before this change:
# the sweeps enqueued ahead, and those of them that did not run from the pipeline
# (quiet: 147 of 150, all behind an early go at the host update and behind the device's own go
# at the device update; each call's last iteration and the first enqueue none)
PARENT = {("quiet", "host"): (147, 0), ("quiet", "device"): (147, 0), ("moving", "host"): (0, 0),
          ("moving", "device"): (0, 0)}
FALLBACKS = ("fpg_aborts", "sm_wide_fallbacks", "pipe_recovered", "phi_device_fallbacks", "phi_fallback_status_mask",
             "pipe_desync")

_ref = {}


def dataset(shape):
    from split_and_merge_gibbs_sampling_amd.data import hamming_mixture
    n, d, k, levels, sigma, seed = SHAPES[shape]
    return hamming_mixture(n, d, k, levels, sigma=sigma, seed=seed)


def chain_reference(oracle, shape):
    """The oracle's traced chain (once per shape, read-only): the state after the first call's
    last iteration and after the last one, and the stream at the end."""
    if shape not in _ref:
        ds = dataset(shape)
        rng = oracle.seed_state(SEED)
        st, ref = oracle.run_markov_chain(ds.codes, ds.attrisize, ds.gamma, ds.v, ds.w, rng=rng, fast=2, trace=True,
                                          iterations=ITERS, c_i=ds.truth, **KW)
        assert st == 0
        out = {"rng2": rng, "moves": int(ref["moves"].sum())}
        assert (out["moves"] == 0) == (shape == "quiet")          # a condition of the test
        for tag, it in (("1", SPLIT - 1), ("2", ITERS - 1)):
            out["c" + tag], out["cen" + tag], out["sig" + tag] = ref["c_i"][it], ref["centers"][it], ref["sigmas"][it]
            out["K" + tag] = int(ref["total_cls"][it])
        for v in out.values():
            if isinstance(v, np.ndarray):
                v.setflags(write=False)
        _ref[shape] = (ds, out)
    return _ref[shape]


def run_chain(hd, ds, device):
    eng = hd.Engine(0)
    eng.set_data(ds.codes, ds.attrisize, ds.gamma, ds.v, ds.w)
    if device:
        eng.set_phi_device(True)
    eng.set_seed(SEED)
    eng.init_chain(eng.chain_params(iterations=ITERS, **KW), c_i=ds.truth)
    out = {}
    eng.iterations(0, SPLIT)
    out["c1"], out["cen1"], out["sig1"] = eng.get_state()
    eng.iterations(SPLIT, ITERS - SPLIT)
    out["c2"], out["cen2"], out["sig2"] = eng.get_state()
    out["rng2"] = eng.rng_state.copy()
    stats = eng.stats()
    eng.close()
    return out, stats


@pytest.mark.parametrize("where", ["host", "device"])
@pytest.mark.parametrize("shape", ["quiet", "moving"])
def test_chain_through_a_junction(hd, oracle, shape, where):
    """150 iterations from the truth in two calls, about 68 sweeps to a window: the chain draws
    from three windows.  Labels, K, centers and sigmas equal the oracle's after each call and the
    625-word stream at the end; nothing fell back, as many sweeps were enqueued ahead as on the
    commit before (the quiet chain: nearly all of them) and no more of them failed to run."""
    ds, ref = chain_reference(oracle, shape)
    out, stats = run_chain(hd, ds, where == "device")
    short = stats["pipe_enqueued"] - stats["pipe_runs"]
    print(shape, where, "oracle moves", ref["moves"],
          {k: stats[k] for k in ("rng_windows", "rng_windows_fresh", "pipe_enqueued", "pipe_runs", "phi_device_calls",
                                 "sweeps") + FALLBACKS}, "short", short)
    for tag in ("1", "2"):
        assert out["cen" + tag].shape[0] == ref["K" + tag], tag
        assert np.array_equal(out["c" + tag], ref["c" + tag]), tag
        assert np.array_equal(out["cen" + tag], ref["cen" + tag]), tag
        assert np.array_equal(out["sig" + tag], ref["sig" + tag]), tag
    assert np.array_equal(out["rng2"], ref["rng2"])
    assert stats["rng_windows"] >= 3, stats          # two junctions were crossed
    assert stats["rng_windows_fresh"] <= 1, stats
    for k in FALLBACKS:
        assert stats[k] == 0, (k, stats[k])
    assert (stats["phi_device_calls"] > 0) == (where == "device"), stats
    enq, parent_short = PARENT[(shape, where)]
    assert stats["pipe_enqueued"] >= enq, (stats["pipe_enqueued"], enq)
    assert short <= parent_short, (short, parent_short)
    if shape == "quiet":
        assert stats["pipe_enqueued"] >= ITERS - 10, stats["pipe_enqueued"]
        # behind the host's early go (host update) or the device's own go (device update)
        assert stats["pipe_early" if where == "host" else "pipe_auto"] == stats["pipe_runs"], stats


if __name__ == "__main__":
    # the chains of test_chain_through_a_junction with the library of the package at ROOT: their
    # pipeline counters, one line each
    sys.path.insert(0, ROOT)
    import split_and_merge_gibbs_sampling_amd as _hd
    for _shape in SHAPES:
        for _where in ("host", "device"):
            _, _st = run_chain(_hd, dataset(_shape), _where == "device")
            print(_shape, _where, "enqueued", _st["pipe_enqueued"], "runs", _st["pipe_runs"], "short",
                  _st["pipe_enqueued"] - _st["pipe_runs"], "windows", _st["rng_windows"], "fresh",
                  _st["rng_windows_fresh"], "device_calls", _st["phi_device_calls"], "early", _st["pipe_early"],
                  "auto", _st["pipe_auto"],
                  {k: _st[k] for k in FALLBACKS}, flush=True)
