"""The HDPM_* environment switches (csrc/switches.hpp) against the CPU oracle: "the chain is the
same with any of them".

The switches select paths and override launch geometry for A/B runs, and they are the only way to
reach, at test sizes, kernel code that otherwise runs at full size only: k_prepass_wide's
double-buffered loop over several chunks per workgroup (HDPM_WIDE_WGS), the fast update_phi's group
sizes 16 / 32 / 64 with a ragged last group and its other workgroup sizes (HDPM_PHI2_*), the stream
generator's jump-ahead and the reuse of its tables (HDPM_MT_WORKGROUPS).

Nearly every switch is read once per process, so each group of settings (CHILDREN) runs its
workloads in a fresh child process -- this file as a script -- which writes its outputs, counters
and the launch readout (hdpm_debug_launches) into an .npz.  The parent computes each workload's
oracle reference once (cached, read-only) and compares labels, K, centers, sigmas and the 625-word
stream bit for bit, log-likelihoods within RTOL; it then asserts from the counters and the readout
that the path a setting asks for ran (an override out of range, or a group size that does not
fit, falls back silently), and that the default path ran in the default child.

A child that ends by a signal, an abort or its time limit sets a latch: every later case fails at
once and starts nothing more on the device.  A child that reports a mismatch does not.
"""
import json
import os
import re
import subprocess
import sys
import time

import numpy as np
import pytest

gpu = pytest.mark.gpu

RTOL = 1e-10
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
U32 = 2.3283064365386963e-10
CHILD_TIMEOUT = 300

# ------------------------------------------------------------------ workloads
# (points, attributes, clusters, levels, data seed)
PHI_SHAPES = {"d33": (3000, 33, 2, 4, 51), "d65": (3000, 65, 6, (2, 6), 52), "d128": (4000, 128, 6, 4, 53),
              "d260": (2500, 260, 5, 6, 54)}
# random L = 20 starts: no pool heads (d = 32, binary planes of 2 words); pool heads (d = 128); rows of
# more than 8 sixteen-byte chunks, which the level-table exact rows do not take, so dense launches go
# to k_exact_rows_mass (kernels.hip launch_exact_rows: nq <= kLanesMaxNq = 8 takes k_exact_rows_lv)
CHAIN_SHAPES = {"small": (6000, 32, 6, 3, 61), "heads": (6000, 128, 8, 4, 62), "mass": (6000, 144, 6, 4, 63)}
WIDE_LAYOUTS = {"ws5_wb2": (300, 37), "ws20_wb2": (1250, 38)}      # attributes, data seed (test_wide_prepass_sweeps)
WIDE_POOL = 3000     # latent pool entries of the wide workloads (any size serves pick_entry; 3 n of them cost the
#                      oracle 14 s at d = 1250)
QUIET = (1000, 32, 4, 3, 5)       # test_gpu_tail.py's quiet shape
SM_SHAPE = (1200, 64, 2, 3, 44)   # test_split_merge_chain_wide_scan_and_give_up's data, shrunk: ~600 per cluster,
#                                   so a move's scan has 3 (split) or 5 (merge) chunks of 256 (k_sm_scan_wide: >= 2)
RNG_PRE = (0, 311, 624)
STAT_KEYS = ("sweeps", "restarts", "phi_device_calls", "phi_device_fallbacks", "phi_fast_calls", "phi_fast_handbacks",
             "dense_launches", "fpg_launches", "exact_mass_launches", "exact_lanes_launches", "sm_wide_scans",
             "sm_wide_fallbacks", "phi_chain_launched", "pipe_auto", "pipe_desync", "pipe_enqueued", "rng_windows",
             "sm_moves")

COUNTED = ("wide_launches", "mt_multi_windows", "dense_direct_launches", "lbound_launches",
           "unsettled_margin_launches")

PHI_ALL = [("phi", s, "conv") for s in PHI_SHAPES] + [("phi", "d65", "unsettled")]
WIDE_1 = [("wide", lay, 1) for lay in WIDE_LAYOUTS]
WIDE_2 = [("wide", lay, 2) for lay in WIDE_LAYOUTS]
CHAINS = [("chain", s) for s in CHAIN_SHAPES]

# name -> (environment, workloads).  Settings that steer different kernels share a child.
# (The wide-prepass children also set HDPM_DENSE_LIST=0: at these sizes -- n >= kDenseMinPoints, and
# at d = 300 with K = 5 the mass exact rows fit -- the default engine takes every launch of the
# ws5_wb2 workload as dense and skips the prepass altogether, which the default child shows.)
CHILDREN = {
    "default": ({}, WIDE_1 + [("sm",)]),
    "default_phi": ({}, PHI_ALL),
    "default_chains": ({}, CHAINS + [("pipe",), ("host",)]),
    "gs8": ({"HDPM_PHI2_GS": "8", "HDPM_PHI2_TREE_THREADS": "1024", "HDPM_PHI2_VALUES_WAVES": "16",
             "HDPM_PHI2_GROUP_THREADS": "128"}, PHI_ALL),
    "gs16": ({"HDPM_PHI2_GS": "16", "HDPM_PHI2_TREE_THREADS": "64", "HDPM_PHI2_VALUES_WAVES": "1",
              "HDPM_PHI2_GROUP_THREADS": "320"}, PHI_ALL),
    # (256 tree threads and 4 value waves: the narrow shapes' own defaults, here for d = 260 too)
    "gs32": ({"HDPM_PHI2_GS": "32", "HDPM_PHI2_TREE_THREADS": "256", "HDPM_PHI2_VALUES_WAVES": "4"}, PHI_ALL),
    "gs64": ({"HDPM_PHI2_GS": "64", "HDPM_PHI2_TREE_THREADS": "64", "HDPM_PHI2_VALUES_WAVES": "16",
              "HDPM_SM_WIDE": "0"}, PHI_ALL + [("sm",)]),
    "wide_wgs1": ({"HDPM_WIDE_WGS": "1", "HDPM_WIDE_CLAIM": "0", "HDPM_DENSE_LIST": "0"}, WIDE_1),
    "wide_wgs1_claim": ({"HDPM_WIDE_WGS": "1", "HDPM_WIDE_CLAIM": "1", "HDPM_DENSE_LIST": "0"}, WIDE_1),
    "wide_wgs2": ({"HDPM_WIDE_WGS": "2", "HDPM_DENSE_LIST": "0"}, WIDE_2),
    "mt2": ({"HDPM_MT_WORKGROUPS": "2", "HDPM_HOST_THREADS": "1"}, [("rng", 2), ("rngchain",), ("host",)]),
    "mt3": ({"HDPM_MT_WORKGROUPS": "3", "HDPM_HOST_THREADS": "3"}, [("rng", 3), ("host",)]),
    "mt7": ({"HDPM_MT_WORKGROUPS": "7", "HDPM_PIN_THREADS": "0"}, [("rng", 7), ("host",)]),
    "mt64": ({"HDPM_MT_WORKGROUPS": "64", "HDPM_SPIN_US": "0"}, [("rng", 64), ("host",)]),
    "dense_list0": ({"HDPM_DENSE_LIST": "0", "HDPM_PHI_CHAIN": "0", "HDPM_STREAM_PRIO": "0"},
                    CHAINS + [("pipe",), ("host",)]),
    "dense_list0_wide": ({"HDPM_DENSE_LIST": "0"}, WIDE_1),
    "dense_direct0": ({"HDPM_DENSE_DIRECT": "0", "HDPM_PIPE_AUTO": "0", "HDPM_STREAM_PRIO": "2"},
                      CHAINS + [("pipe",), ("host",)]),
    "fpg_min1": ({"HDPM_FPG_MIN": "1"}, CHAINS),
    "fpg_min_huge": ({"HDPM_FPG_MIN": "100000000"}, CHAINS),
    "unsettled_unif0": ({"HDPM_FP_UNSETTLED_UNIF": "0"}, CHAINS),
    "lat_bound0": ({"HDPM_LAT_BOUND": "0"}, CHAINS),
    "lv_spec0": ({"HDPM_LV_SPEC": "0"}, CHAINS),
    "mass_static1": ({"HDPM_MASS_STATIC": "1"}, CHAINS),
    "sync_each1": ({"HDPM_SYNC_EACH": "1"}, [("host",)]),
}

# switches whose test is in another file (the completeness check opens it)
COVERED_ELSEWHERE = {"RES_WORD": "test_gpu_tail.py", "PIPE_EARLY": "test_gpu_early_go.py"}
# switches without a parity test, and why
EXEMPT = {
    "SEGV_TRACE": "a fault handler's output; installs nothing the chain runs through",
    "WARM_SYNC": "diagnosis of the warm-up launches, which compute nothing the chain reads",
    "WARM_MASK": "skips warm-up launches, which compute nothing the chain reads",
    "PHI_TRACE": "stderr text only (set by test_gpu_configs.py around a C3 run)",
    "PHI_TIMING": "stderr text only",
    "PHI": "the start value of HDPM_OPT_PHI_DEVICE, which the suite sets through set_phi_device",
    "SM_CHAIN": "the start value of HDPM_OPT_SM_CHAIN, which test_split_merge_device_chain sets",
}


def covered_here():
    return {k[len("HDPM_"):] for env, _ in CHILDREN.values() for k in env}


def wide_points(cus, mult):
    """3 or 4 chunks of 16 points per workgroup at one workgroup per CU, the last chunk partial."""
    return mult * (16 * (3 * cus + cus // 3) + 5)


def resolve(spec, cus):
    """A workload of CHILDREN with its run-time sizes: what the child gets and the reference's key."""
    return ("wide", spec[1], wide_points(cus, spec[2])) if spec[0] == "wide" else tuple(spec)


def key_of(spec):
    return ":".join(str(x) for x in spec)


# ------------------------------------------------------------------ the child's side
def synth(n, d, k, levels, seed):
    from split_and_merge_gibbs_sampling_amd.data import hamming_mixture
    return hamming_mixture(n, d, k, tuple(levels) if isinstance(levels, (list, tuple)) else levels, seed=seed)


def make_engine(hd, ds):
    e = hd.Engine(0)
    e.set_data(ds.codes, ds.attrisize, ds.gamma, ds.v, ds.w)
    return e


def snap(eng, out, tag):
    c, cen, sig = eng.get_state()
    out[tag + "_c"], out[tag + "_cen"], out[tag + "_sig"], out[tag + "_rng"] = c, cen, sig, eng.rng_state.copy()


def finish(eng, out):
    info = {"stats": {k: int(v) for k, v in eng.stats().items() if k in STAT_KEYS}, "launches": eng.debug_launches()}
    eng.close()
    return out, info


def wide_data(layout, n):
    d, seed = WIDE_LAYOUTS[layout]
    return synth(n, d, 5, 4, seed)


def run_wide(hd, layout, n):
    """test_wide_prepass_sweeps' chain (init_chain from the truth, three sweeps with update_phi) on n
    points; the pool regenerated at WIDE_POOL entries from the stream after init_chain.  From the
    truth no point moves, and a wrong margin that only lists a point costs nothing: a fourth sweep
    from the same parameters with every 7th label moved to another cluster, where a point the
    prepass wrongly certifies stays wrong."""
    ds = wide_data(layout, n)
    eng = make_engine(hd, ds)
    eng.set_seed(35)
    eng.init_chain(eng.chain_params(m=3, iterations=1, L=0, burnin=0, neal8=True, split_merge=False), c_i=ds.truth)
    out = {}
    snap(eng, out, "init")
    eng.generate_pool(WIDE_POOL)
    for s in range(3):
        eng.neal8_sweep(3)
        snap(eng, out, f"sweep{s}")
        eng.update_phi()
        snap(eng, out, f"phi{s}")
    c, cen, sig = eng.get_state()
    eng.set_state(perturbed(c, cen.shape[0]), cen, sig)
    eng.neal8_sweep(3)
    snap(eng, out, "sweep3")
    eng.update_phi()
    snap(eng, out, "phi3")
    return finish(eng, out)


def perturbed(c, K):
    """Every 7th label moved to another cluster, each of the K - 1 others in turn (the data come
    sorted by cluster: one fixed shift would never meet the rows a wrong chunk holds)."""
    c = c.copy()
    c[::7] = (c[::7] + 1 + np.arange(len(c[::7])) % (K - 1)) % K
    return c


def phi_case(shape, start):
    import test_gpu_parity as TP
    n, d, K, levels, seed = PHI_SHAPES[shape]
    ds = synth(n, d, K, levels, seed)
    cen, sig = TP.converged_params(ds, ds.truth, K) if start == "conv" else TP.random_params(ds, K, 13)
    return ds, cen, sig


def run_phi(hd, shape, start):
    """sweep_case of test_gpu_parity.py with the device update: 5 sweeps, update_phi after each."""
    ds, cen, sig = phi_case(shape, start)
    eng = make_engine(hd, ds)
    eng.set_phi_device(True)
    eng.set_seed(44)
    eng.set_state(ds.truth, cen, sig)
    eng.generate_pool(3 * ds.n)
    out = {}
    for s in range(5):
        eng.neal8_sweep(3)
        snap(eng, out, f"sweep{s}")
        eng.update_phi()
        snap(eng, out, f"phi{s}")
    return finish(eng, out)


def run_rng(hd, G):
    """Windows around the jump-ahead threshold t = G * 624 * 8 and the tables' reuse limit, a smaller
    window under larger tables, one below the threshold; the readout after each."""
    from split_and_merge_gibbs_sampling_amd.data import load_zoo
    zoo = load_zoo()
    t = G * 624 * 8
    out, seqs = {}, {}
    eng = None
    for pre in RNG_PRE:
        eng = make_engine(hd, zoo)
        eng.set_seed(2718)
        seq = []

        def fill(tag, count):
            out[f"p{pre}_{tag}"] = eng.rng_fill_device(count)
            out[f"p{pre}_{tag}_rng"] = eng.rng_state.copy()
            seq.append([tag, int(count), eng.debug_launches()])
            return seq[-1][2]

        if pre:
            fill("pre", pre)
        fill("a", t - 1)
        fill("b", t)
        L = fill("c", t + 1)
        limit = 624 * L["mt_G"] * L["mt_bpg"] if L["mt_G"] > 0 and L["mt_bpg"] > 0 else t + 2
        fill("d", limit)
        fill("e", limit + 1)
        fill("f", 4 * t + 37)
        fill("g", t)
        fill("h", t // 2)
        # a new stream: the windows start over, small again, under the tables built for the large one
        # (their trailing workgroups have no block)
        eng.set_seed(2719)
        fill("i", t)
        fill("j", t + 1)
        seqs[str(pre)] = seq
        if pre != RNG_PRE[-1]:
            eng.close()
    out, info = finish(eng, out)
    info["seq"] = seqs
    return out, info


def save_chain(res, rng, out):
    out["c_i"], out["total_cls"], out["ll"], out["accepted"] = res["c_i"], res["total_cls"], res["loglikelihood"], \
        res["accepted"]
    out["cen"], out["sig"] = np.concatenate(res["centers"]), np.concatenate(res["sigmas"])
    out["rng"] = rng


ZOO_KW = dict(m=3, iterations=6, L=1, burnin=0, neal8=True, split_merge=False)


def run_rngchain(hd):
    """A short Neal-8 chain on Zoo: its pool and sweeps draw from the device windows."""
    from split_and_merge_gibbs_sampling_amd.data import load_zoo
    zoo = load_zoo()
    eng = make_engine(hd, zoo)
    eng.set_seed(1)
    before = eng.debug_launches()["mt_multi_windows"]
    res = eng.run_markov_chain(c_i=np.zeros(zoo.n, np.int32), keep_params=True, **ZOO_KW)
    out = {}
    save_chain(res, eng.rng_state.copy(), out)
    out, info = finish(eng, out)
    info["multi_windows_before"] = before
    return out, info


CHAIN_KW = dict(m=3, iterations=6, L=20, burnin=0, neal8=True, split_merge=False)


def run_chain(hd, shape):
    """run_markov_chain from a random L = 20 start: dense launches, the device-wide resolver."""
    n, d, K, levels, seed = CHAIN_SHAPES[shape]
    ds = synth(n, d, K, levels, seed)
    eng = make_engine(hd, ds)
    eng.set_seed(seed)
    res = eng.run_markov_chain(keep_params=True, **CHAIN_KW)
    out = {}
    save_chain(res, eng.rng_state.copy(), out)
    return finish(eng, out)


PIPE_KW = dict(m=3, L=1, burnin=0, neal8=True, split_merge=False)
PIPE_ITERS, PIPE_SPLIT, PIPE_SEED = 24, 12, 21


def run_pipe(hd):
    """test_gpu_tail.py's quiet chain with the device update: 24 iterations in two calls."""
    ds = synth(*QUIET)
    eng = make_engine(hd, ds)
    eng.set_phi_device(True)
    eng.set_seed(PIPE_SEED)
    eng.init_chain(eng.chain_params(iterations=PIPE_ITERS, **PIPE_KW), c_i=ds.truth)
    out = {}
    _, ll1 = eng.iterations(0, PIPE_SPLIT)
    snap(eng, out, "call1")
    _, ll2 = eng.iterations(PIPE_SPLIT, PIPE_ITERS - PIPE_SPLIT)
    snap(eng, out, "call2")
    out["ll"] = np.concatenate([ll1, ll2])
    return finish(eng, out)


SM_T, SM_MOVES = 3, 4


def run_sm(hd):
    """Four split-merge moves from the truth (the start of test_gpu_configs.py's sm_steps)."""
    ds = synth(*SM_SHAPE)
    eng = make_engine(hd, ds)
    eng.set_seed(8)
    eng.set_hig_logspace(True)
    eng.init_chain(eng.chain_params(m=3, iterations=1, L=0, burnin=0, neal8=True, split_merge=True, t=SM_T, r=SM_T),
                   c_i=ds.truth)
    out = {}
    snap(eng, out, "init")
    acc = []
    for k in range(SM_MOVES):
        acc.append(eng.split_and_merge(SM_T, SM_T, k))
        snap(eng, out, f"move{k}")
    out["acc"] = np.array(acc, np.int32)
    return finish(eng, out)


def run_host(hd):
    """test_run_markov_chain_zoo_split_merge_golden's chain."""
    from split_and_merge_gibbs_sampling_amd.data import load_zoo
    zoo = load_zoo()
    eng = make_engine(hd, zoo)
    eng.set_seed(7)
    res = eng.run_markov_chain(m=3, iterations=30, L=1, c_i=np.zeros(zoo.n, np.int32), burnin=0, t=10, r=10, neal8=True,
                               split_merge=True)
    out = {"c_i": res["c_i"], "accepted": res["accepted"], "ll": res["loglikelihood"]}
    return finish(eng, out)


RUNNERS = {"wide": run_wide, "phi": run_phi, "rng": run_rng, "rngchain": run_rngchain, "chain": run_chain,
           "pipe": run_pipe, "sm": run_sm, "host": run_host}


def child_main(path, specs):
    sys.path.insert(0, ROOT)
    import split_and_merge_gibbs_sampling_amd as hd
    arrays, infos, before = {}, {}, {}
    for spec in specs:
        t0 = time.perf_counter()
        out, info = RUNNERS[spec[0]](hd, *spec[1:])
        info["seconds"] = time.perf_counter() - t0
        # the readout counts launches per process: this workload's share
        info["counted"] = {k: info["launches"][k] - before.get(k, 0) for k in COUNTED}
        before = info["launches"]
        key = key_of(spec)
        infos[key] = info
        for k, v in out.items():
            arrays[f"{key}|{k}"] = v
    np.savez(path, __info__=np.array(json.dumps(infos)), **arrays)


# ------------------------------------------------------------------ the parent's side
_state = {"latched": None, "cus": None}
_children = {}
_refs = {}


CUS_PROBE = "import torch; print(torch.cuda.get_device_properties(0).multi_processor_count)"


def device_cus():
    """The device's CU count, asked of torch in a process of its own: in this one the engine's HIP
    runtime may already be up (earlier test files), and torch's own then finds no device."""
    if _state["cus"] is None:
        if _state["latched"]:
            pytest.fail(f"not started: an earlier child ({_state['latched']}) faulted, aborted or hung")
        try:
            p = subprocess.run([sys.executable, "-c", CUS_PROBE], stdout=subprocess.PIPE, timeout=CHILD_TIMEOUT)
        except subprocess.TimeoutExpired:
            _state["latched"] = "CU count probe: time limit"
            pytest.fail("the CU count probe ran into its time limit")
        if p.returncode < 0 or p.returncode in (134, 139, 124, 137):
            _state["latched"] = f"CU count probe: exit status {p.returncode}"
            pytest.fail(f"the CU count probe ended with status {p.returncode}")
        assert p.returncode == 0, "the CU count probe failed"
        _state["cus"] = int(p.stdout.decode().split()[-1])
        assert _state["cus"] > 0
    return _state["cus"]


class Result:
    def __init__(self, path, seconds):
        z = np.load(path)
        self.info = json.loads(str(z["__info__"]))
        self.arrays = {}
        for k in z.files:
            if k != "__info__":
                w, name = k.split("|")
                self.arrays.setdefault(w, {})[name] = z[k]
        z.close()
        os.remove(path)          # (the stream windows make it ~100 MB)
        self.seconds = seconds


def run_child(name, tmp_path_factory):
    """The child of CHILDREN[name], once per session.  Sets the latch when the child ends by a
    signal, an abort or a time limit; fails at once when the latch is set."""
    if name in _children:
        if isinstance(_children[name], str):     # it failed: no second process for the cases that depend on it
            pytest.fail(_children[name])
        return _children[name]
    if _state["latched"]:
        pytest.fail(f"not started: an earlier child ({_state['latched']}) faulted, aborted or hung")
    env_set, specs = CHILDREN[name]
    specs = [resolve(s, device_cus()) for s in specs]
    path = str(tmp_path_factory.mktemp(name) / "out.npz")
    env = {k: v for k, v in os.environ.items() if not (k.startswith("HDPM_") and k[5:] in covered_here())}
    env.update(env_set)
    quiet = "HDPM_SYNC_EACH" in env_set         # (a line per kernel launch on stderr)
    t0 = time.perf_counter()
    try:
        p = subprocess.run([sys.executable, os.path.abspath(__file__), path, json.dumps(specs)], env=env,
                           timeout=CHILD_TIMEOUT, stderr=subprocess.PIPE if quiet else None)
    except subprocess.TimeoutExpired:
        _state["latched"] = f"{name}: time limit"
        pytest.fail(f"child {name} ran into its time limit")
    rc = p.returncode
    if rc < 0 or rc in (134, 139, 124, 137):
        _state["latched"] = f"{name}: exit status {rc}"
        pytest.fail(f"child {name} ended with status {rc}")
    if rc != 0:
        _children[name] = f"child {name} failed (status {rc})"
        pytest.fail(_children[name])
    res = Result(path, time.perf_counter() - t0)
    res.stderr = p.stderr.decode(errors="replace") if quiet else ""
    res.specs = specs
    print(f"child {name}: {res.seconds:.2f} s " +
          " ".join(f"{k}={v['seconds']:.2f}" for k, v in res.info.items()))
    _children[name] = res
    return res


def frozen(x):
    for v in (x.values() if isinstance(x, dict) else x):
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
        elif isinstance(v, (dict, list, tuple)):
            frozen(v)
    return x


def same_start(ref, got, tag="init"):
    """The reference was computed from the first child's start state: every child starts there."""
    for k in ("_c", "_cen", "_sig", "_rng"):
        assert np.array_equal(ref[tag + k], got[tag + k]), f"start state differs ({k})"


def same_step(got, tag, ost, rng):
    assert got[tag + "_cen"].shape[0] == ost.K, tag
    assert np.array_equal(got[tag + "_c"], ost.c_i), tag
    assert np.array_equal(got[tag + "_cen"], ost.centers[:ost.K]), tag
    assert np.array_equal(got[tag + "_sig"], ost.sigma[:ost.K]), tag
    assert np.array_equal(got[tag + "_rng"], rng), tag


def steps_of(ost, rng):
    return {"c": ost.c_i.copy(), "K": ost.K, "cen": ost.centers[:ost.K].copy(), "sig": ost.sigma[:ost.K].copy(),
            "rng": rng.copy()}


def same_as(got, tag, st):
    assert got[tag + "_cen"].shape[0] == st["K"], tag
    assert np.array_equal(got[tag + "_c"], st["c"]), tag
    assert np.array_equal(got[tag + "_cen"], st["cen"]), tag
    assert np.array_equal(got[tag + "_sig"], st["sig"]), tag
    assert np.array_equal(got[tag + "_rng"], st["rng"]), tag


def check_sweeps(oracle, key, got, ds, ost, rng, pc, ps, sweeps, init=None, then_perturbed=False):
    """Sweeps with update_phi against the oracle; the oracle's steps cached under `key`."""
    if key not in _refs:
        steps = {}
        for s in range(sweeps + (1 if then_perturbed else 0)):
            if s == sweeps:
                ost = oracle.OracleState(perturbed(ost.c_i, ost.K), ost.K, ost.centers[:ost.K].copy(),
                                         ost.sigma[:ost.K].copy())
            assert oracle.neal8_sweep(ds.codes, ds.attrisize, ds.gamma, ds.v, ds.w, ost, 3, pc, ps, rng, fast=2) == 0
            steps[f"sweep{s}"] = steps_of(ost, rng)
            assert oracle.update_phi(ds.codes, ds.attrisize, ds.v, ds.w, ost, rng) == 0
            steps[f"phi{s}"] = steps_of(ost, rng)
        _refs[key] = frozen({"steps": steps, "init": init})
    ref = _refs[key]
    if ref["init"] is not None:
        same_start(ref["init"], got)
    for tag, st in ref["steps"].items():
        same_as(got, tag, st)


def check_wide(oracle, spec, got):
    key = key_of(spec)
    ds = ost = rng = pc = ps = init = None
    if key not in _refs:
        ds = wide_data(spec[1], spec[2])
        init = {k: v.copy() for k, v in got.items() if k.startswith("init_")}
        ost = oracle.OracleState(init["init_c"], init["init_cen"].shape[0], init["init_cen"], init["init_sig"])
        rng = init["init_rng"].copy()
        pc, ps, s0 = oracle.pool_generate(ds.attrisize, ds.v, ds.w, WIDE_POOL, rng)
        assert s0 == 0
    check_sweeps(oracle, key, got, ds, ost, rng, pc, ps, 3, init, then_perturbed=True)
    ref = _refs[key]["steps"]
    moved = int((ref["sweep3"]["c"] != perturbed(ref["phi2"]["c"], ref["phi2"]["K"])).sum())
    print(key, "points moved by the sweep from the perturbed labels:", moved)
    assert moved > len(ref["sweep3"]["c"]) // 10       # a condition of the test


def check_phi(oracle, spec, got):
    key = key_of(spec)
    ds = ost = rng = pc = ps = None
    if key not in _refs:
        ds, cen, sig = phi_case(spec[1], spec[2])
        ost = oracle.OracleState(ds.truth, cen.shape[0], cen, sig)
        rng = oracle.seed_state(44)
        pc, ps, s0 = oracle.pool_generate(ds.attrisize, ds.v, ds.w, 3 * ds.n, rng)
        assert s0 == 0
    check_sweeps(oracle, key, got, ds, ost, rng, pc, ps, 5)


def check_rng(oracle, spec, got, info):
    """Every window and the stream state after it against the oracle's runif."""
    for pre in RNG_PRE:
        st = oracle.seed_state(2718)
        for tag, count, _ in info["seq"][str(pre)]:
            if tag == "i":
                st = oracle.seed_state(2719)
            ref = oracle.runif(st, count)
            g = got[f"p{pre}_{tag}"]
            assert g.shape == ref.shape and np.array_equal(g.astype(np.float64) * U32, ref), (pre, tag, count)
            assert np.array_equal(got[f"p{pre}_{tag}_rng"], st), (pre, tag, count)


def check_chain_arrays(got, ref, rng):
    assert np.array_equal(got["total_cls"], ref["total_cls"])
    assert np.array_equal(got["c_i"], ref["c_i"])
    assert np.array_equal(got["cen"], np.concatenate(ref["centers"]))
    assert np.array_equal(got["sig"], np.concatenate(ref["sigmas"]))
    assert np.array_equal(got["rng"], rng)
    np.testing.assert_allclose(got["ll"], ref["loglikelihood"], rtol=RTOL, atol=0)


def check_rngchain(oracle, spec, got):
    key = key_of(spec)
    if key not in _refs:
        from split_and_merge_gibbs_sampling_amd.data import load_zoo
        zoo = load_zoo()
        rng = oracle.seed_state(1)
        st, ref = oracle.run_markov_chain(zoo.codes, zoo.attrisize, zoo.gamma, zoo.v, zoo.w, rng=rng, fast=1, trace=True,
                                          c_i=np.zeros(zoo.n, np.int32), **ZOO_KW)
        assert st == 0
        _refs[key] = frozen((ref, rng))
    check_chain_arrays(got, *_refs[key])


def check_chain(oracle, spec, got):
    key = key_of(spec)
    if key not in _refs:
        n, d, K, levels, seed = CHAIN_SHAPES[spec[1]]
        ds = synth(n, d, K, levels, seed)
        rng = oracle.seed_state(seed)
        st, ref = oracle.run_markov_chain(ds.codes, ds.attrisize, ds.gamma, ds.v, ds.w, rng=rng, fast=2, trace=True,
                                          **CHAIN_KW)
        assert st == 0
        _refs[key] = frozen((ref, rng))
    check_chain_arrays(got, *_refs[key])


def check_pipe(oracle, spec, got):
    key = key_of(spec)
    if key not in _refs:
        ds = synth(*QUIET)
        rng = oracle.seed_state(PIPE_SEED)
        st, ref = oracle.run_markov_chain(ds.codes, ds.attrisize, ds.gamma, ds.v, ds.w, rng=rng, fast=2, trace=True,
                                          iterations=PIPE_ITERS, c_i=ds.truth, **PIPE_KW)
        assert st == 0
        rng1 = oracle.seed_state(PIPE_SEED)
        st, _ = oracle.run_markov_chain(ds.codes, ds.attrisize, ds.gamma, ds.v, ds.w, rng=rng1, fast=2,
                                        iterations=PIPE_SPLIT, c_i=ds.truth, **PIPE_KW)
        assert st == 0
        _refs[key] = frozen((ref, rng1, rng))
    ref, rng1, rng2 = _refs[key]
    for tag, it, rng in (("call1", PIPE_SPLIT - 1, rng1), ("call2", PIPE_ITERS - 1, rng2)):
        assert got[tag + "_cen"].shape[0] == ref["total_cls"][it], tag
        assert np.array_equal(got[tag + "_c"], ref["c_i"][it]), tag
        assert np.array_equal(got[tag + "_cen"], ref["centers"][it]), tag
        assert np.array_equal(got[tag + "_sig"], ref["sigmas"][it]), tag
        assert np.array_equal(got[tag + "_rng"], rng), tag
    np.testing.assert_allclose(got["ll"], ref["loglikelihood"], rtol=RTOL, atol=0)


def check_sm(oracle, spec, got):
    key = key_of(spec)
    if key not in _refs:
        ds = synth(*SM_SHAPE)
        init = {k: v.copy() for k, v in got.items() if k.startswith("init_")}
        ost = oracle.OracleState(init["init_c"], init["init_cen"].shape[0], init["init_cen"], init["init_sig"], cap=4096)
        rng = init["init_rng"].copy()
        steps, acc = {}, []
        try:
            oracle.set_hig_logspace(True)
            for k in range(SM_MOVES):
                st, a = oracle.split_and_merge(ds.codes, ds.attrisize, ds.gamma, ds.v, ds.w, ost, SM_T, SM_T, k, rng,
                                               fast=2)
                assert st == 0
                acc.append(a)
                steps[f"move{k}"] = steps_of(ost, rng)
        finally:
            oracle.set_hig_logspace(False)
        _refs[key] = frozen({"init": init, "steps": steps, "acc": np.array(acc, np.int32)})
    ref = _refs[key]
    same_start(ref["init"], got)
    assert np.array_equal(got["acc"], ref["acc"])
    for tag, st in ref["steps"].items():
        same_as(got, tag, st)


def check_host(oracle, spec, got):
    g = np.load(os.path.join(GOLDEN, "zoo_sm_seed7.npz"))
    assert np.array_equal(got["c_i"], g["c_i"])
    assert np.array_equal(got["accepted"], g["accepted"])
    np.testing.assert_allclose(got["ll"], g["loglikelihood"], rtol=RTOL, atol=0)


def check_parity(oracle, res):
    for spec in res.specs:
        key = key_of(spec)
        got, info = res.arrays[key], res.info[key]
        try:
            if spec[0] == "rng":
                check_rng(oracle, spec, got, info)
            else:
                {"wide": check_wide, "phi": check_phi, "rngchain": check_rngchain, "chain": check_chain,
                 "pipe": check_pipe, "sm": check_sm, "host": check_host}[spec[0]](oracle, spec, got)
        except AssertionError as e:
            raise AssertionError(f"workload {key}: {e}") from e


# ------------------------------------------------------------------ evidence that the path ran
def default_gs(T, d):
    """engine.cpp phi_plan without HDPM_PHI2_GS: the largest group size that gives >= 160
    workgroups, else the smallest (every size fits the LDS at these shapes' windows)."""
    for gs in (64, 32, 16, 8):
        if T * -(-d // gs) >= 160:
            return gs
    return 8


def evidence_phi(env, spec, info):
    n, d, K, _, _ = PHI_SHAPES[spec[1]]
    L, S = info["launches"], info["stats"]
    forced = int(env.get("HDPM_PHI2_GS", 0))
    shown = {k: L[k] for k in L if k.startswith("phi_")}
    shown.update({k: S[k] for k in ("phi_device_calls", "phi_device_fallbacks", "phi_fast_calls", "phi_fast_handbacks")})
    print(key_of(spec), shown)
    if forced and L["phi_gs_refused"] == 1:
        # the size does not fit the LDS: no fast path at all (phi_plan), the general kernels ran
        assert S["phi_fast_calls"] == 0 and S["phi_fast_handbacks"] == 0 and S["phi_device_calls"] >= 1, shown
        return False
    assert L["phi_gs_refused"] == (0 if forced else -1), shown
    gs = forced or default_gs(K, d)
    narrow = d <= 256
    assert L["phi_gs"] == gs and L["phi_G"] == -(-d // gs), shown
    assert L["phi_group_threads"] == int(env.get("HDPM_PHI2_GROUP_THREADS", 512)), shown
    assert L["phi_tree_threads"] == int(env.get("HDPM_PHI2_TREE_THREADS", 256 if narrow else 1024)), shown
    if "HDPM_PHI2_VALUES_WAVES" in env:
        assert L["phi_values_waves"] == int(env["HDPM_PHI2_VALUES_WAVES"]), shown
    else:
        assert 1 <= L["phi_values_waves"] <= (4 if narrow else 16), shown
    if spec[2] == "conv":
        assert S["phi_fast_calls"] >= 5 and S["phi_fast_handbacks"] == 0 and S["phi_device_calls"] == 5, shown
    else:
        assert S["phi_fast_calls"] + S["phi_fast_handbacks"] >= 1, shown
        assert S["phi_device_calls"] + S["phi_device_fallbacks"] == 5, shown
    return True


def evidence_wide(env, spec, info):
    L = info["launches"]
    shown = {k: L[k] for k in L if k.startswith("wide_")}
    print(key_of(spec), shown, "CUs", device_cus())
    shown.update(info["counted"])
    if env.get("HDPM_DENSE_LIST") == "0":
        assert info["counted"]["wide_launches"] >= 1, shown
    else:
        # a dense launch skips the prepass (engine.cpp launch_round, dense_direct)
        assert info["counted"]["wide_launches"] >= 1 or info["counted"]["dense_direct_launches"] >= 3, shown
        if not info["counted"]["wide_launches"]:
            return
    assert L["wide_claim"] == (1 if int(env.get("HDPM_WIDE_CLAIM", 0)) else 0), shown
    assert 1 <= L["wide_chunks"] <= -(-spec[2] // 16), shown
    if "HDPM_WIDE_WGS" in env:
        assert L["wide_grid"] == device_cus() * int(env["HDPM_WIDE_WGS"]), shown
        assert L["wide_chunks"] > 2 * L["wide_grid"], shown       # the steady state of the chunk loop ran
    else:
        assert 1 <= L["wide_grid"] <= L["wide_chunks"], shown


def evidence_rng(env, spec, info):
    G = int(env["HDPM_MT_WORKGROUPS"])
    assert spec[1] == G
    t = G * 624 * 8
    assert info["stats"]["rng_windows"] > 0
    for pre, seq in info["seq"].items():
        by = {}
        for tag, count, L in seq:
            by[tag] = L
            print("G", G, "pre", pre, tag, count, {k: L[k] for k in L if k.startswith("mt_")})
            if L["mt_G"] > 0:
                assert L["mt_G"] == G, (pre, tag)
            # a window of at least t draws runs on G workgroups, from tables that reach its end
            assert L["mt_multi"] == (1 if L["mt_window"] >= t else 0), (pre, tag, L)
            if L["mt_multi"]:
                assert L["mt_window"] <= 624 * G * L["mt_bpg"], (pre, tag, L)
        assert by["c"]["mt_G"] == G and by["c"]["mt_bpg"] >= 8, (pre, by["c"])
        assert by["e"]["mt_bpg"] > by["c"]["mt_bpg"], pre              # past the reuse limit: new tables
        assert by["f"]["mt_bpg"] >= 4 * 8, pre
        assert by["g"]["mt_bpg"] == by["f"]["mt_bpg"] == by["h"]["mt_bpg"], pre    # smaller windows reuse them
        assert by["h"]["mt_multi_windows"] > seq[0][2]["mt_multi_windows"] - seq[0][2]["mt_multi"], (pre, by["h"])
        # the reseeded stream's window: new, multi-workgroup, so short that the tables' last workgroup has no block
        assert by["i"]["mt_multi_windows"] > by["h"]["mt_multi_windows"] and by["i"]["mt_multi"] == 1, (pre, by["i"])
        assert by["i"]["mt_bpg"] == by["h"]["mt_bpg"] and by["i"]["mt_window"] <= 624 * by["i"]["mt_bpg"] * (G - 1), (pre, by["i"])


def evidence_chain(env, spec, info, dflt):
    L, S = dict(info["launches"], **info["counted"]), info["stats"]
    shown = {k: S[k] for k in ("dense_launches", "fpg_launches", "exact_mass_launches", "exact_lanes_launches",
                               "restarts", "sweeps")}
    shown.update({k: L[k] for k in ("dense_direct", "lbound", "spec_lv", "mass_static", "dense_direct_launches",
                                    "lbound_launches", "unsettled_margin_launches")})
    print(key_of(spec), shown)
    dL, dS = dict(dflt["launches"], **dflt["counted"]), dflt["stats"]
    if env.get("HDPM_DENSE_LIST") == "0":
        assert S["dense_launches"] == 0 and L["dense_direct_launches"] == 0, shown
    if env.get("HDPM_DENSE_DIRECT") == "0":
        assert S["dense_launches"] > 0 and L["dense_direct_launches"] == 0 and L["dense_direct"] == 0, shown
    if env.get("HDPM_FPG_MIN") == "1":
        assert S["fpg_launches"] >= dS["fpg_launches"] and S["fpg_launches"] > 0, shown
        if spec[1] == "heads":
            # this chain restarts behind new clusters: launches over a sweep's short rest, which expect
            # fewer than 1024 listed points and take k_resolve_fpg only under the lower threshold
            # (seen on an MI355X: 17 against the default's 12; small 13 against 11; mass 7 and 7)
            assert dS["restarts"] > 0 and S["fpg_launches"] > dS["fpg_launches"], (shown, dS)
    if env.get("HDPM_FPG_MIN") == "100000000":
        assert S["fpg_launches"] == 0, shown
    if env.get("HDPM_FP_UNSETTLED_UNIF") == "0":
        # (by default an unsettled launch keeps the uniform's certification wherever the fixed-point
        # resolvers are eligible: no launch lists by margins alone for that reason)
        assert L["unsettled_margin_launches"] >= dL["unsettled_margin_launches"], shown
        if spec[1] == "heads":
            # the fixed-point resolvers are eligible at every launch of this chain and it restarts (unsettled
            # launches): none lists by margins alone by default, some do with the switch off
            # (seen on an MI355X: 8 against 0; mass 1 against 0; small 2 and 2, where a launch is not eligible)
            assert dS["restarts"] > 0 and dL["unsettled_margin_launches"] == 0, dL
            assert L["unsettled_margin_launches"] > 0, shown
    if env.get("HDPM_LAT_BOUND") == "0":
        assert L["lbound_launches"] == 0 and L["lbound"] == 0, shown
    assert L["spec_lv"] == (0 if env.get("HDPM_LV_SPEC") == "0" else 1), shown
    if S["exact_mass_launches"]:
        assert L["mass_static"] == (1 if int(env.get("HDPM_MASS_STATIC", 0)) else 0), shown
    if env.get("HDPM_MASS_STATIC") == "1":
        if spec[1] == "mass":
            assert S["exact_mass_launches"] > 0 and L["mass_static"] == 1, shown


def evidence_default_chains(res):
    """The default child reaches every path the off-settings take away, on at least one shape."""
    infos = [res.info[key_of(s)] for s in res.specs if s[0] == "chain"]
    tot = lambda k: sum(i["stats"][k] for i in infos)         # noqa: E731
    assert tot("dense_launches") > 0 and tot("fpg_launches") > 0 and tot("exact_mass_launches") > 0
    mass = res.info[key_of(("chain", "mass"))]
    assert mass["stats"]["exact_mass_launches"] > 0 and mass["launches"]["mass_static"] == 0
    cnt = lambda k: sum(i["counted"][k] for i in infos)       # noqa: E731
    assert cnt("dense_direct_launches") > 0 and cnt("lbound_launches") > 0, [i["counted"] for i in infos]
    assert res.info[key_of(("chain", "heads"))]["counted"]["lbound_launches"] > 0       # the shape with pool heads


def evidence_pipe(env, spec, info):
    S = info["stats"]
    shown = {k: S[k] for k in ("phi_chain_launched", "pipe_auto", "pipe_desync", "pipe_enqueued", "phi_device_calls")}
    print(key_of(spec), shown)
    assert S["pipe_desync"] == 0, shown
    if env.get("HDPM_PHI_CHAIN") == "0":
        assert S["phi_chain_launched"] == 0, shown
    else:
        assert S["phi_chain_launched"] > 0, shown
    if env.get("HDPM_PIPE_AUTO") == "0":
        assert S["pipe_auto"] == 0, shown
    elif env.get("HDPM_PHI_CHAIN") != "0":         # (the device's own go needs the chained update)
        assert S["pipe_auto"] > 0, shown


def evidence_sm(env, spec, info):
    S = info["stats"]
    shown = {k: S[k] for k in ("sm_wide_scans", "sm_wide_fallbacks", "sm_moves")}
    print(key_of(spec), shown)
    if env.get("HDPM_SM_WIDE") == "0":
        assert S["sm_wide_scans"] == 0, shown
    else:
        assert S["sm_wide_scans"] > 0 and S["sm_wide_fallbacks"] == 0, shown


def check_evidence(name, res, dflt):
    env = CHILDREN[name][0]
    forced_ran = set()
    for spec in res.specs:
        info = res.info[key_of(spec)]
        if spec[0] == "phi":
            if evidence_phi(env, spec, info) and spec[2] == "conv":
                forced_ran.add(spec[1])
        elif spec[0] == "wide":
            evidence_wide(env, spec, info)
        elif spec[0] == "rng":
            evidence_rng(env, spec, info)
        elif spec[0] == "rngchain":
            L = info["launches"]
            print(key_of(spec), {k: L[k] for k in L if k.startswith("mt_")}, "before", info["multi_windows_before"])
            assert L["mt_multi_windows"] > info["multi_windows_before"]      # the chain drew from jumped windows
        elif spec[0] == "chain":
            evidence_chain(env, spec, info, dflt.info[key_of(spec)])
        elif spec[0] == "pipe":
            evidence_pipe(env, spec, info)
        elif spec[0] == "sm":
            evidence_sm(env, spec, info)
    if "HDPM_PHI2_GS" in env:
        # a forced size may be refused where it does not fit, but not on the small ragged shapes (a last
        # group of 1 item): there the child must have run the fast path at that size, not the general kernels
        assert {"d33", "d65"} <= forced_ran, (name, sorted(forced_ran))
    if name == "default_chains":
        evidence_default_chains(res)
    if name == "sync_each1":
        assert res.stderr.count("[sync] ") > 10, res.stderr[:400]      # every launch synchronised and named


@pytest.fixture(scope="module")
def built():
    import split_and_merge_gibbs_sampling_amd as hd
    hd.build()
    return hd


@gpu
@pytest.mark.parametrize("name", list(CHILDREN))
def test_switches_same_chain(built, oracle, tmp_path_factory, name):
    """One child per group of settings: every workload's chain is the oracle's, and the counters
    and the launch readout show that the paths the settings ask for ran."""
    t0 = time.perf_counter()
    dflt = run_child("default_chains", tmp_path_factory) if ("chain", "small") in CHILDREN[name][1] else None
    res = run_child(name, tmp_path_factory)
    print("settings", CHILDREN[name][0])
    check_parity(oracle, res)
    check_evidence(name, res, dflt)
    print(f"case {name}: {time.perf_counter() - t0:.2f} s (child {res.seconds:.2f} s)")


# ------------------------------------------------------------------ completeness (no GPU)
def declared_switches():
    src = open(os.path.join(ROOT, "split_and_merge_gibbs_sampling_amd", "csrc", "switches.hpp")).read()
    names = re.findall(r"^HDPM_SWITCH\((\w+),", src, flags=re.M)
    assert len(names) == len(set(names)) and len(names) >= 31
    return names


def test_every_switch_is_tested_or_exempt():
    """Every HDPM_SWITCH of csrc/switches.hpp is set by a child of this file, named by another
    test file that mentions it, or exempt with a reason; no table names a switch that is gone."""
    names = declared_switches()
    here = covered_here()
    for group in (here, set(COVERED_ELSEWHERE), set(EXEMPT)):
        assert group <= set(names), sorted(group - set(names))
    assert not (here & set(COVERED_ELSEWHERE)) and not (here & set(EXEMPT)) and not (set(COVERED_ELSEWHERE) & set(EXEMPT))
    for n in names:
        assert n in here or n in COVERED_ELSEWHERE or n in EXEMPT, f"HDPM_{n} has no test and no exemption"
    for n, f in COVERED_ELSEWHERE.items():
        assert re.search(rf"\bHDPM_{n}\b", open(os.path.join(ROOT, "tests", f)).read()), (n, f)
    for n, why in EXEMPT.items():
        assert len(why) > 10 and "\n" not in why, n
    # every workload a child names exists
    for name, (env, specs) in CHILDREN.items():
        assert specs and all(s[0] in RUNNERS for s in specs), name


if __name__ == "__main__":
    child_main(sys.argv[1], [tuple(s) for s in json.loads(sys.argv[2])])
