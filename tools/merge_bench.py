"""Merge gains, the merge path and the descent with merges (csrc/trace_merge.hip,
LabelTrace.merge_gains, LabelTrace.merge_path, refine(..., merges=)), on the GPU, beside the
only earlier route to the same numbers: hdpm_trace_losses over every merged candidate.

    python tools/merge_bench.py                   all runs, each a child under its own timeout
    python tools/merge_bench.py --run settled [--reps 7] [--gains-only]
    python tools/merge_bench.py --run unsettled
    python tools/merge_bench.py --run worst

Traces (synthetic, seeded): settled, N = 1,000,000, M = 64, every draw the truth of 20 classes
(what the recorded C5 chains of tools/refine_bench.py look like), the estimate the truth, Ka =
Kz = 20; unsettled, tools/trace_summary_bench.py's labels of the same N and M (every draw the
truth of 10 classes with a tenth of its labels redrawn from 12), the estimate draw 0; worst, the
largest tables the calls allow, N = 100,000, M = 256, Ka = Kz = 255, labels uniform at random.
One JSON line per run:

  merge_gains_vi_s, merge_gains_binder_s
        the medians (smallest, largest) of --reps timed C calls after one warm-up call, the host
        clock around calls that end synchronised with their results on the host, labels already
        int32 and dense.
  baseline_vi_s, baseline_binder_s
        the same clock around hdpm_trace_losses (its code is the parent commit's, untouched
        here) over the Ka (Ka - 1) / 2 merged candidates, built beforehand: the route to the
        same numbers without this change, one table pass per pair.  *_over_baseline is the
        ratio of the medians; "clear" says whether merge_gains' median lies below the
        baseline's by more than the two spreads (largest - smallest) together.  The gains are
        compared with the differences of the baseline's losses (max_abs_diff).
  merge_path_*    merge_path to k_min = 1, and (settled, unsettled) the baseline route repeated
        per level, greedy on its own losses, --path-reps timed repetitions: the C calls only.
  refine_*        refine(..., merges=) from the estimate with two classes merged (join) and with
        one class halved at random (halve): rounds, merges, trials, moved, converged, seconds,
        K, the loss of the estimate, of the start and of the end.
For the kernels' own times run one trace under rocprofv3 --kernel-trace --stats with --gains-only.
"""
import argparse
import ctypes as C
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

RUNS = {"settled": 420, "unsettled": 420, "worst": 300}       # seconds allowed per run


def stats(ts):
    ts = sorted(ts)
    return {"median": round(ts[len(ts) // 2], 6), "min": round(ts[0], 6), "max": round(ts[-1], 6)}


def timed(chk, call, reps):
    chk(call())                                      # warm-up: buffers allocated
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        chk(call())
        ts.append(time.perf_counter() - t0)
    return stats(ts)


def merged_candidates(np, cl, K):
    """the K (K - 1) / 2 partitions with classes a < b of cl (labels 0..K-1, all occupied)
    merged, labels dense, and the pairs"""
    pairs = [(a, b) for a in range(K) for b in range(a + 1, K)]
    out = np.empty((len(pairs), cl.size), np.int32)
    for q, (a, b) in enumerate(pairs):
        m = np.arange(K, dtype=np.int32)
        m[b] = a
        m[b + 1:] -= 1
        out[q] = m[cl]
    return out, pairs


def run(name, reps, path_reps, gains_only):
    import numpy as np
    from split_and_merge_gibbs_sampling_amd._lib import ptr
    from split_and_merge_gibbs_sampling_amd.posterior import LabelTrace, _relabel, refine
    from trace_summary_bench import labels
    rng = np.random.default_rng(1)
    if name == "settled":
        N, M = 1_000_000, 64
        est = rng.integers(0, 20, N).astype(np.int32)
        tr = np.ascontiguousarray(np.tile(est, (M, 1)))
    elif name == "unsettled":
        N, M = 1_000_000, 64
        _, tr = labels(N, M, 7)
        tr = np.ascontiguousarray(_relabel(tr, "iteration"))
        est = tr[0].copy()
    else:
        N, M = 100_000, 256
        tr = rng.integers(0, 255, (M, N)).astype(np.int32)
        tr[:, :255] = np.arange(255)
        tr = np.ascontiguousarray(_relabel(tr, "iteration"))
        est = rng.integers(0, 255, N).astype(np.int32)
        est[:255] = np.arange(255)
    Ka = int(est.max()) + 1
    t = LabelTrace(tr)
    L, h, chk = t.eng._L, t.eng._h, t.eng._check
    res = {"run": name, "N": N, "M": M, "Ka": Ka, "Kz": int(tr.max()) + 1, "reps": reps}
    gain = {k: np.zeros((Ka, Ka)) for k in (0, 1)}
    best, bg = np.zeros(2, np.int32), np.zeros(1)
    for code, key in ((0, "vi"), (1, "binder")):
        res[f"merge_gains_{key}_s"] = timed(
            chk, lambda: L.hdpm_trace_merge_gains(h, ptr(est), Ka, code, ptr(gain[code]), ptr(best), ptr(bg)), reps)
    if name != "worst":
        cands, pairs = merged_candidates(np, est, Ka)
        vi, q, p = np.zeros(len(pairs)), np.zeros(len(pairs), np.uint64), np.zeros(1, np.uint64)
        res["baseline_vi_s"] = timed(
            chk, lambda: L.hdpm_trace_losses(h, ptr(cands), len(pairs), None, ptr(vi), None, None), reps)
        res["baseline_binder_s"] = timed(
            chk, lambda: L.hdpm_trace_losses(h, ptr(cands), len(pairs), None, None, ptr(q), ptr(p)), reps)
        # what was timed is the same numbers: the gains against the differences of the losses
        own_vi = t.vi(est)[0]
        A0, P, Q0 = t.binder_terms(est)
        n = np.bincount(est, minlength=Ka).tolist()
        dv, db = 0.0, 0
        for k, (a, b) in enumerate(pairs):
            dv = max(dv, abs(gain[0][a, b] - (vi[k] - own_vi)))
            # A changes by n_a n_b; the integer M A + P - 2 Q by M n_a n_b - 2 (Q' - Q)
            db = max(db, abs(int(gain[1][a, b]) - (M * n[a] * n[b] - 2 * (int(q[k]) - Q0[0]))))
        res["max_abs_diff"] = {"vi": float(dv), "binder": int(db)}
        assert db == 0 and dv < 1e-9, (dv, db)
        for key in ("vi", "binder"):
            g, b0 = res[f"merge_gains_{key}_s"], res[f"baseline_{key}_s"]
            res[f"{key}_over_baseline"] = round(g["median"] / b0["median"], 5)
            res[f"{key}_clear"] = bool(b0["median"] - g["median"] > (g["max"] - g["min"]) + (b0["max"] - b0["min"]))
        del cands
    if gains_only:
        t.close()
        print(json.dumps(res), flush=True)
        return
    # the path to one class, and the baseline route level by level (greedy on its own losses)
    merge, sg, val = np.zeros((Ka, 2), np.int32), np.zeros(Ka), np.zeros(Ka + 1)
    steps = C.c_int32(0)
    for code, key in ((0, "vi"), (1, "binder")):
        res[f"merge_path_{key}_s"] = timed(
            chk, lambda: L.hdpm_trace_merge_path(h, ptr(est), Ka, code, 1, ptr(merge), ptr(sg), ptr(val),
                                                 C.byref(steps)),
            reps if name != "worst" else 5)
        res[f"merge_path_{key}_steps"] = int(steps.value)
        res[f"merge_path_{key}_value"] = [float(val[0]), float(val[steps.value])]
    if name != "worst":
        ts = []
        for _ in range(path_reps + 1):
            cur, K, dt = est.copy(), Ka, 0.0
            while K > 1:
                cands, pairs = merged_candidates(np, cur, K)
                vi = np.zeros(len(pairs))
                t0 = time.perf_counter()
                chk(L.hdpm_trace_losses(h, ptr(cands), len(pairs), None, ptr(vi), None, None))
                dt += time.perf_counter() - t0
                cur, K = cands[int(np.argmin(vi))].copy(), K - 1
            ts.append(dt)
        res["baseline_path_vi_s"] = stats(ts[1:])
        res["path_vi_over_baseline"] = round(res["merge_path_vi_s"]["median"] / res["baseline_path_vi_s"]["median"], 5)
        # the descent with merges
        join = est.copy()
        join[join == 1] = 0
        halve = est.copy()
        idx = np.flatnonzero(est == 2)
        halve[idx[rng.random(idx.size) < 0.5]] = Ka
        for loss in ("VI", "Binder"):
            own = (t.vi(est) if loss == "VI" else t.binder(est))[0]
            for tag, start in (("join", join), ("halve", halve)):
                t0 = time.perf_counter()
                r = refine(t, start, loss, max_rounds=20, merges=5)
                dt = time.perf_counter() - t0
                res[f"refine_{tag}_{loss.lower()}"] = {
                    "seconds": round(dt, 4), "rounds": r["rounds"], "merges": r["merges"], "trials": r["trials"],
                    "moved": r["moved"], "converged": r["converged"], "K": int(r["cl"].max()), "estimate": float(own),
                    "start": r["start"], "value": r["value"]}
    t.close()
    print(json.dumps(res), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--run", choices=sorted(RUNS))
    ap.add_argument("--reps", type=int, default=7, help="timed calls per quantity (at least 5)")
    ap.add_argument("--path-reps", type=int, default=3, help="timed repetitions of the baseline path")
    ap.add_argument("--gains-only", action="store_true", help="merge_gains and its baseline only (for a profiler run)")
    a = ap.parse_args()
    if a.reps < 5:
        ap.error("--reps must be at least 5")
    if a.run:
        run(a.run, a.reps, a.path_reps, a.gains_only)
        return 0
    # the parent never opens the GPU; a run that fails or overruns ends the tool
    for name, limit in RUNS.items():
        cmd = ["timeout", "-k", "10", str(limit), sys.executable, "-u", os.path.abspath(__file__), "--run", name,
               "--reps", str(a.reps), "--path-reps", str(a.path_reps)] + (["--gains-only"] if a.gains_only else [])
        st = subprocess.run(cmd).returncode
        if st != 0:
            print(json.dumps({"run": name, "failed": st}), flush=True)
            return st
    return 0


if __name__ == "__main__":
    sys.exit(main())
