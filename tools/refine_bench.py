"""Single-point moves and the descent built on them (csrc/trace_refine.hip, LabelTrace.move_gains,
refine), on the GPU, beside the only earlier route to Binder's gains, hdpm_trace_affinity.

    python tools/refine_bench.py                  both traces, each a child under its own timeout
    python tools/refine_bench.py --run c5 [--reps 7] [--no-refine]
    python tools/refine_bench.py --run c4

Traces: the recorded chains of tools/trace_summary_bench.py --uncertainty (c5: N = 1,000,000,
M = 64; c4: N = 70,000, M = 24), the estimate minvi_avg's cut.  One JSON line per trace:

  affinity_s, move_gains_vi_s, move_gains_binder_s
        the medians (smallest, largest) of --reps timed C calls after one warm-up call, the
        host clock around calls that end synchronised with their results on the host, labels
        already int32 and dense.  affinity returns N x Ka uint64 (its code is the parent
        commit's, untouched here), move_gains best and gain, 12 bytes per point.
  move_gains_*_full_s  the same with the N x (Ka + 1) matrix copied out
  refine_vi, refine_binder
        refine() from the cut with 1 % of the points relabelled at random (seed 1): rounds,
        trials, moved, converged, seconds, and the loss of the cut itself, of the start and
        of the end.
  unsettled_vi, unsettled_binder
        refine() on a trace the tree search refuses (tools/trace_summary_bench.py's synthetic
        labels of the same N and M: every draw the truth with a tenth of its labels redrawn,
        so nearly every point is a label column of its own), started from draw 0: the same
        fields, with the loss of the best saved draw in place of the cut's.
For the kernels' own times run one trace under rocprofv3 --kernel-trace --stats with
--no-refine.
"""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

RUNS = {"c4": 300, "c5": 420}       # seconds allowed per run


def run(name, reps, with_refine):
    import numpy as np
    from split_and_merge_gibbs_sampling_amd._lib import ptr
    from split_and_merge_gibbs_sampling_amd.posterior import LabelTrace, _relabel, minvi_avg, refine
    from trace_summary_bench import chain_trace, free_bytes
    free_bytes()
    cfg, M = ("c4", 24) if name == "c4" else ("c5", 64)
    tr = np.ascontiguousarray(_relabel(chain_trace(cfg, M), "iteration"))
    N = tr.shape[1]
    t = LabelTrace(tr)
    cut = np.ascontiguousarray(minvi_avg(t)[0] - 1, dtype=np.int32)
    Ka = int(cut.max()) + 1
    L, h, chk = t.eng._L, t.eng._h, t.eng._check
    aff = np.zeros((N, Ka), np.uint64)
    best, gain, full = np.zeros(N, np.int32), np.zeros(N), np.zeros((N, Ka + 1))
    calls = {
        "affinity": lambda: L.hdpm_trace_affinity(h, ptr(cut), Ka, ptr(aff), None),
        "move_gains_vi": lambda: L.hdpm_trace_move_gains(h, ptr(cut), Ka, 0, ptr(best), ptr(gain), None),
        "move_gains_binder": lambda: L.hdpm_trace_move_gains(h, ptr(cut), Ka, 1, ptr(best), ptr(gain), None),
        "move_gains_vi_full": lambda: L.hdpm_trace_move_gains(h, ptr(cut), Ka, 0, ptr(best), ptr(gain), ptr(full)),
        "move_gains_binder_full": lambda: L.hdpm_trace_move_gains(h, ptr(cut), Ka, 1, ptr(best), ptr(gain), ptr(full)),
    }
    res = {"run": name, "N": N, "M": M, "Ka": Ka, "Kz": int(tr.max()) + 1, "reps": reps}
    for key, call in calls.items():
        chk(call())                                  # warm-up: buffers allocated
        ts = []
        for _ in range(reps):
            t0 = time.perf_counter()
            chk(call())
            ts.append(time.perf_counter() - t0)
        ts.sort()
        res[key + "_s"] = {"median": round(ts[len(ts) // 2], 6), "min": round(ts[0], 6), "max": round(ts[-1], 6)}
    # what was timed is right: Binder's gains are the expression in aff
    me = np.arange(N)
    na = np.bincount(cut, minlength=Ka + 1).astype(np.int64)
    a64 = np.concatenate([aff.astype(np.int64), np.zeros((N, 1), np.int64)], axis=1)
    expr = (M * (na[None, :] - na[cut][:, None] - 1) - 2 * (a64 - a64[me, cut][:, None])).astype(np.float64)
    expr[me, cut] = 0.0
    assert np.array_equal(full, expr) and gain.tobytes() == full[me, best].tobytes()
    res["move_gains_binder_over_affinity"] = round(res["move_gains_binder_s"]["median"] / res["affinity_s"]["median"], 3)
    res["move_gains_vi_over_affinity"] = round(res["move_gains_vi_s"]["median"] / res["affinity_s"]["median"], 3)
    if with_refine:
        rng = np.random.default_rng(1)
        start = cut.copy()
        idx = rng.choice(N, size=N // 100, replace=False)
        start[idx] = rng.integers(0, Ka, idx.size)
        for loss in ("VI", "Binder"):
            own = (t.vi(cut) if loss == "VI" else t.binder(cut))[0]
            t0 = time.perf_counter()
            r = refine(t, start, loss)
            dt = time.perf_counter() - t0
            res["refine_" + loss.lower()] = {
                "seconds": round(dt, 4), "rounds": r["rounds"], "trials": r["trials"], "moved": r["moved"],
                "converged": r["converged"], "K": int(r["cl"].max()), "cut": float(own), "start": r["start"],
                "value": r["value"], "same_as_cut": bool(np.array_equal(_relabel(r["cl"][None, :], "cl")[0],
                                                                         _relabel(cut[None, :], "cl")[0]))}
    t.close()
    if with_refine:
        from split_and_merge_gibbs_sampling_amd.posterior import minbinder, minvi
        from trace_summary_bench import labels
        _, tr = labels(N, M, 7)
        t = LabelTrace(tr)
        for loss in ("VI", "Binder"):
            own = (minvi(t, tr, "draws", loss="VI") if loss == "VI" else minbinder(t, tr))[1]
            t0 = time.perf_counter()
            r = refine(t, tr[0], loss)
            dt = time.perf_counter() - t0
            res["unsettled_" + loss.lower()] = {
                "seconds": round(dt, 4), "rounds": r["rounds"], "trials": r["trials"], "moved": r["moved"],
                "converged": r["converged"], "K": int(r["cl"].max()), "best_draw": float(own), "start": r["start"],
                "value": r["value"]}
        t.close()
    print(json.dumps(res), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--run", choices=sorted(RUNS))
    ap.add_argument("--reps", type=int, default=7, help="timed calls per quantity (at least 5)")
    ap.add_argument("--no-refine", action="store_true", help="the timed calls only (for a profiler run)")
    a = ap.parse_args()
    if a.reps < 5:
        ap.error("--reps must be at least 5")
    if a.run:
        run(a.run, a.reps, not a.no_refine)
        return 0
    # the parent never opens the GPU; a run that fails or overruns ends the tool
    for name, limit in RUNS.items():
        cmd = ["timeout", "-k", "10", str(limit), sys.executable, "-u", os.path.abspath(__file__), "--run", name,
               "--reps", str(a.reps)] + (["--no-refine"] if a.no_refine else [])
        st = subprocess.run(cmd).returncode
        if st != 0:
            print(json.dumps({"run": name, "failed": st}), flush=True)
            return st
    return 0


if __name__ == "__main__":
    sys.exit(main())
