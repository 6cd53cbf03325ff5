"""The profiles of an estimate's classes (csrc/profile.hip, Predictive.profile) on the GPU, beside
the table pass of the same partition, the O(M N) floor that every summary of a partition pays.

    python tools/profile_bench.py                 every shape, each a child under its own timeout
    python tools/profile_bench.py --run l4 [--reps 7]
    python tools/profile_bench.py --out profiles/profile/profile_bench.jsonl

Shapes: a synthetic recorded chain of N = 1,000,000 points, d = 128 attributes, M = 64 draws of
K = 20 clusters.  Each draw's labels are a fixed truth with 5 % of the points moved, its centers
fixed base centers with 2 % of the codes redrawn, its sigmas uniform in 0.3..0.8; the estimate is
the truth (Ka = 20).
  l4    every attribute has 4 levels (ld = 4)
  l255  attrisize mixed 2..255 (ld = 255): level rows of Ka x d x ld x 16 bytes = 10 MB
  ka255 l4 with the estimate cut into Ka = 255 classes (the truth's classes split by index)

One JSON line per shape: the medians (smallest, largest) of --reps timed C calls after one
warm-up call, the host clock around calls that end synchronised with their results on the host,
the partition already int32:
  pass      hdpm_trace_affinity with cross alone: the table pass (k_tr_tables), its transpose and
            the Ka x Ka cross sums -- the call that runs the table pass and little else
  sigma     hdpm_predict_profile with sigma_mean and sigma_var
  trace     the same with sigma_trace (M x Ka x d doubles copied out)
  counts    hdpm_predict_profile with center_cnt alone
  levels    center_cnt and code_pmf
  all       everything but sigma_trace
"*_fold_over_pass" = (median - pass median) / pass median: what the fold of the tables with the
parameter tables costs in table passes (every profile call runs the pass first).
"checked" says that sum_l center_cnt = M n_a and sum_l code_pmf = 1 within 1e-10 held.
For the kernels' own times run one shape under rocprofv3 --kernel-trace --stats.
"""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

N, D, M, K = 1_000_000, 128, 64, 20
SHAPES = {"l4": 300, "l255": 300, "ka255": 300}       # seconds allowed per shape


def inputs(name):
    import numpy as np
    rng = np.random.default_rng(11)
    att = np.full(D, 4, np.int32)
    if name == "l255":
        att = rng.choice([2, 3, 4, 6, 16, 17, 100, 255], size=D).astype(np.int32)
        att[0] = 255
    truth = rng.integers(0, K, N).astype(np.int32)
    base = np.stack([rng.integers(1, att + 1) for _ in range(K)])
    tr = np.empty((M, N), np.int32)
    cens, sigs = [], []
    for s in range(M):
        z = np.where(rng.random(N) < 0.05, rng.integers(0, K, N), truth).astype(np.int32)
        z[rng.permutation(N)[:K]] = np.arange(K)
        tr[s] = z
        redraw = rng.integers(1, att[None, :] + 1, size=(K, D))
        cens.append(np.where(rng.random((K, D)) < 0.02, redraw, base).astype(np.float64))
        sigs.append(rng.uniform(0.3, 0.8, size=(K, D)))
    cl, Ka = truth, K
    if name == "ka255":
        cl, Ka = (truth + K * (np.arange(N) % 13)).astype(np.int32) % 255, 255
    return att, tr, cens, sigs, np.ascontiguousarray(cl, np.int32), Ka


def med(ts):
    ts = sorted(ts)
    return {"median_s": round(ts[len(ts) // 2], 6), "min_s": round(ts[0], 6), "max_s": round(ts[-1], 6)}


def run(name, reps):
    import numpy as np
    import split_and_merge_gibbs_sampling_amd as hd
    from split_and_merge_gibbs_sampling_amd._lib import ptr
    att, tr, cens, sigs, cl, Ka = inputs(name)
    ld = int(att.max())
    trace = hd.LabelTrace(tr)
    t0 = time.perf_counter()
    hd.Predictive(trace, cens, sigs, att, 0.7)
    t_build = time.perf_counter() - t0
    eng = trace.eng
    L, h = eng._L, eng._h
    cross = np.zeros((Ka, Ka), np.uint64)
    cnt, pmf = np.zeros((Ka, D, ld), np.uint64), np.zeros((Ka, D, ld))
    mean, var, trc = np.zeros((Ka, D)), np.zeros((Ka, D)), np.zeros((M, Ka, D))

    def prof(*out):
        return lambda: L.hdpm_predict_profile(h, ptr(cl), Ka, ld, *[ptr(o) for o in out])

    calls = {
        "pass": lambda: L.hdpm_trace_affinity(h, ptr(cl), Ka, None, ptr(cross)),
        "sigma": prof(None, None, mean, var, None),
        "trace": prof(None, None, mean, var, trc),
        "counts": prof(cnt, None, None, None, None),
        "levels": prof(cnt, pmf, None, None, None),
        "all": prof(cnt, pmf, mean, var, None),
    }
    out = {"shape": name, "N": N, "M": M, "K": K, "d": D, "Ka": Ka, "ld": ld, "reps": reps, "build_s": round(t_build, 4),
           "level_row_bytes": Ka * D * ld * 16, "table_bytes": M * Ka * K * 4, "label_bytes": M * N}
    for key, f in calls.items():
        eng._check(f())                               # warm-up: buffers allocated
        ts = []
        for _ in range(reps):
            t0 = time.perf_counter()
            eng._check(f())
            ts.append(time.perf_counter() - t0)
        out[key] = med(ts)
    base = out["pass"]["median_s"]
    for key in calls:
        if key != "pass":
            out[key + "_fold_over_pass"] = round((out[key]["median_s"] - base) / base, 3)
    na = np.bincount(cl, minlength=Ka)
    ok = np.array_equal(cnt.sum(axis=2), np.broadcast_to((M * na)[:, None], (Ka, D)).astype(np.uint64))
    ok = ok and bool(np.all(np.abs(pmf.sum(axis=2)[na > 0] - 1.0) <= 1e-10)) and bool(np.all(mean[na > 0] > 0))
    out["checked"] = bool(ok)
    trace.close()
    print(json.dumps(out), flush=True)
    return 0 if ok else 1


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--run", choices=sorted(SHAPES))
    ap.add_argument("--reps", type=int, default=7, help="timed calls per quantity (at least 5)")
    ap.add_argument("--out", help="append the JSON lines to this file too")
    a = ap.parse_args()
    if a.reps < 5:
        ap.error("--reps must be at least 5")
    if a.run:
        return run(a.run, a.reps)
    # the parent never opens the GPU; a shape that fails or overruns ends the tool
    for name, limit in SHAPES.items():
        cmd = ["timeout", "-k", "10", str(limit), sys.executable, "-u", os.path.abspath(__file__), "--run", name,
               "--reps", str(a.reps)]
        r = subprocess.run(cmd, stdout=subprocess.PIPE, text=True)
        sys.stdout.write(r.stdout)
        sys.stdout.flush()
        if r.returncode != 0:
            print(json.dumps({"shape": name, "failed": r.returncode}), flush=True)
            return r.returncode
        if a.out:
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            with open(a.out, "a") as f:
                f.write(r.stdout)
    return 0


if __name__ == "__main__":
    sys.exit(main())
