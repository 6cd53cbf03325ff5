"""Imputation of missing codes (csrc/predict.hip k_pr_part + k_pr_impute) against the route a
user had before it, on the GPU.

    python tools/impute_bench.py                      every case, each a child under its own timeout
    python tools/impute_bench.py --run c5 --gaps 16   one case in this process
    python tools/impute_bench.py --run c4 --gaps 1 [--reps 3] [--no-baseline]

Cases: the shapes and the synthetic recorded chain of tools/predict_bench.py (c5: ny = 65,536,
M = 256, K = 20, d = 128, 4 levels; c4: ny = 8,192, M = 64, K = 10, d = 784, 6 levels), each
row with `gaps` of its codes set to 0 at random attributes: c5 with 1 and with 16 gaps per
row, c4 with 1.

One JSON line per case: the medians (smallest, largest) of --reps timed C calls after one
warm-up call, wall clock around calls that end in a device synchronise, inputs already in
their C types:
  impute    hdpm_predict_impute, pmf and lpd
  partial   hdpm_predict_partial, lpd and p_new, on the same rows (k_pr_part without the
            scratch of imputation)
  new       hdpm_predict_new on the complete rows (k_pr_new)
  baseline  gaps = 1 only: the fill-in route, levels calls of hdpm_predict_new (lpd) on the
            rows with the gap set to level l; the host work of filling in and of forming
            exp(lpd_l - logsumexp) is not timed, so this is a lower bound on that route.
            Rows with several gaps have no such route (levels^gaps rows per row).
"identity_max_rel" (gaps = 1, with the baseline) is the largest relative difference between
pmf_l and exp(lpd_l) / sum_l exp(lpd_l).
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

CASES = [("c5", 1), ("c5", 16), ("c4", 1)]
LIMIT = 300


def run(name, gaps, reps, baseline):
    import numpy as np
    import split_and_merge_gibbs_sampling_amd as hd
    from split_and_merge_gibbs_sampling_amd._lib import ptr
    from predict_bench import SHAPES, inputs, med
    sh = SHAPES[name]
    ny, M, K, d, levels = sh["ny"], sh["M"], sh["K"], sh["d"], sh["levels"]
    ds, tr, cens, sigs = inputs(**sh)
    full = np.ascontiguousarray(ds.codes)
    rng = np.random.default_rng(9)
    cols = np.argsort(rng.random((ny, d)), axis=1)[:, :gaps]       # `gaps` distinct attributes per row
    Y = full.copy()
    Y[np.arange(ny)[:, None], cols] = 0
    n_missing = ny * gaps
    ld = int(ds.attrisize.max())
    trace = hd.LabelTrace(tr)
    hd.Predictive(trace, cens, sigs, ds.attrisize, ds.gamma)
    eng = trace.eng
    L, h = eng._L, eng._h
    pmf, lpd, pn = np.zeros((n_missing, ld)), np.zeros(ny), np.zeros(ny)
    calls = {
        "impute": lambda: L.hdpm_predict_impute(h, ptr(Y), ny, n_missing, ld, ptr(pmf), ptr(lpd)),
        "partial": lambda: L.hdpm_predict_partial(h, ptr(Y), ny, None, 0, ptr(lpd), ptr(pn), None),
        "new": lambda: L.hdpm_predict_new(h, ptr(full), ny, None, 0, ptr(lpd), ptr(pn), None),
    }
    out = {"shape": name, "gaps": gaps, "ny": ny, "M": M, "K": K, "d": d, "levels": levels, "ld": ld,
           "entries": n_missing, "reps": reps}
    for key, f in calls.items():
        eng._check(f())                               # warm-up
        ts = []
        for _ in range(reps):
            t0 = time.perf_counter()
            eng._check(f())
            ts.append(time.perf_counter() - t0)
        out[key] = med(ts)
    assert np.all(np.isfinite(pmf)) and float(np.abs(pmf.sum(axis=1) - 1.0).max()) < 1e-10
    if baseline and gaps == 1:
        filled = [full.copy() for _ in range(levels)]
        for l in range(levels):
            filled[l][np.arange(ny), cols[:, 0]] = l + 1
        dens = np.zeros((levels, ny))
        eng._check(L.hdpm_predict_new(h, ptr(filled[0]), ny, None, 0, ptr(dens[0]), None, None))    # warm-up
        ts = []
        for _ in range(reps):
            t0 = time.perf_counter()
            for l in range(levels):
                eng._check(L.hdpm_predict_new(h, ptr(filled[l]), ny, None, 0, ptr(dens[l]), None, None))
            ts.append(time.perf_counter() - t0)
        out["baseline"] = med(ts)
        out["baseline_over_impute"] = round(out["baseline"]["median_s"] / out["impute"]["median_s"], 2)
        w = np.exp(dens - dens.max(axis=0))
        w = (w / w.sum(axis=0)).T
        out["identity_max_rel"] = float((np.abs(pmf[:, :levels] - w) / w).max())
    trace.close()
    print(json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--run", choices=["c4", "c5"])
    ap.add_argument("--gaps", type=int, default=1)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--no-baseline", action="store_true")
    a = ap.parse_args()
    if a.run:
        run(a.run, a.gaps, a.reps, not a.no_baseline)
        return 0
    for name, gaps in CASES:
        cmd = [sys.executable, os.path.abspath(__file__), "--run", name, "--gaps", str(gaps), "--reps", str(a.reps)]
        if a.no_baseline:
            cmd.append("--no-baseline")
        try:
            r = subprocess.run(cmd, timeout=LIMIT)
        except subprocess.TimeoutExpired:
            print(json.dumps({"shape": name, "gaps": gaps, "error": "timeout"}), flush=True)
            return 1
        if r.returncode != 0:
            return r.returncode       # nothing more on the device after a failed run
    return 0


if __name__ == "__main__":
    sys.exit(main())
