"""The posterior predictive (csrc/predict.hip) against the route a user had before it, on the GPU.

    python tools/predict_bench.py                 both shapes, each a child under its own timeout
    python tools/predict_bench.py --run c5        one shape in this process
    python tools/predict_bench.py --run c4 [--reps 3] [--no-baseline]

Shapes (synthetic, data.hamming_mixture; the rows serve as new rows and as training rows):
  c5  ny = N = 65,536, M = 256 draws, K = 20, d = 128, 4 levels
  c4  ny = N = 8,192,  M = 64 draws,  K = 10, d = 784, 6 levels
Each draw's labels are the truth with 5 % of the points moved, its centers the mixture's with
2 % of the codes redrawn, its sigmas uniform in 0.3..0.8.

One JSON line per shape: the medians (smallest, largest) of --reps timed C calls after one
warm-up call, wall clock around calls that end in a device synchronise, inputs already in
their C types:
  new          hdpm_predict_new, lpd and p_new
  new_coclass  hdpm_predict_new with coclass against the truth as the partition (Ka = K)
  own          hdpm_predict_own, all three outputs
  baseline     M times hdpm_set_state + hdpm_loglik_matrix on the same rows, once: the ll
               values only (no lse, no sums over draws), so a lower bound on that route
"select_adds" = ny M K d for new, N M d for own; "*_gsa_per_s" is 1e-9 select_adds / median.
"ll_equal" says that draw 0's ll of the two routes are the same bytes.
"""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = {"c5": dict(ny=65536, M=256, K=20, d=128, levels=4, limit=420),
          "c4": dict(ny=8192, M=64, K=10, d=784, levels=6, limit=420)}


def inputs(ny, M, K, d, levels, **_):
    import numpy as np
    from split_and_merge_gibbs_sampling_amd.data import hamming_mixture
    ds = hamming_mixture(n=ny, d=d, k=K, levels=levels, seed=2024)
    rng = np.random.default_rng(5)
    att = ds.attrisize
    base = np.stack([np.array([np.bincount(ds.codes[ds.truth == k, j], minlength=att[j] + 1).argmax()
                               for j in range(d)]) for k in range(K)])
    tr = np.empty((M, ny), np.int32)
    cens, sigs = [], []
    for s in range(M):
        z = np.where(rng.random(ny) < 0.05, rng.integers(0, K, ny), ds.truth).astype(np.int32)
        z[rng.permutation(ny)[:K]] = np.arange(K)
        tr[s] = z
        redraw = rng.integers(1, att[None, :] + 1, size=(K, d))
        cens.append(np.where(rng.random((K, d)) < 0.02, redraw, base).astype(np.float64))
        sigs.append(rng.uniform(0.3, 0.8, size=(K, d)))
    return ds, tr, cens, sigs


def med(ts):
    ts = sorted(ts)
    return {"median_s": round(ts[len(ts) // 2], 5), "min_s": round(ts[0], 5), "max_s": round(ts[-1], 5)}


def run(name, reps, baseline):
    import numpy as np
    import split_and_merge_gibbs_sampling_amd as hd
    from split_and_merge_gibbs_sampling_amd._lib import ptr
    sh = SHAPES[name]
    ny, M, K, d = sh["ny"], sh["M"], sh["K"], sh["d"]
    ds, tr, cens, sigs = inputs(**sh)
    Y = np.ascontiguousarray(ds.codes)
    trace = hd.LabelTrace(tr)
    t0 = time.perf_counter()
    hd.Predictive(trace, cens, sigs, ds.attrisize, ds.gamma)
    t_build = time.perf_counter() - t0
    eng = trace.eng
    L, h = eng._L, eng._h
    lpd, pn, co = np.zeros(ny), np.zeros(ny), np.zeros((ny, K))
    cl = np.ascontiguousarray(ds.truth, np.int32)
    lppd, var, cpo = np.zeros(ny), np.zeros(ny), np.zeros(ny)
    calls = {
        "new": lambda: L.hdpm_predict_new(h, ptr(Y), ny, None, 0, ptr(lpd), ptr(pn), None),
        "new_coclass": lambda: L.hdpm_predict_new(h, ptr(Y), ny, ptr(cl), K, ptr(lpd), ptr(pn), ptr(co)),
        "own": lambda: L.hdpm_predict_own(h, ptr(Y), ptr(lppd), ptr(var), ptr(cpo)),
    }
    out = {"shape": name, "ny": ny, "M": M, "K": K, "d": d, "reps": reps, "build_s": round(t_build, 4),
           "select_adds_new": ny * M * K * d, "select_adds_own": ny * M * d}
    for key, f in calls.items():
        eng._check(f())                               # warm-up
        ts = []
        for _ in range(reps):
            t0 = time.perf_counter()
            eng._check(f())
            ts.append(time.perf_counter() - t0)
        out[key] = med(ts)
        sa = out["select_adds_own"] if key == "own" else out["select_adds_new"]
        out[key + "_gsa_per_s"] = round(1e-9 * sa / out[key]["median_s"], 2)
    assert np.all(np.isfinite(lpd)) and np.all(np.isfinite(co)) and np.all(np.isfinite(cpo))
    if baseline:
        ll0 = np.zeros((ny, K))
        eng._check(L.hdpm_predict_loglik(h, 0, ptr(Y), ny, ptr(ll0), None))
        be = hd.Engine(0)
        try:
            be.set_data(Y, ds.attrisize, ds.gamma, ds.v, ds.w)
            be.set_state(tr[0], cens[0], sigs[0])
            first = be.loglik_matrix(K)[0]            # warm-up
            out["ll_equal"] = bool(first.tobytes() == ll0.tobytes())
            t0 = time.perf_counter()
            for s in range(M):
                be.set_state(tr[s], cens[s], sigs[s])
                be.loglik_matrix(K)
            out["baseline"] = {"total_s": round(time.perf_counter() - t0, 4)}
        finally:
            be.close()
        out["new_over_baseline"] = round(out["baseline"]["total_s"] / out["new"]["median_s"], 2)
        out["new_coclass_over_baseline"] = round(out["baseline"]["total_s"] / out["new_coclass"]["median_s"], 2)
    trace.close()
    print(json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--run", choices=sorted(SHAPES))
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--no-baseline", action="store_true")
    a = ap.parse_args()
    if a.run:
        run(a.run, a.reps, not a.no_baseline)
        return 0
    rc = 0
    for name, sh in SHAPES.items():
        cmd = [sys.executable, os.path.abspath(__file__), "--run", name, "--reps", str(a.reps)]
        if a.no_baseline:
            cmd.append("--no-baseline")
        try:
            r = subprocess.run(cmd, timeout=sh["limit"])
        except subprocess.TimeoutExpired:
            print(json.dumps({"shape": name, "error": "timeout"}), flush=True)
            return 1
        if r.returncode != 0:
            return r.returncode       # nothing more on the device after a failed run
    return rc


if __name__ == "__main__":
    sys.exit(main())
