"""Posterior summaries with and without the N x N matrix, end to end on the GPU.

    python tools/trace_summary_bench.py            both runs, each a child under its own timeout
    python tools/trace_summary_bench.py --run c4   one run in this process
    python tools/trace_summary_bench.py --run c5

One JSON line per run:
  c4  the inputs of tests/test_gpu_posterior.py::test_psm_c4_size (N = 70,000, M = 24, the
      same generator and seed), the 24 draws scored as candidates: the dense path (PSM build
      + vi_lb) and the matrix-free one (LabelTrace build + vi_lb), wall clock from the numpy
      labels to the numpy losses, and the largest relative difference of the two results.
  c5  N = 1,000,000, M = 64 draws of the same 90%-truth shape, 64 candidates: the
      matrix-free path only (the dense one would need 4 TB).
"device_bytes" is the drop in free device memory while the summary object is alive.
"""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

RUNS = {"c4": 600, "c5": 420}       # seconds allowed per run


def labels(N, M, seed):
    import numpy as np
    rng = np.random.default_rng(seed)
    truth = rng.integers(0, 10, N)
    tr = np.where(rng.random((M, N)) < 0.9, truth[None, :], rng.integers(0, 12, (M, N))).astype(np.int32)
    return truth, tr


def free_bytes():
    import torch
    return torch.cuda.mem_get_info(0)[0]


def timed(make, cand):
    """build + vi_lb, first (with the context's and the buffers' creation) and again"""
    out = {}
    for k in ("first", "again"):
        f0 = free_bytes()
        t0 = time.perf_counter()
        obj = make()
        t1 = time.perf_counter()
        v = obj.vi_lb(cand)
        t2 = time.perf_counter()
        out[k] = {"build_s": round(t1 - t0, 4), "vi_lb_s": round(t2 - t1, 4), "total_s": round(t2 - t0, 4),
                  "device_bytes": int(f0 - free_bytes())}
        obj.close()
    return out, v


def run(name):
    import numpy as np
    from split_and_merge_gibbs_sampling_amd.posterior import PSM, LabelTrace
    if name == "c4":
        N, M = 70_000, 24
        _, tr = labels(N, M, 7)
        cand = tr
        res = {"run": "c4", "N": N, "M": M, "ncand": len(cand)}
        res["trace"], vt = timed(lambda: LabelTrace(tr), cand)
        res["dense"], vd = timed(lambda: PSM(tr), cand)
        res["vi_lb_max_rel_diff"] = float(np.max(np.abs(vt - vd) / np.abs(vd)))
        res["trace_over_dense"] = round(res["trace"]["again"]["total_s"] / res["dense"]["again"]["total_s"], 4)
    else:
        N, M = 1_000_000, 64
        truth, tr = labels(N, M, 7)
        _, cand = labels(N, 64, 8)
        cand[0] = truth
        res = {"run": "c5", "N": N, "M": M, "ncand": len(cand)}
        res["trace"], vt = timed(lambda: LabelTrace(tr), cand)
        res["vi_lb_truth"], res["vi_lb_min_other"] = float(vt[0]), float(vt[1:].min())
        t = LabelTrace(tr)
        t0 = time.perf_counter()
        vi = t.vi(cand)
        t1 = time.perf_counter()
        b = t.binder(cand)
        t2 = time.perf_counter()
        t.close()
        res["vi_s"], res["binder_s"] = round(t1 - t0, 4), round(t2 - t1, 4)
        res["vi_argmin"], res["binder_argmin"] = int(np.argmin(vi)), int(np.argmin(b))
    print(json.dumps(res), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--run", choices=sorted(RUNS))
    a = ap.parse_args()
    if a.run:
        run(a.run)
        return 0
    # the parent never opens the GPU; a run that fails or overruns ends the tool
    for name, limit in RUNS.items():
        st = subprocess.run(["timeout", "-k", "10", str(limit), sys.executable, "-u", os.path.abspath(__file__),
                             "--run", name]).returncode
        if st != 0:
            print(json.dumps({"run": name, "failed": st}), flush=True)
            return st
    return 0


if __name__ == "__main__":
    sys.exit(main())
