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

    python tools/trace_summary_bench.py --avg [--dense-n n]
    python tools/trace_summary_bench.py --run avg-c4 | avg-c5 | avg-synth

--avg: minVI(method = "avg") without the matrix (LabelTrace.groups / avg_tree / cut_losses,
minvi_avg) on traces recorded from the bench's own chains (truth init, Neal-8, m = 3, 20
iterations of warm-up, then M consecutive saved iterations): avg-c4 (N = 70,000, M = 24) and
avg-c5 (N = 1,000,000, M = 64); avg-synth is a synthetic settled trace (N = 200,000,
M = 1,000, 8,000 single moved labels) that puts U near the default limit.  One JSON line per run with U (the distinct label columns)
and the times of grouping, counts (S, with its download), tree (host) and cut losses, and
minvi_avg end to end on a fresh trace.  The dense path (PSM + scipy's linkage on the N x N
matrix) is timed beside it on --dense-n evenly spaced points of the same trace (default 4,000;
0 = skip; the full C4 matrix would be 39 GB of doubles on the host and a 70k-point
linkage), with the two partitions compared.

    python tools/trace_summary_bench.py --uncertainty
    python tools/trace_summary_bench.py --run unc-c4 | unc-c5

--uncertainty: how far the estimate can be trusted (LabelTrace.distances / affinity,
csrc/trace_uncertainty.hip) on the recorded chains of --avg, unc-c5 (N = 1,000,000, M = 64)
being the headline; the estimate is minvi_avg's.  One JSON line per run with the medians (and
the smallest and largest) of --reps timed C calls after one warm-up call, labels already
int32 and relabelled: `terms` for the estimate alone, `affinity` (aff only, N x Ka uint64
copied back), `cross` (cross only), both together, and `distances` beside `losses` (VI and
Binder) for the same 8 draws as candidates; "table_reads_TBps" is M N Ka x 4 B over the
`affinity` median.
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
AVG_RUNS = {"avg-c4": 420, "avg-c5": 420, "avg-synth": 420}
UNC_RUNS = {"unc-c4": 300, "unc-c5": 420}


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


def chain_trace(cfg, M, warmup=20):
    """M consecutive saved iterations of the bench's chain on config cfg"""
    import numpy as np
    import split_and_merge_gibbs_sampling_amd as hd
    from split_and_merge_gibbs_sampling_amd.data import config
    ds = config(cfg)
    eng = hd.Engine(0)
    eng.set_data(ds.codes, ds.attrisize, ds.gamma, ds.v, ds.w)
    eng.set_seed(1)
    params = eng.chain_params(m=3, iterations=warmup + M, L=0, burnin=0, neal8=True, split_merge=False, t=10, r=10)
    eng.init_chain(params, c_i=ds.truth)
    eng.iterations(0, warmup)
    tr = np.array(eng.iterations_record(warmup, M)[3])
    eng.close()
    assert tr.shape == (M, ds.n), tr.shape
    return tr


def same_partition(a, b):
    import numpy as np

    def canon(c):
        _, idx, inv = np.unique(c, return_index=True, return_inverse=True)
        rank = np.empty(idx.size, np.int64)
        rank[np.argsort(idx)] = np.arange(idx.size)
        return rank[inv.ravel()]
    return bool(np.array_equal(canon(a), canon(b)))


def run_avg(name, dense_n):
    import numpy as np
    from split_and_merge_gibbs_sampling_amd import HdpmError
    from split_and_merge_gibbs_sampling_amd.posterior import PSM, LabelTrace, minvi, minvi_avg
    free_bytes()                                 # torch's device context first, as in run()
    if name == "avg-synth":
        # a settled base partition with 8,000 single moved labels: every moved point is a
        # column of its own, so U is near the default limit and M = 1,000 is the issue's size
        N, M = 200_000, 1000
        rng = np.random.default_rng(9)
        base = rng.integers(0, 10, N).astype(np.int32)
        tr = np.tile(base, (M, 1))
        pts = rng.choice(N, 8000, replace=False)
        tr[rng.integers(0, M, pts.size), pts] = rng.integers(0, 10, pts.size)
    else:
        cfg, M = ("c4", 24) if name == "avg-c4" else ("c5", 64)
        tr = chain_trace(cfg, M)
    N = tr.shape[1]
    res = {"run": name, "N": N, "M": M,
           "moved_per_draw": round(float(np.mean(tr[1:] != tr[:-1]) * N), 1)}
    f0 = free_bytes()
    t = LabelTrace(tr)
    try:
        t0 = time.perf_counter()
        U = C_groups(t)
        t1 = time.perf_counter()
        counts = np.zeros((U, U), np.uint32)
        t.eng._check(t.eng._L.hdpm_trace_group_info(t.eng._h, None, None, None, counts.ctypes.data))
        t2 = time.perf_counter()
        t.avg_tree()
        t3 = time.perf_counter()
        kmax = min(U, 255, -(-N // 8))
        lb = t.cut_losses(1, kmax)[0]
        t4 = time.perf_counter()
        res.update(U=U, groups_s=round(t1 - t0, 4), counts_s=round(t2 - t1, 4), tree_s=round(t3 - t2, 4),
                   cut_losses_s=round(t4 - t3, 4), cuts=kmax, best_k=int(np.argmin(lb)) + 1,
                   vi_lb=float(lb.min()), device_bytes=int(f0 - free_bytes()))
    except HdpmError as e:
        res["refused"] = str(e)
    t.close()
    if "refused" not in res:
        t0 = time.perf_counter()
        t = LabelTrace(tr)
        cl, v = minvi_avg(t)
        res["minvi_avg_total_s"] = round(time.perf_counter() - t0, 4)
        t.close()
        assert v == res["vi_lb"]
    if dense_n and "refused" not in res:
        sub = np.ascontiguousarray(tr[:, ::max(1, N // dense_n)][:, :dense_n])      # every cluster present
        t0 = time.perf_counter()
        t = LabelTrace(sub)
        cl_t, v_t = minvi_avg(t)
        t1 = time.perf_counter()
        t.close()
        p = PSM(sub)
        cl_p, v_p = minvi(p, method="avg")
        t2 = time.perf_counter()
        p.close()
        res["dense_n"] = {"n": int(sub.shape[1]), "U": int(t.U), "trace_s": round(t1 - t0, 4),
                          "dense_s": round(t2 - t1, 4), "same_partition": same_partition(cl_t, cl_p),
                          "vi_lb_rel_diff": abs(v_t - v_p) / abs(v_p) if v_p else abs(v_t - v_p)}
    print(json.dumps(res), flush=True)


def run_unc(name, reps):
    import numpy as np
    from split_and_merge_gibbs_sampling_amd._lib import ptr
    from split_and_merge_gibbs_sampling_amd.posterior import LabelTrace, _relabel, minvi_avg
    free_bytes()
    cfg, M = ("c4", 24) if name == "unc-c4" else ("c5", 64)
    tr = np.ascontiguousarray(_relabel(chain_trace(cfg, M), "iteration"))
    N = tr.shape[1]
    f0 = free_bytes()
    t = LabelTrace(tr)
    cl = np.ascontiguousarray(minvi_avg(t)[0][None, :] - 1, dtype=np.int32)
    Ka = int(cl.max()) + 1
    cands = np.ascontiguousarray(tr[:: max(1, M // 8)][:8])
    nc = len(cands)
    L, h, chk = t.eng._L, t.eng._h, t.eng._check
    all_, same = np.zeros(N, np.uint64), np.zeros((1, N), np.uint64)
    aff, cross = np.zeros((N, Ka), np.uint64), np.zeros((Ka, Ka), np.uint64)
    vi, b, k = np.zeros((nc, M)), np.zeros((nc, M), np.uint64), np.zeros(M, np.int32)
    lv, lq, lp = np.zeros(nc), np.zeros(nc, np.uint64), np.zeros(1, np.uint64)
    calls = {
        "terms": lambda: L.hdpm_trace_terms(h, ptr(cl), 1, ptr(all_), ptr(same)),
        "affinity": lambda: L.hdpm_trace_affinity(h, ptr(cl), Ka, ptr(aff), None),
        "cross": lambda: L.hdpm_trace_affinity(h, ptr(cl), Ka, None, ptr(cross)),
        "affinity_and_cross": lambda: L.hdpm_trace_affinity(h, ptr(cl), Ka, ptr(aff), ptr(cross)),
        "distances": lambda: L.hdpm_trace_distances(h, ptr(cands), nc, ptr(vi), ptr(b), ptr(k)),
        "losses": lambda: L.hdpm_trace_losses(h, ptr(cands), nc, None, ptr(lv), ptr(lq), ptr(lp)),
    }
    res = {"run": name, "N": N, "M": M, "Ka": Ka, "Kz": int(tr.max()) + 1, "ncand_distances": nc, "reps": reps}
    for key, call in calls.items():
        chk(call())                                  # warm-up: buffers allocated
        ts = []
        for _ in range(reps):
            t0 = time.perf_counter()
            chk(call())
            ts.append(time.perf_counter() - t0)
        ts.sort()
        res[key + "_s"] = {"median": round(ts[len(ts) // 2], 6), "min": round(ts[0], 6), "max": round(ts[-1], 6)}
    res["table_reads_TBps"] = round(M * N * Ka * 4 / res["affinity_s"]["median"] / 1e12, 4)
    res["affinity_over_terms"] = round(res["affinity_s"]["median"] / res["terms_s"]["median"], 3)
    res["distances_over_losses"] = round(res["distances_s"]["median"] / res["losses_s"]["median"], 3)
    res["device_bytes"] = int(f0 - free_bytes())
    # what was timed is right: aff's row sums are `all`, its own column is `same`
    assert np.array_equal(aff.sum(1), all_) and np.array_equal(aff[np.arange(N), cl[0]], same[0])
    assert np.array_equal(cross, cross.T) and int(cross.sum()) == int(all_.sum())
    t.close()
    print(json.dumps(res), flush=True)


def C_groups(t):
    import ctypes
    U = ctypes.c_int32(0)
    t.eng._check(t.eng._L.hdpm_trace_groups(t.eng._h, 16384, 0, ctypes.byref(U)))
    t.U = int(U.value)
    return t.U


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--run", choices=sorted(RUNS) + sorted(AVG_RUNS) + sorted(UNC_RUNS))
    ap.add_argument("--uncertainty", action="store_true", help="distances and affinities on recorded chains")
    ap.add_argument("--reps", type=int, default=7, help="--uncertainty: timed calls per quantity (at least 5)")
    ap.add_argument("--avg", action="store_true", help="the matrix-free average-linkage search on recorded chains")
    ap.add_argument("--dense-n", type=int, default=4000, help="--avg: points of the dense comparison (0: none)")
    a = ap.parse_args()
    if a.reps < 5:
        ap.error("--reps must be at least 5")
    if a.run in UNC_RUNS:
        run_unc(a.run, a.reps)
        return 0
    if a.run in AVG_RUNS:
        run_avg(a.run, a.dense_n)
        return 0
    if a.run:
        run(a.run)
        return 0
    # the parent never opens the GPU; a run that fails or overruns ends the tool
    for name, limit in (UNC_RUNS if a.uncertainty else AVG_RUNS if a.avg else RUNS).items():
        extra = ["--reps", str(a.reps)] if a.uncertainty else ["--dense-n", str(a.dense_n)] if a.avg else []
        st = subprocess.run(["timeout", "-k", "10", str(limit), sys.executable, "-u", os.path.abspath(__file__),
                             "--run", name] + extra).returncode
        if st != 0:
            print(json.dumps({"run": name, "failed": st}), flush=True)
            return st
    return 0


if __name__ == "__main__":
    sys.exit(main())
