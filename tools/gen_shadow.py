"""The generator's shadow on the sweep, from a rocprofv3 --kernel-trace --output-format csv run:
k_prepass launches split into those that overlap a k_mt_gen* interval and those that do not
(medians, share), the generator's calls and time, and the device period (k_pipe_wait start to
the next one's).  The first --skip prepass launches (warm-up) are left out.
Usage: python tools/gen_shadow.py <dir or *_kernel_trace.csv> [--skip N] [--json out.json]"""
import argparse
import csv
import glob
import json
import os
import statistics


def load(path):
    if os.path.isdir(path):
        hits = sorted(glob.glob(os.path.join(path, "**", "*kernel_trace.csv"), recursive=True))
        if not hits:
            raise SystemExit(f"no *kernel_trace.csv under {path}")
        path = hits[-1]
    rows = []
    with open(path, newline="") as f:
        for r in csv.DictReader(f):
            rows.append((r["Kernel_Name"].split("(")[0], int(r["Start_Timestamp"]), int(r["End_Timestamp"])))
    rows.sort(key=lambda r: r[1])
    return rows


def med(v):
    return round(statistics.median(v), 2) if v else None


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("trace")
    ap.add_argument("--skip", type=int, default=5)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    rows = load(a.trace)
    gen = [(s, e) for n, s, e in rows if "k_mt_gen" in n]
    pre = [(s, e) for n, s, e in rows if "k_prepass" in n][a.skip:]
    wait = [s for n, s, e in rows if "k_pipe_wait" in n]
    if not pre:
        raise SystemExit("no k_prepass launches")
    t0 = pre[0][0]
    gen_in = [(s, e) for s, e in gen if e > t0]
    shadow, clear = [], []
    for s, e in pre:
        hit = any(gs < e and s < ge for gs, ge in gen_in)
        (shadow if hit else clear).append((e - s) / 1e3)
    wait = [s for s in wait if s >= t0]
    period = [(b - a_) / 1e3 for a_, b in zip(wait, wait[1:])]
    res = {
        "sweeps": len(pre),
        "prepass_clear": {"n": len(clear), "median_us": med(clear)},
        "prepass_shadow": {"n": len(shadow), "median_us": med(shadow)},
        "shadow_share": round(len(shadow) / len(pre), 3),
        "gen_calls": len(gen_in),
        "gen_total_us": round(sum(min(e, pre[-1][1]) - max(s, t0) for s, e in gen_in if s < pre[-1][1]) / 1e3, 1),
        "gen_median_us": med([(e - s) / 1e3 for s, e in gen_in]),
        "period_us": {"median": med(period), "mean": round(sum(period) / len(period), 2) if period else None},
    }
    print(json.dumps(res))
    if a.json:
        with open(a.json, "w") as f:
            f.write(json.dumps(res) + "\n")


if __name__ == "__main__":
    main()
