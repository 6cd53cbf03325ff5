"""The pipeline counters of bench.py's timed window (hdpm_stats: pipe_enqueued, pipe_runs,
pipe_early, pipe_early_ran, pipe_early_off, ...), which bench.py's result line does not print:
the same calls as bench.py main (init_chain from the ground truth, warmup, drop_prepared,
reset_stats, one hdpm_iterations call), one JSON line.

    python tools/early_go_stats.py [--config c5] [--steps 300] [--warmup 20]
"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

KEYS = ("sweeps", "moves", "pipe_enqueued", "pipe_runs", "pipe_early", "pipe_early_ran", "pipe_early_off",
        "pipe_refused", "pipe_recovered", "pipe_auto", "pipe_desync", "phi_device_calls", "phi_spec_runs")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="c5")
    ap.add_argument("--steps", type=int, default=300)
    ap.add_argument("--warmup", type=int, default=20)
    args = ap.parse_args()
    import split_and_merge_gibbs_sampling_amd as hd
    from split_and_merge_gibbs_sampling_amd.data import config
    ds = config(args.config)
    eng = hd.Engine(0)
    eng.set_data(ds.codes, ds.attrisize, ds.gamma, ds.v, ds.w)
    eng.set_seed(1)
    params = eng.chain_params(m=3, iterations=args.steps + args.warmup, L=0, burnin=0, neal8=True, split_merge=False)
    eng.init_chain(params, c_i=ds.truth)
    eng.iterations(0, args.warmup)
    eng.drop_prepared()
    eng.synchronize()
    eng.reset_stats()
    eng.iterations(args.warmup, args.steps)
    eng.synchronize()
    st = eng.stats()
    eng.close()
    print(json.dumps({"config": args.config, "steps": args.steps, **{k: int(st[k]) for k in KEYS}}))


if __name__ == "__main__":
    main()
