"""Device time of the candidate filter (launchLogitFilter: top_k / min_p) next to a device-to-device
copy of the same logits and to launchSample on the rows it leaves.

For 64 and 1 active rows of 128256 bell-shaped logits at temperature 0.8 and the filters top_k = 40,
min_p = 0.05, both, and top_k = 1, `ops.bench_logit_filter` times between two device events, after 5
warm-up rounds, `iters` back-to-back repeats of: a device copy of the logits; that copy followed by
the filter on the copy (the filter works in place, so every launch needs fresh rows; the filter's
own time is the difference); launchSample (top-p 0.9) on the filtered rows. The filter reads a row up
to four times (three selection passes and the mask; min_p alone: twice) and writes it once; with
back-to-back launches on the same rows it works from the caches, not from HBM.

  python scripts/bench_logit_filter.py [--iters 200] [--vocab 128256]

`scripts/bench_api.py --n 64 [--filters]` gives the serving-level comparison.
"""
import argparse
import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--vocab", type=int, default=128256)
    args = ap.parse_args()
    import distributed_llama_multiusers_amd as dl
    C = dl.native()
    if C.hip_device_count() < 1:
        raise SystemExit("bench_logit_filter: no HIP device")
    off = float("-inf")
    delta = C.cpu_ops.min_p_delta(0.8, 0.05)
    out = []
    for rows in (64, 1):
        for name, top_k, d in (("top_k=40", 40, off), ("min_p=0.05", 0, delta), ("top_k=40,min_p=0.05", 40, delta),
                               ("top_k=1", 1, off)):
            copy_us, both_us, sample_us = C.ops.bench_logit_filter(rows, args.vocab, top_k, d, args.iters)
            r = {"rows": rows, "vocab": args.vocab, "filter": name, "memcpy_d2d_us": round(copy_us, 2),
                 "copy_plus_filter_us": round(both_us, 2), "logit_filter_us": round(both_us - copy_us, 2),
                 "sample_us": round(sample_us, 2)}
            print(r, flush=True)
            out.append(r)
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
