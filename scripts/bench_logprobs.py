"""Device time of the log-probability kernel (launchLogprobs) next to the argmax kernel.

For 1, 16 and 64 rows of 128256 random logits and k = 0 / 20 alternatives, `ops.bench_logprobs`
times `iters` back-to-back launches of each kernel between two device events in the same call
(after 5 warm-up launches). Both kernels read every logit once, so the argmax is the yardstick; with
back-to-back launches on the same rows both read them from the caches, not from HBM.

  python scripts/bench_logprobs.py [--iters 200] [--vocab 128256] [--targets]

--targets: the prompt-scoring shape instead: 64 and 1024 rows (a prefill chunk), every row scoring a
given token (LogprobArgs::target) rather than the id the argmax wrote.

`scripts/bench_api.py --n 16 [--logprobs 5]` gives the serving-level comparison.
"""
import argparse
import json
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--vocab", type=int, default=128256)
    ap.add_argument("--targets", action="store_true", help="64 and 1024 rows, every row scoring a given token")
    args = ap.parse_args()
    import distributed_llama_multiusers_amd as dl
    C = dl.native()
    if C.hip_device_count() < 1:
        raise SystemExit("bench_logprobs: no HIP device")
    rng = np.random.default_rng(0)
    out = []
    for rows in ((64, 1024) if args.targets else (1, 16, 64)):
        x = (rng.standard_normal((rows, args.vocab), dtype=np.float32) * 6)
        for k in (0, 20):
            lp_us, am_us = C.ops.bench_logprobs(x, rows, k, args.iters, args.targets)
            r = {"rows": rows, "targets": args.targets, "vocab": args.vocab, "k": k, "logprobs_us": round(lp_us, 2), "argmax_us": round(am_us, 2),
                 "ratio": round(lp_us / am_us, 2)}
            print(r, flush=True)
            out.append(r)
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
