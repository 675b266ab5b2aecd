"""Device time of the logit-processor kernels (launchLogitProc, launchLogitProcCount) next to a
device-to-device copy of the same logits.

For 1, 16 and 64 active rows of 128256 logits with 0 and 300 bias entries per slot,
`ops.bench_logit_proc` times `iters` back-to-back launches of each kernel between two device events
(after 5 warm-up launches); `bench_memcpy_d2d` copies rows x vocab x 4 bytes the same way in the
same process. The processor reads the logits and the slot's counts and writes the processed logits,
about 1.5 times the bytes the copy moves (read + write of the logits alone); with back-to-back
launches on the same rows both work from the caches, not from HBM.

  python scripts/bench_logit_proc.py [--iters 200] [--vocab 128256]

`scripts/bench_api.py --n 64 [--penalties]` gives the serving-level comparison.
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
        raise SystemExit("bench_logit_proc: no HIP device")
    out = []
    for rows in (1, 16, 64):
        copy_us = C.bench_memcpy_d2d(rows * args.vocab * 4, args.iters)
        for n_bias in (0, 300):
            proc_us, count_us = C.ops.bench_logit_proc(rows, args.vocab, n_bias, args.iters)
            r = {"rows": rows, "vocab": args.vocab, "n_bias": n_bias, "logit_proc_us": round(proc_us, 2),
                 "count_us": round(count_us, 2), "memcpy_d2d_us": round(copy_us, 2), "ratio": round(proc_us / copy_us, 2)}
            print(r, flush=True)
            out.append(r)
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
