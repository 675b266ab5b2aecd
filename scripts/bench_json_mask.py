"""Device time of JSON mode's kernels (launchJsonMask, launchJsonAdvance) next to a device-to-device
copy of the same logits, launchLogitFilter (top_k 40) and launchSample, and the host's jsonMaskHost
for one row.

The vocabulary is the synthetic tokenizer's at 128256 tokens (256 byte pieces, merges, fillers, 5
specials). Rows all sit in one state: START, where most tokens reject at their first byte, or inside
a string, where most run to their end (the long case). `ops.bench_json_mask` times between two device
events, after 5 warm-up rounds, `iters` back-to-back repeats; the mask works in place, so it is timed
behind a copy of the logits and its own time is the difference. The host figure is the median of 5
calls of `JsonTable.mask_host` on one row.

  python scripts/bench_json_mask.py [--iters 200] [--vocab 128256]

`scripts/bench_api.py --n 64 [--json]` gives the serving-level comparison.
"""
import argparse
import json
import os
import sys
import tempfile
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--vocab", type=int, default=128256)
    args = ap.parse_args()
    import numpy as np
    import distributed_llama_multiusers_amd as dl
    from distributed_llama_multiusers_amd.models.synthetic import make_tokenizer
    C = dl.native()
    if C.hip_device_count() < 1:
        raise SystemExit("bench_json_mask: no HIP device")
    info = make_tokenizer(os.path.join(tempfile.mkdtemp(), "tok.t"), args.vocab)
    table = C.JsonTable(info["tokens"], info["bos_id"], info["eos"])
    row = np.random.default_rng(0).standard_normal(args.vocab).astype(np.float32)
    out = []
    for name, prefix in (("START", b""), ("in-string", b'{"k":"v')):
        state = C.cpu_ops.json_walk(prefix)
        host = []
        for _ in range(5):
            t0 = time.perf_counter()
            masked = table.mask_host(row, state)
            host.append((time.perf_counter() - t0) * 1e6)
        for rows in (64, 1):
            copy_us, mask_us, adv_us, filt_us, sample_us = C.ops.bench_json_mask(rows, table, state, args.iters)
            r = {"rows": rows, "vocab": args.vocab, "state": name, "allowed": int(np.isfinite(masked).sum()),
                 "table_bytes": table.bytes, "memcpy_d2d_us": round(copy_us, 2), "copy_plus_mask_us": round(mask_us, 2),
                 "json_mask_us": round(mask_us - copy_us, 2), "json_advance_us": round(adv_us, 2),
                 "logit_filter_top_k_40_us": round(filt_us - copy_us, 2), "sample_us": round(sample_us, 2),
                 "json_mask_host_1_row_us": round(sorted(host)[2], 1)}
            print(r, flush=True)
            out.append(r)
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
