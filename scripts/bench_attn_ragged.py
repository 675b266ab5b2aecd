#!/usr/bin/env python3
"""Mixed serving forwards with and without the ragged prefill attention (csrc/hip/attn_ragged.hip).

Each forward is timed on a synthetic Llama-3.1-8B Q40 engine with an f32 KV cache, once with
DL_ATTN_RAGGED=0 and once with DL_ATTN_RAGGED=1 (the switch is read per engine, so both live in one
process and see the same clocks). Two figures per forward and switch:
  forward   median wall ms of eng.forward over --reps replays of the captured graph
  attention device ms of the forward's attention launches, summed over the layers (profile_forward)
The cache holds whatever the allocation left there: attention time does not depend on the values.

    python scripts/bench_attn_ragged.py --json out.json          # the table of profiles/attn_ragged.md
"""
import argparse
import json
import os
import statistics
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
from bench import LLAMA31_8B  # noqa: E402


def forwards(max_decode=17):
    """(name, positions, slots): d decode rows (slots 1..d) ahead of a prompt chunk of slot 0."""
    out = []
    for end in (1024, 4096):
        for chunk in (64, 1024):
            for keys in (150, 1024, 4000):
                for d in (1, 5, 17):
                    pos = [keys - 1] * d + list(range(end - chunk, end))
                    out.append((f"d={d}@{keys} + {chunk} rows ending at {end}", pos, list(range(1, d + 1)) + [0] * chunk))
    out.append(("two 32-row chunks, slots 0 / 1, ending at 1024 / 700", list(range(992, 1024)) + list(range(668, 700)), [0] * 32 + [1] * 32))
    out.append(("pure decode, 16 rows @1024", [1023] * 16, list(range(16))))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--layers", type=int, default=32)
    ap.add_argument("--only", default="", help="substring of the forwards to run")
    ap.add_argument("--json", default="")
    args = ap.parse_args()
    import distributed_llama_multiusers_amd as dl
    C = dl.native()
    shape = dict(LLAMA31_8B, n_layers=args.layers, seq_len=4096)
    engines = {}
    for sw in ("0", "1"):
        os.environ["DL_ATTN_RAGGED"] = sw
        engines[sw] = C.HipEngine("", "q80", synthetic=shape, max_seq_len=4096, max_batch=1024 + 17, n_slots=18,
                                  kv_dtype="f32", gpu_index=0, seed=1234)
    rows = []
    for name, pos, slots in forwards():
        if args.only not in name:
            continue
        toks = [1 + i % 1000 for i in range(len(pos))]
        rec = {"forward": name, "rows": len(pos)}
        for sw, eng in engines.items():
            for _ in range(3):  # eager, capture, first replay
                eng.forward(toks, pos, slots)
            ts = []
            for _ in range(args.reps):
                t0 = time.perf_counter()
                eng.forward(toks, pos, slots)
                ts.append((time.perf_counter() - t0) * 1e3)
            cls = eng.profile_forward(toks, pos, slots, temperatures=[0.0] * len(pos))
            rec[f"forward_ms_{sw}"] = statistics.median(ts)
            rec[f"forward_spread_{sw}"] = (max(ts) - min(ts)) / statistics.median(ts)
            rec[f"attention_ms_{sw}"] = cls.get("attention", float("nan"))
        rows.append(rec)
        print(f"{name:58s} forward {rec['forward_ms_0']:8.3f} -> {rec['forward_ms_1']:8.3f} ms   attention "
              f"{rec['attention_ms_0']:7.3f} -> {rec['attention_ms_1']:7.3f} ms", flush=True)
    if args.json:
        with open(args.json, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
