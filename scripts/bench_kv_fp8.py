"""Decode attention per KV cache type (f32 / bf16 / fp8) and the KV capacity the HBM check admits
(profiles/kv_fp8.md). Llama-3.1-8B attention shapes (32 query heads, 8 KV heads, head size 128).

  python scripts/bench_kv_fp8.py            # prints one JSON line per measurement

Timing: C.bench_attention (a captured graph of `iters` launches cycling over `copies` caches, device
events around it); the three cache types alternate inside each of `ROUNDS` rounds and every figure of a
round is printed, so the spread is visible. The launch is launchAttention's own choice per type: the
VALU kernel for f32, attnDecodeMfmaKernel for bf16 (>= 1024 positions), attnDecodeFp8Kernel for fp8.
Capacity: an engine far too large is refused by the HBM check, whose message names the positions that
would fit.
"""
import json
import os
import re
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import distributed_llama_multiusers_amd as dl  # noqa: E402

C = dl.native()
ROUNDS = 3
TYPES = {"f32": (False, False), "bf16": (True, False), "fp8": (False, True)}
H8B = dict(dim=4096, hidden_dim=14336, n_layers=32, n_heads=32, n_kv_heads=8, vocab_size=128256, seq_len=8192,
           rope_theta=500000, weight_type=2)


def attention():
    for pos, batch, copies, iters in ((1024, 1, 16, 200), (4096, 1, 8, 200), (32768, 1, 4, 100), (1024, 64, 4, 100),
                                      (4096, 64, 2, 50)):
        seq = (pos + 256) // 256 * 256
        for r in range(ROUNDS):
            for name, (bf, f8) in TYPES.items():
                us = C.bench_attention(32, 4, 128, seq, pos, batch, copies, iters, kv_bf16=bf, kv_fp8=f8)
                kv_bytes = 2 * batch * (pos + 1) * 8 * 128 * {"f32": 4, "bf16": 2, "fp8": 1}[name]
                print(json.dumps(dict(what="attention", kv=name, pos=pos, batch=batch, round=r, us=round(us, 2),
                                      kv_gbps=round(kv_bytes / us / 1e3, 1))), flush=True)


def capacity():
    for name in TYPES:
        try:
            C.HipEngine("", "q80", synthetic=H8B, max_seq_len=8192, n_slots=4096, max_batch=32, kv_dtype=name)
            print(json.dumps(dict(what="capacity", kv=name, error="not refused")))
        except RuntimeError as e:
            m = re.search(r"fits (\d+) positions", str(e))
            print(json.dumps(dict(what="capacity", kv=name, positions=int(m.group(1)) if m else None,
                                  slots_x_8192=int(m.group(1)) // 8192 if m else None, message=str(e))), flush=True)


if __name__ == "__main__":
    capacity()
    attention()
