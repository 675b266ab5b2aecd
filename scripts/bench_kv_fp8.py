"""Decode and prefill attention per KV cache type (f32 / bf16 / fp8) and the KV capacity the HBM check
admits (profiles/kv_fp8.md). Llama-3.1-8B attention shapes (32 query heads, 8 KV heads, head size 128).

  python scripts/bench_kv_fp8.py            # prints one JSON line per measurement
  python scripts/bench_kv_fp8.py prefill    # only the prefill part (attention launches, short contexts, the prompt)

Timing: C.bench_attention (a captured graph of `iters` launches cycling over `copies` caches, device
events around it); the three cache types alternate inside each of `ROUNDS` rounds and every figure of a
round is printed, so the spread is visible. The launch is launchAttention's own choice per type: the
VALU kernel for f32, attnDecodeMfmaKernel for bf16 (>= 1024 positions), attnDecodeFp8Kernel for fp8.
Prefill: the same harness on one prompt block (row_block: `rows` consecutive positions of one slot ending
at `end` keys, f16 output as in a batched forward) through launchAttentionPrefill, and for fp8 also row by
row through launchAttention, which is what an engine does with DL_PREFILL_FP8_MIN above the context (and
did before attnPrefillFp8Kernel existed). The end-to-end figure is a 4096-token prompt in forwards of
512 rows on the synthetic 8B model, host clock around forwards that end in a stream synchronise, one
child process per setting (the variable is read once per process), the settings alternating.
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


def prefill():
    for rows, end, copies, iters in ((64, 256, 8, 200), (64, 1024, 8, 200), (64, 4096, 4, 100), (64, 32768, 2, 30),
                                     (1024, 1024, 4, 50), (1024, 4096, 2, 20), (1024, 32768, 2, 5)):
        for r in range(ROUNDS):
            for name, bf, f8, block in (("fp8", False, True, 1), ("fp8 row by row", False, True, 2),
                                        ("bf16", True, False, 1), ("f32", False, False, 1)):
                us = C.bench_attention(32, 4, 128, end, end - 1, rows, copies, iters, kv_bf16=bf, kv_fp8=f8, row_block=block)
                print(json.dumps(dict(what="prefill", kv=name, rows=rows, end=end, round=r, us=round(us, 2))), flush=True)


def crossover():
    """Short contexts, where the row-by-row decode kernel may still win: the DL_PREFILL_FP8_MIN decision."""
    for rows, end in ((64, 64), (64, 128), (64, 192), (64, 256), (64, 320), (64, 384), (64, 512), (64, 768), (128, 128),
                      (256, 256), (256, 320), (256, 384), (512, 512)):
        for r in range(ROUNDS):
            for name, block in (("fp8", 1), ("fp8 row by row", 2)):
                us = C.bench_attention(32, 4, 128, (end + 255) // 256 * 256, end - 1, rows, 8, 200, kv_bf16=False, kv_fp8=True,
                                       row_block=block)
                print(json.dumps(dict(what="crossover", kv=name, rows=rows, end=end, round=r, us=round(us, 2))), flush=True)


def prompt(n=4096, chunk=512, runs=3):
    """ms per prompt token of this process's engine (DL_PREFILL_FP8_MIN as inherited)."""
    import time
    eng = C.HipEngine("", "q80", synthetic=dict(H8B, seq_len=n), max_seq_len=n, max_batch=chunk, kv_dtype="fp8")
    ms = []
    for _ in range(1 + runs):  # the first run warms every shape up
        t0 = time.perf_counter()
        for p0 in range(0, n, chunk):
            eng.forward([1 + p % 1000 for p in range(p0, p0 + chunk)], list(range(p0, p0 + chunk)), [0] * chunk)
        ms.append((time.perf_counter() - t0) * 1e3 / n)
    print(json.dumps(dict(what="prompt", tokens=n, chunk=chunk, fp8_min=os.environ.get("DL_PREFILL_FP8_MIN", "0"),
                          kernel=eng.prefill_attn_kernel(chunk, n - 1), ms_per_token=[round(x, 4) for x in ms[1:]])), flush=True)


def prompts():
    import subprocess
    for _ in range(2):
        for fp8_min in ("0", "1000000000"):
            subprocess.run([sys.executable, os.path.abspath(__file__), "prompt"], check=True, timeout=300,
                           env=dict(os.environ, DL_PREFILL_FP8_MIN=fp8_min))


if __name__ == "__main__":
    if sys.argv[1:] == ["prompt"]:
        prompt()
    elif sys.argv[1:] == ["crossover"]:
        crossover()
    elif sys.argv[1:] == ["prefill"]:
        prefill()
        crossover()
        prompts()
    else:
        capacity()
        attention()
        prefill()
        crossover()
        prompts()
