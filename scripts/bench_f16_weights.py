#!/usr/bin/env python3
"""F16-weight kernels and model next to their F32 / Q80 counterparts on one GPU (profiles/f16_weights.md).

  python scripts/bench_f16_weights.py [--out DIR] [--repeats 3] [--skip-model] [--wide-only]

Kernels: us per launch (device events around a graph of back-to-back launches over rotating weight
copies, engine_bench.cpp) of gemvF16wKernel vs the F32 GEMV and gemmF16wKernel vs gemmF32Kernel on the
Llama-3.1-8B wcls / w13 / wo shapes, alternating, with the weight bytes per second of each.
Wide: us per pass over 65..1024 tokens as one gemmF16wWideKernel launch vs 64-token narrow launches
(profiles/f16_wide_gemm.md).
Model: `dllama inference --synthetic llama3_1_8b` with f16 and q80 synthetic weights, alternating: a
64-token prompt + 128 predicted (decode) and a 1025-token prompt + 63 predicted (prefill)."""
import argparse
import json
import os
import re
import subprocess
import sys
import tempfile

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

SHAPES = {"wcls": (128256, 4096), "w13": (28672, 4096), "wo": (4096, 4096)}


def kernels(C, repeats):
    rows_out = []
    for name, (rows, n) in SHAPES.items():
        copies = 64 if name == "wo" else 8
        for what, tokens in (("gemv", 1), ("gemm", 16), ("gemm", 64)):
            us = {"f32": [], "f16": []}
            for _ in range(repeats):
                for kind in ("f32", "f16"):
                    if what == "gemv":
                        t = C.bench_gemv_f16w(rows, n, 0, 0, 1, 0, 0, kind == "f32", copies, 200)
                    else:
                        t = C.bench_gemm_f16w(rows, n, tokens, kind == "f32", copies, 30)
                    us[kind].append(round(t, 2))
            r = {"shape": name, "kernel": what, "tokens": tokens, "us": us,
                 "tbps": {k: round(rows * n * (4 if k == "f32" else 2) / (min(v) * 1e-6) / 1e12, 2) for k, v in us.items()}}
            print(json.dumps(r), flush=True)
            rows_out.append(r)
    return rows_out


def wide_kernels(C, repeats):
    """One pass over `tokens` rows as one gemmF16wWideKernel launch against the chunked narrow launches
    of <= 64 (an engine without the wide kernel), alternating; TFLOP/s of the fastest wide repeat."""
    rows_out = []
    for name, (rows, n) in SHAPES.items():
        copies = 64 if name == "wo" else 8
        for tokens in (65, 128, 256, 512, 1024):
            us = {"narrow": [], "wide": []}
            for _ in range(repeats):
                for kind in ("narrow", "wide"):
                    us[kind].append(round(C.bench_gemm_f16w(rows, n, tokens, False, copies, 30, kind == "wide"), 1))
            r = {"shape": name, "tokens": tokens, "us": us, "narrow_over_wide": round(min(us["narrow"]) / min(us["wide"]), 2),
                 "wide_tflops": round(2.0 * rows * n * tokens / (min(us["wide"]) * 1e-6) / 1e12, 1)}
            print(json.dumps(r), flush=True)
            rows_out.append(r)
    return rows_out


def model_point(weights, prompt_tokens, steps, tok):
    exe = os.path.join(REPO, "build", "dllama")
    prompt = ("The quick brown fox jumps over the lazy dog " * 40)[:prompt_tokens]
    cmd = [exe, "inference", "--synthetic", "llama3_1_8b", "--synthetic-weights", weights, "--tokenizer", tok, "--prompt",
           prompt, "--steps", str(prompt_tokens + steps), "--temperature", "0", "--max-seq-len", "2048",
           "--buffer-float-type", "f32" if weights == "f16" else "q80", "--kv-dtype", "f32", "--log-level", "0"]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    m = re.findall(r"tokens/s:\s*([\d.]+)\s*\(([\d.]+) ms/tok\)", r.stdout)
    if r.returncode != 0 or len(m) < 2:
        raise RuntimeError((r.stdout + r.stderr)[-600:])
    return {"weights": weights, "prompt": prompt_tokens, "eval_ms_per_token": float(m[0][1]), "pred_ms_per_token": float(m[1][1])}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="")
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--skip-model", action="store_true")
    ap.add_argument("--wide-only", action="store_true", help="the wide GEMM section alone")
    a = ap.parse_args()
    import distributed_llama_multiusers_amd as dl
    from distributed_llama_multiusers_amd.models.synthetic import make_tokenizer
    res = {"kernels": [] if a.wide_only else kernels(dl.native(), a.repeats), "wide": wide_kernels(dl.native(), a.repeats),
           "model": []}
    a.skip_model = a.skip_model or a.wide_only
    if not a.skip_model:
        with tempfile.TemporaryDirectory() as d:
            tok = os.path.join(d, "llama3_synth.t")
            make_tokenizer(tok, 128256)
            for prompt_tokens, steps in ((64, 128), (1025, 63)):
                for _ in range(2):
                    for weights in ("f16", "q80"):
                        p = model_point(weights, prompt_tokens, steps, tok)
                        print(json.dumps(p), flush=True)
                        res["model"].append(p)
    if a.out:
        os.makedirs(a.out, exist_ok=True)
        with open(os.path.join(a.out, "f16_weights.json"), "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
