"""Device time of the structured-output kernels (launchGrammarMask, launchGrammarAdvance) next to a
device-to-device copy of the same logits, launchJsonMask and launchSample on the same rows, the
host's grammarMaskHost for one row, and the host compile time of a set of schemas.

The vocabulary is the synthetic tokenizer's at 128256 tokens (256 byte pieces, merges, fillers, 5
specials). Rows all follow one typical schema and sit in one state: the start state, where most
tokens reject at their first byte, or inside a free string, where most run to their end (the long
case). `ops.bench_grammar_mask` times between two device events, after warm-up rounds, `iters`
back-to-back repeats; the masks work in place, so they are timed behind a copy of the logits and
their own time is the difference. Host figures are medians of 5 calls.

  python scripts/bench_grammar_mask.py [--iters 200] [--vocab 128256]

`scripts/bench_api.py --n 64 [--schema]` gives the serving-level comparison.
"""
import argparse
import json
import os
import sys
import tempfile
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)


def obj(props):
    return dict(type="object", properties=props, required=list(props), additionalProperties=False)


TYPICAL = obj({"name": {"type": "string"}, "age": {"type": "integer"}, "email": {"type": ["string", "null"]},
               "tags": {"type": "array", "items": {"type": "string"}, "maxItems": 8},
               "role": {"enum": ["admin", "user", "guest"]}, "score": {"type": "number"}, "active": {"type": "boolean"}})
SCHEMAS = {
    "typical": TYPICAL,
    "flat_scalars": obj({k: {"type": t} for k, t in zip("abcde", ["string", "number", "integer", "boolean", "null"])}),
    "nested": obj({"user": obj({"id": {"type": "integer"}, "address": obj({"city": {"type": "string"}, "zip": {"type": "string", "maxLength": 10}})}),
                   "items": {"type": "array", "items": obj({"sku": {"type": "string"}, "qty": {"type": "integer"}}), "maxItems": 4}}),
    "bounded_strings": obj({"code": {"type": "string", "minLength": 4, "maxLength": 32}, "kind": {"enum": ["a", "b", "c"]}}),
}


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
        raise SystemExit("bench_grammar_mask: no HIP device")
    info = make_tokenizer(os.path.join(tempfile.mkdtemp(), "tok.t"), args.vocab)
    table = C.JsonTable(info["tokens"], info["bos_id"], info["eos"])
    out = []
    for name, schema in SCHEMAS.items():
        text, ms = json.dumps(schema), []
        for _ in range(5):
            t0 = time.perf_counter()
            g = C.Grammar.from_schema(text, table)
            ms.append((time.perf_counter() - t0) * 1e3)
        r = {"schema": name, "states": g.n_states, "classes": g.n_classes, "table_bytes": 2 * g.n_states * g.n_classes,
             "compile_ms": round(sorted(ms)[2], 2)}
        print(r, flush=True)
        out.append(r)
    g = C.Grammar.from_schema(json.dumps(TYPICAL), table)
    row = np.random.default_rng(0).standard_normal(args.vocab).astype(np.float32)
    for name, prefix in (("start", b""), ("in-string", b'{"name":"v')):
        state = g.walk(prefix)
        host = []
        for _ in range(5):
            t0 = time.perf_counter()
            masked = g.mask_host(row, state)
            host.append((time.perf_counter() - t0) * 1e6)
        for rows in (64, 1):
            copy_us, mask_us, adv_us, json_us, sample_us = C.ops.bench_grammar_mask(rows, table, g, state, args.iters)
            r = {"rows": rows, "vocab": args.vocab, "state": name, "allowed": int(np.isfinite(masked).sum()),
                 "memcpy_d2d_us": round(copy_us, 2), "copy_plus_mask_us": round(mask_us, 2),
                 "grammar_mask_us": round(mask_us - copy_us, 2), "grammar_advance_us": round(adv_us, 2),
                 "json_mask_at_start_us": round(json_us - copy_us, 2), "sample_us": round(sample_us, 2),
                 "grammar_mask_host_1_row_us": round(sorted(host)[2], 1)}
            print(r, flush=True)
            out.append(r)
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
