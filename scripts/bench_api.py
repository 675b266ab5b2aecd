"""Serving throughput of `dllama-api` on one GPU: N concurrent chat requests, greedy vs sampled.

Starts build/dllama-api on random-init Llama-3.1-8B weights (--synthetic, a synthetic 128256-token
tokenizer), fires N concurrent /v1/chat/completions requests of max_tokens each (threads, one HTTP
connection per request), and reports the aggregate completion tokens/s for temperature 0 (greedy)
and temperature 0.8 / top_p 0.9 with per-request seeds (device sampling: only token ids come back
to the host). One untimed round first captures the graphs.

  python scripts/bench_api.py [--n 64] [--max-tokens 64] [--port 0] [--logprobs K] [--penalties] [--filters] [--json] [--schema]
                              [--embeddings] [--score]

--embeddings: after the chat rounds, one /v1/embeddings request of N inputs of token ids (about 48
tokens each), alone and next to a greedy chat round: inputs/s and prompt tokens/s.

--score: after the chat rounds, N /v1/completions scoring requests (echo, max_tokens 0, logprobs 5;
prompts of token ids, about 48 tokens each) sent together, next to the same prompts sent as
max_tokens 1 requests without logprobs: prompt tokens/s of both, on the same server.
"""
import argparse
import http.client
import json
import os
import socket
import subprocess
import sys
import tempfile
import threading
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)


def _port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _post(port, body, out, i):
    try:
        c = http.client.HTTPConnection("127.0.0.1", port, timeout=300)
        c.request("POST", "/v1/chat/completions", json.dumps(body), {"Content-Type": "application/json"})
        r = c.getresponse()
        data = json.loads(r.read())
        out[i] = data["usage"]["completion_tokens"]
    except Exception as e:  # noqa: BLE001 - counted as a failed request
        out[i] = e


def _embed_round(port, n, tokens_each=48):
    """One /v1/embeddings request of n token-id inputs: (prompt tokens, seconds)."""
    body = {"input": [[1000 + (37 * i + 11 * j) % 100000 for j in range(tokens_each)] for i in range(n)],
            "encoding_format": "base64"}
    t0 = time.perf_counter()
    c = http.client.HTTPConnection("127.0.0.1", port, timeout=300)
    c.request("POST", "/v1/embeddings", json.dumps(body), {"Content-Type": "application/json"})
    r = c.getresponse()
    data = json.loads(r.read())
    if r.status != 200 or len(data["data"]) != n:
        raise RuntimeError(f"embeddings failed: {r.status} {str(data)[:200]}")
    return data["usage"]["prompt_tokens"], time.perf_counter() - t0


def _completions_round(port, n, score, tokens_each=48):
    """n concurrent /v1/completions requests over the same token-id prompts: scoring (echo, max_tokens
    0, logprobs 5) or plain max_tokens 1 without logprobs. Returns (prompt tokens, seconds)."""
    out = [None] * n

    def one(i):
        body = {"prompt": [1000 + (37 * i + 11 * j) % 100000 for j in range(tokens_each)], "temperature": 0}
        body.update(dict(echo=True, max_tokens=0, logprobs=5) if score else dict(max_tokens=1))
        try:
            c = http.client.HTTPConnection("127.0.0.1", port, timeout=300)
            c.request("POST", "/v1/completions", json.dumps(body), {"Content-Type": "application/json"})
            r = c.getresponse()
            data = json.loads(r.read())
            if score and len(data["choices"][0]["logprobs"]["token_logprobs"]) != tokens_each:
                raise RuntimeError("a scoring response without its records")
            out[i] = data["usage"]["prompt_tokens"]
        except Exception as e:  # noqa: BLE001 - counted as a failed request
            out[i] = e

    th = [threading.Thread(target=one, args=(i,)) for i in range(n)]
    t0 = time.perf_counter()
    for t in th:
        t.start()
    for t in th:
        t.join()
    dt = time.perf_counter() - t0
    bad = [o for o in out if not isinstance(o, int)]
    if bad:
        raise RuntimeError(f"{len(bad)} completions requests failed: {bad[:3]}")
    return sum(out), dt


EXTRA = {}  # request fields added to every body (--logprobs, --penalties, --filters, --json, --schema)


def _round(port, n, max_tokens, temperature, seed0):
    out = [None] * n
    th = []
    for i in range(n):
        body = {"messages": [{"role": "user", "content": f"hello world {i} the"}], "max_tokens": max_tokens,
                "temperature": temperature, "top_p": 0.9, "seed": seed0 + i, **EXTRA}
        th.append(threading.Thread(target=_post, args=(port, body, out, i)))
    t0 = time.perf_counter()
    for t in th:
        t.start()
    for t in th:
        t.join()
    dt = time.perf_counter() - t0
    bad = [o for o in out if not isinstance(o, int)]
    if bad:
        raise RuntimeError(f"{len(bad)} requests failed: {bad[:3]}")
    return sum(out), dt


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=64)
    ap.add_argument("--max-tokens", type=int, default=64)
    ap.add_argument("--port", type=int, default=0)
    ap.add_argument("--max-batch", type=int, default=0,
                    help="rows per forward (default 4 x --n: prompts prefill in big chunks, MALL-resident weights)")
    ap.add_argument("--kv-pages", type=int, default=0,
                    help="paged KV cache: pool pages per layer (0: contiguous slots x seq_len)")
    ap.add_argument("--kv-page-size", type=int, default=64)
    ap.add_argument("--kv-dtype", default="f32", choices=["f32", "bf16"], help="KV cache (f32: the reference's, the default)")
    ap.add_argument("--logprobs", type=int, default=-1,
                    help="K >= 0: every request asks for logprobs with top_logprobs K (default: none)")
    ap.add_argument("--penalties", action="store_true",
                    help="every request sends frequency_penalty 0.5, presence_penalty 0.5 and a 16-entry logit_bias")
    ap.add_argument("--filters", action="store_true",
                    help="every request sends top_k 40 and min_p 0.05: they act in the sampled round "
                         "(temperature 0.8), the greedy round ignores them")
    ap.add_argument("--json", action="store_true",
                    help="every request sends response_format json_object (JSON mode: both rounds are masked)")
    ap.add_argument("--schema", action="store_true",
                    help="every request sends response_format json_schema with a small object schema (structured "
                         "outputs: both rounds are masked by the compiled grammar)")
    ap.add_argument("--embeddings", action="store_true",
                    help="also time one /v1/embeddings request of --n inputs, alone and next to a greedy chat round")
    ap.add_argument("--score", action="store_true",
                    help="also time --n /v1/completions scoring requests (echo, max_tokens 0, logprobs 5) next to "
                         "the same prompts as max_tokens 1 requests without logprobs")
    args = ap.parse_args()
    if args.filters:
        EXTRA.update(top_k=40, min_p=0.05)
    if args.json:
        EXTRA.update(response_format={"type": "json_object"})
    if args.schema:
        props = {"name": {"type": "string"}, "age": {"type": "integer"}, "tags": {"type": "array", "items": {"type": "string"}, "maxItems": 8},
                 "role": {"enum": ["admin", "user", "guest"]}, "active": {"type": "boolean"}}
        EXTRA.update(response_format={"type": "json_schema", "json_schema": {"name": "person", "strict": True, "schema": {
            "type": "object", "properties": props, "required": list(props), "additionalProperties": False}}})
    if args.penalties:
        EXTRA.update(frequency_penalty=0.5, presence_penalty=0.5, logit_bias={str(1000 + 37 * i): (i % 5) - 2 for i in range(16)})
    if args.logprobs >= 0:
        EXTRA.update(logprobs=True, top_logprobs=args.logprobs)
    from distributed_llama_multiusers_amd.models.synthetic import make_tokenizer
    tmp = tempfile.mkdtemp()
    tok = os.path.join(tmp, "tok.t")
    make_tokenizer(tok, 128256)
    port = args.port or _port()
    cmd = [os.path.join(REPO, "build", "dllama-api"), "--synthetic", "llama3_1_8b", "--tokenizer", tok,
           "--gpu-index", "0", "--port", str(port), "--slots", str(args.n), "--max-batch", str(args.max_batch or 4 * args.n),
           "--max-seq-len", str(64 + args.max_tokens + 32), "--buffer-float-type", "q80", "--kv-dtype", args.kv_dtype]
    if args.kv_pages:
        cmd += ["--kv-pages", str(args.kv_pages), "--kv-page-size", str(args.kv_page_size)]
    log = open(os.path.join(tmp, "api.log"), "w")
    srv = subprocess.Popen(cmd, stdout=log, stderr=subprocess.STDOUT)
    try:
        for _ in range(600):
            try:
                c = http.client.HTTPConnection("127.0.0.1", port, timeout=2)
                c.request("GET", "/v1/models")
                if c.getresponse().status == 200:
                    break
            except OSError:
                pass
            if srv.poll() is not None:
                raise RuntimeError("dllama-api exited: " + open(log.name).read()[-2000:])
            time.sleep(0.2)
        _round(port, args.n, 8, 0.0, 0)      # untimed: graph capture for the batch sizes
        _round(port, args.n, 8, 0.8, 100)
        res = {}

        def health():
            c = http.client.HTTPConnection("127.0.0.1", port, timeout=10)
            c.request("GET", "/health")
            return json.loads(c.getresponse().read())

        for name, temp, seed in (("greedy", 0.0, 0), ("sampled", 0.8, 1000)):
            h0 = health()
            toks, dt = _round(port, args.n, args.max_tokens, temp, seed)
            h1 = health()
            d = {k: h1[k] - h0[k] for k in ("forwards", "rows", "prefill_rows", "decode_rows", "busy_ms") if k in h1}
            res[name] = {"completion_tokens": toks, "s": round(dt, 3), "tok_s": round(toks / dt, 1),
                         "forwards": d.get("forwards"), "rows": d.get("rows"), "prefill_rows": d.get("prefill_rows"),
                         "forward_ms": round(d.get("busy_ms", 0.0), 1),
                         "host_ms": round(dt * 1000 - d.get("busy_ms", 0.0), 1)}
            print(name, res[name], flush=True)
        res["sampled_vs_greedy"] = round(res["sampled"]["tok_s"] / res["greedy"]["tok_s"], 3)
        res["concurrent_requests"] = args.n
        res["kv_cache"] = args.kv_dtype
        res["max_batch"] = args.max_batch or 4 * args.n
        res["max_tokens"] = args.max_tokens
        res["top_logprobs"] = args.logprobs if args.logprobs >= 0 else None
        res["penalties"] = bool(args.penalties)
        res["filters"] = bool(args.filters)
        res["json"] = bool(args.json)
        res["schema"] = bool(args.schema)
        if args.embeddings:
            _embed_round(port, args.n)  # untimed: graph capture
            toks, dt = _embed_round(port, args.n)
            res["embeddings"] = {"inputs": args.n, "prompt_tokens": toks, "s": round(dt, 3),
                                 "inputs_s": round(args.n / dt, 1), "tok_s": round(toks / dt, 1)}
            box = {}
            th = threading.Thread(target=lambda: box.update(e=_embed_round(port, args.n)))
            th.start()
            ctoks, cdt = _round(port, args.n // 2 or 1, args.max_tokens, 0.0, 0)
            th.join()
            res["embeddings_next_to_chat"] = {"embed_s": round(box["e"][1], 3), "chat_tok_s": round(ctoks / cdt, 1)}
            print("embeddings", res["embeddings"], res["embeddings_next_to_chat"], flush=True)
        if args.score:
            for score in (False, True):  # untimed: graph capture
                _completions_round(port, args.n, score)
            for name, score in (("score_plain_max_tokens_1", False), ("score", True), ("score_plain_max_tokens_1_again", False),
                                ("score_again", True)):
                toks, dt = _completions_round(port, args.n, score)
                res[name] = {"requests": args.n, "prompt_tokens": toks, "s": round(dt, 3), "tok_s": round(toks / dt, 1)}
                print(name, res[name], flush=True)
        print(json.dumps(res), flush=True)
    finally:
        srv.terminate()
        try:
            srv.wait(timeout=30)
        except subprocess.TimeoutExpired:
            srv.kill()
        log.close()
        print(open(log.name).read()[-1500:])


if __name__ == "__main__":
    main()
