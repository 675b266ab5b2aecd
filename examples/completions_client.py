"""A short /v1/completions client for dllama-api: scores a sentence (echo, max_tokens 0, logprobs)
and prints each token's log-probability under the model, and the sentence's perplexity.

  build/dllama-api --model <model.m> --tokenizer <tokenizer.t> --buffer-float-type q80 --port 9990 &
  python examples/completions_client.py [--url http://127.0.0.1:9990] [--top 3] "the quick brown fox"

Row i of the prompt scores token i + 1, so the first token (BOS) has no log-probability.
"""
import argparse
import json
import math
import urllib.request


def score(url, text, top=0):
    body = {"prompt": text, "echo": True, "max_tokens": 0, "logprobs": top}
    req = urllib.request.Request(url + "/v1/completions", data=json.dumps(body).encode(),
                                 headers={"Content-Type": "application/json"})
    return json.loads(urllib.request.urlopen(req, timeout=300).read())["choices"][0]["logprobs"]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--url", default="http://127.0.0.1:9990")
    ap.add_argument("--top", type=int, default=3, help="alternatives shown per token (0..20)")
    ap.add_argument("text", nargs="?", default="the quick brown fox jumps over the lazy dog")
    args = ap.parse_args()
    lp = score(args.url, args.text, args.top)
    scored = [v for v in lp["token_logprobs"] if v is not None]
    for tok, v, top in zip(lp["tokens"], lp["token_logprobs"], lp["top_ids"]):
        best = "" if not top else "   best: " + ", ".join(f"{i} {p:.2f}" for i, p in top)
        print(f"{tok!r:>20} {'-' if v is None else format(v, '8.3f')}{best}")
    print(f"{len(scored)} scored tokens, sum {sum(scored):.3f}, perplexity {math.exp(-sum(scored) / max(1, len(scored))):.2f}")


if __name__ == "__main__":
    main()
