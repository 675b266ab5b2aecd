"""A short parallel-sampling client for dllama-api: asks for n answers to one prompt in one request
(one prefill on the server, choice i drawn with seed + i) and prints them with the majority answer.

  build/dllama-api --model <model.m> --tokenizer <tokenizer.t> --buffer-float-type q80 --slots 8 --port 9990 &
  python examples/parallel_sampling_client.py [--url http://127.0.0.1:9990] [--n 4] [--seed 1] [--stream] prompt
"""
import argparse
import collections
import json
import urllib.request


def _request(url, prompt, n, max_tokens, temperature, seed, stream):
    body = {"messages": [{"role": "user", "content": prompt}], "max_tokens": max_tokens, "temperature": temperature,
            "n": n, "stream": stream}
    if seed is not None:
        body["seed"] = seed
    req = urllib.request.Request(url + "/v1/chat/completions", data=json.dumps(body).encode(),
                                 headers={"Content-Type": "application/json"})
    return urllib.request.urlopen(req, timeout=300)


def ask(url, prompt, n=4, max_tokens=128, temperature=0.8, seed=None):
    """The n answers, ordered by choice index, and the usage (the prompt is counted once)."""
    d = json.loads(_request(url, prompt, n, max_tokens, temperature, seed, False).read())
    return [c["message"]["content"] for c in d["choices"]], d["usage"]


def ask_stream(url, prompt, n=4, max_tokens=128, temperature=0.8, seed=None):
    """The same from one multiplexed SSE stream: every chunk names its choice's index."""
    texts = [""] * n
    for raw in _request(url, prompt, n, max_tokens, temperature, seed, True):
        line = raw.decode().strip()
        if not line.startswith("data: ") or line == "data: [DONE]":
            continue
        ch = json.loads(line[6:])["choices"][0]
        texts[ch["index"]] += ch["delta"].get("content", "")
    return texts


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--url", default="http://127.0.0.1:9990")
    ap.add_argument("--n", type=int, default=4)
    ap.add_argument("--max-tokens", type=int, default=128)
    ap.add_argument("--temperature", type=float, default=0.8)
    ap.add_argument("--seed", type=int, default=None)
    ap.add_argument("--stream", action="store_true")
    ap.add_argument("prompt", nargs="?", default="What is 17 * 23? Answer with the number only.")
    args = ap.parse_args()
    if args.stream:
        texts = ask_stream(args.url, args.prompt, args.n, args.max_tokens, args.temperature, args.seed)
    else:
        texts, usage = ask(args.url, args.prompt, args.n, args.max_tokens, args.temperature, args.seed)
        print(f"usage: {usage['prompt_tokens']} prompt tokens (once) + {usage['completion_tokens']} completion tokens")
    for i, t in enumerate(texts):
        print(f"[{i}] {t}")
    best, votes = collections.Counter(t.strip() for t in texts).most_common(1)[0]
    print(f"majority ({votes}/{len(texts)}): {best}")


if __name__ == "__main__":
    main()
