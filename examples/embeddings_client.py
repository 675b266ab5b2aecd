"""A short /v1/embeddings client for dllama-api: embeds a few texts in one request and prints their
cosine similarities (the vectors are L2-normalised, so a dot product).

  build/dllama-api --model <model.m> --tokenizer <tokenizer.t> --buffer-float-type q80 --port 9990 &
  python examples/embeddings_client.py [--url http://127.0.0.1:9990] [--pooling mean|last] text ...
"""
import argparse
import base64
import json
import struct
import urllib.request


def embed(url, texts, pooling="mean"):
    body = {"input": texts, "encoding_format": "base64", "pooling": pooling}
    req = urllib.request.Request(url + "/v1/embeddings", data=json.dumps(body).encode(),
                                 headers={"Content-Type": "application/json"})
    resp = json.loads(urllib.request.urlopen(req, timeout=300).read())
    vectors = []
    for item in sorted(resp["data"], key=lambda d: d["index"]):
        raw = base64.b64decode(item["embedding"])  # little-endian f32
        vectors.append(struct.unpack(f"<{len(raw) // 4}f", raw))
    return vectors, resp["usage"]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--url", default="http://127.0.0.1:9990")
    ap.add_argument("--pooling", default="mean", choices=["mean", "last"])
    ap.add_argument("texts", nargs="*", default=["the quick brown fox", "a fast auburn fox", "tensor parallelism"])
    args = ap.parse_args()
    vectors, usage = embed(args.url, args.texts, args.pooling)
    print(f"{len(vectors)} vectors of {len(vectors[0])} floats, {usage['prompt_tokens']} prompt tokens")
    for i, a in enumerate(vectors):
        print("  ".join(f"{sum(x * y for x, y in zip(a, b)):+.3f}" for b in vectors), " ", args.texts[i])


if __name__ == "__main__":
    main()
