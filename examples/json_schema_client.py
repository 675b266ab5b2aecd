"""A short structured-output client for dllama-api: asks for a reply that follows a JSON schema and
parses it.

  build/dllama-api --model <model.m> --tokenizer <tokenizer.t> --buffer-float-type q80 --port 9990 &
  python examples/json_schema_client.py [--url http://127.0.0.1:9990] [--max-tokens 256] prompt

The server accepts OpenAI's strict subset (see the README): every property is required, in the
order of `properties`, and `additionalProperties` is false.
"""
import argparse
import json
import urllib.error
import urllib.request

SCHEMA = {
    "type": "object",
    "properties": {
        "city": {"type": "string", "maxLength": 40},
        "country": {"type": "string"},
        "population_millions": {"type": "number"},
        "coastal": {"type": "boolean"},
        "climate": {"enum": ["tropical", "dry", "temperate", "continental", "polar"]},
        "landmarks": {"type": "array", "items": {"type": "string"}, "minItems": 1, "maxItems": 3},
    },
    "required": ["city", "country", "population_millions", "coastal", "climate", "landmarks"],
    "additionalProperties": False,
}


def ask(url, prompt, max_tokens=256, temperature=0.7):
    body = {"messages": [{"role": "user", "content": prompt}], "max_tokens": max_tokens, "temperature": temperature,
            "response_format": {"type": "json_schema", "json_schema": {"name": "city", "strict": True, "schema": SCHEMA}}}
    req = urllib.request.Request(url + "/v1/chat/completions", data=json.dumps(body).encode(),
                                 headers={"Content-Type": "application/json"})
    try:
        choice = json.loads(urllib.request.urlopen(req, timeout=300).read())["choices"][0]
    except urllib.error.HTTPError as e:  # 400: the schema is outside the subset, and the message says why
        raise SystemExit(f"{e.code}: {json.loads(e.read())['error']}")
    return choice["message"]["content"], choice["finish_reason"]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--url", default="http://127.0.0.1:9990")
    ap.add_argument("--max-tokens", type=int, default=256)
    ap.add_argument("prompt", nargs="?", default="Describe Lisbon.")
    args = ap.parse_args()
    text, finish = ask(args.url, args.prompt, args.max_tokens)
    if finish == "stop":  # the object was closed: the text parses and has every key of the schema
        print(json.dumps(json.loads(text), indent=2, ensure_ascii=False))
    else:  # max_tokens or the context ended it first: a valid prefix
        print(f"(cut by {finish}) {text}")


if __name__ == "__main__":
    main()
