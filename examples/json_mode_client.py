"""A short JSON-mode client for dllama-api: asks for a JSON object and parses the reply.

  build/dllama-api --model <model.m> --tokenizer <tokenizer.t> --buffer-float-type q80 --port 9990 &
  python examples/json_mode_client.py [--url http://127.0.0.1:9990] [--max-tokens 256] prompt
"""
import argparse
import json
import urllib.request


def ask(url, prompt, max_tokens=256, temperature=0.7):
    body = {"messages": [{"role": "system", "content": "Answer with a JSON object."}, {"role": "user", "content": prompt}],
            "max_tokens": max_tokens, "temperature": temperature, "response_format": {"type": "json_object"}}
    req = urllib.request.Request(url + "/v1/chat/completions", data=json.dumps(body).encode(),
                                 headers={"Content-Type": "application/json"})
    choice = json.loads(urllib.request.urlopen(req, timeout=300).read())["choices"][0]
    return choice["message"]["content"], choice["finish_reason"]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--url", default="http://127.0.0.1:9990")
    ap.add_argument("--max-tokens", type=int, default=256)
    ap.add_argument("prompt", nargs="?", default="Name three primary colours under the key \"colours\".")
    args = ap.parse_args()
    text, finish = ask(args.url, args.prompt, args.max_tokens)
    if finish == "stop":  # the object was closed: the text parses
        print(json.dumps(json.loads(text), indent=2))
    else:  # max_tokens or the context ended it first: a valid prefix
        print(f"(cut by {finish}) {text}")


if __name__ == "__main__":
    main()
