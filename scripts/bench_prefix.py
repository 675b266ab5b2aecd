"""Prefix KV reuse, measured (profiles/prefix_cache.md):

  copy   HipEngine.copy_prefix on the Llama-3.1-8B shapes (32 layers x K,V x 8 KV heads x 128), n =
         256 / 2048 / 8192 positions, f32 and bf16 caches, contiguous and paged (256-position pages),
         as GB/s of bytes read + written, beside a device-to-device hipMemcpyAsync of the same byte
         count. Timed on the host around `iters` back-to-back copies between two stream syncs (the
         copies are asynchronous; a paged copy also uploads the page table, which is part of its cost).
  ttft   time to the first streamed token through dllama-api for a ~2048-token shared prefix plus a
         short distinct suffix, with and without --prefix-cache 1 (same box, same run).

  python scripts/bench_prefix.py [copy] [ttft] [--iters 20] [--reps 5]
"""
import argparse
import http.client
import json
import os
import socket
import statistics
import subprocess
import sys
import tempfile
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

H8B = dict(dim=4096, hidden_dim=14336, n_layers=32, n_heads=32, n_kv_heads=8, vocab_size=128256, seq_len=8448,
           rope_theta=500000, weight_type=2)


def bench_copy(iters):
    import distributed_llama_multiusers_amd as dl
    C = dl.native()
    rows = []
    for kv_bf16 in (False, True):
        for page in (0, 256):
            kw = dict(synthetic=H8B, max_seq_len=8448, n_slots=2, max_batch=8, kv_bf16=kv_bf16)
            if page:
                kw.update(kv_pages=2 * 8448 // page, kv_page_size=page)
            eng = C.HipEngine("", "q80", **kw)
            eng.forward([1], [8191], [0])  # slot 0 reaches 8192 positions (paged: its pages are mapped)
            for n in (256, 2048, 8192):
                nbytes = 32 * 2 * 8 * 128 * (2 if kv_bf16 else 4) * n
                for _ in range(3):
                    eng.copy_prefix(0, 1, n)
                eng.synchronize()
                t0 = time.perf_counter()
                for _ in range(iters):
                    eng.copy_prefix(0, 1, n)
                eng.synchronize()
                us = (time.perf_counter() - t0) / iters * 1e6
                ref = C.bench_memcpy_d2d(nbytes, iters)
                row = dict(kv="bf16" if kv_bf16 else "f32", layout=f"paged{page}" if page else "contiguous", n=n,
                           mib=round(nbytes / 2**20, 1), copy_us=round(us, 1), copy_gbs=round(2 * nbytes / us / 1e3, 1),
                           memcpy_us=round(ref, 1), memcpy_gbs=round(2 * nbytes / ref / 1e3, 1))
                rows.append(row)
                print(json.dumps(row), flush=True)
            del eng
    return rows


def _port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _ttft(port, content):
    """ms from sending the request to its first streamed chunk."""
    body = {"messages": [{"role": "user", "content": content}], "max_tokens": 4, "temperature": 0, "stream": True}
    c = http.client.HTTPConnection("127.0.0.1", port, timeout=300)
    t0 = time.perf_counter()
    c.request("POST", "/v1/chat/completions", json.dumps(body), {"Content-Type": "application/json"})
    r = c.getresponse()
    first = None
    while True:
        line = r.readline()
        if not line:
            break
        if line.startswith(b"data: ") and first is None:
            first = (time.perf_counter() - t0) * 1e3
    return first


def bench_ttft(reps):
    from distributed_llama_multiusers_amd.models.synthetic import make_tokenizer
    tmp = tempfile.mkdtemp()
    tok = os.path.join(tmp, "tok.t")
    make_tokenizer(tok, 128256)
    shared = " hello world the" * 341  # 6 tokens per repeat with the synthetic merges: ~2047 tokens
    out = {}
    for name, extra in (("plain", []), ("prefix_cache", ["--prefix-cache", "1"])):
        port = _port()
        cmd = [os.path.join(REPO, "build", "dllama-api"), "--synthetic", "llama3_1_8b", "--tokenizer", tok,
               "--gpu-index", "0", "--port", str(port), "--slots", "4", "--max-seq-len", "4096",
               "--buffer-float-type", "q80"] + extra
        log = open(os.path.join(tmp, name + ".log"), "w")
        srv = subprocess.Popen(cmd, stdout=log, stderr=subprocess.STDOUT)
        try:
            for _ in range(900):
                try:
                    c = http.client.HTTPConnection("127.0.0.1", port, timeout=2)
                    c.request("GET", "/health")
                    if c.getresponse().status == 200:
                        break
                except OSError:
                    pass
                if srv.poll() is not None:
                    raise RuntimeError("dllama-api exited: " + open(log.name).read()[-2000:])
                time.sleep(0.2)
            for i in range(3):  # untimed: graph capture, code objects; seeds the shared prefix
                _ttft(port, shared + f" warm {i} and the end of the world is not the end of it at all")

            def health():
                c = http.client.HTTPConnection("127.0.0.1", port, timeout=10)
                c.request("GET", "/health")
                return json.loads(c.getresponse().read())

            h0 = health()
            ms = [_ttft(port, shared + f" run {i} and the end of the world is not the end of it at all")
                  for i in range(reps)]
            h = health()
            if h["completed"] - h0["completed"] != reps:
                raise RuntimeError(f"requests failed: {h}")
            # ttft includes the host's tokenization of the prompt (the same on both servers);
            # forward_ms is the scheduler's time in forwards per request (prefill + 4 decode steps)
            out[name] = dict(ttft_ms=[round(m, 2) for m in ms], median_ms=round(statistics.median(ms), 2),
                             prefill_rows_per_request=(h["prefill_rows"] - h0["prefill_rows"]) / reps,
                             forward_ms_per_request=round((h["busy_ms"] - h0["busy_ms"]) / reps, 2),
                             prefix_hits=h.get("prefix_hits"), prefix_tokens=h.get("prefix_tokens"))
            print(name, json.dumps(out[name]), flush=True)
        finally:
            srv.terminate()
            try:
                srv.wait(timeout=30)
            except subprocess.TimeoutExpired:
                srv.kill()
            log.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("what", nargs="*", default=["copy", "ttft"])
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--reps", type=int, default=5)
    args = ap.parse_args()
    res = {}
    if "copy" in args.what:
        res["copy"] = bench_copy(args.iters)
    if "ttft" in args.what:
        res["ttft"] = bench_ttft(args.reps)
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
