"""Prefix KV reuse, measured (profiles/prefix_cache.md):

  copy   HipEngine.copy_prefix on the Llama-3.1-8B shapes (32 layers x K,V x 8 KV heads x 128), n =
         256 / 2048 / 8192 positions, f32 and bf16 caches, contiguous and paged (256-position pages),
         as GB/s of bytes read + written, beside a device-to-device hipMemcpyAsync of the same byte
         count. Timed on the host around `iters` back-to-back copies between two stream syncs (the
         copies are asynchronous; a paged copy also uploads the page table, which is part of its cost).
  ttft   time to the first streamed token through dllama-api for a ~2048-token shared prefix plus a
         short distinct suffix, with and without --prefix-cache 1 (same box, same run).
  fork   HipEngine.fork_prefix(0, [1..m], n) against m back-to-back copy_prefix(0, i, n) calls
         (profiles/parallel_sampling.md): the same shapes, n = 512 / 4096, m = 1 / 3 / 7, timed like
         `copy`, the two alternating `reps` times in one process; the copies' spread is reported.
  chat   one n = 4 chat request with a ~1k-token prompt against four concurrent single requests on
         the 8B synthetic model: wall time and the /health prefill_rows delta (--api: the server
         binary, so that another build can be measured by the same script).

  python scripts/bench_prefix.py [copy] [ttft] [fork] [chat] [--iters 20] [--reps 5] [--api build/dllama-api]
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


def bench_fork(iters, reps):
    import distributed_llama_multiusers_amd as dl
    C = dl.native()
    rows = []
    for kv_bf16 in (False, True):
        for page in (0, 256):
            kw = dict(synthetic=H8B, max_seq_len=4224, n_slots=8, max_batch=8, kv_bf16=kv_bf16)
            if page:
                kw.update(kv_pages=8 * 4352 // page, kv_page_size=page)
            eng = C.HipEngine("", "q80", **kw)
            eng.forward([1], [4095], [0])  # slot 0 reaches 4096 positions (paged: its pages are mapped)
            for n in (512, 4096):
                nbytes = 32 * 2 * 8 * 128 * (2 if kv_bf16 else 4) * n
                for m in (1, 3, 7):
                    dsts = list(range(1, m + 1))

                    def fork():
                        eng.fork_prefix(0, dsts, n)

                    def copies():
                        for d in dsts:
                            eng.copy_prefix(0, d, n)

                    def timed(f):
                        for _ in range(3):
                            f()
                        eng.synchronize()
                        t0 = time.perf_counter()
                        for _ in range(iters):
                            f()
                        eng.synchronize()
                        return (time.perf_counter() - t0) / iters * 1e6

                    fk, cp = [], []
                    for _ in range(reps):  # alternating, so that both see the same neighbours
                        cp.append(timed(copies))
                        fk.append(timed(fork))
                    f_us, c_us = statistics.median(fk), statistics.median(cp)
                    row = dict(kv="bf16" if kv_bf16 else "f32", layout=f"paged{page}" if page else "contiguous", n=n, m=m,
                               mib=round(nbytes / 2**20, 1), copies_us=round(c_us, 1),
                               copies_spread_us=round(max(cp) - min(cp), 1), fork_us=round(f_us, 1),
                               fork_spread_us=round(max(fk) - min(fk), 1), ratio=round(f_us / c_us, 3),
                               by_bytes=round((1 + m) / (2 * m), 3), fork_gbs=round((1 + m) * nbytes / f_us / 1e3, 1),
                               copies_gbs=round(2 * m * nbytes / c_us / 1e3, 1))
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


def bench_chat(api, reps):
    """Wall ms and prefill rows of one n = 4 request, and of four concurrent single requests."""
    import concurrent.futures
    from distributed_llama_multiusers_amd.models.synthetic import make_tokenizer
    tmp = tempfile.mkdtemp()
    tok = os.path.join(tmp, "tok.t")
    make_tokenizer(tok, 128256)
    port = _port()
    cmd = [api, "--synthetic", "llama3_1_8b", "--tokenizer", tok, "--gpu-index", "0", "--port", str(port), "--slots", "4",
           "--max-seq-len", "2048", "--buffer-float-type", "q80"]
    log = open(os.path.join(tmp, "chat.log"), "w")
    srv = subprocess.Popen(cmd, stdout=log, stderr=subprocess.STDOUT)

    def post(content, **kw):
        body = {"messages": [{"role": "user", "content": content}], "max_tokens": 16, "temperature": 0.8, "seed": 1}
        body.update(kw)
        c = http.client.HTTPConnection("127.0.0.1", port, timeout=300)
        c.request("POST", "/v1/chat/completions", json.dumps(body), {"Content-Type": "application/json"})
        return json.loads(c.getresponse().read())

    def health():
        c = http.client.HTTPConnection("127.0.0.1", port, timeout=10)
        c.request("GET", "/health")
        return json.loads(c.getresponse().read())

    out = {}
    try:
        for _ in range(900):
            try:
                health()
                break
            except OSError:
                pass
            if srv.poll() is not None:
                raise RuntimeError("dllama-api exited: " + open(log.name).read()[-2000:])
            time.sleep(0.2)
        shared = " hello world the" * 170  # ~1k tokens with the synthetic merges
        for i in range(2):  # untimed: code objects, graphs
            post(shared + f" warm {i}")
        with concurrent.futures.ThreadPoolExecutor(4) as ex:
            list(ex.map(lambda i: post(shared + " warm", seed=i), range(4)))
        for name in ("four_singles", "n4"):
            ms, rows, choices, ptoks = [], [], 0, 0
            for i in range(reps):
                content = shared + f" run {name} {i} and the end of the world"
                h0 = health()
                t0 = time.perf_counter()
                if name == "n4":
                    d = post(content, n=4)
                    choices = len(d["choices"])
                else:
                    with concurrent.futures.ThreadPoolExecutor(4) as ex:
                        ds = list(ex.map(lambda k: post(content, seed=1 + k), range(4)))
                    d, choices = ds[0], sum(len(x["choices"]) for x in ds)
                ms.append((time.perf_counter() - t0) * 1e3)
                rows.append(health()["prefill_rows"] - h0["prefill_rows"])
                ptoks = d["usage"]["prompt_tokens"]
            out[name] = dict(wall_ms=[round(x, 1) for x in ms], median_ms=round(statistics.median(ms), 1),
                             prefill_rows=rows, prompt_tokens=ptoks, choices=choices)
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
    ap.add_argument("--api", default=os.path.join(REPO, "build", "dllama-api"))
    args = ap.parse_args()
    res = {}
    if "copy" in args.what:
        res["copy"] = bench_copy(args.iters)
    if "ttft" in args.what:
        res["ttft"] = bench_ttft(args.reps)
    if "fork" in args.what:
        res["fork"] = bench_fork(args.iters, args.reps)
    if "chat" in args.what:
        res["chat"] = bench_chat(args.api, args.reps)
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
