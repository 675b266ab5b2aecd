"""Prefix KV reuse (`--prefix-cache 1`) on the CPU backend: Backend.copy_prefix is a byte copy of a
slot's first n positions, the scheduler starts requests behind the longest prefix a slot already
holds (in place in an idle slot, through a copy when the holder is still active), and the texts stay
those of a server without the feature - also with the copy command relayed to TCP workers."""
import concurrent.futures
import json
import os
import socket
import subprocess
import threading
import time
import urllib.error
import urllib.request

import numpy as np
import pytest

from conftest import REPO

API = os.path.join(REPO, "build", "dllama-api")
DLLAMA = os.path.join(REPO, "build", "dllama")

# ---------------------------------------------------------------------------- Backend.copy_prefix

_RNG = np.random.default_rng(11)
_P = [int(t) for t in _RNG.integers(0, 500, 40)]    # the prompt whose prefix is copied
_DEC = [int(t) for t in _RNG.integers(0, 500, 4)]   # decode tokens fed after it
_Q = [int(t) for t in _RNG.integers(0, 500, 10)]    # a bystander sequence in slot 2


def _backend(C, assets):
    return C.cpu_backend(assets["q40"], "q80", 2, 128, 64, 3)


def _tail(be, n, slot):
    """Forward P[n:] as one chunk, then the 4 decode tokens, in `slot`: all logits."""
    out = [be.forward(_P[n:], list(range(n, 40)), [slot] * (40 - n))]
    for i, t in enumerate(_DEC):
        out.append(be.forward([t], [40 + i], [slot]))
    return np.concatenate(out)


@pytest.fixture(scope="module")
def untouched(C, assets):
    """A backend that never copies: the next decode row of slot 0 (P) and of slot 2 (Q)."""
    be = _backend(C, assets)
    be.forward(_P, list(range(40)), [0] * 40)
    be.forward(_Q, list(range(10)), [2] * 10)
    return be.forward([7], [40], [0]).copy(), be.forward([9], [10], [2]).copy()


@pytest.mark.parametrize("n", [1, 17, 39])
def test_cpu_backend_copy_prefix_is_exact(C, assets, untouched, n):
    a = _backend(C, assets)
    a.forward(_P, list(range(40)), [0] * 40)
    a.forward(_Q, list(range(10)), [2] * 10)
    a.copy_prefix(0, 1, n)
    got = _tail(a, n, 1)
    b = _backend(C, assets)
    b.forward(_P[:n], list(range(n)), [1] * n)
    want = _tail(b, n, 1)
    assert np.array_equal(got, want)
    # the source and the bystander slot are untouched
    assert np.array_equal(a.forward([7], [40], [0]), untouched[0])
    assert np.array_equal(a.forward([9], [10], [2]), untouched[1])


def test_cpu_backend_copy_prefix_rejects_bad_arguments(C, assets):
    be = _backend(C, assets)
    be.forward(_P, list(range(40)), [0] * 40)
    for src, dst, n in [(0, 0, 4), (0, 1, 0), (0, 1, 128), (0, 1, 500), (0, 3, 4), (3, 0, 4), (-1, 0, 4), (0, -1, 4)]:
        with pytest.raises(RuntimeError):
            be.copy_prefix(src, dst, n)


# ---------------------------------------------------------------------------- dllama-api

def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _start_api(model, tok, extra=()):
    port = _free_port()
    proc = subprocess.Popen([API, "--model", model, "--tokenizer", tok, "--buffer-float-type", "q80", "--port",
                             str(port), "--nthreads", "2", "--slots", "4", "--temperature", "0", "--max-seq-len", "128",
                             *extra], stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    url = f"http://127.0.0.1:{port}"
    for _ in range(400):
        try:
            urllib.request.urlopen(url + "/health", timeout=1).read()
            return proc, url
        except Exception:
            if proc.poll() is not None:
                break
            time.sleep(0.05)
    proc.kill()
    raise RuntimeError("server did not start: " + proc.stdout.read().decode(errors="replace"))


PREFIX_FLAGS = ("--prefix-cache", "1", "--prefix-cache-min", "4")


@pytest.fixture(scope="module")
def plain(assets):
    proc, url = _start_api(assets["q40"], assets["tok"])
    yield url
    proc.kill()
    proc.wait()


@pytest.fixture
def cached(assets):
    """A fresh server with prefix reuse per test: the first request of a test finds no record."""
    proc, url = _start_api(assets["q40"], assets["tok"], PREFIX_FLAGS)
    yield url
    proc.kill()
    proc.wait()


def _body(content, max_tokens, role="user", **kw):
    body = {"messages": [{"role": role, "content": content}], "max_tokens": max_tokens, "temperature": 0}
    body.update(kw)
    return json.dumps(body).encode()


def _chat(url, content, max_tokens=12, role="user"):
    req = urllib.request.Request(url + "/v1/chat/completions", data=_body(content, max_tokens, role),
                                 headers={"Content-Type": "application/json"})
    return json.loads(urllib.request.urlopen(req, timeout=60).read())


def _cached_tokens(d):
    return d["usage"]["prompt_tokens_details"]["cached_tokens"]


def _health(url):
    return json.loads(urllib.request.urlopen(url + "/health", timeout=10).read())


def _stream(url, content, max_tokens, started):
    """A streaming request; `started` is set at its first delta (its prompt is prefilled and it
    keeps decoding). Returns the whole text."""
    req = urllib.request.Request(url + "/v1/chat/completions", data=_body(content, max_tokens, stream=True),
                                 headers={"Content-Type": "application/json"})
    text = ""
    try:
        r = urllib.request.urlopen(req, timeout=60)
        for raw in r:
            line = raw.decode().strip()
            if not line.startswith("data: ") or line == "data: [DONE]":
                continue
            started.set()
            text += json.loads(line[6:])["choices"][0]["delta"].get("content", "")
    finally:
        started.set()
    return text


FAMILY_A = "the quick brown fox jumps over the lazy dog and then "
FAMILY_B = "hello world this is the other family of prompts with "
LONG = FAMILY_A + "it runs to the end of the context"                  # decodes until the context ends
SHORT = [f + s for s in ("one", "two and", "three") for f in (FAMILY_A, FAMILY_B)] + [FAMILY_A + "four"]


def _same_prompt_twice(url, plain_url, content):
    want = _chat(plain_url, content)["generated_text"]
    first = _chat(url, content)
    h1 = _health(url)
    second = _chat(url, content)
    h2 = _health(url)
    assert first["generated_text"] == want and second["generated_text"] == want
    assert _cached_tokens(first) == 0
    assert _cached_tokens(second) == second["usage"]["prompt_tokens"] - 1
    assert second["usage"]["prompt_tokens"] == first["usage"]["prompt_tokens"]
    assert h2["prefill_rows"] - h1["prefill_rows"] == 1
    assert h2["prefix_hits"] == 1 and h2["prefix_tokens"] == _cached_tokens(second) and h2["prefix_copies"] == 0


def _concurrent_families(url, plain_url, long_tokens=0):
    """One long request of family A first (long_tokens 0: to the end of the context); once it
    decodes, 7 more of both families at once over the 4 slots: the first of them find their prefix
    in the slot of a request that is still active."""
    want_long = _chat(plain_url, LONG, max_tokens=long_tokens)["generated_text"]
    want = [_chat(plain_url, p, max_tokens=16)["generated_text"] for p in SHORT]
    h0 = _health(url)
    started = threading.Event()
    with concurrent.futures.ThreadPoolExecutor(8) as ex:
        long_f = ex.submit(_stream, url, LONG, long_tokens, started)
        assert started.wait(60)
        got = list(ex.map(lambda p: _chat(url, p, max_tokens=16), SHORT))
        assert long_f.result() == want_long
    assert [g["generated_text"] for g in got] == want
    h = _health(url)
    assert h["prefix_copies"] - h0["prefix_copies"] >= 1, h
    assert h["completed"] - h0["completed"] == 8 and h["active"] == 0
    # (the streamed long request may have reused a few tokens itself; its chunks carry no usage)
    assert 0 < sum(_cached_tokens(g) for g in got) <= h["prefix_tokens"] - h0["prefix_tokens"]


def test_api_same_prompt_twice_prefills_one_row(cached, plain):
    _same_prompt_twice(cached, plain, "tell me about the world and the end of it")


def test_api_shared_leading_part(cached, plain):
    a, b = FAMILY_A + "alpha", FAMILY_A + "something else entirely"
    _chat(cached, a)
    d = _chat(cached, b)
    assert 0 < _cached_tokens(d) < d["usage"]["prompt_tokens"]
    assert d["generated_text"] == _chat(plain, b)["generated_text"]
    assert _chat(plain, b)["usage"]["prompt_tokens_details"]["cached_tokens"] == 0  # the feature is off there


def test_api_concurrent_families_copy_from_active_slot(cached, plain):
    _concurrent_families(cached, plain)


def test_api_more_prompts_than_slots_lru(cached, plain):
    """Six prompts that share less than the minimum (their roles differ right after the header
    token) over 4 slots, one after the other: each takes the least recently used idle slot, so the
    first prompt's record is gone when it comes again while the last one's is still there."""
    roles = ["alpha", "bravo", "charlie", "delta", "echo", "foxtrot"]
    text = "the world and the end of the world"
    want = [_chat(plain, text, role=r)["generated_text"] for r in roles]
    got = [_chat(cached, text, role=r) for r in roles]
    assert [g["generated_text"] for g in got] == want
    assert all(_cached_tokens(g) == 0 for g in got)
    again_first = _chat(cached, text, role=roles[0])
    again_last = _chat(cached, text, role=roles[-1])
    assert again_first["generated_text"] == want[0] and again_last["generated_text"] == want[-1]
    assert _cached_tokens(again_first) == 0
    assert _cached_tokens(again_last) == again_last["usage"]["prompt_tokens"] - 1
    h = _health(cached)
    assert h["completed"] == 8 and h["prefix_hits"] == 1 and h["prefix_evictions"] == 0


def test_metrics_expose_prefix_counters(cached):
    _chat(cached, "count me", max_tokens=2)
    _chat(cached, "count me", max_tokens=2)
    text = urllib.request.urlopen(cached + "/v1/metrics").read().decode()
    vals = dict(l.split() for l in text.splitlines() if l and not l.startswith("#"))
    assert float(vals["dllama_prefix_hits_total"]) == 1 and float(vals["dllama_prefix_tokens_total"]) >= 4
    assert float(vals["dllama_prefix_copies_total"]) == 0 and float(vals["dllama_prefix_evictions_total"]) == 0


# ---------------------------------------------------------------------------- TCP workers

@pytest.fixture(scope="module")
def kv3(tmp_path_factory):
    """3 KV heads: a root and two workers hold one each."""
    from distributed_llama_multiusers_amd.models.synthetic import make_test_assets
    from distributed_llama_multiusers_amd.utils.mfile import FloatType
    d = str(tmp_path_factory.mktemp("kv3"))
    m, t, _ = make_test_assets(d, "tiny", FloatType.Q40, seq_len=128, seed=7, dim=384, n_heads=6, n_kv_heads=3,
                               hidden_dim=768, vocab_size=510)
    return {"q40": m, "tok": t}


def test_prefix_cache_over_tcp_workers(kv3):
    """Cmd::COPY_PREFIX: every rank copies its own heads. Root + 2 `dllama worker` processes with the
    exact f32 exchange give the texts of a single-process server without the feature."""
    ports = [_free_port() for _ in range(2)]
    workers = [subprocess.Popen([DLLAMA, "worker", "--port", str(p), "--nthreads", "1"], stdout=subprocess.PIPE,
                                stderr=subprocess.STDOUT) for p in ports]
    procs = list(workers)
    try:
        time.sleep(0.2)
        solo, solo_url = _start_api(kv3["q40"], kv3["tok"])
        procs.append(solo)
        tp, tp_url = _start_api(kv3["q40"], kv3["tok"], ("--sync-type", "f32", *PREFIX_FLAGS, "--workers",
                                                          *[f"127.0.0.1:{p}" for p in ports]))
        procs.append(tp)
        assert _health(tp_url)["nodes"] == 3
        _same_prompt_twice(tp_url, solo_url, "tell me about the world and the end of it")
        # 40 tokens for the long request: the f32 exchange sums partials in rank order, which is not
        # bitwise one rank's accumulation; greedy texts agree over short continuations (as
        # test_distributed_cpu.py pins), while at 60 tokens plain tensor parallelism, without any
        # prefix reuse, already leaves the single-process text on this prompt
        _concurrent_families(tp_url, solo_url, long_tokens=40)
        for w in workers:
            assert w.poll() is None
    finally:
        for p in procs:
            p.kill()
        logs = [p.communicate()[0].decode(errors="replace") for p in procs]
    for l in logs[:2]:
        assert "Worker error" not in l, l
