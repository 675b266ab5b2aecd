"""Parallel sampling (`n` of /v1/chat/completions) on the CPU backend: the choices are the members of
one scheduler group (Scheduler::submitGroup) that share one prefill: the leader prefills the prompt,
the followers start behind Backend.fork_prefix at the prompt's last row. Choice i must be the solo
request with seed + i (the CPU backend's rows are batch-independent), the prompt is prefilled once,
and the fork command reaches TCP workers."""
import concurrent.futures
import json
import socket
import subprocess
import threading
import time
import urllib.error
import urllib.request

import numpy as np
import pytest

from test_prefix_cache import DLLAMA, PREFIX_FLAGS, _free_port, _health, _start_api

CONTENT = "tell me about the world and the end of it"
LONG = "the quick brown fox jumps over the lazy dog and then it runs to the end of the context"
SEED, TEMP = 7, 0.8


def _post(url, content=CONTENT, max_tokens=10, **kw):
    body = {"messages": [{"role": "user", "content": content}], "max_tokens": max_tokens, "temperature": TEMP, "seed": SEED}
    body.update(kw)
    req = urllib.request.Request(url + "/v1/chat/completions", data=json.dumps(body).encode(),
                                 headers={"Content-Type": "application/json"})
    return urllib.request.urlopen(req, timeout=60)


def _chat(url, **kw):
    return json.loads(_post(url, **kw).read())


def _texts(d):
    assert [c["index"] for c in d["choices"]] == list(range(len(d["choices"])))
    return [c["message"]["content"] for c in d["choices"]]


def _solos(url, n, **kw):
    """The solo requests choice 0..n-1 must equal: the same fields, seed SEED + i."""
    return [_chat(url, seed=SEED + i, **kw) for i in range(n)]


def _stream_choices(url, **kw):
    """A streamed request by choice index: (texts, roles of each index's first chunk, finish_reason
    chunks per index, log-probability records per index, number of [DONE] lines)."""
    text, first_role, finishes, recs, done = {}, {}, {}, {}, 0
    for raw in _post(url, stream=True, **kw):
        line = raw.decode().strip()
        if not line.startswith("data: "):
            continue
        if line == "data: [DONE]":
            done += 1
            continue
        assert done == 0  # nothing follows [DONE]
        (ch,) = json.loads(line[6:])["choices"]
        i = ch["index"]
        first_role.setdefault(i, ch["delta"].get("role"))
        text[i] = text.get(i, "") + ch["delta"].get("content", "")
        if ch["logprobs"]:
            recs.setdefault(i, []).extend(ch["logprobs"]["content"])
        if ch["finish_reason"] is not None:
            finishes.setdefault(i, []).append(ch["finish_reason"])
    return text, first_role, finishes, recs, done


@pytest.fixture(scope="module")
def srv(assets):
    proc, url = _start_api(assets["q40"], assets["tok"])
    yield url
    proc.kill()
    proc.wait()


# ---------------------------------------------------------------------------- choices and usage

def test_n_returns_that_many_choices(srv):
    d = _chat(srv, n=3)
    assert len(d["choices"]) == 3 and [c["index"] for c in d["choices"]] == [0, 1, 2]
    assert all(c["message"]["role"] == "assistant" and c["finish_reason"] in ("stop", "length") for c in d["choices"])


def test_choices_equal_solo_requests_and_usage(srv):
    d = _chat(srv, n=3)
    solo = _solos(srv, 3)
    assert _texts(d) == [s["generated_text"] for s in solo]
    assert len(set(_texts(d))) > 1  # the seeds differ: so do the draws
    assert d["generated_text"] == d["choices"][0]["message"]["content"]
    assert d["usage"]["prompt_tokens"] == solo[0]["usage"]["prompt_tokens"]
    assert d["usage"]["completion_tokens"] == sum(s["usage"]["completion_tokens"] for s in solo)
    assert d["usage"]["total_tokens"] == d["usage"]["prompt_tokens"] + d["usage"]["completion_tokens"]
    assert d["usage"]["prompt_tokens_details"]["cached_tokens"] == 0


def test_greedy_choices_all_equal_the_solo_answer(srv):
    d = _chat(srv, n=3, temperature=0)
    want = _chat(srv, temperature=0)["generated_text"]
    assert _texts(d) == [want] * 3


def test_prompt_is_prefilled_once(srv):
    """P + 2 prompt rows for three choices (the leader's P, one row per follower) where three requests
    cost 3 P; the fork counters move, the prefix-cache counters do not."""
    h0 = _health(srv)
    d = _chat(srv, n=3)
    h1 = _health(srv)
    P = d["usage"]["prompt_tokens"]
    delta = lambda k: h1[k] - h0[k]
    assert P > 8
    assert delta("prefill_rows") == P + 2
    assert delta("fork_groups") == 1 and delta("forked_requests") == 2 and delta("fork_tokens") == 2 * (P - 1)
    assert delta("prefix_hits") == 0 and delta("prefix_tokens") == 0 and delta("prefix_copies") == 0
    assert delta("completed") == 3 and h1["active"] == 0 and h1["queued"] == 0
    vals = dict(l.split() for l in urllib.request.urlopen(srv + "/v1/metrics").read().decode().splitlines()
                if l and not l.startswith("#"))
    assert float(vals["dllama_fork_groups_total"]) == h1["fork_groups"]
    assert float(vals["dllama_forked_requests_total"]) == h1["forked_requests"]
    assert float(vals["dllama_fork_tokens_total"]) == h1["fork_tokens"]


def test_streaming_multiplexes_the_choices(srv):
    text, first_role, finishes, _, done = _stream_choices(srv, n=2)
    assert sorted(text) == [0, 1]
    assert first_role == {0: "assistant", 1: "assistant"}
    assert {i: len(f) for i, f in finishes.items()} == {0: 1, 1: 1} and done == 1
    assert [text[0], text[1]] == _texts(_chat(srv, n=2))


def test_logprobs_per_choice(srv):
    d = _chat(srv, n=2, logprobs=True, top_logprobs=2, max_tokens=12)
    solo = _solos(srv, 2, logprobs=True, top_logprobs=2, max_tokens=12)
    for c, s in zip(d["choices"], solo):
        content = c["logprobs"]["content"]
        want = s["choices"][0]["logprobs"]["content"]
        assert len(content) == s["usage"]["completion_tokens"] and len(content) == len(want)
        assert [e["token_id"] for e in content] == [e["token_id"] for e in want]
        assert all(len(e["top_logprobs"]) == 2 for e in content)
    _, _, _, recs, _ = _stream_choices(srv, n=2, logprobs=True, top_logprobs=2, max_tokens=12)
    for i in (0, 1):
        assert [e["token_id"] for e in recs[i]] == [e["token_id"] for e in d["choices"][i]["logprobs"]["content"]]


def test_n_validation(srv):
    slots = _health(srv)["slots"]
    for bad in (0, -1, 1.5, "2", slots + 1):
        with pytest.raises(urllib.error.HTTPError) as e:
            _post(srv, n=bad)
        assert e.value.code == 400
        msg = json.loads(e.value.read())["error"]
        assert "n must be an integer from 1 to" in msg and str(slots) in msg
    for one in (1, None):
        assert len(_chat(srv, n=one)["choices"]) == 1
    assert len(_chat(srv, n=slots)["choices"]) == slots


# ---------------------------------------------------------------------------- followers that wait

def _hold_a_slot(url, ex, max_tokens=60):
    """A long solo streaming request that has started decoding: (future of its text)."""
    started = threading.Event()

    def run():
        text = ""
        try:
            for raw in _post(url, LONG, max_tokens, stream=True, temperature=0):
                line = raw.decode().strip()
                if line.startswith("data: ") and line != "data: [DONE]":
                    started.set()
                    text += json.loads(line[6:])["choices"][0]["delta"].get("content", "")
        finally:
            started.set()
        return text

    f = ex.submit(run)
    assert started.wait(60)
    return f


def _waiting_followers(assets, extra):
    """--slots 3 with one slot held by a long request: the third member of an n: 3 group finds no slot
    when the others join and forks later (or, once no member is left, prefills for itself)."""
    proc, url = _start_api(assets["q40"], assets["tok"], ("--slots", "3", *extra))
    try:
        assert _health(url)["slots"] == 3
        want_long = _chat(url, content=LONG, max_tokens=60, temperature=0)["generated_text"]
        want = [s["generated_text"] for s in _solos(url, 3, max_tokens=16)]
        with concurrent.futures.ThreadPoolExecutor(2) as ex:
            long_f = _hold_a_slot(url, ex)
            d = _chat(url, n=3, max_tokens=16)
            assert long_f.result() == want_long
        assert _texts(d) == want
        h = _health(url)
        assert h["active"] == 0 and h["queued"] == 0 and h["forked_requests"] >= 1, h
        return h
    finally:
        proc.kill()
        out = proc.communicate()[0].decode(errors="replace")
    assert "exhausted" not in out, out


def test_followers_wait_for_a_slot(assets):
    _waiting_followers(assets, ())


def test_followers_wait_with_kv_pages_flags(assets):
    """The same under --kv-pages / --kv-page-size. Only the HIP engine pages its cache (the CPU backend
    reports none, so the scheduler reserves no pages here): the page accounting itself is exercised on
    the GPU, in test_gpu_parallel_sampling.py."""
    _waiting_followers(assets, ("--kv-pages", "6", "--kv-page-size", "32"))


def test_with_prefix_cache(assets, srv):
    proc, url = _start_api(assets["q40"], assets["tok"], PREFIX_FLAGS)
    try:
        want = _texts(_chat(srv, n=3))
        d = _chat(url, n=3)
        assert _texts(d) == want
        h = _health(url)
        assert h["prefix_hits"] == 0 and h["forked_requests"] == 2
        again = _chat(url)  # an identical solo request afterwards: the members' slots hold its prompt
        assert again["generated_text"] == want[0]
        assert again["usage"]["prompt_tokens_details"]["cached_tokens"] == again["usage"]["prompt_tokens"] - 1
        assert _health(url)["prefix_hits"] == 1
    finally:
        proc.kill()
        proc.wait()


@pytest.mark.parametrize("fields", [dict(response_format={"type": "json_object"}), dict(frequency_penalty=1.0)],
                         ids=["json_object", "frequency_penalty"])
def test_followers_start_with_fresh_slot_state(srv, fields):
    """Penalty counts and the JSON state are per slot: a follower's first drawn row resets its own
    slot's, or it would continue whatever request used the slot before."""
    _chat(srv, n=3, max_tokens=16, frequency_penalty=1.5, response_format={"type": "json_object"})  # soil the slots
    d = _chat(srv, n=2, max_tokens=16, **fields)
    assert _texts(d) == [s["generated_text"] for s in _solos(srv, 2, max_tokens=16, **fields)]


def test_client_disconnect_cancels_every_member(srv):
    h0 = _health(srv)
    host, port = srv.split("//")[1].split(":")
    body = json.dumps({"messages": [{"role": "user", "content": LONG}], "max_tokens": 0, "temperature": TEMP, "seed": SEED,
                       "stream": True, "n": 3}).encode()
    sock = socket.create_connection((host, int(port)), timeout=30)
    sock.sendall(b"POST /v1/chat/completions HTTP/1.1\r\nHost: x\r\nContent-Type: application/json\r\n"
                 b"Content-Length: " + str(len(body)).encode() + b"\r\n\r\n" + body)
    assert b"200" in sock.recv(64)  # response started: generation is under way
    sock.setsockopt(socket.SOL_SOCKET, socket.SO_LINGER, b"\x01\x00\x00\x00\x00\x00\x00\x00")  # RST
    sock.close()
    for _ in range(400):
        h = _health(srv)
        if h["active"] == 0 and h["queued"] == 0 and h["cancelled"] + h["completed"] >= h0["cancelled"] + h0["completed"] + 3:
            break
        time.sleep(0.05)
    assert h["active"] == 0 and h["queued"] == 0, h
    # (a member may have reached its end before the hang-up was seen; none is left running)
    assert h["cancelled"] + h["completed"] == h0["cancelled"] + h0["completed"] + 3 and h["cancelled"] > h0["cancelled"], h
    assert len(_chat(srv, n=2, max_tokens=3)["choices"]) == 2


# ---------------------------------------------------------------------------- Backend.fork_prefix

_RNG = np.random.default_rng(11)
_P = [int(t) for t in _RNG.integers(0, 500, 40)]
_DEC = [int(t) for t in _RNG.integers(0, 500, 4)]
_Q = [int(t) for t in _RNG.integers(0, 500, 10)]


def _backend(C, assets):
    return C.cpu_backend(assets["q40"], "q80", 2, 128, 64, 4)


def _tail(be, n, slot):
    out = [be.forward(_P[n:], list(range(n, 40)), [slot] * (40 - n))]
    for i, t in enumerate(_DEC):
        out.append(be.forward([t], [40 + i], [slot]))
    return np.concatenate(out)


@pytest.mark.parametrize("n", [1, 17, 39])
def test_cpu_backend_fork_prefix_is_exact(C, assets, n):
    a = _backend(C, assets)
    a.forward(_P, list(range(40)), [0] * 40)
    a.forward(_Q, list(range(10)), [3] * 10)
    a.fork_prefix(0, [1, 2], n)
    b = _backend(C, assets)  # never forks: slot 0 the prompt, slot 3 the bystander
    b.forward(_P, list(range(40)), [0] * 40)
    b.forward(_Q, list(range(10)), [3] * 10)
    want = _tail(b, n, 0)  # decoding from n on the source itself
    assert np.array_equal(_tail(a, n, 1), want)
    assert np.array_equal(_tail(a, n, 2), want)
    assert np.array_equal(_tail(a, n, 0), want)
    assert np.array_equal(a.forward([9], [10], [3]), b.forward([9], [10], [3]))  # a slot not named


def test_cpu_backend_fork_prefix_rejects_bad_arguments(C, assets):
    be = _backend(C, assets)
    be.forward(_P, list(range(40)), [0] * 40)
    be.forward(_Q, list(range(10)), [1] * 10)
    before = be.forward([9], [10], [1]).copy()
    for src, dsts, n in [(0, [1, 1], 4), (0, [1, 0], 4), (0, [0], 4), (0, [1, 4], 4), (0, [1, -1], 4), (4, [1], 4),
                         (-1, [1], 4), (0, [], 4), (0, [1, 2], 0), (0, [1, 2], 128), (0, [1, 2], 500)]:
        with pytest.raises(RuntimeError):
            be.fork_prefix(src, dsts, n)
    # every check runs before the first copy: slot 1, named first in the refused calls, is as it was
    assert np.array_equal(be.forward([9], [10], [1]), before)


# ---------------------------------------------------------------------------- TCP workers

def test_n_over_tcp_workers(assets):
    """Cmd::FORK_PREFIX: root + 1 `dllama worker` with the exact f32 exchange; n: 2 equals the solos on
    the same server (so the worker's slots were forked like the root's)."""
    port = _free_port()
    worker = subprocess.Popen([DLLAMA, "worker", "--port", str(port), "--nthreads", "1"], stdout=subprocess.PIPE,
                              stderr=subprocess.STDOUT)
    procs = [worker]
    try:
        time.sleep(0.2)
        tp, url = _start_api(assets["q40"], assets["tok"], ("--sync-type", "f32", "--workers", f"127.0.0.1:{port}"))
        procs.append(tp)
        assert _health(url)["nodes"] == 2
        h0 = _health(url)
        d = _chat(url, n=2)
        h1 = _health(url)
        assert h1["forked_requests"] - h0["forked_requests"] == 1
        assert h1["prefill_rows"] - h0["prefill_rows"] == d["usage"]["prompt_tokens"] + 1
        assert _texts(d) == [s["generated_text"] for s in _solos(url, 2)]
        assert worker.poll() is None
    finally:
        for p in procs:
            p.kill()
        logs = [p.communicate()[0].decode(errors="replace") for p in procs]
    assert "Worker error" not in logs[0], logs[0]
