"""Per-token log-probabilities (`logprobs` / `top_logprobs` of the chat API) on the CPU backend:
the host reference `logprobs_host`, `Backend.forward_logprobs`, and `dllama-api` (blocking, streamed,
validation, concurrent, with TCP workers).

Values are compared with numpy float64 `x - logsumexp(x)` of the same f32 logits at 1e-4 absolute:
an f32 tree sum over up to 2^17 terms is off by about 20 * 2^-24 relative (2e-6 in log space), the
fast exponential adds a few 2^-22, the rounding of `logit - lse` below magnitude 256 up to 1.5e-5;
1e-4 leaves several times that and is far below any gap a reader of these numbers cares about.
Token ids are compared exactly: a stable sort by (-logit, id)."""
import concurrent.futures
import json
import math
import subprocess
import time
import urllib.error
import urllib.request

import numpy as np
import pytest

from test_prefix_cache import DLLAMA, _free_port, _health, _start_api

TOL = 1e-4
SLOTS = 21  # the chosen token + 20 alternatives


def reference(x, k):
    """(float64 log_softmax of the f32 row, ids of its k best by (logit descending, id ascending))."""
    x = np.asarray(x, np.float32)
    x64 = x.astype(np.float64)
    m = x64.max()
    lp = x64 - (m + np.log(np.exp(x64 - m).sum()))
    return lp, np.argsort(-x, kind="stable")[:k]


def check_row(x, chosen, k, vals, ids, tol=TOL):
    """One row's 21 (logprob, id) slots against the reference."""
    lp, order = reference(x, k)
    assert ids[0] == chosen and abs(vals[0] - lp[chosen]) <= tol
    n = min(k, len(x))
    assert list(ids[1:1 + n]) == list(order[:n])
    assert np.abs(vals[1:1 + n] - lp[order[:n]]).max(initial=0) <= tol
    assert (ids[1 + n:] == -1).all()


# ---------------------------------------------------------------------------- logprobs_host

@pytest.mark.parametrize("k", [0, 1, 20])
@pytest.mark.parametrize("vocab", [50, 517, 32000])
def test_logprobs_host_matches_reference(C, vocab, k):
    rng = np.random.default_rng(vocab + k)
    x = (rng.standard_normal(vocab) * 6).astype(np.float32)
    x[rng.integers(0, vocab, 8)] = x.max()  # ties at the top: lowest id first
    chosen = int(rng.integers(0, vocab))
    vals, ids = C.cpu_ops.logprobs_host(x, chosen, k)
    assert vals.shape == (SLOTS,) and ids.shape == (SLOTS,)
    check_row(x, chosen, k, vals, ids)


def test_logprobs_host_k_beyond_vocabulary(C):
    x = np.asarray([0.5, -1, 3, 3, 0, 2, -7], np.float32)
    vals, ids = C.cpu_ops.logprobs_host(x, 4, 20)
    assert list(ids[:8]) == [4, 2, 3, 5, 0, 4, 1, 6] and (ids[8:] == -1).all()
    check_row(x, 4, 20, vals, ids)
    assert abs(np.exp(vals[1:8].astype(np.float64)).sum() - 1) < 1e-5


# ---------------------------------------------------------------------------- Backend.forward_logprobs

def _backend(C, assets):
    return C.cpu_backend(assets["q40"], "q80", 2, 128, 64, 3)


def _forward_logprobs_cases(make):
    """Shared with the GPU test: `make()` builds a backend / engine with 3 slots. A decode row, then a
    4-row chunk with an unsampled row, two sampled rows with requests and a sampled row without."""
    rng = np.random.default_rng(3)
    prompt = [int(t) for t in rng.integers(0, 500, 6)]
    be = make()
    be.forward(prompt, list(range(6)), [0] * 6)
    logits = be.forward([17], [6], [0])
    ids, vals, top = be.forward_logprobs([17], [6], [0], [0.0], [0.9], [0.3], [20])
    assert ids == be.forward_sample([17], [6], [0], [0.0], [0.9], [0.3]) == [int(np.argmax(logits[0]))]
    assert vals.shape == (1, SLOTS) and top.shape == (1, SLOTS) and vals.dtype == np.float32
    check_row(logits[0], ids[0], 20, vals[0], top[0])
    assert top[0, 1] == ids[0] and vals[0, 1] == vals[0, 0]  # greedy: the chosen token is the best one

    toks, pos, slots = prompt[:4], [0, 1, 2, 3], [1] * 4
    temps, topps, coins, req = [-1.0, 0.0, 0.8, 0.7], [0.9, 0.9, 0.9, 1.0], [0.1, 0.2, 0.63, 0.4], [-1, 5, 20, -1]
    logits = be.forward(toks, pos, slots)
    ids, vals, top = be.forward_logprobs(toks, pos, slots, temps, topps, coins, req)
    assert ids == be.forward_sample(toks, pos, slots, temps, topps, coins)
    assert ids[0] == -1 and all(i >= 0 for i in ids[1:])
    assert (top[0] == -1).all() and (top[3] == -1).all()  # not sampled / no request
    check_row(logits[1], ids[1], 5, vals[1], top[1])
    check_row(logits[2], ids[2], 20, vals[2], top[2])
    # no row asks: nothing is computed, every slot is empty
    ids2, _, top2 = be.forward_logprobs(toks, pos, slots, temps, topps, coins, [-1] * 4)
    assert ids2 == ids and (top2 == -1).all()


def test_cpu_backend_forward_logprobs(C, assets):
    _forward_logprobs_cases(lambda: _backend(C, assets))


# ---------------------------------------------------------------------------- dllama-api

PROMPTS = ["the quick brown fox", "hello world this is", "tell me about the end of", "one two three four five"]


def _post(url, content, max_tokens=10, **kw):
    body = {"messages": [{"role": "user", "content": content}], "max_tokens": max_tokens, "temperature": 0}
    body.update(kw)
    req = urllib.request.Request(url + "/v1/chat/completions", data=json.dumps(body).encode(),
                                 headers={"Content-Type": "application/json"})
    return urllib.request.urlopen(req, timeout=60)


def _chat(url, content, max_tokens=10, **kw):
    return json.loads(_post(url, content, max_tokens, **kw).read())


def _stream(url, content, max_tokens=10, **kw):
    """(text, log-probability records, finish_reason) of a streamed request."""
    text, recs, finish = "", [], None
    for raw in _post(url, content, max_tokens, stream=True, **kw):
        line = raw.decode().strip()
        if not line.startswith("data: ") or line == "data: [DONE]":
            continue
        ch = json.loads(line[6:])["choices"][0]
        text += ch["delta"].get("content", "")
        if ch["logprobs"] is not None:
            recs += ch["logprobs"]["content"]
        finish = ch["finish_reason"] or finish
    return text, recs, finish


def _content(d):
    return d["choices"][0]["logprobs"]["content"]


def check_response(d, k, tok, greedy):
    """Shape and self-consistency of a response's records."""
    content = _content(d)
    assert len(content) == d["usage"]["completion_tokens"] > 0
    for e in content:
        assert set(e) == {"token", "token_id", "logprob", "bytes", "top_logprobs"}
        assert e["logprob"] <= 0
        top = e["top_logprobs"]
        assert len(top) == k
        assert all(a["logprob"] >= b["logprob"] for a, b in zip(top, top[1:]))
        assert sum(math.exp(t["logprob"]) for t in top) <= 1 + 1e-4
        for t in [e] + top:
            piece = tok.piece(t["token_id"])
            assert bytes(t["bytes"]) == piece
            assert t["token"] == piece.decode("utf-8", errors="replace")
        assert e["logprob"] <= top[0]["logprob"] if k else True
        if greedy and k:
            assert {x: e[x] for x in ("token_id", "logprob")} == {x: top[0][x] for x in ("token_id", "logprob")}
        if k:
            assert len({t["token_id"] for t in top}) == k


@pytest.fixture(scope="module")
def api(assets):
    proc, url = _start_api(assets["q40"], assets["tok"])
    yield url
    proc.kill()
    proc.wait()


@pytest.fixture(scope="module")
def tok(C, assets):
    return C.Tokenizer(assets["tok"])


@pytest.mark.parametrize("k", [0, 5, 20])
def test_api_logprobs_shape_greedy(api, tok, k):
    d = _chat(api, PROMPTS[0], logprobs=True, top_logprobs=k)
    check_response(d, k, tok, greedy=True)


def test_api_logprobs_without_top_logprobs(api, tok):
    d = _chat(api, PROMPTS[1], logprobs=True)
    check_response(d, 0, tok, greedy=True)


def test_api_logprobs_null_when_not_requested(api):
    assert _chat(api, PROMPTS[0])["choices"][0]["logprobs"] is None
    assert _chat(api, PROMPTS[0], logprobs=False)["choices"][0]["logprobs"] is None
    text, recs, _ = _stream(api, PROMPTS[0])
    assert text and recs == []


@pytest.mark.parametrize("sampling", [dict(temperature=0), dict(temperature=0.9, top_p=0.8, seed=11),
                                      dict(temperature=1.3, top_p=1.0, seed=5)])
def test_api_logprobs_do_not_change_the_text(api, tok, sampling):
    plain = _chat(api, PROMPTS[2], 16, **sampling)
    with_lp = _chat(api, PROMPTS[2], 16, logprobs=True, top_logprobs=3, **sampling)
    assert with_lp["generated_text"] == plain["generated_text"]
    assert with_lp["usage"] == plain["usage"]
    check_response(with_lp, 3, tok, greedy=sampling["temperature"] == 0)


def test_api_logprobs_streamed_equal_blocking(api):
    for kw in (dict(temperature=0), dict(temperature=0.9, top_p=0.8, seed=3)):
        d = _chat(api, PROMPTS[3], 12, logprobs=True, top_logprobs=4, **kw)
        text, recs, finish = _stream(api, PROMPTS[3], 12, logprobs=True, top_logprobs=4, **kw)
        assert text == d["generated_text"] and finish == d["choices"][0]["finish_reason"]
        assert recs == _content(d)


@pytest.mark.parametrize("bad", [dict(logprobs=True, top_logprobs=21), dict(logprobs=True, top_logprobs=-1),
                                 dict(logprobs=True, top_logprobs="3"), dict(logprobs=True, top_logprobs=2.5),
                                 dict(top_logprobs=3), dict(logprobs=False, top_logprobs=3)])
def test_api_logprobs_validation(api, bad):
    with pytest.raises(urllib.error.HTTPError) as e:
        _chat(api, PROMPTS[0], **bad)
    assert e.value.code == 400 and "error" in json.loads(e.value.read())


def assert_same_records(got, want):
    """Records equal exactly; the first difference is named."""
    assert len(got) == len(want)
    for i, (g, w) in enumerate(zip(got, want)):
        assert (g["token_id"], g["logprob"]) == (w["token_id"], w["logprob"]), i
        assert [(t["token_id"], t["logprob"]) for t in g["top_logprobs"]] == \
            [(t["token_id"], t["logprob"]) for t in w["top_logprobs"]], i
    assert got == want


SAMPLING = [dict(temperature=0), dict(temperature=0.8, top_p=0.9, seed=2), dict(temperature=0), dict(temperature=1.1, seed=9)]


def concurrent_equal_solo(api, kw=SAMPLING, records=True):
    """4 requests with logprobs next to 4 without, over 4 slots: the records (records=False: only
    the texts) and texts are those of the same requests served alone."""
    solo_lp = [_chat(api, p, 14, logprobs=True, top_logprobs=5, **k) for p, k in zip(PROMPTS, kw)]
    solo_plain = [_chat(api, p, 14, **k) for p, k in zip(PROMPTS, kw)]
    with concurrent.futures.ThreadPoolExecutor(8) as ex:
        f_lp = [ex.submit(_chat, api, p, 14, logprobs=True, top_logprobs=5, **k) for p, k in zip(PROMPTS, kw)]
        f_plain = [ex.submit(_chat, api, p, 14, **k) for p, k in zip(PROMPTS, kw)]
        got_lp, got_plain = [f.result() for f in f_lp], [f.result() for f in f_plain]
    for g, s in zip(got_lp, solo_lp):
        assert g["generated_text"] == s["generated_text"]
        if records:
            assert_same_records(_content(g), _content(s))
    for g, s, l in zip(got_plain, solo_plain, solo_lp):
        assert g["generated_text"] == s["generated_text"] == l["generated_text"]
        assert g["choices"][0]["logprobs"] is None


def test_api_logprobs_concurrent_equal_solo(api):
    concurrent_equal_solo(api)  # (the CPU backend computes a row independently of its batch)


# ---------------------------------------------------------------------------- TCP workers

def test_api_logprobs_over_tcp_workers(C, tmp_path_factory):
    """Root + 2 `dllama worker` processes: the root scores the gathered logits, the workers take no
    part. Tensor parallelism is not bitwise the single process, so shape and self-consistency only."""
    from distributed_llama_multiusers_amd.models.synthetic import make_test_assets
    from distributed_llama_multiusers_amd.utils.mfile import FloatType
    d = str(tmp_path_factory.mktemp("kv3_logprobs"))
    model, tpath, _ = make_test_assets(d, "tiny", FloatType.Q40, seq_len=128, seed=7, dim=384, n_heads=6, n_kv_heads=3,
                                       hidden_dim=768, vocab_size=510)
    ports = [_free_port() for _ in range(2)]
    procs = [subprocess.Popen([DLLAMA, "worker", "--port", str(p), "--nthreads", "1"], stdout=subprocess.PIPE,
                              stderr=subprocess.STDOUT) for p in ports]
    try:
        time.sleep(0.2)
        tp, url = _start_api(model, tpath, ("--sync-type", "f32", "--workers", *[f"127.0.0.1:{p}" for p in ports]))
        procs.append(tp)
        assert _health(url)["nodes"] == 3
        tok = C.Tokenizer(tpath)
        plain = _chat(url, PROMPTS[0], 12)
        d = _chat(url, PROMPTS[0], 12, logprobs=True, top_logprobs=20)
        check_response(d, 20, tok, greedy=True)
        assert d["generated_text"] == plain["generated_text"]
        s = _chat(url, PROMPTS[1], 12, logprobs=True, top_logprobs=2, temperature=0.9, seed=4)
        check_response(s, 2, tok, greedy=False)
        text, recs, _ = _stream(url, PROMPTS[1], 12, logprobs=True, top_logprobs=2, temperature=0.9, seed=4)
        assert text == s["generated_text"] and recs == _content(s)
        for w in procs[:2]:
            assert w.poll() is None
    finally:
        for p in procs:
            p.kill()
        logs = [p.communicate()[0].decode(errors="replace") for p in procs]
    for l in logs[:2]:
        assert "Worker error" not in l, l
