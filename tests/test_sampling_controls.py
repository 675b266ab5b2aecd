"""`frequency_penalty`, `presence_penalty` and `logit_bias` of the chat API on the CPU backend: the
host reference `logit_proc_host`, the per-row processors of `Backend.forward_sample` /
`forward_logprobs`, and `dllama-api` (validation, forced and banned tokens, slot reuse, defaults).

The reference is numpy float32 applying OpenAI's formula one operation at a time (numpy does not
fuse); the arithmetic is specified exactly, so values are compared bitwise (`tobytes()`)."""
import json
import urllib.error

import numpy as np
import pytest

from test_logprobs import PROMPTS, _chat, _content
from test_prefix_cache import _start_api

F32 = np.float32


def np_proc(x, counts, presence, frequency, bias=None):
    """x[t] - frequency * float(c[t]) - presence where c[t] > 0, then + bias[t]: separate f32 steps."""
    x = np.asarray(x, F32)
    c = np.asarray(counts, np.uint32)
    y = x.copy()
    m = c > 0
    fc = F32(frequency) * c[m].astype(F32)
    assert fc.dtype == F32
    y[m] = x[m] - fc
    y[m] = y[m] - F32(presence)
    for t, v in (bias or {}).items():
        y[t] = y[t] + F32(v)
    assert y.dtype == F32
    return y


def proc_case(vocab, seed, n_bias):
    """(logits, counts with 0 / 1 / 70000 and more, bias over ids 0, vocab - 1 and a counted token)."""
    rng = np.random.default_rng(seed)
    x = (rng.standard_normal(vocab) * 6).astype(F32)
    x[rng.integers(0, vocab, 3)] = F32(-0.0)  # copied bit for bit where nothing applies
    c = np.where(rng.random(vocab) < 0.3, rng.integers(1, 40, vocab), 0).astype(np.uint32)
    c[vocab // 2] = 70000  # past 16 bits
    c[vocab // 3] = 1
    c[0] = 0
    ids = [0, vocab - 1, vocab // 2] + [int(t) for t in rng.permutation(np.arange(1, vocab - 1))]
    ids = list(dict.fromkeys(ids))[:min(n_bias, vocab)]
    bias = {t: float(F32(rng.uniform(-100, 100))) for t in ids}
    return x, c, bias


# ---------------------------------------------------------------------------- logit_proc_host

@pytest.mark.parametrize("pen", [(0.5, 1.5), (-2.0, -0.75), (0.0, 0.0), (0.3, 0.0), (0.0, 1.1)])
@pytest.mark.parametrize("vocab,n_bias", [(7, 0), (7, 3), (517, 300), (32000, 40)])
def test_logit_proc_host_matches_numpy(C, vocab, n_bias, pen):
    x, c, bias = proc_case(vocab, vocab + n_bias, n_bias)
    got = C.cpu_ops.logit_proc_host(x, c, pen[0], pen[1], list(bias), list(bias.values()))
    want = np_proc(x, c, pen[0], pen[1], bias)
    assert got.dtype == F32 and got.tobytes() == want.tobytes()
    untouched = (c == 0) & ~np.isin(np.arange(vocab), list(bias))
    assert got[untouched].tobytes() == x[untouched].tobytes()


# ---------------------------------------------------------------------------- Backend.forward_sample

PROMPT = [int(t) for t in np.random.default_rng(21).integers(0, 500, 6)]


def penalties_loop(be, logits_of, steps, presence, frequency, slot=0, bias=None, fresh_first=True):
    """Greedy steps of one sequence in `slot` behind PROMPT with a processor on every step; every id
    must be the lowest-index argmax of the numpy-processed logits `logits_of(token, pos)` gives for
    the same row, with the counts kept here. Returns the ids."""
    vocab = None
    tok, pos, ids, counts = PROMPT[-1], len(PROMPT) - 1, [], None
    for s in range(steps):
        raw = logits_of(tok, pos)
        if counts is None:
            vocab = raw.shape[0]
            counts = np.zeros(vocab, np.uint32)
        proc = dict(presence=presence, frequency=frequency, fresh=fresh_first and s == 0)
        if proc["fresh"]:
            proc["bias"] = bias or {}
        got = be.forward_sample([tok], [pos], [slot], [0.0], [0.9], [0.0], logit_procs=[proc])
        want = int(np.argmax(np_proc(raw, counts, presence, frequency, bias)))
        assert got == [want], (s, got, want)
        counts[want] += 1
        ids.append(want)
        tok, pos = want, pos + 1
    return ids


def run_penalties_loop(make, steps=24):
    """Shared with the GPU test: `make()` builds a backend / engine with 3 slots."""
    be = make()
    be.forward(PROMPT[:-1], list(range(len(PROMPT) - 1)), [0] * (len(PROMPT) - 1))
    ids = penalties_loop(be, lambda t, p: be.forward([t], [p], [0])[0], steps, 0.5, 1.5)
    # both penalties at 0 and no bias: the plain greedy ids
    plain = make()
    plain.forward(PROMPT[:-1], list(range(len(PROMPT) - 1)), [0] * (len(PROMPT) - 1))
    tok, pos, want = PROMPT[-1], len(PROMPT) - 1, []
    for s in range(steps):
        want += plain.forward_argmax([tok], [pos], [0])
        tok, pos = want[-1], pos + 1
    zero = make()
    zero.forward(PROMPT[:-1], list(range(len(PROMPT) - 1)), [0] * (len(PROMPT) - 1))
    assert penalties_loop(zero, lambda t, p: zero.forward([t], [p], [0])[0], steps, 0.0, 0.0) == want
    return be, ids


def _backend(C, assets):
    return C.cpu_backend(assets["q40"], "q80", 2, 128, 64, 3)


def test_cpu_backend_penalties_loop(C, assets):
    run_penalties_loop(lambda: _backend(C, assets))


def test_cpu_backend_slot_reuse_starts_from_zero_counts(C, assets):
    """A second generation in the same slot (its first row marked fresh) sees all-zero counts and
    the bias it brings, not the first one's."""
    be, ids = run_penalties_loop(lambda: _backend(C, assets), steps=8)
    n = len(PROMPT) - 1
    be.forward(PROMPT[:-1], list(range(n)), [0] * n)
    again = penalties_loop(be, lambda t, p: be.forward([t], [p], [0])[0], 8, 0.5, 1.5)
    assert again == ids
    be.forward(PROMPT[:-1], list(range(n)), [0] * n)
    banned = penalties_loop(be, lambda t, p: be.forward([t], [p], [0])[0], 4, 0.5, 1.5, bias={ids[0]: -100.0})
    assert banned[0] != ids[0]


def test_cpu_backend_forced_token_and_raw_logprobs(C, assets):
    """{t: 100} forces t; the log-probabilities score the raw logits, so the top entry is the raw best."""
    be = _backend(C, assets)
    n = len(PROMPT) - 1
    be.forward(PROMPT[:-1], list(range(n)), [0] * n)
    raw = be.forward([PROMPT[-1]], [n], [0])[0]
    plain = be.forward_logprobs([PROMPT[-1]], [n], [0], [0.0], [0.9], [0.0], [2])
    t = 123
    ids, vals, top = be.forward_logprobs([PROMPT[-1]], [n], [0], [0.0], [0.9], [0.0], [2],
                                         logit_procs=[dict(fresh=True, bias={t: 100.0})])
    assert ids == [t] and plain[0] == [int(np.argmax(raw))] != [t]
    assert top[0, 0] == t and top[0, 1] == plain[2][0, 1] and vals[0, 0] < vals[0, 1]
    assert vals[0, 1:].tobytes() == plain[1][0, 1:].tobytes() and top[0, 1:].tobytes() == plain[2][0, 1:].tobytes()


def test_cpu_backend_rejects_bad_processors(C, assets):
    be = _backend(C, assets)
    args = ([3], [0], [0], [0.0], [0.9], [0.0])
    for bias in ({512: 1.0}, {-1: 1.0}, {i: 1.0 for i in range(301)}):
        with pytest.raises(RuntimeError):
            be.forward_sample(*args, logit_procs=[dict(fresh=True, bias=bias)])
    with pytest.raises(RuntimeError):
        be.forward_sample(*args, logit_procs=[None, None])
    assert be.forward_sample(*args, logit_procs=[None]) == be.forward_sample(*args)


# ---------------------------------------------------------------------------- dllama-api

@pytest.fixture(scope="module")
def api(assets):
    proc, url = _start_api(assets["q40"], assets["tok"])
    yield url
    proc.kill()
    proc.wait()


VOCAB = 512  # the tiny model's


@pytest.mark.parametrize("bad", [dict(frequency_penalty=2.5), dict(frequency_penalty=-2.01), dict(presence_penalty=3),
                                 dict(presence_penalty=-2.5), dict(presence_penalty="1"), dict(frequency_penalty=True),
                                 dict(logit_bias={"abc": 1}), dict(logit_bias={"1.5": 1}), dict(logit_bias={"-1": 1}),
                                 dict(logit_bias={str(VOCAB): 1}), dict(logit_bias={"5": 101}),
                                 dict(logit_bias={"5": -100.5}), dict(logit_bias={"5": "1"}), dict(logit_bias=[1, 2]),
                                 dict(logit_bias={str(i): 1 for i in range(301)})])
def test_api_sampling_controls_validation(api, bad):
    with pytest.raises(urllib.error.HTTPError) as e:
        _chat(api, PROMPTS[0], **bad)
    assert e.value.code == 400 and "error" in json.loads(e.value.read())


def test_api_sampling_controls_accepts_limits_and_null(api):
    kw = dict(frequency_penalty=2, presence_penalty=-2, logit_bias={str(i): (-100 if i % 2 else 100) for i in range(300)})
    assert _chat(api, PROMPTS[0], 4, **kw)["usage"]["completion_tokens"] == 4
    plain = _chat(api, PROMPTS[0], 6)
    assert _chat(api, PROMPTS[0], 6, frequency_penalty=None, presence_penalty=None,
                 logit_bias=None)["generated_text"] == plain["generated_text"]


@pytest.mark.parametrize("sampling", [dict(temperature=0), dict(temperature=0.8, seed=7)])
def test_api_logit_bias_forces_a_token(api, C, assets, sampling):
    t = 123
    assert not C.Tokenizer(assets["tok"]).is_eos(t)
    d = _chat(api, PROMPTS[1], 9, logit_bias={str(t): 100}, logprobs=True, **sampling)
    assert [e["token_id"] for e in _content(d)] == [t] * 9
    assert d["usage"]["completion_tokens"] == 9 and d["choices"][0]["finish_reason"] == "length"


def test_api_logit_bias_bans_the_first_greedy_token(api):
    a = _content(_chat(api, PROMPTS[2], 1, logprobs=True, top_logprobs=2))[0]
    t0, t1 = (t["token_id"] for t in a["top_logprobs"])
    assert a["token_id"] == t0
    b = _content(_chat(api, PROMPTS[2], 1, logprobs=True, top_logprobs=2, logit_bias={str(t0): -100}))[0]
    assert b["token_id"] == t1
    # logprobs come from the raw logits: the banned token still leads, the chosen one scores below it
    assert b["top_logprobs"] == a["top_logprobs"] and b["logprob"] == a["top_logprobs"][1]["logprob"]


def test_api_penalties_change_the_text_and_slots_start_clean(api):
    kw = dict(frequency_penalty=1.5, presence_penalty=0.5)
    plain = _chat(api, PROMPTS[3], 24)
    first = _chat(api, PROMPTS[3], 24, **kw)
    assert first["generated_text"] != plain["generated_text"]
    # the same request again (the freed slot is reused): counts start from zero, so the same text
    for _ in range(2):
        assert _chat(api, PROMPTS[3], 24, **kw)["generated_text"] == first["generated_text"]
    assert _chat(api, PROMPTS[3], 24)["generated_text"] == plain["generated_text"]


@pytest.mark.parametrize("sampling", [dict(temperature=0), dict(temperature=0.9, top_p=0.8, seed=11)])
def test_api_default_fields_equal_omitted(api, sampling):
    plain = _chat(api, PROMPTS[0], 16, logprobs=True, top_logprobs=3, **sampling)
    dflt = _chat(api, PROMPTS[0], 16, logprobs=True, top_logprobs=3, frequency_penalty=0, presence_penalty=0.0,
                 logit_bias={}, **sampling)
    assert dflt["generated_text"] == plain["generated_text"] and _content(dflt) == _content(plain)
    assert dflt["usage"] == plain["usage"]


def test_api_counts_requests_with_a_processor(api):
    import urllib.request
    before = json.loads(urllib.request.urlopen(api + "/health", timeout=10).read())["logit_proc_requests"]
    _chat(api, PROMPTS[1], 3)
    _chat(api, PROMPTS[1], 3, presence_penalty=1)
    _chat(api, PROMPTS[1], 3, logit_bias={"7": 5})
    assert json.loads(urllib.request.urlopen(api + "/health", timeout=10).read())["logit_proc_requests"] == before + 2
    text = urllib.request.urlopen(api + "/v1/metrics", timeout=10).read().decode()
    assert "dllama_logit_proc_requests_total" in text
