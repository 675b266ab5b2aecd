"""`top_k` and `min_p` of the chat API on the CPU backend: the host reference `logit_filter_host`, the
per-row filters of `Backend.forward_sample`, and `dllama-api` (validation, off values, greedy
equivalence, defaults, the request counter).

The reference is numpy float32: thr = max(k-th largest value, max + delta) and
`np.where(x >= thr, x, -inf)`; the filter does no arithmetic on the survivors, so rows are compared
bitwise (`tobytes()`). delta comes from `cpu_ops.min_p_delta`, the one place a logarithm is taken."""
import json
import urllib.error
import urllib.request

import numpy as np
import pytest

from test_logprobs import PROMPTS, _chat, _content
from test_prefix_cache import _start_api
from test_sampling_controls import PROMPT

F32 = np.float32
NEG_INF = F32(-np.inf)
VOCABS = [7, 50, 517, 8193]


def k_values(vocab):
    return [0, 1, 2, 40, vocab - 1, vocab, vocab + 5]


def deltas(C):
    """off, a usual min_p, min_p = 1 (only the maximum's value survives), a tiny min_p."""
    d = [float("-inf"), C.cpu_ops.min_p_delta(0.8, 0.05), C.cpu_ops.min_p_delta(1.3, 1.0),
         C.cpu_ops.min_p_delta(0.5, 1e-6)]
    assert d[2] == 0.0 and d[1] < 0 and d[3] < d[1]
    return d


def np_filter(x, k, delta):
    x = np.asarray(x, F32)
    thr = NEG_INF
    if 1 <= k < x.shape[0]:
        thr = np.sort(x)[::-1][k - 1]
    if delta > -np.inf:
        thr_p = x.max() + F32(delta)
        assert thr_p.dtype == F32
        thr = np.maximum(thr, thr_p)
    y = np.where(x >= thr, x, NEG_INF)
    assert y.dtype == F32
    return y


def filter_case(vocab, k, seed, variant="tie"):
    """Logits in multiples of 0.25. With 1 <= k < vocab the (k+1)-th largest is made equal to the k-th,
    so a tie straddles the cut. "zero": the row is shifted so that the k-th value is 0 and the tie's
    members are +0.0 and -0.0. "inf": a third of the row is already -inf."""
    rng = np.random.default_rng(seed)
    x = (np.round(rng.standard_normal(vocab) * 24) / 4).astype(F32)
    if variant == "inf":
        x[rng.random(vocab) < 0.34] = NEG_INF
        x[vocab // 2] = F32(1.5)
    if 1 <= k < vocab:
        order = np.argsort(-x, kind="stable")
        if variant == "zero":
            x = (x - x[order[k - 1]]).astype(F32)  # (exact: multiples of 0.25)
            x[order[k - 1]] = F32(0.0)
            x[order[k]] = F32(-0.0)
        else:
            x[order[k]] = x[order[k - 1]]
        vk = np.sort(x)[::-1][k - 1]
        assert np.count_nonzero(x >= vk) > k, "the case must tie at the k-th value"
        if variant == "zero":
            assert vk == 0 and np.signbit(x[order[k]]) and not np.signbit(x[order[k - 1]])
    return x


# ---------------------------------------------------------------------------- logit_filter_host

def test_min_p_delta_is_t_log_min_p(C):
    for T, p in [(0.8, 0.05), (1.3, 1.0), (0.5, 1e-6), (2.0, 0.5)]:
        want = float(F32(T)) * np.log(float(F32(p)))
        assert abs(C.cpu_ops.min_p_delta(T, p) - want) <= 1e-6 * max(1.0, abs(want))
    assert C.cpu_ops.min_p_delta(0.8, 0.0) == float("-inf")


@pytest.mark.parametrize("variant", ["tie", "zero", "inf"])
@pytest.mark.parametrize("vocab", VOCABS)
def test_logit_filter_host_matches_numpy(C, vocab, variant):
    for k in k_values(vocab):
        x = filter_case(vocab, k, vocab + k, variant)
        for delta in deltas(C):
            got = C.cpu_ops.logit_filter_host(x, k, delta)
            want = np_filter(x, k, delta)
            assert got.dtype == F32 and got.tobytes() == want.tobytes(), (k, delta)
            assert got[int(np.argmax(x))] == x.max()  # the maximum always survives
            if 1 <= k < vocab and delta == -np.inf:  # top_k alone keeps at least k (of the finite ones)
                assert np.count_nonzero(got > NEG_INF) >= min(k, np.count_nonzero(x > NEG_INF))
            if k == 0 or k >= vocab:  # top_k off
                assert got.tobytes() == np_filter(x, 0, delta).tobytes()
                if delta == -np.inf:
                    assert got.tobytes() == x.tobytes()


# ---------------------------------------------------------------------------- Backend.forward_sample

T_LOOP, TOPK_SET, MINP_SET = 0.9, 5, 0.2
SET_COINS = [float(c) for c in np.linspace(0.01, 0.995, 32)]


def run_top1_loop(make, steps=16):
    """Shared with the GPU test. top_k = 1 at temperature 0.9: whatever the coin, the draw is the
    argmax of `forward`'s logits for the same row (random-init logits have no tie at the top)."""
    be = make()
    n = len(PROMPT) - 1
    be.forward(PROMPT[:-1], list(range(n)), [0] * n)
    tok, pos = PROMPT[-1], n
    for s in range(steps):
        raw = be.forward([tok], [pos], [0])[0]
        coin, topp = (0.03 + 0.061 * s) % 1.0, (0.9, 1.0)[s % 2]
        got = be.forward_sample([tok], [pos], [0], [T_LOOP], [topp], [coin],
                                logit_procs=[dict(top_k=1, fresh=s == 0)])
        assert got == [int(np.argmax(raw))], (s, coin, topp)
        tok, pos = got[0], pos + 1
    return be


def run_survivor_set(make, C):
    """Shared with the GPU test. top_k = 5, min_p = 0.2: over 32 coins every draw lies in the numpy
    survivor set of `forward`'s logits, and for at least one of those coins the draw without the
    fields lies outside it (the witness that the fields act: a random-init model's distribution is
    flat, and a multinomial draw with a coin near 1 lands far from the top)."""
    be = make()
    n = len(PROMPT) - 1
    be.forward(PROMPT[:-1], list(range(n)), [0] * n)
    args = ([PROMPT[-1]], [n], [0])
    raw = be.forward(*args)[0]
    keep = np_filter(raw, TOPK_SET, C.cpu_ops.min_p_delta(T_LOOP, MINP_SET))
    survivors = set(np.nonzero(keep > NEG_INF)[0].tolist())
    assert 1 <= len(survivors) <= TOPK_SET
    outside = 0
    for i, coin in enumerate(SET_COINS):
        proc = dict(top_k=TOPK_SET, min_p=MINP_SET, fresh=i == 0)
        got = be.forward_sample(*args, [T_LOOP], [1.0], [coin], logit_procs=[proc])
        assert got[0] in survivors, (coin, got)
        plain = be.forward_sample(*args, [T_LOOP], [1.0], [coin])
        outside += plain[0] not in survivors
    assert outside >= 1
    # off values and a greedy row: the plain forward's ids
    for proc in (dict(top_k=0, min_p=0.0), dict(top_k=raw.shape[0]), dict(top_k=raw.shape[0] + 7)):
        assert be.forward_sample(*args, [T_LOOP], [0.9], [0.77], logit_procs=[proc]) == \
            be.forward_sample(*args, [T_LOOP], [0.9], [0.77])
    assert be.forward_sample(*args, [0.0], [0.9], [0.5], logit_procs=[dict(top_k=3, min_p=0.5)]) == [int(np.argmax(raw))]


def _backend(C, assets):
    return C.cpu_backend(assets["q40"], "q80", 2, 128, 64, 3)


def test_cpu_backend_top_k_1_draws_the_argmax(C, assets):
    run_top1_loop(lambda: _backend(C, assets))


def test_cpu_backend_draws_stay_in_the_survivor_set(C, assets):
    run_survivor_set(lambda: _backend(C, assets), C)


def test_cpu_backend_rejects_bad_filters(C, assets):
    be = _backend(C, assets)
    args = ([3], [0], [0], [0.8], [0.9], [0.3])
    for proc in (dict(top_k=-1), dict(min_p=-0.1), dict(min_p=1.5), dict(min_p=float("nan"))):
        with pytest.raises(RuntimeError):
            be.forward_sample(*args, logit_procs=[proc])


# ---------------------------------------------------------------------------- dllama-api

@pytest.fixture(scope="module")
def api(assets):
    proc, url = _start_api(assets["q40"], assets["tok"])
    yield url
    proc.kill()
    proc.wait()


VOCAB = 512  # the tiny model's


@pytest.mark.parametrize("bad", [dict(top_k=1.5), dict(top_k=-1), dict(top_k="40"), dict(top_k=True), dict(top_k=[40]),
                                 dict(min_p=-0.01), dict(min_p=1.01), dict(min_p="0.1"), dict(min_p=False),
                                 dict(min_p={"p": 0.1})])
def test_api_filters_validation(api, bad):
    with pytest.raises(urllib.error.HTTPError) as e:
        _chat(api, PROMPTS[0], temperature=0.8, **bad)
    assert e.value.code == 400 and "error" in json.loads(e.value.read())


def test_api_filters_accept_limits_null_and_off_values(api):
    plain = _chat(api, PROMPTS[0], 8, temperature=0.8, seed=3)
    for kw in (dict(top_k=None, min_p=None), dict(top_k=0, min_p=0), dict(top_k=0.0, min_p=0.0),
               dict(top_k=VOCAB), dict(top_k=10 ** 9)):
        assert _chat(api, PROMPTS[0], 8, temperature=0.8, seed=3, **kw)["generated_text"] == plain["generated_text"], kw
    for kw in (dict(top_k=VOCAB - 1, min_p=1), dict(top_k=1, min_p=1.0), dict(top_k=40.0, min_p=0.05)):
        assert _chat(api, PROMPTS[0], 4, temperature=0.8, seed=3, **kw)["usage"]["completion_tokens"] == 4


@pytest.mark.parametrize("seed", [1, 7])
def test_api_top_k_1_returns_the_greedy_text(api, seed):
    greedy = _chat(api, PROMPTS[1], 16, logprobs=True)
    got = _chat(api, PROMPTS[1], 16, temperature=0.8, seed=seed, top_k=1, logprobs=True)
    assert got["generated_text"] == greedy["generated_text"]
    assert [e["token_id"] for e in _content(got)] == [e["token_id"] for e in _content(greedy)]
    # min_p = 1 keeps the maximum's value alone
    assert _chat(api, PROMPTS[1], 16, temperature=0.8, seed=seed, min_p=1)["generated_text"] == greedy["generated_text"]


@pytest.mark.parametrize("sampling", [dict(temperature=0), dict(temperature=0.9, top_p=0.8, seed=11)])
def test_api_default_filter_fields_equal_omitted(api, sampling):
    plain = _chat(api, PROMPTS[0], 16, logprobs=True, top_logprobs=3, **sampling)
    dflt = _chat(api, PROMPTS[0], 16, logprobs=True, top_logprobs=3, top_k=0, min_p=0.0, **sampling)
    assert dflt["generated_text"] == plain["generated_text"] and _content(dflt) == _content(plain)
    assert dflt["usage"] == plain["usage"]


def test_api_greedy_ignores_valid_filters(api):
    plain = _chat(api, PROMPTS[2], 12)
    assert _chat(api, PROMPTS[2], 12, top_k=3, min_p=0.5)["generated_text"] == plain["generated_text"]


def test_api_counts_requests_with_a_filter(api):
    health = lambda: json.loads(urllib.request.urlopen(api + "/health", timeout=10).read())
    before = health()
    _chat(api, PROMPTS[1], 3, temperature=0.8)
    _chat(api, PROMPTS[1], 3, temperature=0.8, top_k=40)
    _chat(api, PROMPTS[1], 3, temperature=0.8, min_p=0.05)
    _chat(api, PROMPTS[1], 3, top_k=40)  # greedy: ignored
    _chat(api, PROMPTS[1], 3, temperature=0.8, top_k=0, min_p=0)
    _chat(api, PROMPTS[1], 3, temperature=0.8, presence_penalty=1)
    after = health()
    assert after["logit_filter_requests"] == before["logit_filter_requests"] + 2
    assert after["logit_proc_requests"] == before["logit_proc_requests"] + 1
    text = urllib.request.urlopen(api + "/v1/metrics", timeout=10).read().decode()
    assert "dllama_logit_filter_requests_total" in text
