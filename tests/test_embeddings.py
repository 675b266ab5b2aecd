"""Embeddings (`POST /v1/embeddings`) on the CPU backend: the host reference `pool_host`,
`Backend.forward_embed`, and `dllama-api` (input forms, validation, batching, counters).

`pool_host` is compared with a numpy float64 evaluation of the same formula on the same f32 rows:
h = norm_w * rmsnorm(x), p = mean of the rows' h (or the last row's), out = p / |p|. The bound per
element of the unit vector is (N + log2(dim) + 4) * 2^-23, computed from N and dim: N roundings of
the sequential f32 sum, log2(dim) for each norm's sum of squares as a tree, and 4 for the products,
the division by N and the final division. Relative to an element of a unit vector (at most 1) this
is a worst-case bound, not a fitted one."""
import base64
import concurrent.futures
import json
import math
import urllib.error
import urllib.request

import numpy as np
import pytest

from test_prefix_cache import _health, _start_api


def bound(n, dim):
    return (n + math.log2(dim) + 4) * 2.0 ** -23


def reference(x, w, eps, mode):
    x = np.asarray(x, np.float32).astype(np.float64)
    h = np.asarray(w, np.float32).astype(np.float64) * (x / np.sqrt((x * x).mean(-1, keepdims=True) + eps))
    p = h.mean(0) if mode == "mean" else h[-1]
    ss = float((p * p).sum())
    return p / math.sqrt(ss) if ss > 0 else np.zeros_like(p)


def rows(n, dim, seed):
    rng = np.random.default_rng(seed)
    x = (rng.standard_normal((n, dim)) * rng.uniform(0.2, 3.0, (n, 1))).astype(np.float32)
    w = rng.uniform(0.5, 1.5, dim).astype(np.float32)
    return x, w


# ---------------------------------------------------------------------------- pool_host

@pytest.mark.parametrize("mode", ["mean", "last"])
@pytest.mark.parametrize("n", [1, 2, 33, 70])
@pytest.mark.parametrize("dim", [32, 64, 4096])
def test_pool_host_matches_reference(C, dim, n, mode):
    x, w = rows(n, dim, 1000 * dim + n)
    got = C.cpu_ops.pool_host(x, w, 1e-5, mode)
    ref = reference(x, w, 1e-5, mode)
    assert got.shape == (dim,) and got.dtype == np.float32
    err = float(np.abs(got.astype(np.float64) - ref).max())
    print(f"dim {dim} N {n} {mode}: max error {err:.3e}, bound {bound(n, dim):.3e}")
    assert err <= bound(n, dim)
    assert abs(float(np.linalg.norm(got.astype(np.float64))) - 1) < 1e-6


@pytest.mark.parametrize("mode", ["mean", "last"])
def test_pool_host_zero_rows_give_zeros(C, mode):
    x = np.zeros((5, 64), np.float32)
    w = np.ones(64, np.float32)
    got = C.cpu_ops.pool_host(x, w, 1e-5, mode)
    assert np.isfinite(got).all() and (got == 0).all()


def test_pool_host_add_operand(C):
    x, w = rows(7, 64, 5)
    y, _ = rows(7, 64, 6)
    got = C.cpu_ops.pool_host(x, w, 1e-5, "mean", y)
    assert np.array_equal(got, C.cpu_ops.pool_host(x + y, w, 1e-5, "mean"))


# ---------------------------------------------------------------------------- Backend.forward_embed

def _backend(C, assets):
    return C.cpu_backend(assets["q40"], "q80", 2, 128, 64, 3)


def spec(at, n, mode="mean"):
    return {"first": at == 0, "last": at == n - 1, "count": n, "mode": mode}


def embed(be, tokens, chunk, slot=0, mode="mean"):
    """The prompt through all-embedding forwards of `chunk` rows: the finalised vector."""
    n, out = len(tokens), None
    for c0 in range(0, n, chunk):
        k = min(chunk, n - c0)
        ids, slots, vecs = be.forward_embed(tokens[c0:c0 + k], list(range(c0, c0 + k)), [slot] * k,
                                            [spec(c0 + i, n, mode) for i in range(k)])
        assert ids == [-1] * k
        if c0 + k == n:
            assert slots == [slot] and vecs.shape[0] == 1
            out = vecs[0].copy()
        else:
            assert slots == [] and vecs.shape[0] == 0
    return out


TOKENS = [int(t) for t in np.random.default_rng(21).integers(0, 500, 23)]


@pytest.mark.parametrize("mode", ["mean", "last"])
def test_cpu_backend_forward_embed_is_pool_host_of_its_hidden_rows(C, assets, mode):
    be = _backend(C, assets)
    n = len(TOKENS)
    hidden, w = be.forward_hidden(TOKENS, list(range(n)), [1] * n)
    want = C.cpu_ops.pool_host(hidden, w, be.header["norm_epsilon"], mode)
    got = embed(be, TOKENS, n, slot=0, mode=mode)
    assert np.array_equal(got, want)
    assert np.array_equal(embed(be, TOKENS, 1, slot=2, mode=mode), got)  # chunks of 1
    assert np.array_equal(embed(be, TOKENS, 5, slot=0, mode=mode), got)
    assert abs(float(np.linalg.norm(got.astype(np.float64))) - 1) < 1e-5


def test_cpu_backend_mixed_forward_pools_behind_the_draw(C, assets):
    """Embedding rows next to a drawn row of another slot: the drawn id is the one the row draws
    alone, the vector the one the request gives alone."""
    be = _backend(C, assets)
    n = len(TOKENS)
    alone = embed(be, TOKENS, n, slot=0)
    be.forward(TOKENS[:6], list(range(6)), [1] * 6)
    want_id = be.forward_sample([17], [6], [1], [0.0], [0.9], [0.3])
    toks, pos, slots = TOKENS + [17], list(range(n)) + [6], [0] * n + [1]
    pooling = [spec(i, n) for i in range(n)] + [None]
    ids, done, vecs = be.forward_embed(toks, pos, slots, pooling, [-1.0] * n + [0.0], [0.9] * (n + 1), [0.3] * (n + 1))
    assert ids == [-1] * n + want_id and done == [0]
    assert np.array_equal(vecs[0], alone)


def test_pooling_rows_out_of_order_are_refused(C, assets):
    be = _backend(C, assets)
    with pytest.raises(Exception, match="ascending"):
        be.forward_embed([3, 4], [1, 0], [0, 0], [spec(1, 2), spec(0, 2)])


# ---------------------------------------------------------------------------- dllama-api

@pytest.fixture(scope="module")
def api(assets):
    proc, url = _start_api(assets["q40"], assets["tok"])
    yield url
    proc.kill()
    proc.wait()


def _embed_raw(url, body):
    req = urllib.request.Request(url + "/v1/embeddings", data=json.dumps(body).encode(),
                                 headers={"Content-Type": "application/json"})
    return json.loads(urllib.request.urlopen(req, timeout=120).read())


def _vectors(resp):
    assert resp["object"] == "list"
    assert [d["index"] for d in resp["data"]] == list(range(len(resp["data"])))
    assert all(d["object"] == "embedding" for d in resp["data"])
    return [np.asarray(d["embedding"], np.float32) for d in resp["data"]]


def _chat(url, content, max_tokens=12):
    body = {"messages": [{"role": "user", "content": content}], "max_tokens": max_tokens, "temperature": 0}
    req = urllib.request.Request(url + "/v1/chat/completions", data=json.dumps(body).encode(),
                                 headers={"Content-Type": "application/json"})
    return json.loads(urllib.request.urlopen(req, timeout=120).read())["choices"][0]["message"]["content"]


TEXTS = ["the quick brown fox", "hello world this is", "tell me about the end of", "one two three four five",
         "a", "the lazy dog and then the quick brown fox jumps over it again and again", "hello", "this is the end"]


def test_api_embeddings_shape_and_input_forms(C, assets, api):
    tok = C.Tokenizer(assets["tok"])
    one = _embed_raw(api, {"input": TEXTS[0], "model": "anything"})
    v = _vectors(one)
    dim = len(v[0])
    assert len(v) == 1 and dim > 0 and isinstance(one["model"], str)
    ids = [tok.encode(t, True, False) for t in TEXTS[:3]]
    assert one["usage"] == {"prompt_tokens": len(ids[0]), "total_tokens": len(ids[0])}
    # a string and its own token ids give identical vectors, alone and in lists
    assert np.array_equal(_vectors(_embed_raw(api, {"input": ids[0]}))[0], v[0])
    many = _embed_raw(api, {"input": TEXTS[:3]})
    many_ids = _embed_raw(api, {"input": ids})
    assert many["usage"]["prompt_tokens"] == sum(len(i) for i in ids) == many["usage"]["total_tokens"]
    for a, b in zip(_vectors(many), _vectors(many_ids)):
        assert np.array_equal(a, b)
    assert np.array_equal(_vectors(many)[0], v[0])
    for x in _vectors(many):
        assert x.shape == (dim,) and abs(float(np.linalg.norm(x.astype(np.float64))) - 1) <= 1e-5
    assert not np.array_equal(_vectors(many)[0], _vectors(many)[1])


def test_api_embeddings_base64_and_pooling(api):
    f = _vectors(_embed_raw(api, {"input": TEXTS[:2], "encoding_format": "float"}))
    b = _embed_raw(api, {"input": TEXTS[:2], "encoding_format": "base64"})
    for i, d in enumerate(b["data"]):
        assert d["index"] == i and isinstance(d["embedding"], str)
        assert np.array_equal(np.frombuffer(base64.b64decode(d["embedding"]), "<f4"), f[i])
    last = _vectors(_embed_raw(api, {"input": TEXTS[:2], "pooling": "last"}))
    mean = _vectors(_embed_raw(api, {"input": TEXTS[:2], "pooling": "mean"}))
    assert np.array_equal(mean[0], f[0]) and not np.array_equal(last[0], f[0])
    for x in last:
        assert abs(float(np.linalg.norm(x.astype(np.float64))) - 1) <= 1e-5


@pytest.mark.parametrize("body", [
    {}, {"input": []}, {"input": ""}, {"input": ["ok", ""]}, {"input": [[]]}, {"input": [[1, 2], []]},
    {"input": [1, 10 ** 7]}, {"input": [[1, -1]]}, {"input": [1.5]}, {"input": list(range(1, 130))},
    {"input": "x", "dimensions": 8}, {"input": "x", "encoding_format": "hex"}, {"input": "x", "pooling": "max"},
    {"input": 5}, {"input": ["a", [1]]}, {"input": ["a"] * 2049},
], ids=lambda b: json.dumps(b)[:40])
def test_api_embeddings_invalid_requests(api, body):
    with pytest.raises(urllib.error.HTTPError) as e:
        _embed_raw(api, body)
    assert e.value.code == 400
    assert "error" in json.loads(e.value.read())


def test_api_embeddings_batch_equals_alone_and_counters(api):
    before = _health(api)["embedding_requests"]
    together = _vectors(_embed_raw(api, {"input": TEXTS}))
    alone = [_vectors(_embed_raw(api, {"input": t}))[0] for t in TEXTS]
    for a, b in zip(together, alone):
        assert np.array_equal(a, b)
    assert _health(api)["embedding_requests"] == before + 2 * len(TEXTS)
    metrics = urllib.request.urlopen(api + "/v1/metrics", timeout=10).read().decode()
    line = [l for l in metrics.splitlines() if l.startswith("dllama_embedding_requests_total ")]
    assert line and float(line[0].split()[1]) == before + 2 * len(TEXTS)


def test_api_chat_next_to_embeddings_returns_its_solo_text(api):
    solo = _chat(api, "tell me about the quick brown fox")
    with concurrent.futures.ThreadPoolExecutor(3) as ex:
        chat = ex.submit(_chat, api, "tell me about the quick brown fox")
        embs = [ex.submit(_embed_raw, api, {"input": TEXTS[:3]}) for _ in range(2)]
        assert chat.result() == solo
        ref = _vectors(_embed_raw(api, {"input": TEXTS[:3]}))
        for e in embs:
            for a, b in zip(_vectors(e.result()), ref):
                assert np.array_equal(a, b)
