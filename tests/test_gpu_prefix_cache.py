"""Prefix KV reuse on the HIP engine: HipEngine.copy_prefix (one kvCopyPrefix launch over every
layer, K and V, every KV head; contiguous cache and paged pool) is a byte copy, and `dllama-api
--prefix-cache 1` under `--batch-invariant 1` returns exactly the texts of a server without it."""
import numpy as np
import pytest

from test_prefix_cache import (PREFIX_FLAGS, _cached_tokens, _chat, _concurrent_families, _health,
                               _same_prompt_twice, _start_api)

pytestmark = pytest.mark.gpu

NS = (1, 31, 32, 33, 64, 69)  # page edges of 32- and 64-position pages, a partial last page


@pytest.fixture(scope="module")
def medium(tmp_path_factory):
    from distributed_llama_multiusers_amd.models.synthetic import make_test_assets
    from distributed_llama_multiusers_amd.utils.mfile import FloatType
    d = str(tmp_path_factory.mktemp("medium"))
    m, _, _ = make_test_assets(d, "tiny", FloatType.Q40, seq_len=512, seed=3, dim=1024, hidden_dim=12288,
                               n_heads=8, n_kv_heads=2, n_layers=2, vocab_size=2048)
    return m


def _chunks(lo, hi, size=40):
    return [(a, min(hi, a + size)) for a in range(lo, hi, size)]


@pytest.mark.parametrize("page", [0, 32, 64])
@pytest.mark.parametrize("kv_bf16", [True, False])
def test_engine_copy_prefix_bitwise(C, medium, kv_bf16, page):
    """Engine A copies slot 0's first n positions into slot 1, engine B computes them in slot 1 with
    the forwards that computed them in slot 0 (40 + 30 rows): every forward after position n (the
    rest of the prompt, 3 decode rows) gives bitwise the same logits, and slots 0 and 2 decode as on
    the engine that never copied. Slot 0's prefill is interleaved with slot 2's, so its pages are
    not adjacent in the pool."""
    rng = np.random.default_rng(5)
    seq = [int(t) for t in rng.integers(0, 2048, 80)]
    oth = [int(t) for t in rng.integers(0, 2048, 40)]
    kw = dict(kv_bf16=kv_bf16, max_batch=64, n_slots=3)
    if page:
        kw.update(kv_pages=12, kv_page_size=page)
    a, b = C.HipEngine(medium, "q80", **kw), C.HipEngine(medium, "q80", **kw)
    pages = lambda n: -(-n // page)

    def prefill(e, slot):
        for lo, hi in ((0, 40), (40, 70)):
            e.forward(seq[lo:hi], list(range(lo, hi)), [slot] * (hi - lo))

    for e in (a, b):
        e.forward(seq[:40], list(range(40)), [0] * 40)
        e.forward(oth[:3], [0, 1, 2], [2] * 3)
        e.forward(seq[40:70], list(range(40, 70)), [0] * 30)
        e.forward(oth[3:5], [3, 4], [2] * 2)
    if page:
        assert a.kv_pages_free == 12 - pages(70) - 1
    p0, p2 = 70, 5  # next positions of slots 0 and 2
    for n in NS:
        # slot 1 of A holds another sequence's 70 positions (and their pages) when the copy arrives
        a.forward(oth[:40], list(range(40)), [1] * 40)
        a.forward(oth[:30], list(range(40, 70)), [1] * 30)
        free = a.kv_pages_free
        a.copy_prefix(0, 1, n)
        if page:
            assert a.kv_pages_free == free + pages(70) - pages(n), n
        else:
            assert a.kv_pages_free == -1
        prefill(b, 1)
        for lo, hi in _chunks(n, 70):
            toks, pos, slots = seq[lo:hi], list(range(lo, hi)), [1] * (hi - lo)
            assert np.array_equal(a.forward(toks, pos, slots), b.forward(toks, pos, slots)), (n, lo)
        for p in range(70, 73):
            assert np.array_equal(a.forward([seq[p]], [p], [1]), b.forward([seq[p]], [p], [1])), (n, p)
        # the neighbours: an overrun past the last head would land in their slot or page
        assert np.array_equal(a.forward([oth[p0 % 40]], [p0], [0]), b.forward([oth[p0 % 40]], [p0], [0])), n
        assert np.array_equal(a.forward([oth[p2]], [p2], [2]), b.forward([oth[p2]], [p2], [2])), n
        p0, p2 = p0 + 1, p2 + 1


def test_engine_copy_prefix_refusals(C, medium):
    """Host-side refusals, nothing launched: bad arguments, a prefix the source's pages never reached,
    a pool that cannot hold the copy (the destination then holds no pages)."""
    e = C.HipEngine(medium, "q80", kv_bf16=True, max_batch=64, n_slots=3, kv_pages=5, kv_page_size=32)
    e.forward(list(range(1, 41)), list(range(40)), [0] * 40)       # slot 0: 2 pages
    e.forward(list(range(41, 71)), list(range(40, 70)), [0] * 30)  # 3 pages
    e.forward([5], [0], [2])                                       # slot 2: 1 page
    e.forward([6], [0], [1])                                       # slot 1: 1 page, none free
    assert e.kv_pages_free == 0
    for src, dst, n in [(0, 0, 4), (0, 1, 0), (0, 1, 512), (0, 3, 4), (3, 1, 4), (-1, 1, 4)]:
        with pytest.raises(RuntimeError):
            e.copy_prefix(src, dst, n)
    with pytest.raises(RuntimeError, match="never reached"):
        e.copy_prefix(2, 1, 33)
    assert e.kv_pages_free == 0
    with pytest.raises(RuntimeError, match="KV page pool exhausted"):
        e.copy_prefix(0, 1, 33)  # 2 pages: slot 1's own page and nothing else
    assert e.kv_pages_free == 1  # slot 1 gave its page back and holds none
    e.copy_prefix(0, 1, 32)  # one page: fits
    assert e.kv_pages_free == 0


# ---------------------------------------------------------------------------- dllama-api

@pytest.fixture(scope="module")
def model(tmp_path_factory):
    from distributed_llama_multiusers_amd.models.synthetic import make_test_assets
    from distributed_llama_multiusers_amd.utils.mfile import FloatType
    d = str(tmp_path_factory.mktemp("prefix_api"))
    m, t, _ = make_test_assets(d, "tiny", FloatType.Q40, seq_len=256, seed=5, dim=512, n_heads=8, n_kv_heads=4,
                               hidden_dim=1024)
    return m, t


def _gpu_api(model, pages, prefix):
    flags = ["--gpu-index", "0", "--batch-invariant", "1", "--max-seq-len", "256", "--kv-pages", str(pages),
             "--kv-page-size", "32"]
    return _start_api(model[0], model[1], flags + (list(PREFIX_FLAGS) if prefix else []))


@pytest.fixture(scope="module")
def plain(model):
    proc, url = _gpu_api(model, 16, False)
    yield url
    proc.kill()
    proc.wait()


def test_api_gpu_repeat_and_eviction(model, plain):
    """A pool of 7 pages of 32 positions under 4 slots: the same prompt twice prefills one row; six
    prompts of 2 pages each with nothing in common force idle slots out for their pages; the texts
    are the plain server's throughout."""
    proc, url = _gpu_api(model, 7, True)
    try:
        _same_prompt_twice(url, plain, "tell me about the world and the end of it")
        roles = ["alpha", "bravo", "charlie", "delta", "echo", "foxtrot"]
        text = "the world and the end of the world"
        want = [_chat(plain, text, role=r)["generated_text"] for r in roles]
        got = [_chat(url, text, role=r) for r in roles]
        assert [g["generated_text"] for g in got] == want
        again = _chat(url, text, role=roles[0])
        assert again["generated_text"] == want[0]
        last = _chat(url, text, role=roles[-1])
        assert last["generated_text"] == want[-1] and _cached_tokens(last) == last["usage"]["prompt_tokens"] - 1
        h = _health(url)
        assert h["prefix_evictions"] >= 1 and h["completed"] == 10 and h["active"] == 0, h
    finally:
        proc.kill()
        proc.wait()


def test_api_gpu_concurrent_families(model, plain):
    proc, url = _gpu_api(model, 16, True)
    try:
        _concurrent_families(url, plain, long_tokens=100)
    finally:
        proc.kill()
        proc.wait()
