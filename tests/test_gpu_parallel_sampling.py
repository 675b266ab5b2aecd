"""Parallel sampling on the HIP engine: HipEngine.fork_prefix (kvForkPrefixKernel: the source's
prefix read once, stored to up to hip_max_fork_dst destinations per launch; contiguous cache and
paged pool) is a byte copy to every destination, decoding behind it is decoding behind a prefill, and
`dllama-api --batch-invariant 1` answers `n` with the solo requests' texts from one prefill."""
import concurrent.futures

import numpy as np
import pytest

from test_gpu_prefix_cache import medium, model  # noqa: F401 (fixtures)
from test_parallel_sampling import _chat, _hold_a_slot, _solos, _texts
from test_prefix_cache import _health, _start_api

pytestmark = pytest.mark.gpu

NS = (1, 31, 32, 33, 67)  # below, at and across a page / chunk edge of 32 positions, a partial last step
_RNG = np.random.default_rng(5)
SEQ = [int(t) for t in _RNG.integers(0, 2048, 80)]
OTH = [int(t) for t in _RNG.integers(0, 2048, 80)]


@pytest.mark.parametrize("page", [0, 32])
@pytest.mark.parametrize("kv_bf16", [True, False])
def test_engine_fork_prefix_bitwise(C, medium, kv_bf16, page):
    """Engines A and B hold the same caches; A forks slot 0's first n positions to m slots in one
    fork_prefix, B copies them with m copy_prefix calls (test_engine_copy_prefix_bitwise pins those
    against a prefill). Read through forwards, as that test reads the cache: for every destination
    the rest of the prompt from n and a decode row give bitwise the logits of the source slot itself
    continuing from n (so [0, n) equals the source's) and of B; before that, on the contiguous cache, a
    row at position 70 that attends the destination's earlier contents beyond n equals B's (positions
    >= n are as they were); slot 0 and the unnamed last slot decode as on B, and the pool holds as many
    free pages as B's. m = hip_max_fork_dst + 1 takes two launches. The synthetic fixtures have a head
    size of 128 (rows of 256 or 512 bytes), so only the 16-byte access width is reached here; the 4-
    and 2-byte instances share every line of the kernel but the access type."""
    K = C.hip_max_fork_dst()
    assert K >= 2
    nslots = K + 3  # the source, K + 1 destinations, a bystander
    kw = dict(kv_bf16=kv_bf16, max_batch=128, n_slots=nslots)
    if page:
        kw.update(kv_pages=3 * nslots + 2, kv_page_size=page)
    a, b = C.HipEngine(medium, "q80", **kw), C.HipEngine(medium, "q80", **kw)
    by = nslots - 1
    for e in (a, b):  # slot 0's prefill interleaved with the bystander's: its pages are not adjacent
        e.forward(SEQ[:40], list(range(40)), [0] * 40)
        e.forward(OTH[:3], [0, 1, 2], [by] * 3)
        e.forward(SEQ[40:70], list(range(40, 70)), [0] * 30)
    pby = 3
    for m in (1, 2, K, K + 1):
        dsts = list(range(1, m + 1))
        for n in NS:
            for e in (a, b):  # every destination holds another sequence's 70 positions when the fork arrives
                for d in dsts:
                    e.forward(OTH[:70], list(range(70)), [d] * 70)
            a.fork_prefix(0, dsts, n)
            for d in dsts:
                b.copy_prefix(0, d, n)
            assert a.kv_pages_free == b.kv_pages_free
            if page:
                assert a.kv_pages_free == 3 * nslots + 2 - 3 - 1 - m * -(-n // page)
            rest, pos = SEQ[n:70], list(range(n, 70))
            want = None
            for d in dsts:
                if not page:
                    assert np.array_equal(a.forward([7], [70], [d]), b.forward([7], [70], [d])), (m, n, d)
                got = np.concatenate([a.forward(rest, pos, [d] * len(rest)), a.forward([SEQ[70]], [70], [d])])
                ref = np.concatenate([b.forward(rest, pos, [d] * len(rest)), b.forward([SEQ[70]], [70], [d])])
                assert np.array_equal(got, ref), (m, n, d)
                if want is None:  # the source slot itself from n: the same rows rewrite the same values
                    want = np.concatenate([a.forward(rest, pos, [0] * len(rest)), a.forward([SEQ[70]], [70], [0])])
                    assert np.array_equal(want, np.concatenate([b.forward(rest, pos, [0] * len(rest)),
                                                                b.forward([SEQ[70]], [70], [0])])), (m, n)
                assert np.array_equal(got, want), (m, n, d)
            assert np.array_equal(a.forward([OTH[pby]], [pby], [by]), b.forward([OTH[pby]], [pby], [by])), (m, n)
            pby += 1


def test_decode_behind_fork_equals_decode_behind_prefill(C, medium):
    """batch_invariant engine, 32-position pages, L = 45 crosses one page: slots 1 and 2 forked from
    slot 0 at L, slot 3 prefills the prompt itself; the last prompt row and 8 greedy steps give bitwise
    the same logits and ids in all four."""
    e = C.HipEngine(medium, "q80", kv_bf16=True, max_batch=64, n_slots=4, batch_invariant=True, kv_pages=12,
                    kv_page_size=32)
    L = 45
    prompt = SEQ[:L + 1]
    e.forward(prompt[:L], list(range(L)), [0] * L)
    e.fork_prefix(0, [1, 2], L)
    e.forward(prompt[:L], list(range(L)), [3] * L)
    rows = {s: [] for s in range(4)}
    tok = {s: prompt[L] for s in range(4)}
    for step in range(9):
        for s in (3, 1, 0, 2):
            lg = e.forward([tok[s]], [L + step], [s])
            rows[s].append(lg.copy())
            tok[s] = int(lg[-1].argmax())
    for s in (0, 1, 2):
        assert np.array_equal(np.concatenate(rows[s]), np.concatenate(rows[3])), s
    assert tok[0] == tok[1] == tok[2] == tok[3]


def test_engine_fork_prefix_refusals(C, medium):
    """Host-side refusals, nothing launched: bad arguments, a prefix the source's pages never reached,
    a pool that cannot supply every destination (then no destination has lost or gained a page), a
    forward that was launched and not collected."""
    e = C.HipEngine(medium, "q80", kv_bf16=True, max_batch=64, n_slots=4, kv_pages=6, kv_page_size=32)
    e.forward(list(range(1, 41)), list(range(40)), [0] * 40)       # slot 0: 2 pages
    e.forward(list(range(41, 71)), list(range(40, 70)), [0] * 30)  # 3 pages
    e.forward([5], [0], [1])                                       # slots 1 and 2: 1 page each
    e.forward([6], [0], [2])
    assert e.kv_pages_free == 1
    for src, dsts, n in [(0, [0], 4), (0, [1, 0], 4), (0, [1, 1], 4), (0, [], 4), (0, [1, 2], 0), (0, [1, 2], 512),
                         (0, [1, 4], 4), (0, [1, -1], 4), (4, [1], 4), (-1, [1], 4)]:
        with pytest.raises(RuntimeError):
            e.fork_prefix(src, dsts, n)
    with pytest.raises(RuntimeError, match="never reached"):
        e.fork_prefix(1, [2, 3], 33)
    assert e.kv_pages_free == 1
    with pytest.raises(RuntimeError, match="KV page pool exhausted"):
        e.fork_prefix(0, [1, 2], 33)  # 2 x 2 pages: the two they hold and one free page do not do
    assert e.kv_pages_free == 1  # nothing released, nothing mapped
    e.forward([9], [1], [1])  # slot 1 still has its page: a second row maps none
    assert e.kv_pages_free == 1
    e.launch_ids([9], [1], [2])
    with pytest.raises(RuntimeError, match="not collected"):
        e.fork_prefix(0, [1], 4)
    assert len(e.collect_ids()) == 1
    e.fork_prefix(0, [1, 2, 3], 32)  # one page each: the two given back and the free one
    assert e.kv_pages_free == 0


# ---------------------------------------------------------------------------- dllama-api

def _gpu_api(model, extra=()):
    return _start_api(model[0], model[1], ["--gpu-index", "0", "--batch-invariant", "1", "--max-seq-len", "256", *extra])


def test_api_gpu_n_equals_solos_from_one_prefill(model):
    proc, url = _gpu_api(model)
    try:
        want = [s["generated_text"] for s in _solos(url, 3, max_tokens=16)]
        h0 = _health(url)
        d = _chat(url, n=3, max_tokens=16)
        h1 = _health(url)
        assert _texts(d) == want
        P = d["usage"]["prompt_tokens"]
        assert h1["prefill_rows"] - h0["prefill_rows"] == P + 2
        assert h1["forked_requests"] - h0["forked_requests"] == 2 and h1["fork_tokens"] - h0["fork_tokens"] == 2 * (P - 1)
    finally:
        proc.kill()
        proc.wait()


def test_api_gpu_followers_wait_for_pages(model):
    """3 slots over a pool of 10 pages of 32 positions: the long request reserves 6 pages (74 prompt
    tokens + 100 + 1), every member of the n: 3 group 2 (38 + 16 + 1), so the third member fits only
    once the long request or a sibling has ended. Everything completes with the solo texts and the
    pool is never exhausted."""
    proc, url = _gpu_api(model, ("--slots", "3", "--kv-pages", "10", "--kv-page-size", "32"))
    try:
        from test_parallel_sampling import LONG
        want_long = _chat(url, content=LONG, max_tokens=100, temperature=0)["generated_text"]
        solo = _solos(url, 3, max_tokens=16)
        assert solo[0]["usage"]["prompt_tokens"] == 38  # the page arithmetic above
        want = [s["generated_text"] for s in solo]
        with concurrent.futures.ThreadPoolExecutor(2) as ex:
            long_f = _hold_a_slot(url, ex, max_tokens=100)
            d = _chat(url, n=3, max_tokens=16)
            assert long_f.result() == want_long
        assert _texts(d) == want
        h = _health(url)
        assert h["active"] == 0 and h["queued"] == 0 and h["forked_requests"] >= 1, h
    finally:
        proc.kill()
        out = proc.communicate()[0].decode(errors="replace")
    assert "exhausted" not in out, out
