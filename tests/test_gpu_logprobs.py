"""Per-token log-probabilities on the HIP engine: the launchLogprobs kernel (`ops.logprobs`) against
numpy float64 log_softmax with ids from a stable sort, its independence of the batch and of earlier
calls, `HipEngine.forward_logprobs`, tensor parallelism (the root scores the gathered logits) and
`dllama-api --batch-invariant 1`. Tolerance and reference: see test_logprobs.py."""
import numpy as np
import pytest

from test_gpu_xgmi import _run, _setup
from test_logprobs import (SLOTS, _chat, _forward_logprobs_cases, check_response, check_row, concurrent_equal_solo)
from test_prefix_cache import _start_api

pytestmark = pytest.mark.gpu

REQ = [-1, 0, 1, 5, 20]  # per row: none, the chosen token only, k = 1 / 5 / 20


@pytest.fixture(scope="module")
def ops():
    from distributed_llama_multiusers_amd import ops
    return ops


def _rows(vocab, scale, seed, rows=5):
    rng = np.random.default_rng(seed)
    x = (rng.standard_normal((rows, vocab)) * scale).astype(np.float32)
    return x, [int(i) for i in rng.integers(0, vocab, rows)]


def _check_call(x, ids, req, vals, top):
    assert vals.shape == (len(ids), SLOTS) and top.shape == (len(ids), SLOTS)
    for b, k in enumerate(req):
        if k < 0:
            assert (top[b] == -2).all() and (vals[b] == 0).all()  # the row was not written
        else:
            check_row(x[b], ids[b], k, vals[b], top[b])


@pytest.mark.parametrize("scale", [1, 6, 30])
@pytest.mark.parametrize("vocab", [128256, 32000, 517, 50, 7])
def test_logprobs_kernel_matches_reference(ops, vocab, scale):
    x, ids = _rows(vocab, scale, vocab + scale)
    vals, top = ops.logprobs(x, ids, REQ)
    _check_call(x, ids, REQ, vals, top)


@pytest.mark.parametrize("vocab", [8192, 8193, 16385, 525289])
def test_logprobs_kernel_group_and_tile_edges(ops, vocab):
    """One workgroup per row up to 8192 logits, then one per 8192; beyond 64 x 8192 a workgroup takes
    a second tile and carries its best list over (525289: a 16-element second tile)."""
    x, ids = _rows(vocab, 6, vocab)
    x[:, -3:] = x.max() + 1  # the last elements of the last slice lead, tied
    vals, top = ops.logprobs(x, ids, REQ)
    _check_call(x, ids, REQ, vals, top)


@pytest.mark.parametrize("vocab", [128256, 525289, 50])
def test_logprobs_kernel_ties(ops, vocab):
    """Logits rounded to multiples of 0.5: thousands of equal values; the ids are exactly the stable
    reference order."""
    x, ids = _rows(vocab, 1, 77)
    x = np.round(x * 2) / 2
    vals, top = ops.logprobs(x, ids, REQ)
    _check_call(x, ids, REQ, vals, top)


def test_logprobs_kernel_row_independent_and_reproducible(ops):
    """A row's output is bitwise the same alone, among 5 and among 64 rows, and from call to call; a
    call on the scratch an earlier call with other inputs used is correct (counters left clean)."""
    x, ids = _rows(128256, 6, 5, rows=64)
    alone = ops.logprobs(x[:1], ids[:1], [20])
    five = ops.logprobs(x[:5], ids[:5], [20, -1, 5, 0, 20])
    full = ops.logprobs(x, ids, [20] * 64)
    again = ops.logprobs(x, ids, [20] * 64)
    for a, b in ((alone, five), (alone, full)):
        assert a[0][0].tobytes() == b[0][0].tobytes() and a[1][0].tobytes() == b[1][0].tobytes()
    assert full[0].tobytes() == again[0].tobytes() and full[1].tobytes() == again[1].tobytes()
    assert five[0][4].tobytes() == full[0][4].tobytes() and five[1][4].tobytes() == full[1][4].tobytes()
    check_row(x[63], ids[63], 20, full[0][63], full[1][63])
    y, ids2 = _rows(128256, 30, 6, rows=5)
    vals, top = ops.logprobs(y, ids2, REQ, warm=(x[:5], ids[:5]))
    _check_call(y, ids2, REQ, vals, top)
    fresh = ops.logprobs(y, ids2, REQ)
    assert vals[1:].tobytes() == fresh[0][1:].tobytes() and top[1:].tobytes() == fresh[1][1:].tobytes()


# ---------------------------------------------------------------------------- HipEngine.forward_logprobs

def test_engine_forward_logprobs(C, assets):
    """One decode row (where a greedy forward takes the argmax tail and stores no logits) and a mixed
    4-row call, against engine.forward's logits; ids equal forward_sample's."""
    _forward_logprobs_cases(lambda: C.HipEngine(assets["q40"], "q80", kv_bf16=False, max_batch=64, n_slots=3))


def test_engine_forward_logprobs_over_graph_replays(C, assets):
    """The kernel runs behind the forward's graph, not in it: eager, captured and replayed forwards
    give the same records, and a forward without a request in between returns none."""
    e = C.HipEngine(assets["q40"], "q80", kv_bf16=False, max_batch=8, n_slots=1)
    e.forward([3, 4, 5], [0, 1, 2], [0] * 3)
    args = ([9], [3], [0], [0.8], [0.9], [0.41])
    runs = [e.forward_logprobs(*args, [7]) for _ in range(2)]
    none = e.forward_logprobs(*args, [-1])
    runs += [e.forward_logprobs(*args, [7]) for _ in range(2)]
    assert (none[2] == -1).all() and none[0] == runs[0][0]
    for r in runs[1:]:
        assert r[0] == runs[0][0] and r[1].tobytes() == runs[0][1].tobytes() and r[2].tobytes() == runs[0][2].tobytes()
    check_row(e.forward([9], [3], [0])[0], runs[0][0][0], 7, runs[0][1][0], runs[0][2][0])


# ---------------------------------------------------------------------------- tensor parallelism

def _engine_tp_logprobs(rank, world, port, model, tokens, temps, topps, coins, req, q):
    try:
        C, comm, dist = _setup(rank, world, port, 1 << 16)
        eng = C.HipEngine(model, "q80", kv_bf16=False, rank=rank, world=world, comm=comm, sync_type="f32",
                          max_batch=8, n_slots=1)
        n = len(tokens)
        got = [eng.forward_logprobs(tokens, list(range(n)), [0] * n, temps, topps, coins, req) for _ in range(3)]
        lg = eng.forward(tokens, list(range(n)), [0] * n)
        if comm.timed_out():
            raise AssertionError("a flag wait timed out")
        dist.barrier()
        q.put((rank, (got, lg if rank == 0 else None)))
    except Exception as e:
        q.put((rank, repr(e)))


def test_xgmi_engine_tp_logprobs_on_root(tmp_path):
    """TP = 2 on one GPU: rank 0 scores the logits gathered to it (its own forward's logits are the
    reference), over eager and replayed forwards; rank 1 computes no records."""
    from distributed_llama_multiusers_amd.models.synthetic import make_test_assets
    from distributed_llama_multiusers_amd.utils.mfile import FloatType
    m, _, _ = make_test_assets(str(tmp_path), "tiny", FloatType.Q40, seq_len=128, seed=9, dim=512, n_heads=8,
                               n_kv_heads=4, hidden_dim=1024, vocab_size=1024)
    tokens, temps, topps = [5, 99, 300, 7], [0.0, 0.7, -1.0, 1.1], [0.9, 0.9, 0.9, 1.0]
    coins, req = [0.1, 0.35, 0.2, 0.85], [20, 3, -1, 0]
    res = _run(_engine_tp_logprobs, 2, m, tokens, temps, topps, coins, req)
    assert all(isinstance(v, tuple) for v in res.values()), res
    got, lg = res[0]
    for ids, vals, top in got:
        assert ids == got[0][0] and vals.tobytes() == got[0][1].tobytes() and top.tobytes() == got[0][2].tobytes()
    ids, vals, top = got[0]
    for b, k in enumerate(req):
        if k < 0:
            assert (top[b] == -1).all()
        else:
            check_row(lg[b], ids[b], k, vals[b], top[b])
    assert all((t == -1).all() for _, _, t in res[1][0])


# ---------------------------------------------------------------------------- dllama-api

@pytest.fixture(scope="module")
def gpu_api(tmp_path_factory):
    from distributed_llama_multiusers_amd.models.synthetic import make_test_assets
    from distributed_llama_multiusers_amd.utils.mfile import FloatType
    d = str(tmp_path_factory.mktemp("logprobs_api"))
    m, t, _ = make_test_assets(d, "tiny", FloatType.Q40, seq_len=256, seed=5, dim=512, n_heads=8, n_kv_heads=4,
                               hidden_dim=1024)
    proc, url = _start_api(m, t, ["--gpu-index", "0", "--batch-invariant", "1", "--max-seq-len", "256"])
    yield url, t
    proc.kill()
    proc.wait()


GREEDY = [dict(temperature=0)] * 4  # the device sampler's workgroups per row depend on the batch, so
                                     # draws at temperature > 0 are not pinned across batch sizes


def test_api_gpu_logprobs_texts_unchanged(C, gpu_api):
    """--batch-invariant 1: requests with logprobs served together with plain ones return the texts
    of the same requests served alone, the plain ones are unchanged, and the flag does not change a
    request's text, greedy or sampled with a seed."""
    url, tpath = gpu_api
    concurrent_equal_solo(url, GREEDY, records=False)
    tok = C.Tokenizer(tpath)
    for kw in (dict(temperature=0), dict(temperature=0.9, top_p=0.8, seed=11)):
        d = _chat(url, "tell me about the end of", 16, logprobs=True, top_logprobs=20, **kw)
        check_response(d, 20, tok, greedy=kw["temperature"] == 0)
        assert d["generated_text"] == _chat(url, "tell me about the end of", 16, **kw)["generated_text"]


def test_api_gpu_logprobs_concurrent_records_equal_solo(gpu_api):
    """--batch-invariant 1: the records of requests served together are exactly those of the same
    requests served alone (prompts prefilled next to others, in forwards of more than 32 rows, leave
    the KV of the same prompts prefilled alone: the attention's head grouping is pinned)."""
    concurrent_equal_solo(gpu_api[0], GREEDY)


def test_invariant_prefill_logits_independent_of_rows_beyond_32(C, assets):
    """batch_invariant engines: a 30-row prompt prefilled alone and inside forwards of 33 / 71 rows
    (where the decode attention would otherwise group two query heads per workgroup) gives bitwise
    the same logits, so the KV it leaves - and every later record - does not depend on the company."""
    rng = np.random.default_rng(0)
    prompt = [int(t) for t in rng.integers(0, 500, 30)]
    other = [int(t) for t in rng.integers(0, 500, 41)]
    mk = lambda: C.HipEngine(assets["q40"], "q80", kv_bf16=False, max_batch=128, n_slots=2, batch_invariant=True)
    ref = mk().forward(prompt, list(range(30)), [0] * 30)
    for o in (3, 41):
        got = mk().forward(prompt + other[:o], list(range(30)) + list(range(o)), [0] * 30 + [1] * o)[:30]
        assert np.array_equal(got, ref), (o, float(np.abs(got - ref).max()))
