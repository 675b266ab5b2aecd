"""top_k and min_p on the HIP engine: the launchLogitFilter kernels (`ops.logit_filter`) against numpy
float32 bitwise and their independence of the batch, the device sampler on masked (-inf) logits,
`HipEngine.forward_sample` / `forward_logprobs` with per-row filters (eager, captured and replayed),
tensor parallelism (the root filters the gathered logits) and `dllama-api --batch-invariant 1`.
Reference: see test_sampling_filters.py."""
import concurrent.futures
import itertools
import json

import numpy as np
import pytest

from test_gpu_xgmi import _run, _setup
from test_logprobs import PROMPTS, _post
from test_prefix_cache import _start_api
from test_sampling_controls import PROMPT
from test_sampling_filters import (F32, NEG_INF, deltas, filter_case, k_values, np_filter, run_survivor_set,
                                   run_top1_loop)

pytestmark = pytest.mark.gpu

FILL = -7777.25  # rows the kernel must neither read nor write hold it before and after
KINDS = ("active", "inactive", "skip", "greedy")  # filtered; active flag off; T < 0; T == 0


@pytest.fixture(scope="module")
def ops():
    from distributed_llama_multiusers_amd import ops
    return ops


def row_kinds(rows):
    kinds = [KINDS[b % 4] if rows > 1 else "active" for b in range(rows)]
    if rows >= 5:
        kinds[3] = "active"  # neighbours of every kind
    return kinds


def launch(ops, x, kinds, ks, ds):
    temps = [{"skip": -1.0, "greedy": 0.0}.get(k, 0.8) for k in kinds]
    return ops.logit_filter(x, temps, ks, ds, [k != "inactive" for k in kinds], fill=FILL)


def want_row(x, kind, k, d):
    return np_filter(x, k, d) if kind == "active" else np.full(x.shape[0], FILL, F32)


@pytest.mark.parametrize("rows", [1, 5, 64])
@pytest.mark.parametrize("vocab", [7, 50, 517, 8193, 128256])
def test_logit_filter_kernel_matches_numpy(C, ops, vocab, rows):
    """Every (k, delta, variant) of the CPU test goes through an active row; the launches' other rows
    carry a k and a delta too and keep the sentinel."""
    combos = list(itertools.product(k_values(vocab), deltas(C), ("tie", "zero", "inf")))
    kinds = row_kinds(rows)
    per = kinds.count("active")
    rng = np.random.default_rng(vocab + rows)
    filler = (np.round(rng.standard_normal(vocab) * 24) / 4).astype(F32)
    for at in range(0, len(combos), per):
        todo = iter(combos[at:at + per] + combos[:per])  # (the last launch wraps around)
        x, ks, ds = np.empty((rows, vocab), F32), [], []
        for b, kind in enumerate(kinds):
            k, d, variant = next(todo) if kind == "active" else (2, -1.0, "tie")
            x[b] = filter_case(vocab, k, vocab + 31 * k + b, variant) if kind == "active" else filler
            ks.append(k)
            ds.append(d)
        got = launch(ops, x, kinds, ks, ds)
        assert got.shape == (rows, vocab) and got.dtype == F32
        for b, kind in enumerate(kinds):
            assert got[b].tobytes() == want_row(x[b], kind, ks[b], ds[b]).tobytes(), (at, b, kind, ks[b], ds[b])


def test_logit_filter_kernel_row_independent_and_reproducible(C, ops):
    """A row's output is bitwise the same alone, among 5 and among 64 rows, and from call to call."""
    vocab, kinds = 128256, row_kinds(64)
    assert kinds[0] == kinds[3] == "active"
    rng = np.random.default_rng(3)
    x = (np.round(rng.standard_normal((64, vocab)) * 24) / 4).astype(F32)
    d = deltas(C)
    ks = [(40, 1, 0, 3000)[b % 4] for b in range(64)]
    ds = [d[(b // 2) % 4] for b in range(64)]
    run = lambda n: launch(ops, x[:n], kinds[:n], ks[:n], ds[:n])
    full, again, five, alone = run(64), run(64), run(5), run(1)
    assert full.tobytes() == again.tobytes()
    assert alone[0].tobytes() == five[0].tobytes() == full[0].tobytes() == np_filter(x[0], ks[0], ds[0]).tobytes()
    assert five[3].tobytes() == full[3].tobytes() == np_filter(x[3], ks[3], ds[3]).tobytes()
    assert np.count_nonzero(full[0] > NEG_INF) >= 40 and np.count_nonzero(full[0] > NEG_INF) < vocab


# ---------------------------------------------------------------------------- the sampler on masked rows

def _draw_ok(logits, temp, topp, coin, tok, tol=2e-4):
    """test_gpu_ops._draw_ok: `tok` is a valid draw for `coin` under exact (f64) arithmetic, up to
    `tol` of cumulative mass; masked entries have probability 0."""
    x = logits.astype(np.float64)
    with np.errstate(over="ignore", invalid="ignore"):
        p = np.exp(x / temp - (x / temp).max())
    p /= p.sum()
    if topp <= 0.0 or topp >= 1.0:
        cdf = np.cumsum(p)
        lo = cdf[tok - 1] if tok > 0 else 0.0
        return lo - tol <= coin <= cdf[tok] + tol
    cutoff = (1.0 - topp) / (len(p) - 1)
    cand = np.nonzero(p >= cutoff * (1 - 1e-5))[0]
    order = cand[np.argsort(-p[cand], kind="stable")]
    cum = np.cumsum(p[order])
    last = min(int(np.searchsorted(cum, topp, side="right")), len(order) - 1)
    r = coin * cum[last]
    where = np.nonzero(order == tok)[0]
    if len(where) == 0 or where[0] > last + 1:
        return False
    i = where[0]
    lo = cum[i - 1] if i > 0 else 0.0
    return lo - tol <= r <= cum[i] + tol


def test_sampler_draws_finite_candidates_of_masked_rows(ops):
    """Rows as the filter leaves them: the first 120000 of 128256 logits -inf (most sampler chunks are
    masked whole), and a row with one finite entry. Every draw is a finite-logit index and valid
    for its coin; unmasked rows in the same launch draw what they draw alone."""
    vocab, masked = 128256, 120000
    rng = np.random.default_rng(17)
    base = rng.standard_normal((4, vocab)).astype(F32)
    combos = list(itertools.product((0.6, 1.0), (0.0, 0.9), (0.02, 0.21, 0.4, 0.63, 0.87, 0.985)))
    head = base[0].copy()
    head[:masked] = NEG_INF
    single = np.full(vocab, NEG_INF, F32)
    single[99001] = F32(-3.25)
    rows, specs = [], []
    for temp, topp, coin in combos:
        rows += [head, single]
        specs += [(temp, topp, coin)] * 2
    plain_specs = [(0.6, 0.9, 0.37), (1.0, 0.0, 0.52), (0.6, 0.0, 0.11), (1.0, 0.9, 0.93)]
    x = np.stack(rows + [base[i] for i in range(4)])
    specs += plain_specs
    got = ops.sample(x, [s[0] for s in specs], [s[1] for s in specs], [s[2] for s in specs])
    for b, (temp, topp, coin) in enumerate(specs):
        assert 0 <= got[b] < vocab and np.isfinite(x[b, got[b]]), (b, specs[b], got[b])
        assert _draw_ok(x[b], temp, topp, coin, got[b]), (b, specs[b], got[b])
    assert [got[b] for b in range(1, 2 * len(combos), 2)] == [99001] * len(combos)
    alone = ops.sample(base, [s[0] for s in plain_specs], [s[1] for s in plain_specs], [s[2] for s in plain_specs])
    assert got[-4:] == alone


# ---------------------------------------------------------------------------- HipEngine

def _engine(C, assets, **kw):
    return C.HipEngine(assets["q40"], "q80", kv_bf16=False, max_batch=64, n_slots=4, **kw)


@pytest.mark.parametrize("graphs", [False, True])
def test_engine_top_k_1_draws_the_argmax(C, assets, graphs):
    """(with graphs the 16 steps cover the eager first use of the shape, the capture and the replays)"""
    run_top1_loop(lambda: _engine(C, assets, use_graphs=graphs))


@pytest.mark.parametrize("graphs", [False, True])
def test_engine_draws_stay_in_the_survivor_set(C, assets, graphs):
    run_survivor_set(lambda: _engine(C, assets, use_graphs=graphs), C)


def test_engine_filter_over_graph_replays(C, assets):
    """The same calls on an engine that captures and replays graphs and on one that launches eagerly
    give the same ids; forwards without a filter in between (plain, greedy, penalties only) give
    what they give on an engine that never saw a filter."""
    g, eager, never = _engine(C, assets), _engine(C, assets, use_graphs=False), _engine(C, assets)
    n = len(PROMPT) - 1
    for e in (g, eager, never):
        e.forward(PROMPT[:-1], list(range(n)), [0] * n)
    toks, poss, slots = [PROMPT[-1], 7, 90, 200], [n, 0, 0, 0], [0, 1, 2, 3]
    temps, topps = [0.9, 0.0, 0.7, -1.0], [0.95, 0.9, 1.0, 0.9]
    raw = g.forward(toks, poss, slots)
    best = [int(np.argmax(r)) for r in raw]
    for s in range(6):
        coins = [(0.37 + 0.11 * s) % 1, 0.0, (0.13 + 0.07 * s) % 1, 0.0]
        args = (toks, poss, slots, temps, topps, coins)
        procs = [dict(top_k=1, fresh=s == 0), dict(top_k=2, min_p=0.5), None, dict(top_k=1)]
        ids = g.forward_sample(*args, logit_procs=procs)
        assert ids == eager.forward_sample(*args, logit_procs=procs)
        plain = never.forward_sample(*args)
        assert ids[0] == best[0] and ids[1] == best[1] and ids[2:] == plain[2:] and ids[3] == -1
        assert g.forward_sample(*args) == plain
        # (on slot 2, whose rows above carry no processor: the filtered rows' tokens are counted)
        pen = [None, None, dict(presence=0.5, frequency=0.5, fresh=s == 0), None]
        assert g.forward_sample(*args, logit_procs=pen) == never.forward_sample(*args, logit_procs=pen)


def test_engine_logprobs_with_top_k_score_raw_logits(C, assets):
    e = _engine(C, assets)
    n = len(PROMPT) - 1
    e.forward(PROMPT[:-1], list(range(n)), [0] * n)
    head = ([PROMPT[-1]], [n], [0])
    ids0, vals0, top0 = e.forward_logprobs(*head, [0.0], [0.9], [0.0], [20])
    ids, vals, top = e.forward_logprobs(*head, [0.8], [0.9], [0.93], [20], logit_procs=[dict(top_k=1, fresh=True)])
    assert ids == ids0
    # the masked tokens keep their raw log-probabilities
    assert vals.tobytes() == vals0.tobytes() and top.tobytes() == top0.tobytes()
    assert np.all(np.isfinite(vals[0])) and vals[0, 0] == vals[0, 1]


# ---------------------------------------------------------------------------- tensor parallelism

def _engine_tp_filters(rank, world, port, model, q):
    try:
        C, comm, dist = _setup(rank, world, port, 1 << 16)
        eng = C.HipEngine(model, "q80", kv_bf16=False, rank=rank, world=world, comm=comm, sync_type="f32",
                          max_batch=8, n_slots=2)
        n = len(PROMPT) - 1
        eng.forward(PROMPT[:-1], list(range(n)), [0] * n)
        root = rank == 0
        tok, pos, steps = PROMPT[-1], n, []
        for s in range(6):
            raw = eng.forward([tok], [pos], [0])
            proc = [dict(top_k=1, fresh=s == 0)] if root else None  # the workers' schedule is unchanged
            got = eng.forward_sample([tok], [pos], [0], [0.8], [(0.9, 1.0)[s % 2]], [(0.21 + 0.17 * s) % 1],
                                     logit_procs=proc)
            box = [got[0]]
            dist.broadcast_object_list(box, src=0)  # every rank feeds the root's token
            steps.append((raw[0] if root else None, box[0]))
            tok, pos = box[0], pos + 1
        if comm.timed_out():
            raise AssertionError("a flag wait timed out")
        dist.barrier()
        q.put((rank, steps if root else "worker"))
    except Exception as e:
        q.put((rank, repr(e)))


def test_xgmi_engine_tp_filter_on_root(tmp_path):
    """TP = 2 on one GPU: the root filters the logits gathered to it; top_k = 1 at temperature 0.8
    equals the argmax of forward's gathered logits for 6 steps, no flag wait timed out."""
    from distributed_llama_multiusers_amd.models.synthetic import make_test_assets
    from distributed_llama_multiusers_amd.utils.mfile import FloatType
    m, _, _ = make_test_assets(str(tmp_path), "tiny", FloatType.Q40, seq_len=128, seed=9, dim=512, n_heads=8,
                               n_kv_heads=4, hidden_dim=1024, vocab_size=1024)
    res = _run(_engine_tp_filters, 2, m)
    assert isinstance(res[0], list) and res[1] == "worker", res
    for s, (raw, got) in enumerate(res[0]):
        assert got == int(np.argmax(raw)), (s, got)


# ---------------------------------------------------------------------------- dllama-api

@pytest.fixture(scope="module")
def gpu_api(tmp_path_factory):
    from distributed_llama_multiusers_amd.models.synthetic import make_test_assets
    from distributed_llama_multiusers_amd.utils.mfile import FloatType
    d = str(tmp_path_factory.mktemp("sampling_filters_api"))
    m, t, _ = make_test_assets(d, "tiny", FloatType.Q40, seq_len=256, seed=5, dim=512, n_heads=8, n_kv_heads=4,
                               hidden_dim=1024)
    proc, url = _start_api(m, t, ["--gpu-index", "0", "--batch-invariant", "1", "--max-seq-len", "256"])
    yield url
    proc.kill()
    proc.wait()


def _chat(url, content, max_tokens, **kw):
    """(a random model may end a text inside a UTF-8 sequence: such bytes are read as U+FFFD)"""
    return json.loads(_post(url, content, max_tokens, **kw).read().decode("utf-8", errors="replace"))


def _token_ids(d):
    return [e["token_id"] for e in d["choices"][0]["logprobs"]["content"]]


def test_api_gpu_top_k_1_returns_the_greedy_text(gpu_api):
    greedy = _chat(gpu_api, PROMPTS[2], 16, logprobs=True)
    for seed in (1, 7):
        got = _chat(gpu_api, PROMPTS[2], 16, temperature=0.8, seed=seed, top_k=1, logprobs=True)
        assert got["generated_text"] == greedy["generated_text"] and _token_ids(got) == _token_ids(greedy)


def test_api_gpu_filtered_and_plain_concurrent_equal_solo(gpu_api):
    """--batch-invariant 1: a sampled request without the fields returns the same text alone and next
    to a concurrent request with top_k and min_p, and so does the filtered request."""
    plain_kw = dict(temperature=0.8, seed=5, logprobs=True)
    filt_kw = dict(temperature=0.8, seed=9, top_k=40, min_p=0.05, logprobs=True)
    solo_plain = _chat(gpu_api, PROMPTS[0], 20, **plain_kw)
    solo_filt = _chat(gpu_api, PROMPTS[1], 20, **filt_kw)
    with concurrent.futures.ThreadPoolExecutor(2) as ex:
        f_plain = ex.submit(_chat, gpu_api, PROMPTS[0], 20, **plain_kw)
        f_filt = ex.submit(_chat, gpu_api, PROMPTS[1], 20, **filt_kw)
        got_plain, got_filt = f_plain.result(), f_filt.result()
    assert got_plain["generated_text"] == solo_plain["generated_text"] and _token_ids(got_plain) == _token_ids(solo_plain)
    assert got_filt["generated_text"] == solo_filt["generated_text"] and _token_ids(got_filt) == _token_ids(solo_filt)
