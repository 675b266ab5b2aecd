"""Penalties and logit bias on the HIP engine: the launchLogitProc / launchLogitProcCount kernels
(`ops.logit_proc`, `ops.logit_proc_count`) against numpy float32 bitwise, their independence of
the batch, `HipEngine.forward_sample` / `forward_logprobs` with per-row processors (eager, captured
and replayed), tensor parallelism (the root processes the gathered logits) and
`dllama-api --batch-invariant 1`. Reference: see test_sampling_controls.py."""
import concurrent.futures
import json

import numpy as np
import pytest

from test_gpu_xgmi import _run, _setup
from test_logprobs import PROMPTS, _post
from test_prefix_cache import _start_api
from test_sampling_controls import F32, PROMPT, np_proc, run_penalties_loop

pytestmark = pytest.mark.gpu

FILL = -7777.25  # the output's sentinel: rows that are not drawn keep it
PENALTIES = [(0.5, 1.5), (-2.0, -0.75), (0.0, 0.0), (0.3, 0.0), (0.0, 1.1)]  # (presence, frequency)


@pytest.fixture(scope="module")
def ops():
    from distributed_llama_multiusers_amd import ops
    return ops


def make_case(vocab, rows, seed):
    """rows x vocab logits; rows + 3 slots, row b on slot rows + 2 - b; rows cycle through active,
    drawn but inactive, and not drawn; counts hold 0, 1, 70000; the slots' bias lists cycle through
    none, ids 0 / vocab - 1 / a counted token, and 300 entries."""
    rng = np.random.default_rng(seed)
    S = rows + 3
    x = (rng.standard_normal((rows, vocab)) * 6).astype(F32)
    x[:, vocab // 5] = F32(-0.0)
    c = np.where(rng.random((S, vocab)) < 0.3, rng.integers(1, 40, (S, vocab)), 0).astype(np.uint32)
    c[:, vocab // 2] = 70000
    c[:, vocab // 3] = 1
    c[:, vocab - 2] = 0
    slots = [rows + 2 - b for b in range(rows)]
    kind = [("active", "copy", "skip")[b % 3] if rows > 1 else "active" for b in range(rows)]
    if rows >= 5:
        kind[3] = "active"  # neighbours of every kind
    bias = []
    for s in range(S):
        pick = (s + s // 3) % 3  # (active rows sit 3 slots apart: every kind reaches one of them)
        if pick == 0:
            bias.append({})
        elif pick == 1:
            bias.append({t: float(F32(rng.uniform(-100, 100))) for t in {0, vocab - 1, vocab // 2}})
        else:
            ids = [0, vocab - 1, vocab // 2] + [int(t) for t in rng.permutation(vocab)]
            bias.append({t: float(F32(rng.uniform(-100, 100))) for t in list(dict.fromkeys(ids))[:min(300, vocab)]})
    pen = [PENALTIES[b % len(PENALTIES)] for b in range(rows)]
    temps = [-1.0 if k == "skip" else (0.0, 0.8)[b % 2] for b, k in enumerate(kind)]
    return x, c, slots, kind, bias, pen, temps


def run_case(ops, case):
    x, c, slots, kind, bias, pen, temps = case
    return ops.logit_proc(x, temps, slots, [k == "active" for k in kind], [p[0] for p in pen], [p[1] for p in pen],
                          c, bias, fill=FILL)


def want_row(case, b):
    x, c, slots, kind, bias, pen, _ = case
    if kind[b] == "skip":
        return np.full(x.shape[1], FILL, F32)
    if kind[b] == "copy":
        return x[b]
    return np_proc(x[b], c[slots[b]], pen[b][0], pen[b][1], bias[slots[b]])


@pytest.mark.parametrize("rows", [1, 5, 64])
@pytest.mark.parametrize("vocab", [7, 50, 517, 8193, 128256])
def test_logit_proc_kernel_matches_numpy(ops, vocab, rows):
    case = make_case(vocab, rows, vocab + rows)
    got = run_case(ops, case)
    assert got.shape == (rows, vocab) and got.dtype == F32
    for b in range(rows):
        assert got[b].tobytes() == want_row(case, b).tobytes(), (b, case[3][b])


def test_logit_proc_kernel_row_independent_and_reproducible(ops):
    """A row's output is bitwise the same alone, among 5 and among 64 rows, and from call to call."""
    x, c, slots, kind, bias, pen, temps = make_case(128256, 64, 3)
    sub = lambda n: (x[:n], c, slots[:n], kind[:n], bias, pen[:n], temps[:n])
    assert kind[0] == kind[3] == "active"
    full, again = run_case(ops, sub(64)), run_case(ops, sub(64))
    five, alone = run_case(ops, sub(5)), run_case(ops, sub(1))
    assert full.tobytes() == again.tobytes()
    assert alone[0].tobytes() == five[0].tobytes() == full[0].tobytes()
    assert five[3].tobytes() == full[3].tobytes() == want_row(sub(64), 3).tobytes()


def test_logit_proc_count_kernel_increments_exactly(ops):
    """(slot, id) of the active rows with an id, nothing else: the whole table is compared."""
    rng = np.random.default_rng(8)
    vocab, S = 517, 9
    c = rng.integers(0, 5, (S, vocab)).astype(np.uint32)
    c[7, 516] = 70000
    ids = [516, -1, 0, 33, 516, 12]
    slots = [7, 6, 5, 4, 3, 0]
    active = [1, 1, 1, 0, 1, 1]
    want = c.copy()
    for i, s, a in zip(ids, slots, active):
        if a and i >= 0:
            want[s, i] += 1
    got = ops.logit_proc_count(c, ids, slots, active)
    assert got.dtype == np.uint32 and got.tobytes() == want.tobytes() and got[7, 516] == 70001


# ---------------------------------------------------------------------------- HipEngine

def _engine(C, assets, **kw):
    return C.HipEngine(assets["q40"], "q80", kv_bf16=False, max_batch=64, n_slots=4, **kw)


def test_engine_penalties_loop_single_row(C, assets):
    """24 greedy steps with frequency 1.5 / presence 0.5 against numpy on engine.forward's logits; a
    plain greedy single row would take the argmax tail, a row with a processor takes the sampler."""
    run_penalties_loop(lambda: _engine(C, assets))


def test_engine_penalties_loop_among_inactive_rows(C, assets):
    """The penalised sequence as row 0 of 4-row calls whose other rows have no processor (greedy,
    sampled, not drawn): row 0 matches numpy, the others equal an engine that never saw one."""
    a, b = _engine(C, assets), _engine(C, assets)
    n = len(PROMPT) - 1
    for e in (a, b):
        e.forward(PROMPT[:-1], list(range(n)), [0] * n)
    tok, pos, counts = PROMPT[-1], n, None
    for s in range(24):
        toks, poss, slots = [tok, 7 + s, 90 + s, 200 + s], [pos, s, s, s], [0, 1, 2, 3]
        temps, topps, coins = [0.0, 0.0, 0.7, -1.0], [0.9] * 4, [0.0, 0.0, (0.13 + 0.07 * s) % 1, 0.0]
        raw = a.forward(toks, poss, slots)
        counts = np.zeros(raw.shape[1], np.uint32) if counts is None else counts
        procs = [dict(presence=0.5, frequency=1.5, fresh=s == 0), None, None, None]
        got = a.forward_sample(toks, poss, slots, temps, topps, coins, logit_procs=procs)
        want = int(np.argmax(np_proc(raw[0], counts, 0.5, 1.5)))
        assert got[0] == want, (s, got, want)
        assert got[1:] == b.forward_sample(toks, poss, slots, temps, topps, coins)[1:] and got[3] == -1
        counts[want] += 1
        tok, pos = want, pos + 1


def test_engine_processor_over_graph_replays(C, assets):
    """The same calls on an engine that captures and replays graphs and on one that launches eagerly
    give the same ids; a forward without a processor in between gives what it gives on an engine
    that never saw one."""
    g, eager, never = _engine(C, assets), _engine(C, assets, use_graphs=False), _engine(C, assets)
    n = len(PROMPT) - 1
    for e in (g, eager, never):
        e.forward(PROMPT[:-1], list(range(n)), [0] * n)
    args = ([PROMPT[-1]], [n], [0], [0.9], [0.95], [0.37])
    raw = g.forward(*args[:3])[0]
    best = int(np.argmax(raw))
    for s in range(6):
        proc = dict(presence=2.0, frequency=2.0, fresh=s == 0, bias={best: -100.0})
        ids = g.forward_sample(*args, logit_procs=[proc])
        assert ids == eager.forward_sample(*args, logit_procs=[proc]) and ids != [best]
        plain = g.forward_sample(*args)
        assert plain == never.forward_sample(*args)
        greedy = g.forward_sample(args[0], args[1], args[2], [0.0], [0.9], [0.0])
        assert greedy == never.forward_sample(args[0], args[1], args[2], [0.0], [0.9], [0.0]) == [best]


def test_engine_logprobs_with_bias_score_raw_logits(C, assets):
    e = _engine(C, assets)
    n = len(PROMPT) - 1
    e.forward(PROMPT[:-1], list(range(n)), [0] * n)
    args = ([PROMPT[-1]], [n], [0], [0.0], [0.9], [0.0], [20])
    ids0, vals0, top0 = e.forward_logprobs(*args)
    t = 123
    ids, vals, top = e.forward_logprobs(*args, logit_procs=[dict(fresh=True, bias={t: 100.0})])
    assert ids == [t] != ids0 and top[0, 0] == t
    assert vals[0, 1:].tobytes() == vals0[0, 1:].tobytes() and top[0, 1:].tobytes() == top0[0, 1:].tobytes()
    # the chosen entry is the biased token scored on the raw logits
    raw = e.forward(*args[:3])[0].astype(np.float64)
    lse = raw.max() + np.log(np.exp(raw - raw.max()).sum())
    assert abs(vals[0, 0] - (raw[t] - lse)) <= 1e-4 and vals[0, 0] < vals[0, 1]


# ---------------------------------------------------------------------------- tensor parallelism

def _engine_tp_procs(rank, world, port, model, q):
    try:
        C, comm, dist = _setup(rank, world, port, 1 << 16)
        eng = C.HipEngine(model, "q80", kv_bf16=False, rank=rank, world=world, comm=comm, sync_type="f32",
                          max_batch=8, n_slots=2)
        n = len(PROMPT) - 1
        eng.forward(PROMPT[:-1], list(range(n)), [0] * n)
        root = rank == 0
        forced = eng.forward_sample([PROMPT[-1]], [n], [0], [0.8], [0.9], [0.4],
                                    logit_procs=[dict(fresh=True, bias={123: 100.0})] if root else None)
        tok, pos, steps = PROMPT[-1], n, []
        for s in range(6):
            raw = eng.forward([tok], [pos], [0])
            proc = [dict(presence=0.5, frequency=1.5, fresh=s == 0)] if root else None  # the workers' schedule is unchanged
            got = eng.forward_sample([tok], [pos], [0], [0.0], [0.9], [0.0], logit_procs=proc)
            box = [got[0]]
            dist.broadcast_object_list(box, src=0)  # every rank feeds the root's token
            steps.append((raw[0] if root else None, box[0]))
            tok, pos = box[0], pos + 1
        if comm.timed_out():
            raise AssertionError("a flag wait timed out")
        dist.barrier()
        q.put((rank, (forced, steps) if root else ("worker", None)))
    except Exception as e:
        q.put((rank, repr(e)))


def test_xgmi_engine_tp_processors_on_root(tmp_path):
    """TP = 2 on one GPU: the root processes the logits gathered to it; {t: 100} forces t, a 6-step
    penalties loop matches numpy on forward's gathered logits, no flag wait timed out."""
    from distributed_llama_multiusers_amd.models.synthetic import make_test_assets
    from distributed_llama_multiusers_amd.utils.mfile import FloatType
    m, _, _ = make_test_assets(str(tmp_path), "tiny", FloatType.Q40, seq_len=128, seed=9, dim=512, n_heads=8,
                               n_kv_heads=4, hidden_dim=1024, vocab_size=1024)
    res = _run(_engine_tp_procs, 2, m)
    assert all(isinstance(v, tuple) for v in res.values()), res
    forced, steps = res[0]
    assert forced == [123]
    counts = np.zeros(1024, np.uint32)
    for s, (raw, got) in enumerate(steps):
        want = int(np.argmax(np_proc(raw, counts, 0.5, 1.5)))
        assert got == want, (s, got, want)
        counts[want] += 1


# ---------------------------------------------------------------------------- dllama-api

@pytest.fixture(scope="module")
def gpu_api(tmp_path_factory):
    from distributed_llama_multiusers_amd.models.synthetic import make_test_assets
    from distributed_llama_multiusers_amd.utils.mfile import FloatType
    d = str(tmp_path_factory.mktemp("sampling_controls_api"))
    m, t, _ = make_test_assets(d, "tiny", FloatType.Q40, seq_len=256, seed=5, dim=512, n_heads=8, n_kv_heads=4,
                               hidden_dim=1024)
    proc, url = _start_api(m, t, ["--gpu-index", "0", "--batch-invariant", "1", "--max-seq-len", "256"])
    yield url
    proc.kill()
    proc.wait()


def _chat(url, content, max_tokens, **kw):
    """The response; a penalised random model may end a text inside a UTF-8 sequence, which the
    server passes on as it is: such bytes are read as U+FFFD."""
    return json.loads(_post(url, content, max_tokens, **kw).read().decode("utf-8", errors="replace"))


def _token_ids(d):
    return [e["token_id"] for e in d["choices"][0]["logprobs"]["content"]]


def test_api_gpu_processors_concurrent_equal_solo(gpu_api):
    """--batch-invariant 1, greedy: a request without the fields returns the same text alone and next
    to a concurrent request with penalties and a bias, and so does the penalised request."""
    first = lambda d: _token_ids(d)[0]
    t0 = first(_chat(gpu_api, PROMPTS[1], 1, logprobs=True))  # the unbiased first token: banned below
    ctl = dict(frequency_penalty=1.5, presence_penalty=0.5, logit_bias={"40": 4, str(t0): -100}, logprobs=True)
    solo_plain = _chat(gpu_api, PROMPTS[0], 20)
    solo_ctl = _chat(gpu_api, PROMPTS[1], 20, **ctl)
    with concurrent.futures.ThreadPoolExecutor(2) as ex:
        f_plain = ex.submit(_chat, gpu_api, PROMPTS[0], 20)
        f_ctl = ex.submit(_chat, gpu_api, PROMPTS[1], 20, **ctl)
        got_plain, got_ctl = f_plain.result(), f_ctl.result()
    assert got_plain["generated_text"] == solo_plain["generated_text"]
    assert got_ctl["generated_text"] == solo_ctl["generated_text"] and _token_ids(got_ctl) == _token_ids(solo_ctl)
    assert first(solo_ctl) != t0 and first(got_ctl) == first(solo_ctl)


def test_api_gpu_logit_bias_forces_a_token(gpu_api):
    for kw in (dict(temperature=0), dict(temperature=0.8, seed=7)):
        d = _chat(gpu_api, PROMPTS[2], 9, logit_bias={"123": 100}, logprobs=True, **kw)
        assert _token_ids(d) == [123] * 9
