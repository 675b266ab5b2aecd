"""Structured outputs on the HIP engine: the launchGrammarMask / launchGrammarAdvance kernels
(`ops.grammar_mask`, `ops.grammar_advance`) against the numpy table walk bitwise and their
independence of the batch, `HipEngine.forward_sample` with per-row `grammar` (eager, captured and
replayed, a reused slot with another schema, rows of every kind in one forward), tensor parallelism
(the root masks) and `dllama-api --batch-invariant 1`. Reference: see test_json_schema.py."""
import concurrent.futures
import json

import numpy as np
import pytest

from test_gpu_json_mode import make_pieces
from test_gpu_xgmi import _run, _setup
from test_json_schema import (CASES, F32, FINITE, NAMED_PREFIXES, NEG_INF, NpVocab, compile_case, edge_dfas, np_token_walk,
                              run_grammar_rows, schema_format, valid_document)
from test_logprobs import PROMPTS, _post
from test_prefix_cache import _start_api

pytestmark = pytest.mark.gpu

FILL = -7777.25  # rows the kernel must neither read nor write hold it before and after
# constrained at T > 0; no constraint; T < 0; constrained at T == 0; a JSON-mode row of the same launch
KINDS = ("on", "off", "skip", "greedy", "json")
VOCABS = (261, 517, 8193, 128256)


@pytest.fixture(scope="module")
def ops():
    from distributed_llama_multiusers_amd import ops
    return ops


@pytest.fixture(scope="module")
def vocabs(C):
    out = {}
    for vocab in VOCABS:
        pieces, bos_id, eos = make_pieces(vocab)
        out[vocab] = (C.JsonTable(pieces, bos_id, eos), NpVocab(pieces, bos_id, eos))
    return out


@pytest.fixture(scope="module")
def slots_pool(C):
    """(grammar, state, name) of every slot the mask tests use: the flat schema walked to the named
    states, two other schemas, and the raw edge tables in several of their states."""
    flat = compile_case(C, "flat")
    pool = [(flat, flat.walk(p), name) for name, p in NAMED_PREFIXES.items()]
    arr = compile_case(C, "array")
    pool += [(arr, arr.walk(b'{"l":[{"x":-'), "array"), (compile_case(C, "enum"), compile_case(C, "enum").walk(b'{"e":"'), "enum")]
    for name, g in edge_dfas(C, None):
        pool += [(g, g.start, name + "/start"), (g, 0, name + "/0"), (g, g.n_states // 2, name + "/mid")]
    assert all(s is not None for _, s, _ in pool)
    return pool


def row_kinds(rows):
    kinds = [KINDS[b % 5] if rows > 1 else "on" for b in range(rows)]
    if rows >= 5:
        kinds[3] = "on"  # neighbours of every kind
    return kinds


def launch(ops, x, kinds, table, slots):
    temps = [{"skip": -1.0, "greedy": 0.0}.get(k, 0.8) for k in kinds]
    names = [{"off": "none", "json": "json"}.get(k, "grammar") for k in kinds]
    return ops.grammar_mask(x, temps, names, table, [g for g, _, _ in slots], [s for _, s, _ in slots], fill=FILL)


_WALKED = {}  # (vocabulary, slot name) -> np_token_walk's result: the reference is computed once


def walked(slot, npv):
    g, state, name = slot
    key = (npv.n, name)
    if key not in _WALKED:
        _WALKED[key] = np_token_walk(g.tables(), state, npv)
    return _WALKED[key]


def want_row(x, kind, slot, npv):
    if kind not in ("on", "greedy"):
        return np.full(x.shape[0], FILL, F32)
    return np.where(walked(slot, npv)[0], x, NEG_INF).astype(F32)


def logits(rows, vocab, seed):
    rng = np.random.default_rng(seed)
    x = (np.round(rng.standard_normal((rows, vocab)) * 24) / 4).astype(F32)
    x[:, 5] = NEG_INF
    x[:, 7] = F32(-0.0)
    return x


@pytest.mark.parametrize("rows", [1, 5, 64])
@pytest.mark.parametrize("vocab", VOCABS)
def test_grammar_mask_kernel_matches_the_numpy_walk(ops, vocabs, slots_pool, vocab, rows):
    """Every slot of the pool goes through a constrained row; slots differ in grammar within one launch;
    the launches' other rows (a JSON-mode row among them) keep the sentinel."""
    table, npv = vocabs[vocab]
    kinds = row_kinds(rows)
    per = sum(k in ("on", "greedy") for k in kinds)
    x = logits(rows, vocab, vocab + rows)
    for at in range(0, len(slots_pool), per):
        slots, k = [], at
        for kind in kinds:  # constrained rows take the pool's slots in turn
            slots.append(slots_pool[k % len(slots_pool)])
            k += kind in ("on", "greedy")
        got = launch(ops, x, kinds, table, slots)
        assert got.shape == (rows, vocab) and got.dtype == F32
        for b, kind in enumerate(kinds):
            want = want_row(x[b], kind, slots[b], npv)
            assert got[b].tobytes() == want.tobytes(), (at, b, kind, slots[b][2])
            if kind in ("on", "greedy"):
                assert 1 <= np.count_nonzero(want > NEG_INF) < vocab, slots[b][2]
                if slots[b][2] == "done":  # only the two EOS ids
                    assert np.nonzero(want > NEG_INF)[0].tolist() == [vocab - 4, vocab - 1]


def test_grammar_mask_kernel_row_independent_and_reproducible(ops, vocabs, slots_pool):
    """A row's output is bitwise the same alone, among 5 and among 64 rows, and from call to call."""
    vocab, kinds = 128256, row_kinds(64)
    table, npv = vocabs[vocab]
    slots = [slots_pool[(2 + b) % len(slots_pool)] for b in range(64)]
    x = logits(64, vocab, 3)
    run = lambda n: launch(ops, x[:n], kinds[:n], table, slots[:n])
    full, again, five, alone = run(64), run(64), run(5), run(1)
    assert full.tobytes() == again.tobytes()
    assert alone[0].tobytes() == five[0].tobytes() == full[0].tobytes() == want_row(x[0], "on", slots[0], npv).tobytes()
    assert five[3].tobytes() == full[3].tobytes() == want_row(x[3], "on", slots[3], npv).tobytes()


@pytest.mark.parametrize("vocab", [517, 128256])
def test_grammar_advance_kernel_matches_the_host(ops, vocabs, slots_pool, vocab):
    """Half of the drawn ids are taken from the allowed ones of the row's state, the rest are random,
    -1 and `vocab` included; rows that are not constrained, or do not draw, keep their state."""
    table, npv = vocabs[vocab]
    rng = np.random.default_rng(vocab)
    walks = [walked(slot, npv) for slot in slots_pool]
    for rows in (1, 5, 64):
        kinds = row_kinds(rows)
        pick = [int(rng.integers(len(slots_pool))) for _ in range(rows)]
        slots = [slots_pool[i] for i in pick]
        ids = [int(rng.choice(np.flatnonzero(walks[i][0]))) if rng.random() < 0.5 else int(rng.integers(-1, vocab + 1)) for i in pick]
        if rows == 64:
            ids[0], ids[3] = -1, vocab
        temps = [{"skip": -1.0, "greedy": 0.0}.get(k, 0.8) for k in kinds]
        names = [{"off": "none", "json": "json"}.get(k, "grammar") for k in kinds]
        got = ops.grammar_advance(temps, names, ids, table, [g for g, _, _ in slots], [s for _, s, _ in slots])
        moved = 0
        for b, kind in enumerate(kinds):
            allowed, nxt = walks[pick[b]]
            want = slots[b][1]
            if kind in ("on", "greedy") and 0 <= ids[b] < vocab and allowed[ids[b]]:
                want = int(nxt[ids[b]])
            assert got[b] == want, (rows, b, kind, ids[b])
            moved += want != slots[b][1]
        assert moved >= 1 or rows < 64


# ---------------------------------------------------------------------------- HipEngine

@pytest.fixture(scope="module")
def synth_table(C, tmp_path_factory):
    from distributed_llama_multiusers_amd.models.synthetic import make_tokenizer
    info = make_tokenizer(str(tmp_path_factory.mktemp("schema_tok_gpu") / "t.t"), 512)
    return C.JsonTable(info["tokens"], info["bos_id"], info["eos"])


def _engine(C, assets, table, **kw):
    e = C.HipEngine(assets["q40"], "q80", kv_bf16=False, max_batch=64, n_slots=4, **kw)
    e.set_json_table(table)
    return e


@pytest.mark.parametrize("graphs", [False, True])
def test_engine_grammar_rows_follow_the_host_pipeline(C, assets, synth_table, graphs):
    """(with graphs the steps cover the eager first use of the shape, the capture and the replays; the
    second request reuses the slots with other schemas: the stale-table case)"""
    run_grammar_rows(_engine(C, assets, synth_table, use_graphs=graphs), C, synth_table, steps=6)


@pytest.fixture(scope="module")
def stage_backends(C, assets, synth_table):
    """One HIP engine with graphs on and the CPU backend, for every stage set: f32 weights and f32 KV,
    where the two backends' logits agree to 1e-4 of their range (test_gpu_engine.py)."""
    gpu = C.HipEngine(assets["f32"], "f32", kv_bf16=False, max_batch=64, n_slots=4, use_graphs=True)
    cpu = C.cpu_backend(assets["f32"], "f32", 2, 128, 64, 4)
    gpu.set_json_table(synth_table)
    cpu.set_json_table(synth_table)
    return gpu, cpu


@pytest.mark.parametrize("grammar", [False, True])
@pytest.mark.parametrize("json_mode", [False, True])
@pytest.mark.parametrize("filtered", [False, True])
def test_engine_every_stage_set_draws_what_the_cpu_backend_draws(C, stage_backends, synth_table, filtered, json_mode, grammar):
    """The 8 sets of draw stages that a forward with processors can have, each as the same 2-row forward
    run three times from fresh slots on one engine: the eager first use of its graph key, the capture
    and a replay. Every set has the rows, bucket and flags of the others, so only its stages keep its
    graph apart from theirs; all three runs equal the CPU backend's draw for the same rows. Both rows
    are drawn flat (T = 1.5, no top-p) with coins past the mass of their 3 best tokens, so top_k = 3
    changes a draw in every set (the grammar's start state allows one token: there the other row's
    draw moves), which the CPU backend's own ids must show."""
    gpu, cpu = stage_backends

    def procs(with_filter):
        row0 = dict(presence=0.5, frequency=0.25, bias={34: 1.0}, fresh=True)
        row1 = dict(bias={35: 0.5}, fresh=True)
        if grammar:
            row0["grammar"] = compile_case(C, "flat", synth_table)
            row1["json"] = json_mode
        else:
            row0["json"] = json_mode
        if with_filter:
            row0["top_k"] = row1["top_k"] = 3
        return [row0, row1]

    args = ([65, 66], [0, 0], [0, 1], [1.5, 1.5], [1.0, 1.0], [0.9, 0.5])
    want = cpu.forward_sample(*args, logit_procs=procs(filtered))
    assert want != cpu.forward_sample(*args, logit_procs=procs(not filtered))  # the filter decides a draw
    for use in ("eager", "capture", "replay"):
        assert gpu.forward_sample(*args, logit_procs=procs(filtered)) == want, use


def test_engine_mixed_forward_equals_each_row_on_its_own_path(C, assets, synth_table):
    """One forward with a schema row, a JSON-mode row, a penalties row and a plain row: every row draws
    what it draws in an engine whose forwards hold that row's processor only (the existing paths for
    rows 1 to 3). All engines are fed the mixed forward's tokens, so their logits are the same."""
    g = compile_case(C, "flat", synth_table)
    mixed = _engine(C, assets, synth_table)
    alone = [_engine(C, assets, synth_table) for _ in range(4)]
    toks = [65, 66, 67, 68]
    for s in range(6):
        args = (toks, [s] * 4, [0, 1, 2, 3], [0.8, 0.0, 0.7, 0.9], [0.9, 0.9, 1.0, 0.9], [(0.3 + 0.13 * s) % 1, 0.0, 0.6, 0.45])
        procs = [dict(grammar=g, fresh=s == 0), dict(json=True, fresh=s == 0), dict(presence=0.5, frequency=0.2, fresh=s == 0), None]
        got = mixed.forward_sample(*args, logit_procs=procs)
        for b in range(4):
            only = [p if i == b else None for i, p in enumerate(procs)]
            assert alone[b].forward_sample(*args, logit_procs=only if b < 3 else None)[b] == got[b], (s, b)
        toks = got


def test_engine_forwards_without_a_grammar_are_what_they_were(C, assets, synth_table):
    bare = C.HipEngine(assets["q40"], "q80", kv_bf16=False, max_batch=64, n_slots=4)
    g = compile_case(C, "finite", synth_table)
    with pytest.raises(RuntimeError):
        bare.forward_sample([3], [0], [0], [0.8], [0.9], [0.3], logit_procs=[dict(grammar=g, fresh=True)])
    e = _engine(C, assets, synth_table)
    args = ([65, 66, 67], [0, 0, 0], [0, 1, 2], [0.8, 0.0, 0.7], [0.9, 0.9, 1.0], [0.3, 0.0, 0.6])
    for s in range(4):
        pen = [dict(presence=0.5, fresh=s == 0), None, dict(top_k=4, fresh=s == 0)]
        assert e.forward_sample(*args) == bare.forward_sample(*args)
        assert e.forward_sample(*args, logit_procs=pen) == bare.forward_sample(*args, logit_procs=pen)
        e.forward_sample([65], [s], [3], [0.8], [0.9], [0.4], logit_procs=[dict(grammar=g, fresh=s == 0)])


# ---------------------------------------------------------------------------- tensor parallelism

def _engine_tp_grammar(rank, world, port, model, q):
    try:
        C, comm, dist = _setup(rank, world, port, 1 << 16)
        from distributed_llama_multiusers_amd.models.synthetic import SPECIAL_TOKENS
        eng = C.HipEngine(model, "q80", kv_bf16=False, rank=rank, world=world, comm=comm, sync_type="f32",
                          max_batch=8, n_slots=2)
        pieces = [bytes([i]) for i in range(256)] + [b"ab%d" % i for i in range(1024 - 256 - 5)] + SPECIAL_TOKENS
        table = C.JsonTable(pieces, 1019, [1020, 1023])
        root = rank == 0
        g = C.Grammar.from_schema(json.dumps(CASES["flat"][0]), table)
        if root:
            eng.set_json_table(table)
        tok, steps, state = 65, [], g.start
        for s in range(6):
            raw = eng.forward([tok], [s], [0])
            proc = [dict(grammar=g, fresh=s == 0)] if root else None  # the workers' schedule is unchanged
            got = eng.forward_sample([tok], [s], [0], [0.0], [0.9], [0.0], logit_procs=proc)
            box = [got[0]]
            dist.broadcast_object_list(box, src=0)  # every rank feeds the root's token
            if root:
                want = C.cpu_ops.sample_host(g.mask_host(raw[0], state), 0.0, 0.9, 0.0)
                state = g.advance_host(state, box[0])
                steps.append((want, box[0]))
            tok = box[0]
        if comm.timed_out():
            raise AssertionError("a flag wait timed out")
        dist.barrier()
        q.put((rank, steps if root else "worker"))
    except Exception as e:
        q.put((rank, repr(e)))


def test_xgmi_engine_tp_grammar_mask_on_root(tmp_path):
    """TP = 2 on one GPU: the root masks the logits gathered to it; 6 greedy constrained steps equal the
    host pipeline on forward's gathered logits, no flag wait timed out."""
    from distributed_llama_multiusers_amd.models.synthetic import make_test_assets
    from distributed_llama_multiusers_amd.utils.mfile import FloatType
    m, _, _ = make_test_assets(str(tmp_path), "tiny", FloatType.Q40, seq_len=128, seed=9, dim=512, n_heads=8,
                               n_kv_heads=4, hidden_dim=1024, vocab_size=1024)
    res = _run(_engine_tp_grammar, 2, m)
    assert isinstance(res[0], list) and res[1] == "worker", res
    assert len(res[0]) == 6
    for s, (want, got) in enumerate(res[0]):
        assert got == want, (s, got, want)


# ---------------------------------------------------------------------------- dllama-api

@pytest.fixture(scope="module")
def gpu_api(tmp_path_factory):
    from distributed_llama_multiusers_amd.models.synthetic import make_test_assets
    from distributed_llama_multiusers_amd.utils.mfile import FloatType
    d = str(tmp_path_factory.mktemp("json_schema_api"))
    m, t, _ = make_test_assets(d, "tiny", FloatType.Q40, seq_len=256, seed=5, dim=512, n_heads=8, n_kv_heads=4,
                               hidden_dim=1024)
    proc, url = _start_api(m, t, ["--gpu-index", "0", "--batch-invariant", "1", "--max-seq-len", "256"])
    yield url
    proc.kill()
    proc.wait()


def _chat(url, content, max_tokens, **kw):
    return json.loads(_post(url, content, max_tokens, **kw).read().decode("utf-8", errors="replace"))


def test_api_gpu_six_schema_requests_together_equal_alone(gpu_api):
    """--batch-invariant 1: six schema requests sent together return what each returns alone, and every
    reply is a document of its schema."""
    rf = schema_format(FINITE)
    reqs = [dict(temperature=0.8, seed=3 + i, response_format=rf, logprobs=True) for i in range(4)]
    reqs += [dict(temperature=0, response_format=rf, logprobs=True),
             dict(temperature=0.8, seed=9, top_k=40, presence_penalty=0.5, response_format=rf, logprobs=True)]
    prompts = [PROMPTS[i % len(PROMPTS)] for i in range(6)]
    ids = lambda d: [e["token_id"] for e in d["choices"][0]["logprobs"]["content"]]
    alone = [_chat(gpu_api, p, 100, **kw) for p, kw in zip(prompts, reqs)]
    with concurrent.futures.ThreadPoolExecutor(6) as ex:
        futs = [ex.submit(_chat, gpu_api, p, 100, **kw) for p, kw in zip(prompts, reqs)]
        together = [f.result() for f in futs]
    for a, t in zip(alone, together):
        assert t["generated_text"] == a["generated_text"] and ids(t) == ids(a)
        assert a["choices"][0]["finish_reason"] == t["choices"][0]["finish_reason"] == "stop"
        assert valid_document(FINITE, a["generated_text"].encode()), a["generated_text"]
