"""JSON mode on the HIP engine: the launchJsonMask / launchJsonAdvance kernels (`ops.json_mask`,
`ops.json_advance`) against `JsonTable.mask_host` / `advance_host` bitwise and their independence of
the batch, `HipEngine.forward_sample` / `forward_logprobs` with per-row `json` (eager, captured and
replayed, over several steps and a reused slot), tensor parallelism (the root masks) and
`dllama-api --batch-invariant 1`. Reference: see test_json_mode.py."""
import concurrent.futures
import json
import random

import numpy as np
import pytest

from test_gpu_xgmi import _run, _setup
from test_json_mode import (CORNER_PREFIXES, F32, JSON, LEX_DONE, MAX_DEPTH, MAX_WS, NEG_INF, c_lex,
                            check_bias_driven_object, run_json_rows)
from test_logprobs import PROMPTS, _post
from test_prefix_cache import _start_api

pytestmark = pytest.mark.gpu

FILL = -7777.25  # rows the kernel must neither read nor write hold it before and after
KINDS = ("on", "off", "skip", "greedy")  # constrained at T > 0; flag off; T < 0; constrained at T == 0
# START, in a string, mid-escape, mid-\u, mid-UTF-8, mid-number, depth 64, whitespace at the cap, DONE, ...
STATE_PREFIXES = [b"", b'{"k":"v', b'{"k":"\\', b'{"\\u1', b'{"k":"\xe6\x97', b'{"k":1.5', b'{"k":-',
                  b'{"a":' + b"[" * (MAX_DEPTH - 1), b"{" + b" " * MAX_WS, b"{}", b'{"k":[1', b'{"k":[{"a":"b"',
                  b'{"k":tr', b'{"k"']


@pytest.fixture(scope="module")
def ops():
    from distributed_llama_multiusers_amd import ops
    return ops


def make_pieces(vocab):
    """256 byte pieces, generated pieces up to the last 5 ids, 5 specials (2 of them EOS). The
    generated ones: fragments of JSON text of 1 to more than 64 bytes, pieces that close several
    containers, pieces that split a UTF-8 sequence, all-whitespace pieces and an empty piece."""
    rng = random.Random(vocab)
    fixed = [b"", b'"}]}', b'"}', b'"]}', b"}]}", b"]]", b'":"', b'":', b'",', b'","', b"\xe6", b"\x97\xa5", b"\xe6\x97",
             b"\xa5", b"\xf0\x9f", b"\x98\x80", b" ", b"  ", b"\n", b" \n\t\r", b" " * MAX_WS, b" " * (MAX_WS + 1), b"true",
             b"false", b"null", b"1.5e-3", b'{"', b"[[", b'\\u00e9', b"\\n", b"x" * 64, b"y" * 65, b"z" * 130, b"0" * 70]
    atoms = [b"a", b"b", b" ", b"e", b"1", b"0", b".", b"-", b'"', b",", b":", b"{", b"}", b"[", b"]", b"\\", b"n", b"u",
             b"t", b"\xc3\xa9", b"\xe6\x97\xa5", b"\n"]
    pieces = [bytes([i]) for i in range(256)]
    n_regular = vocab - 5
    for p in fixed:
        if len(pieces) < n_regular:
            pieces.append(p)
    while len(pieces) < n_regular:
        n = rng.choice([1, 2, 2, 3, 3, 4, 5, 6, 8, 12, 20, 40, 66])
        text = b"".join(rng.choice(atoms[:5] if rng.random() < 0.6 else atoms) for _ in range(n))
        pieces.append(text)
    pieces += [b"<|bos|>", b"<|eos|>", b"<|a|>", b"<|b|>", b"<|eot|>"]
    return pieces, n_regular, [n_regular + 1, n_regular + 4]


@pytest.fixture(scope="module")
def tables(C):
    out = {}
    for vocab in (261, 517, 8193, 128256):
        pieces, bos_id, eos = make_pieces(vocab)
        out[vocab] = (C.JsonTable(pieces, bos_id, eos), pieces)
    return out


def row_kinds(rows):
    kinds = [KINDS[b % 4] if rows > 1 else "on" for b in range(rows)]
    if rows >= 5:
        kinds[3] = "on"  # neighbours of every kind
    return kinds


def launch(ops, x, kinds, table, states):
    temps = [{"skip": -1.0, "greedy": 0.0}.get(k, 0.8) for k in kinds]
    return ops.json_mask(x, temps, [k != "off" for k in kinds], table, states, fill=FILL)


def want_row(table, x, kind, state):
    return table.mask_host(x, state) if kind in ("on", "greedy") else np.full(x.shape[0], FILL, F32)


def logits(rows, vocab, seed):
    rng = np.random.default_rng(seed)
    x = (np.round(rng.standard_normal((rows, vocab)) * 24) / 4).astype(F32)
    x[:, 5] = NEG_INF
    x[:, 7] = F32(-0.0)
    return x


@pytest.mark.parametrize("rows", [1, 5, 64])
@pytest.mark.parametrize("vocab", [261, 517, 8193, 128256])
def test_json_mask_kernel_matches_host(C, ops, tables, vocab, rows):
    """Every state goes through a constrained row; the launches' other rows carry a state too and keep
    the sentinel."""
    table, _ = tables[vocab]
    states = [C.cpu_ops.json_walk(p) for p in STATE_PREFIXES]
    kinds = row_kinds(rows)
    per = sum(k in ("on", "greedy") for k in kinds)
    x = logits(rows, vocab, vocab + rows)
    survivors = 0
    for at in range(0, len(states), per):
        row_states = [states[(at + b) % len(states)] for b in range(rows)]
        got = launch(ops, x, kinds, table, row_states)
        assert got.shape == (rows, vocab) and got.dtype == F32
        for b, kind in enumerate(kinds):
            want = want_row(table, x[b], kind, row_states[b])
            assert got[b].tobytes() == want.tobytes(), (at, b, kind)
            if kind in ("on", "greedy"):
                n = np.count_nonzero(want > NEG_INF)
                assert 1 <= n < vocab
                survivors += n
                if c_lex(row_states[b]) == LEX_DONE:  # only the two EOS ids
                    assert np.nonzero(want > NEG_INF)[0].tolist() == [vocab - 4, vocab - 1]
    assert survivors > 0


def test_json_mask_kernel_row_independent_and_reproducible(C, ops, tables):
    """A row's output is bitwise the same alone, among 5 and among 64 rows, and from call to call."""
    vocab, kinds = 128256, row_kinds(64)
    table, _ = tables[vocab]
    states = [C.cpu_ops.json_walk(STATE_PREFIXES[(1 + b) % len(STATE_PREFIXES)]) for b in range(64)]
    x = logits(64, vocab, 3)
    run = lambda n: launch(ops, x[:n], kinds[:n], table, states[:n])
    full, again, five, alone = run(64), run(64), run(5), run(1)
    assert full.tobytes() == again.tobytes()
    assert alone[0].tobytes() == five[0].tobytes() == full[0].tobytes() == table.mask_host(x[0], states[0]).tobytes()
    assert five[3].tobytes() == full[3].tobytes() == table.mask_host(x[3], states[3]).tobytes()


@pytest.mark.parametrize("vocab", [517, 128256])
def test_json_advance_kernel_matches_host(C, ops, tables, vocab):
    """Random drawn tokens, half of them taken from the allowed ones of the row's state (random ids are
    mostly forbidden); rows that are not constrained, or do not draw, keep their state."""
    table, _ = tables[vocab]
    rng = np.random.default_rng(vocab)
    base = [C.cpu_ops.json_walk(p) for p in STATE_PREFIXES + CORNER_PREFIXES]
    ones = np.ones(vocab, F32)
    allowed = [np.nonzero(table.mask_host(ones, s) > NEG_INF)[0] for s in base]
    for rows in (1, 5, 64):
        kinds = row_kinds(rows)
        pick = [int(rng.integers(len(base))) for _ in range(rows)]
        states = [base[i] for i in pick]
        ids = [int(rng.choice(allowed[i])) if rng.random() < 0.5 else int(rng.integers(-1, vocab + 1)) for i in pick]
        temps = [{"skip": -1.0, "greedy": 0.0}.get(k, 0.8) for k in kinds]
        got = ops.json_advance(temps, [k != "off" for k in kinds], ids, table, states)
        moved = 0
        for b, kind in enumerate(kinds):
            want = table.advance_host(states[b], ids[b]) if kind in ("on", "greedy") else states[b]
            assert list(got[b]) == list(want), (rows, b, kind, ids[b])
            moved += list(want) != list(states[b])
        assert moved >= 1 or rows < 64


# ---------------------------------------------------------------------------- HipEngine

@pytest.fixture(scope="module")
def synth_table(C, tmp_path_factory):
    from distributed_llama_multiusers_amd.models.synthetic import make_tokenizer
    info = make_tokenizer(str(tmp_path_factory.mktemp("json_tok_gpu") / "t.t"), 512)
    return C.JsonTable(info["tokens"], info["bos_id"], info["eos"])


def _engine(C, assets, table, **kw):
    e = C.HipEngine(assets["q40"], "q80", kv_bf16=False, max_batch=64, n_slots=4, **kw)
    e.set_json_table(table)
    return e


@pytest.mark.parametrize("graphs", [False, True])
def test_engine_json_rows_follow_the_host_pipeline(C, assets, synth_table, graphs):
    """(with graphs the steps cover the eager first use of the shape, the capture and the replays; the
    state lives on the device from step to step)"""
    run_json_rows(_engine(C, assets, synth_table, use_graphs=graphs), C, synth_table, steps=6)


def test_engine_json_needs_a_table_and_leaves_other_forwards_alone(C, assets, synth_table):
    bare = C.HipEngine(assets["q40"], "q80", kv_bf16=False, max_batch=64, n_slots=4)
    with pytest.raises(RuntimeError):
        bare.forward_sample([3], [0], [0], [0.8], [0.9], [0.3], logit_procs=[dict(json=True, fresh=True)])
    e = _engine(C, assets, synth_table)
    args = ([65, 66, 67], [0, 0, 0], [0, 1, 2], [0.8, 0.0, 0.7], [0.9, 0.9, 1.0], [0.3, 0.0, 0.6])
    for s in range(4):
        pen = [dict(presence=0.5, fresh=s == 0), None, dict(top_k=4, fresh=s == 0)]
        assert e.forward_sample(*args) == bare.forward_sample(*args)
        assert e.forward_sample(*args, logit_procs=pen) == bare.forward_sample(*args, logit_procs=pen)
        # (on a slot of its own: a constrained row's tokens are counted in its slot like any processor row's)
        e.forward_sample([65], [s], [3], [0.8], [0.9], [0.4], logit_procs=[dict(json=True, fresh=s == 0)])


def test_engine_logprobs_with_json_score_raw_logits(C, assets, synth_table):
    e = _engine(C, assets, synth_table)
    head = ([65], [0], [0])
    raw = e.forward(*head)[0]
    ids0, vals0, top0 = e.forward_logprobs(*head, [0.0], [0.9], [0.0], [20])
    ids, vals, top = e.forward_logprobs(*head, [0.0], [0.9], [0.0], [20], logit_procs=[dict(json=True, fresh=True)])
    want = C.cpu_ops.sample_host(synth_table.mask_host(raw, C.cpu_ops.json_walk(b"")), 0.0, 0.9, 0.0)
    assert ids == [want] and synth_table.advance_host(C.cpu_ops.json_walk(b""), want) != C.cpu_ops.json_walk(b"")
    # the best-token list scores the raw logits, masked tokens included
    assert vals[:, 1:].tobytes() == vals0[:, 1:].tobytes() and top[:, 1:].tobytes() == top0[:, 1:].tobytes()
    assert top[0, 0] == want and np.isfinite(vals[0, 0])


# ---------------------------------------------------------------------------- tensor parallelism

def _engine_tp_json(rank, world, port, model, q):
    try:
        C, comm, dist = _setup(rank, world, port, 1 << 16)
        from distributed_llama_multiusers_amd.models.synthetic import SPECIAL_TOKENS
        eng = C.HipEngine(model, "q80", kv_bf16=False, rank=rank, world=world, comm=comm, sync_type="f32",
                          max_batch=8, n_slots=2)
        pieces = [bytes([i]) for i in range(256)] + [b"ab%d" % i for i in range(1024 - 256 - 5)] + SPECIAL_TOKENS
        table = C.JsonTable(pieces, 1019, [1020, 1023])
        root = rank == 0
        if root:
            eng.set_json_table(table)
        tok, steps = 65, []
        state = C.cpu_ops.json_walk(b"")
        for s in range(6):
            raw = eng.forward([tok], [s], [0])
            proc = [dict(json=True, fresh=s == 0)] if root else None  # the workers' schedule is unchanged
            got = eng.forward_sample([tok], [s], [0], [0.0], [0.9], [0.0], logit_procs=proc)
            box = [got[0]]
            dist.broadcast_object_list(box, src=0)  # every rank feeds the root's token
            if root:
                want = C.cpu_ops.sample_host(table.mask_host(raw[0], state), 0.0, 0.9, 0.0)
                state = table.advance_host(state, box[0])
                steps.append((want, box[0]))
            tok = box[0]
        if comm.timed_out():
            raise AssertionError("a flag wait timed out")
        dist.barrier()
        q.put((rank, steps if root else "worker"))
    except Exception as e:
        q.put((rank, repr(e)))


def test_xgmi_engine_tp_json_mask_on_root(tmp_path):
    """TP = 2 on one GPU: the root masks the logits gathered to it; 6 greedy constrained steps equal the
    host pipeline on forward's gathered logits, no flag wait timed out."""
    from distributed_llama_multiusers_amd.models.synthetic import make_test_assets
    from distributed_llama_multiusers_amd.utils.mfile import FloatType
    m, _, _ = make_test_assets(str(tmp_path), "tiny", FloatType.Q40, seq_len=128, seed=9, dim=512, n_heads=8,
                               n_kv_heads=4, hidden_dim=1024, vocab_size=1024)
    res = _run(_engine_tp_json, 2, m)
    assert isinstance(res[0], list) and res[1] == "worker", res
    assert len(res[0]) == 6
    for s, (want, got) in enumerate(res[0]):
        assert got == want, (s, got, want)


# ---------------------------------------------------------------------------- dllama-api

@pytest.fixture(scope="module")
def gpu_api(tmp_path_factory):
    from distributed_llama_multiusers_amd.models.synthetic import make_test_assets
    from distributed_llama_multiusers_amd.utils.mfile import FloatType
    d = str(tmp_path_factory.mktemp("json_mode_api"))
    m, t, _ = make_test_assets(d, "tiny", FloatType.Q40, seq_len=256, seed=5, dim=512, n_heads=8, n_kv_heads=4,
                               hidden_dim=1024)
    proc, url = _start_api(m, t, ["--gpu-index", "0", "--batch-invariant", "1", "--max-seq-len", "256"])
    yield url
    proc.kill()
    proc.wait()


def _chat(url, content, max_tokens, **kw):
    return json.loads(_post(url, content, max_tokens, **kw).read().decode("utf-8", errors="replace"))


def test_api_gpu_bias_driven_reply_is_the_empty_pair(gpu_api):
    check_bias_driven_object(gpu_api)


def test_api_gpu_six_constrained_together_equal_alone(gpu_api):
    """--batch-invariant 1: six constrained requests sent together return what each returns alone."""
    reqs = [dict(temperature=0.8, seed=3 + i, response_format=JSON, logprobs=True) for i in range(4)]
    reqs += [dict(temperature=0, response_format=JSON, logprobs=True),
             dict(temperature=0.8, seed=9, top_k=40, presence_penalty=0.5, response_format=JSON, logprobs=True)]
    prompts = [PROMPTS[i % len(PROMPTS)] for i in range(6)]
    ids = lambda d: [e["token_id"] for e in d["choices"][0]["logprobs"]["content"]]
    alone = [_chat(gpu_api, p, 20, **kw) for p, kw in zip(prompts, reqs)]
    with concurrent.futures.ThreadPoolExecutor(6) as ex:
        futs = [ex.submit(_chat, gpu_api, p, 20, **kw) for p, kw in zip(prompts, reqs)]
        together = [f.result() for f in futs]
    for a, t in zip(alone, together):
        assert t["generated_text"] == a["generated_text"] and ids(t) == ids(a)
        assert t["choices"][0]["finish_reason"] == a["choices"][0]["finish_reason"]
        assert a["generated_text"].lstrip(" \t\r\n").startswith("{")
