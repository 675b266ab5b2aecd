"""Prompt scoring on the HIP engine: the launchLogprobs kernel with targets (`ops.logprobs(...,
targets=...)`: slot 0 scores a given token on a row that draws none) against numpy float64, its
bitwise independence of the batch and of the argument's presence, `HipEngine.forward_logprobs` with
targets (chunks, a single row, graph replays, tensor parallelism) and `/v1/completions` of
`dllama-api --batch-invariant 1`. Tolerance and reference: see test_logprobs.py."""
import numpy as np
import pytest

from test_completions import P6, concurrent_equal_solo, prompt_ids, targets_cases, teacher_forcing
from test_gpu_xgmi import _run, _setup
from test_logprobs import SLOTS, check_row
from test_prefix_cache import _start_api

pytestmark = pytest.mark.gpu

REQ = [-1, 0, 1, 5, 20]  # per row: none, the scored token only, k = 1 / 5 / 20


@pytest.fixture(scope="module")
def ops():
    from distributed_llama_multiusers_amd import ops
    return ops


def same(a, b):
    return a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes()


@pytest.mark.parametrize("vocab", [128256, 8193, 50])
def test_logprobs_kernel_targets_match_reference(ops, vocab):
    """Row 0 asks for nothing, row 1 has no target (its sampled id is scored), row 2's target is one of
    several tied maxima (not the lowest id), row 3 scores the last token of the vocabulary, row 4 a
    target among k = 20."""
    rng = np.random.default_rng(vocab)
    x = (rng.standard_normal((5, vocab)) * 6).astype(np.float32)
    ties = sorted(int(i) for i in rng.choice(vocab, 4, replace=False))
    x[2, ties] = x[2].max() + 1
    ids = [int(i) for i in rng.integers(0, vocab, 5)]
    targets = [3, -1, ties[2], vocab - 1, int(rng.integers(0, vocab))]
    vals, top = ops.logprobs(x, ids, REQ, targets=targets)
    assert vals.shape == (5, SLOTS) and top.shape == (5, SLOTS)
    assert (top[0] == -2).all() and (vals[0] == 0).all()  # the row was not written
    for b in range(1, 5):
        check_row(x[b], targets[b] if targets[b] >= 0 else ids[b], REQ[b], vals[b], top[b])
    assert top[2, 0] == ties[2] and top[2, 1] == ties[0] and vals[2, 0] == vals[2, 1]  # the lowest id leads the tie


def test_logprobs_kernel_targets_independent(ops):
    """No targets, targets=None and all -1 are bitwise one call; a target row is bitwise the same
    alone, among 5 and among 64 rows, whatever the other rows ask for."""
    rng = np.random.default_rng(9)
    x = (rng.standard_normal((64, 128256)) * 6).astype(np.float32)
    ids = [int(i) for i in rng.integers(0, 128256, 64)]
    plain = ops.logprobs(x[:5], ids[:5], REQ)
    assert same(plain, ops.logprobs(x[:5], ids[:5], REQ, targets=None))
    assert same(plain, ops.logprobs(x[:5], ids[:5], REQ, targets=[-1] * 5))
    t = 77777
    alone = ops.logprobs(x[:1], ids[:1], [20], targets=[t])
    five = ops.logprobs(x[:5], ids[:5], [20, -1, 5, 0, 20], targets=[t, -1, 4, -1, 128255])
    full = ops.logprobs(x, ids, [20] * 64, targets=[t] + [-1, 5] * 31 + [9])
    for other in (five, full):
        assert alone[0][0].tobytes() == other[0][0].tobytes() and alone[1][0].tobytes() == other[1][0].tobytes()
    check_row(x[0], t, 20, alone[0][0], alone[1][0])
    check_row(x[63], 9, 20, full[0][63], full[1][63])
    # slots 1..k do not depend on what slot 0 scores
    assert full[0][0, 1:].tobytes() == ops.logprobs(x[:1], ids[:1], [20])[0][0, 1:].tobytes()


# ---------------------------------------------------------------------------- HipEngine.forward_logprobs

def test_engine_forward_logprobs_targets(C, assets):
    """The 6-row chunk, the 4 + 2 split and (n = 1 takes other GEMV paths) a single-row forward with a
    target, each against engine.forward's logits."""
    e = targets_cases(lambda: C.HipEngine(assets["q40"], "q80", kv_bf16=False, max_batch=64, n_slots=3))
    e.forward(P6[:3], [0, 1, 2], [0] * 3)
    logits = e.forward([P6[3]], [3], [0])
    for k in (0, 20):
        ids, vals, top = e.forward_logprobs([P6[3]], [3], [0], [-1.0], [0.9], [0.0], [k], targets=[P6[4]])
        assert ids == [-1]
        check_row(logits[0], P6[4], k, vals[0], top[0])
    with pytest.raises(Exception):  # a row with a target draws nothing
        e.forward_logprobs([P6[3]], [3], [0], [0.0], [0.9], [0.0], [2], targets=[P6[4]])
    ids, _, top = e.forward_logprobs([P6[3]], [3], [0], [0.0], [0.9], [0.0], [2])  # the refusal left nothing behind
    assert top[0, 0] == ids[0] == int(np.argmax(logits[0]))


def test_engine_targets_over_graph_replays(C, assets):
    """The targets ride behind the forward's graph: eager, captured and replayed forwards agree
    bitwise, and a forward without targets in between returns no target records."""
    e = C.HipEngine(assets["q40"], "q80", kv_bf16=False, max_batch=8, n_slots=1)
    args = (P6[:4], [0, 1, 2, 3], [0] * 4, [-1.0] * 4, [0.9] * 4, [0.0] * 4, [7, 7, 7, -1])
    runs = [e.forward_logprobs(*args, targets=P6[1:4] + [-1]) for _ in range(2)]
    none = e.forward_logprobs(*args)
    runs += [e.forward_logprobs(*args, targets=P6[1:4] + [-1]) for _ in range(2)]
    assert (none[2][:, 0] == -1).all() and none[2][:3, 1:8].tobytes() == runs[0][2][:3, 1:8].tobytes()
    for r in runs[1:]:
        assert r[0] == runs[0][0] and r[1].tobytes() == runs[0][1].tobytes() and r[2].tobytes() == runs[0][2].tobytes()
    logits = e.forward(P6[:4], [0, 1, 2, 3], [0] * 4)
    for i in range(3):
        check_row(logits[i], P6[i + 1], 7, runs[0][1][i], runs[0][2][i])
    assert (runs[0][2][3] == -1).all()


# ---------------------------------------------------------------------------- tensor parallelism

def _engine_tp_targets(rank, world, port, model, tokens, req, targets, q):
    try:
        C, comm, dist = _setup(rank, world, port, 1 << 16)
        eng = C.HipEngine(model, "q80", kv_bf16=False, rank=rank, world=world, comm=comm, sync_type="f32",
                          max_batch=8, n_slots=1)
        n = len(tokens)
        got = [eng.forward_logprobs(tokens, list(range(n)), [0] * n, [-1.0] * n, [0.9] * n, [0.0] * n, req,
                                    targets=targets if rank == 0 else None) for _ in range(3)]
        lg = eng.forward(tokens, list(range(n)), [0] * n)
        if comm.timed_out():
            raise AssertionError("a flag wait timed out")
        dist.barrier()
        q.put((rank, (got, lg if rank == 0 else None)))
    except Exception as e:
        q.put((rank, repr(e)))


def test_xgmi_engine_tp_targets_on_root(tmp_path):
    """TP = 2 on one GPU: rank 0 scores the given tokens on the logits gathered to it (its own
    forward's logits are the reference), over eager and replayed forwards; rank 1 computes no records."""
    from distributed_llama_multiusers_amd.models.synthetic import make_test_assets
    from distributed_llama_multiusers_amd.utils.mfile import FloatType
    m, _, _ = make_test_assets(str(tmp_path), "tiny", FloatType.Q40, seq_len=128, seed=9, dim=512, n_heads=8,
                               n_kv_heads=4, hidden_dim=1024, vocab_size=1024)
    tokens, req, targets = [5, 99, 300, 7], [20, 3, 0, -1], [99, 300, 1023, -1]
    res = _run(_engine_tp_targets, 2, m, tokens, req, targets)
    assert all(isinstance(v, tuple) for v in res.values()), res
    got, lg = res[0]
    for ids, vals, top in got:
        assert ids == [-1] * 4 and vals.tobytes() == got[0][1].tobytes() and top.tobytes() == got[0][2].tobytes()
    _, vals, top = got[0]
    for b in range(3):
        check_row(lg[b], targets[b], req[b], vals[b], top[b])
    assert (top[3] == -1).all()
    assert all((t == -1).all() for _, _, t in res[1][0])


# ---------------------------------------------------------------------------- dllama-api

@pytest.fixture(scope="module")
def gpu_api(tmp_path_factory):
    from distributed_llama_multiusers_amd.models.synthetic import make_test_assets
    from distributed_llama_multiusers_amd.utils.mfile import FloatType
    d = str(tmp_path_factory.mktemp("completions_api"))
    m, t, _ = make_test_assets(d, "tiny", FloatType.Q40, seq_len=256, seed=5, dim=512, n_heads=8, n_kv_heads=4,
                               hidden_dim=1024)
    proc, url = _start_api(m, t, ["--gpu-index", "0", "--batch-invariant", "1", "--max-seq-len", "256"])
    yield url
    proc.kill()
    proc.wait()


def test_gpu_api_teacher_forcing_exact(gpu_api):
    teacher_forcing(gpu_api)


def test_gpu_api_scoring_concurrent_equal_solo(gpu_api):
    concurrent_equal_solo(gpu_api, prompt_ids(gpu_api))
