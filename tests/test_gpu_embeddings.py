"""Embeddings on the HIP engine: the launchPool kernels (`ops.pool`) against the float64 reference
and their bitwise independence of how a request's rows are split over launches and of what shares
them, `HipEngine.forward_embed` against the CPU backend (eager, captured and replayed), the EMBED
forward's kernel classes, simulated tensor parallelism and `dllama-api --batch-invariant 1`.
Reference and bound: see test_embeddings.py."""
import concurrent.futures

import numpy as np
import pytest

from test_embeddings import TEXTS, _chat, _embed_raw, _vectors, bound, embed, reference, rows, spec
from test_gpu_engine import _rel
from test_prefix_cache import _start_api

pytestmark = pytest.mark.gpu

EPS = 1e-5
COUNTS = [1, 2, 33, 70]


@pytest.fixture(scope="module")
def ops():
    import distributed_llama_multiusers_amd.ops as o
    return o


def launch(x, slots, take, first, last, count, mode, add=None):
    return {"x": x, "add": add, "slots": slots, "take": take, "first": first, "last": last, "count": count, "mode": mode}


def request_rows(x, slot, mode, lo=0, hi=None, add=None):
    """Rows [lo, hi) of a request of len(x) rows as one launch."""
    n = len(x)
    hi = n if hi is None else hi
    k = hi - lo
    return launch(x[lo:hi], [slot] * k, [1] * k, [lo + i == 0 for i in range(k)], [lo + i == n - 1 for i in range(k)],
                  [n] * k, [mode] * k, None if add is None else add[lo:hi])


# ---------------------------------------------------------------------------- ops.pool

@pytest.mark.parametrize("with_add", [False, True])
@pytest.mark.parametrize("mode", ["mean", "last"])
@pytest.mark.parametrize("dim", [64, 4096, 8192])
def test_pool_matches_reference(ops, dim, mode, with_add):
    """Slots of 1, 2, 33 and 70 rows in one launch, three of them between rows that take no part:
    those rows' inputs are NaN, the outputs and accumulators of the slots nobody finalises hold a
    sentinel, and both are intact afterwards."""
    xs, adds = {}, {}
    for s, n in enumerate(COUNTS):
        xs[s], w = rows(n, dim, 7 * dim + n)
        adds[s] = rows(n, dim, 11 * dim + n)[0] if with_add else None
    _, w = rows(1, dim, dim)
    # layout: slot 3's rows, a bystander, slot 0, bystander, slot 1, bystander, slot 2's rows, bystander
    order = [3, None, 0, None, 1, None, 2, None]
    X, A, slots, take, first, last, count = [], [], [], [], [], [], []
    for s in order:
        n = 1 if s is None else COUNTS[s]
        X.append(np.full((1, dim), np.nan, np.float32) if s is None else xs[s])
        A.append(np.full((1, dim), np.nan, np.float32) if s is None or not with_add else adds[s])
        slots += [5 if s is None else s] * n
        take += [0 if s is None else 1] * n
        first += [False] * n if s is None else [i == 0 for i in range(n)]
        last += [False] * n if s is None else [i == n - 1 for i in range(n)]
        count += [n] * n
    X = np.concatenate(X)
    n_slots = 6
    sentinel = np.full((n_slots, dim), 12345.0, np.float32)
    out, acc = ops.pool([launch(X, slots, take, first, last, count, [mode] * len(slots),
                                np.concatenate(A) if with_add else None)], w, EPS, n_slots, sentinel, sentinel)
    assert (out[4:] == 12345.0).all() and (acc[4:] == 12345.0).all()  # slots 4 and 5: nobody's
    for s, n in enumerate(COUNTS):
        x = xs[s] + adds[s] if with_add else xs[s]
        ref = reference(x, w, EPS, mode)
        err = float(np.abs(out[s].astype(np.float64) - ref).max())
        print(f"dim {dim} N {n} {mode} add {with_add}: max error {err:.3e}, bound {bound(n, dim):.3e}")
        assert np.isfinite(out[s]).all()
        assert err <= bound(n, dim)


def test_pool_zero_rows_and_no_taker(ops):
    dim = 64
    w = np.ones(dim, np.float32)
    out, _ = ops.pool([request_rows(np.zeros((3, dim), np.float32), 0, "mean")], w, EPS, 1)
    assert np.isfinite(out).all() and (out == 0).all()
    # a launch in which no row takes part is never enqueued: nothing changes
    nan = np.full((2, dim), np.nan, np.float32)
    fill = np.full((1, dim), 7.0, np.float32)
    out, acc = ops.pool([launch(nan, [0, 0], [0, 0], [0, 0], [0, 0], [0, 0], ["mean"] * 2)], w, EPS, 1, fill, fill)
    assert (out == 7.0).all() and (acc == 7.0).all()


@pytest.mark.parametrize("mode", ["mean", "last"])
@pytest.mark.parametrize("dim", [64, 4096, 8192])
def test_pool_bitwise_split_and_company(ops, dim, mode):
    x, w = rows(70, dim, 3 * dim)
    y, _ = rows(70, dim, 5 * dim)
    whole, _ = ops.pool([request_rows(x, 0, mode, add=y)], w, EPS, 1)
    again, _ = ops.pool([request_rows(x, 0, mode, add=y)], w, EPS, 1)
    assert np.array_equal(whole, again)
    split, _ = ops.pool([request_rows(x, 0, mode, 0, 69, y), request_rows(x, 0, mode, 69, 70, y)], w, EPS, 1)
    assert np.array_equal(split, whole)
    single, _ = ops.pool([request_rows(x, 0, mode, i, i + 1, y) for i in range(70)], w, EPS, 1)
    assert np.array_equal(single, whole)
    # the same slot among 64 rows of other slots: 32 rows before it, 32 behind, four requests of 16
    ox, _ = rows(64, dim, 9 * dim)
    oy, _ = rows(64, dim, 13 * dim)
    parts = [request_rows(ox[16 * k:16 * k + 16], 1 + k, "mean", add=oy[16 * k:16 * k + 16]) for k in range(4)]
    mine = request_rows(x, 0, mode, add=y)
    seq = parts[:2] + [mine] + parts[2:]
    merged = {k: (np.concatenate([p[k] for p in seq]) if k in ("x", "add") else sum((list(p[k]) for p in seq), []))
              for k in mine}
    among, _ = ops.pool([merged], w, EPS, 5)
    assert np.array_equal(among[0], whole[0])
    for k in range(4):
        alone, _ = ops.pool([parts[k]], w, EPS, 5)
        assert np.array_equal(among[1 + k], alone[1 + k])


def test_pool_plan_refuses_inconsistent_rows(ops):
    x, w = rows(2, 64, 1)
    with pytest.raises(Exception, match="pooling"):  # a row behind its slot's last row
        ops.pool([launch(x, [0, 0], [1, 1], [1, 0], [1, 0], [1, 1], ["mean"] * 2)], w, EPS, 1)


# ---------------------------------------------------------------------------- HipEngine.forward_embed

PROMPT = [int(t) for t in np.random.default_rng(33).integers(0, 500, 70)]


@pytest.mark.parametrize("graphs", [False, True])
@pytest.mark.parametrize("kind,kv_bf16", [("q40", True), ("q40", False), ("f32", False), ("f32", True)])
def test_engine_forward_embed_matches_cpu(C, assets, kind, kv_bf16, graphs):
    """70 tokens in chunks of 32 (32 + 32 + 6), GPU against the CPU backend's vector, within the
    bounds tests/test_gpu_engine.py sets for GPU-vs-CPU logits of the same model on the path the rows
    take: test_engine_matches_cpu's for single rows (3e-2 Q40, 2e-2 f32 weights with a bf16 cache,
    1e-4 f32 throughout), and for the chunks, which run the MFMA GEMMs on f16 activations, the same
    except 1e-2 for f32 weights with an f32 cache (test_engine_batched_prefill_f32's bound against
    the CPU; measured here: 2.1e-4). With graphs the same prompt is embedded three times: the second
    use of a shape captures its EMBED graph, the third replays it, and all three give the same bytes."""
    buf = "q80" if kind == "q40" else "f32"
    row_tol = 3e-2 if kind == "q40" else (2e-2 if kv_bf16 else 1e-4)
    tol = max(row_tol, 1e-2) if kind == "f32" else row_tol
    cpu = C.cpu_backend(assets[kind], buf, 4, 128, 64, 1)
    gpu = C.HipEngine(assets[kind], buf, kv_bf16=kv_bf16, max_batch=32, use_graphs=graphs)
    for mode in ("mean", "last"):
        ref = embed(cpu, PROMPT, 32, mode=mode)
        got = embed(gpu, PROMPT, 32, mode=mode)
        print(f"{kind} kv_bf16 {kv_bf16} {mode}: rel {_rel(got, ref):.3e}, bound {tol}")
        assert _rel(got, ref) < tol
        assert abs(float(np.linalg.norm(got.astype(np.float64))) - 1) < 1e-5
        for _ in range(2):
            assert np.array_equal(embed(gpu, PROMPT, 32, mode=mode), got)
    # single rows (the GEMV path, the fused attention block): the same request, one row per forward
    one = embed(gpu, PROMPT[:9], 1)
    rel = _rel(one, embed(cpu, PROMPT[:9], 1))
    print(f"{kind} kv_bf16 {kv_bf16} single rows: rel {rel:.3e}, bound {row_tol}")
    assert rel < row_tol


def test_engine_embed_bitwise_next_to_chat_rows(C, assets):
    """batch_invariant: the vector is bitwise the same alone and next to drawn rows of other slots."""
    gpu = C.HipEngine(assets["q40"], "q80", kv_bf16=False, max_batch=64, n_slots=3, batch_invariant=True)
    n = 40
    alone = embed(gpu, PROMPT[:n], n, slot=0)
    gpu.forward(PROMPT[40:50], list(range(10)), [1] * 10)
    gpu.forward(PROMPT[50:56], list(range(6)), [2] * 6)
    want = gpu.forward_sample([17, 23], [10, 6], [1, 2], [0.0, 0.0], [0.9, 0.9], [0.1, 0.2])
    toks = [17] + PROMPT[:n] + [23]
    pos = [10] + list(range(n)) + [6]
    slots = [1] + [0] * n + [2]
    pooling = [None] + [spec(i, n) for i in range(n)] + [None]
    temps = [0.0] + [-1.0] * n + [0.0]
    ids, done, vecs = gpu.forward_embed(toks, pos, slots, pooling, temps, [0.9] * (n + 2), [0.1] * (n + 2))
    assert [ids[0], ids[-1]] == want and ids[1:-1] == [-1] * n and done == [0]
    assert np.array_equal(vecs[0], alone)


def test_embed_forward_runs_no_logits_kernels(C, assets):
    gpu = C.HipEngine(assets["q40"], "q80", kv_bf16=False, max_batch=32, n_slots=2, use_graphs=False)
    n = 8
    toks, pos = PROMPT[:n], list(range(n))
    pooling = [spec(i, n) for i in range(n)]
    table = gpu.profile_forward(toks, pos, [0] * n, [-1.0] * n, pooling)
    assert "pool" in table and not {"gemv_logits", "argmax", "sample"} & set(table), table
    mixed = gpu.profile_forward(toks + [5], pos + [0], [0] * n + [1], [-1.0] * n + [0.7], pooling + [None])
    assert {"pool", "gemv_logits", "sample"} <= set(mixed), mixed
    plain = gpu.profile_forward(toks, pos, [0] * n, [0.7] * n, None)
    assert "pool" not in plain and "gemv_logits" in plain, plain


# ---------------------------------------------------------------------------- tensor parallelism

@pytest.fixture(scope="module")
def kv4_gpu(tmp_path_factory):
    from distributed_llama_multiusers_amd.models.synthetic import make_test_assets
    from distributed_llama_multiusers_amd.utils.mfile import FloatType
    d = str(tmp_path_factory.mktemp("kv4e"))
    m, t, _ = make_test_assets(d, "tiny", FloatType.Q40, seq_len=128, seed=9, dim=512, n_heads=8, n_kv_heads=4,
                               hidden_dim=1024, vocab_size=1024)
    return m


@pytest.mark.parametrize("tokens,chunk", [([5], 1), ([5, 99, 300, 7, 1000, 2], 1), ([5, 99, 300, 7, 1000, 2, 41, 8], 8)],
                         ids=["one-token", "single-rows", "chunk-of-8"])
def test_simulated_tp2_embedding_matches_single(C, kv4_gpu, tokens, chunk):
    """World 2 on one GPU (host-staged collectives): the root's vector against the TP1 vector within
    the bound of test_simulated_tensor_parallel_matches_single. Single rows take the non-prenorm
    schedule in an all-embedding forward."""
    single = C.HipEngine(kv4_gpu, "q80", kv_bf16=False, max_batch=8)
    ref = embed(single, tokens, chunk)
    got = C.simulate_tp_embed(kv4_gpu, "q80", 2, tokens, chunk)
    print(f"TP2 {len(tokens)} tokens chunk {chunk}: rel {_rel(got, ref):.3e}")
    assert got.shape == ref.shape and _rel(got, ref) < 3e-2
    assert abs(float(np.linalg.norm(got.astype(np.float64))) - 1) < 1e-5


# ---------------------------------------------------------------------------- dllama-api

@pytest.fixture(scope="module")
def gpu_api(tmp_path_factory):
    from distributed_llama_multiusers_amd.models.synthetic import make_test_assets
    from distributed_llama_multiusers_amd.utils.mfile import FloatType
    d = str(tmp_path_factory.mktemp("embeddings_api"))
    m, t, _ = make_test_assets(d, "tiny", FloatType.Q40, seq_len=256, seed=5, dim=512, n_heads=8, n_kv_heads=4,
                               hidden_dim=1024)
    proc, url = _start_api(m, t, ["--gpu-index", "0", "--batch-invariant", "1", "--max-seq-len", "256"])
    yield url
    proc.kill()
    proc.wait()


def test_api_gpu_embeddings_together_equal_alone(gpu_api):
    """--batch-invariant 1: six inputs sent together equal the same six sent alone, bitwise, and a
    concurrent greedy chat request returns its solo text."""
    six = TEXTS[:6]
    alone = [_vectors(_embed_raw(gpu_api, {"input": t}))[0] for t in six]
    solo = _chat(gpu_api, "tell me about the quick brown fox")
    with concurrent.futures.ThreadPoolExecutor(2) as ex:
        chat = ex.submit(_chat, gpu_api, "tell me about the quick brown fox")
        together = ex.submit(_embed_raw, gpu_api, {"input": six})
        assert chat.result() == solo
        got = _vectors(together.result())
    for a, b in zip(got, alone):
        assert abs(float(np.linalg.norm(a.astype(np.float64))) - 1) <= 1e-5
        assert np.array_equal(a, b)
