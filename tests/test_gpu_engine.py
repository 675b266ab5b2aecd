"""HIP engine (gfx950 kernels) vs the CPU reference backend / torch oracle."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import gpu_available

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def medium(tmp_path_factory):
    # wide enough to exercise the 32- and 64-lane GEMV row groups (n/32 >= 192 / 384)
    from distributed_llama_multiusers_amd.models.synthetic import make_test_assets
    from distributed_llama_multiusers_amd.utils.mfile import FloatType
    d = str(tmp_path_factory.mktemp("medium"))
    m, t, spec = make_test_assets(d, "tiny", FloatType.Q40, seq_len=512, seed=3, dim=1024, hidden_dim=12288,
                                  n_heads=8, n_kv_heads=2, n_layers=2, vocab_size=2048)
    return m


def _rel(a, b):
    return float(np.abs(a - b).max() / np.abs(b).max())


def _seq(be, tokens, slot=0):
    return np.stack([be.forward([t], [p], [slot])[0] for p, t in enumerate(tokens)])


def _assert_replays_equal(be, tokens, first):
    """The same forward again (same rows and positions: the KV rows are rewritten with the same
    values): the 2nd use of a shape is captured into a hipGraph and the 3rd replays it; both must
    equal the eager 1st run bitwise (graphs=False: three eager runs, deterministic kernels)."""
    n = len(tokens)
    for _ in range(2):
        again = be.forward(tokens, list(range(n)), [0] * n)
        assert np.array_equal(again, first)


@pytest.mark.parametrize("kind,kv_bf16", [("q40", True), ("q40", False), ("f32", False), ("f32", True)])
def test_engine_matches_cpu(C, assets, kind, kv_bf16):
    buf = "q80" if kind == "q40" else "f32"
    cpu = C.cpu_backend(assets[kind], buf, 4)
    gpu = C.HipEngine(assets[kind], buf, kv_bf16=kv_bf16, max_batch=8)
    tokens = [3, 17, 101, 7, 250, 9, 44, 300, 5, 6]
    ref = _seq(cpu, tokens)
    got = _seq(gpu, tokens)
    tol = 3e-2 if kind == "q40" else (2e-2 if kv_bf16 else 1e-4)
    assert _rel(got, ref) < tol
    # every row's argmax agrees unless the CPU's own logits are a near-tie between the two picks
    for r in range(len(tokens)):
        a, b = int(got[r].argmax()), int(ref[r].argmax())
        if a != b:
            assert ref[r][b] - ref[r][a] <= tol * float(np.abs(ref[r]).max()), (r, a, b)


def _first_divergence(got, ref):
    for i, (a, b) in enumerate(zip(got, ref)):
        if a != b:
            return i
    return None


@pytest.mark.parametrize("kind", ["f32", "q40"])
def test_greedy_64_tokens_equal_cpu(C, assets, kind):
    """Free-running greedy decode, f32 KV: the GPU (prompt forwards, then the captured
    forward->argmax chain) emits exactly the CPU reference's 64 tokens. A divergence is accepted
    only where the CPU's own logits are a near-tie between the two candidates (f32 weights: 1e-4 of
    the logit range; Q40 weights x Q80 activations, where a 1-ulp input difference can move a Q80
    rounding: 3e-2), and for f32 weights not before token 48."""
    buf = "q80" if kind == "q40" else "f32"
    cpu = C.cpu_backend(assets[kind], buf, 4)
    gpu = C.HipEngine(assets[kind], buf, kv_bf16=False, max_batch=8)
    prompt, steps = [3, 17, 101, 7], 64
    for p, t in enumerate(prompt):
        lg = cpu.forward([t], [p], [0])[0]
    ref, ref_lg = [], []
    tok = int(lg.argmax())
    for s in range(steps):
        ref.append(tok)
        ref_lg.append(lg)
        lg = cpu.forward([tok], [len(prompt) + s], [0])[0]
        tok = int(lg.argmax())
    for p, t in enumerate(prompt):
        glg = gpu.forward([t], [p], [0])[0]
    g0 = int(glg.argmax())
    _, rest = gpu.decode_greedy(steps - 1, [g0], [len(prompt)], [0])
    got = [g0] + list(rest)
    i = _first_divergence(got, ref)
    if i is None:
        return
    scale = float(np.abs(ref_lg[i]).max())
    margin = float(ref_lg[i][ref[i]] - ref_lg[i][got[i]])
    assert margin <= (1e-4 if kind == "f32" else 3e-2) * scale, (i, margin, scale, got, ref)
    if kind == "f32":
        assert i >= 48, (i, got, ref)


def test_engine_medium_matches_cpu(C, medium):
    cpu = C.cpu_backend(medium, "q80", 8)
    gpu = C.HipEngine(medium, "q80", kv_bf16=False, max_batch=8)
    tokens = [1, 2, 3, 500, 1000, 2000, 7]
    assert _rel(_seq(gpu, tokens), _seq(cpu, tokens)) < 3e-2


@pytest.mark.parametrize("graphs,n", [(True, 7), (False, 7), (True, 8), (False, 13)])
def test_engine_batched_prefill_gemv_chunks(C, assets, graphs, n, monkeypatch):
    """GEMV batch path (chunks of 4 / 2 / 1 rows of the same int8 ring kernel: 7 = 4+2+1, 8 = 4+4,
    13 = 4+4+4+1) == n sequential decodes."""
    monkeypatch.setenv("DL_GEMM_MIN", "1000")
    a = C.HipEngine(assets["q40"], "q80", kv_bf16=False, max_batch=16, use_graphs=graphs)
    b = C.HipEngine(assets["q40"], "q80", kv_bf16=False, max_batch=16, use_graphs=graphs)
    tokens = [9, 8, 7, 6, 5, 4, 3, 11, 12, 13, 14, 15, 16][:n]
    seq = _seq(a, tokens)
    bat = b.forward(tokens, list(range(n)), [0] * n)
    assert _rel(bat, seq) < 1e-4
    _assert_replays_equal(b, tokens, bat)


@pytest.mark.parametrize("graphs", [True, False])
@pytest.mark.parametrize("n", [2, 7, 16, 23, 40, 64, 72, 100, 128])
def test_engine_batched_prefill_mfma(C, assets, graphs, n, monkeypatch):
    """MFMA GEMM batch path (f16 dequantized Q40 x f16 activations, split-K, fused epilogues) vs
    sequential int8 GEMV decodes and vs the CPU reference backend. Up to 64 rows run the narrow
    64-row tiles; 72, 100 and 128 rows the wide 128 x 128 tiles (split-K on the thin matrices)."""
    monkeypatch.setenv("DL_GEMM_MIN", "2")
    rng = np.random.default_rng(n)
    tokens = [int(t) for t in rng.integers(0, 512, n)]
    a = C.HipEngine(assets["q40"], "q80", kv_bf16=False, max_batch=256, use_graphs=graphs)
    b = C.HipEngine(assets["q40"], "q80", kv_bf16=False, max_batch=256, use_graphs=graphs)
    seq = _seq(a, tokens)
    bat = b.forward(tokens, list(range(n)), [0] * n)
    assert _rel(bat, seq) < 2e-2
    assert (bat.argmax(-1) == seq.argmax(-1)).mean() >= 0.85
    _assert_replays_equal(b, tokens, bat)
    cpu = C.cpu_backend(assets["q40"], "q80", 2, max_batch=256)
    ref = cpu.forward(tokens, list(range(n)), [0] * n)
    assert _rel(bat, ref) < 3e-2


@pytest.mark.parametrize("n", [100, 256])
def test_engine_wide_gemm_matches_narrow(C, medium, n, monkeypatch):
    """The wide 128 x 128 GEMM (one launch over all token tiles) and the narrow 64-row kernel
    (DL_GEMM_WIDE=0: 128-token launches) give the same forward within f32 reassociation, with the
    bf16 cache's MFMA prefill attention in between."""
    rng = np.random.default_rng(7 + n)
    toks = [int(t) for t in rng.integers(0, 2048, n)]
    monkeypatch.setenv("DL_GEMM_MIN", "2")
    wide = C.HipEngine(medium, "q80", kv_bf16=True, max_batch=256)
    got = wide.forward(toks, list(range(n)), [0] * n)
    monkeypatch.setenv("DL_GEMM_WIDE", "0")
    env = dict(os.environ, PYTHONPATH=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    out = subprocess.run([sys.executable, "-c", _NARROW_CHILD, medium, json.dumps(toks)], env=env,
                         capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-2000:]
    ref = np.array(json.loads(out.stdout.strip().splitlines()[-1]), dtype=np.float32)
    assert _rel(got, ref) < 2e-3
    assert (got.argmax(-1) == ref.argmax(-1)).mean() >= 0.95


# the knob is read once per process: the narrow reference runs in a child
_NARROW_CHILD = """
import json, sys
import distributed_llama_multiusers_amd as dl
C = dl.native()
toks = json.loads(sys.argv[2])
n = len(toks)
e = C.HipEngine(sys.argv[1], "q80", kv_bf16=True, max_batch=256)
print(json.dumps(e.forward(toks, list(range(n)), [0] * n).tolist()))
"""


@pytest.mark.parametrize("n", [7, 40, 72])
def test_engine_batched_prefill_f32(C, assets, n, monkeypatch):
    """F32-weight models on the batched path (K5: gemmF32Kernel + fused epilogues) vs sequential
    f32 GEMV decodes and the CPU reference (the batched path's only rounding: f16 activations)."""
    rng = np.random.default_rng(100 + n)
    tokens = [int(t) for t in rng.integers(0, 512, n)]
    a = C.HipEngine(assets["f32"], "f32", kv_bf16=False, max_batch=128)
    b = C.HipEngine(assets["f32"], "f32", kv_bf16=False, max_batch=128)
    seq = _seq(a, tokens)
    bat = b.forward(tokens, list(range(n)), [0] * n)
    assert _rel(bat, seq) < 1e-2
    assert (bat.argmax(-1) == seq.argmax(-1)).mean() >= 0.9
    cpu = C.cpu_backend(assets["f32"], "f32", 2, max_batch=128)
    assert _rel(bat, cpu.forward(tokens, list(range(n)), [0] * n)) < 1e-2


@pytest.mark.parametrize("gemm_min,tol", [("1000", 1e-4), ("2", 2e-2)])
def test_engine_slots_independent(C, assets, monkeypatch, gemm_min, tol):
    """Two sequences in different KV slots in one batch == each alone (GEMV batch path exactly,
    MFMA batch path within f16 dequant tolerance)."""
    monkeypatch.setenv("DL_GEMM_MIN", gemm_min)
    g = C.HipEngine(assets["q40"], "q80", kv_bf16=False, max_batch=4, n_slots=3)
    x, y = [11, 12, 13, 14], [200, 201, 202, 203]
    for p in range(4):
        both = g.forward([x[p], y[p]], [p, p], [2, 0])
    r1 = C.HipEngine(assets["q40"], "q80", kv_bf16=False)
    r2 = C.HipEngine(assets["q40"], "q80", kv_bf16=False)
    assert _rel(both[0], _seq(r1, x)[-1]) < tol
    assert _rel(both[1], _seq(r2, y)[-1]) < tol


def test_decode_greedy_chain_matches_stepwise(C, assets):
    g1 = C.HipEngine(assets["q40"], "q80", kv_bf16=True)
    g2 = C.HipEngine(assets["q40"], "q80", kv_bf16=True)
    ms, chain = g1.decode_greedy(20, [42], [0], [0])
    tok, step = 42, []
    for p in range(20):
        tok = g2.forward_argmax([tok], [p], [0])[0]
        step.append(tok)
    assert chain == step
    assert ms > 0


def test_argmax_matches_logits(C, assets):
    g = C.HipEngine(assets["q40"], "q80")
    lg = g.forward([1, 2, 3], [0, 1, 2], [0, 0, 0])
    g2 = C.HipEngine(assets["q40"], "q80")
    ids = g2.forward_argmax([1, 2, 3], [0, 1, 2], [0, 0, 0])
    assert list(lg.argmax(-1)) == ids


def test_long_context_split_attention(C, tmp_path):
    """Positions beyond one 256-key chunk exercise the split-K attention + combine path."""
    from distributed_llama_multiusers_amd.models.synthetic import make_test_assets
    from distributed_llama_multiusers_amd.utils.mfile import FloatType
    m, t, spec = make_test_assets(str(tmp_path), "tiny", FloatType.Q40, seq_len=1100, seed=5, n_layers=1)
    cpu = C.cpu_backend(m, "q80", 8)
    gpu = C.HipEngine(m, "q80", kv_bf16=False, max_batch=32)
    rng = np.random.default_rng(0)
    toks = rng.integers(0, spec.vocab_size, 1040).tolist()
    # prefill in chunks of 32 rows, then compare the last rows
    for s in range(0, 1024, 32):
        c = cpu.forward(toks[s:s + 32], list(range(s, s + 32)), [0] * 32)
        g = gpu.forward(toks[s:s + 32], list(range(s, s + 32)), [0] * 32)
    assert _rel(g, c) < 3e-2
    c = cpu.forward([toks[1024]], [1024], [0])
    g = gpu.forward([toks[1024]], [1024], [0])
    assert _rel(g, c) < 3e-2


def test_synthetic_8b_shape_smoke(C):
    """Random-init Llama-3.1-8B shapes on device; a few greedy steps must run and be finite."""
    h = dict(dim=4096, hidden_dim=14336, n_layers=2, n_heads=32, n_kv_heads=8, vocab_size=128256, seq_len=256,
             rope_theta=500000, weight_type=2)
    g = C.HipEngine("", "q80", synthetic=h, max_seq_len=256)
    lg = g.forward([1], [0], [0])
    assert np.isfinite(lg).all() and lg.std() > 0
    ms, toks = g.decode_greedy(8, [1], [1], [0])
    assert len(toks) == 8 and all(0 <= t < 128256 for t in toks)


@pytest.fixture(scope="module")
def kv4_gpu(tmp_path_factory):
    from distributed_llama_multiusers_amd.models.synthetic import make_test_assets
    from distributed_llama_multiusers_amd.utils.mfile import FloatType
    d = str(tmp_path_factory.mktemp("kv4g"))
    # head size 64, 4 kv heads, hidden shard 1024/4 = 256: exercises Q80 and f32 h hand-offs
    m, t, _ = make_test_assets(d, "tiny", FloatType.Q40, seq_len=128, seed=9, dim=512, n_heads=8, n_kv_heads=4,
                               hidden_dim=1024, vocab_size=1024)
    return m


@pytest.mark.parametrize("world", [2, 4])
def test_simulated_tensor_parallel_matches_single(C, kv4_gpu, world):
    """N ranks (threads) on one GPU with host-staged collectives: same logits as TP=1."""
    tokens = [5, 99, 300, 7, 1000, 2]
    single = C.HipEngine(kv4_gpu, "q80", kv_bf16=False)
    ref = np.stack([single.forward([t], [p], [0])[0] for p, t in enumerate(tokens)])
    got = C.simulate_tp(kv4_gpu, "q80", world, tokens)
    assert _rel(got, ref) < 3e-2
    assert (got.argmax(-1) == ref.argmax(-1)).all()


@pytest.fixture(scope="module")
def kv8_gpu(tmp_path_factory):
    from distributed_llama_multiusers_amd.models.synthetic import make_test_assets
    from distributed_llama_multiusers_amd.utils.mfile import FloatType
    d = str(tmp_path_factory.mktemp("kv8g"))
    # 32 query heads of 64 over 8 KV heads (kvMul 4): TP8 leaves one KV head and 4 query heads per rank
    m, t, _ = make_test_assets(d, "tiny", FloatType.Q40, seq_len=128, seed=9, dim=2048, n_heads=32, n_kv_heads=8,
                               hidden_dim=2048, vocab_size=1024)
    return m


def test_simulated_tp8_matches_single(C, kv8_gpu, monkeypatch):
    """TP8 (one KV head per rank, q0 = 256, kv0 = 64) simulated on one GPU: same logits as TP1, and
    every rank's single decode rows run the fused attention block (forced: with one KV group per
    rank the engine's default is the three launches)."""
    tokens = [5, 99, 300, 7, 1000, 2]
    single = C.HipEngine(kv8_gpu, "q80", kv_bf16=False)
    ref = np.stack([single.forward([t], [p], [0])[0] for p, t in enumerate(tokens)])
    monkeypatch.setenv("DL_ATTN_BLOCK", "1")
    got, blocks = C.simulate_tp(kv8_gpu, "q80", 8, tokens, attn_block_flags=True)
    assert _rel(got, ref) < 3e-2
    assert (got.argmax(-1) == ref.argmax(-1)).all()
    assert all(blocks), blocks


def test_simulated_tp8_70b_attention_shapes(C, tmp_path, monkeypatch):
    """Llama-3.3-70B attention shapes at TP8 (dim 8192, 64 query / 8 KV heads of 128: per rank
    q0 = 1024, kv0 = 128, kvMul 8), one layer with a narrow FFN: simulated TP8 vs TP1 logits, the
    fused attention block (forced) on every rank."""
    from distributed_llama_multiusers_amd.models.synthetic import make_test_assets
    from distributed_llama_multiusers_amd.utils.mfile import FloatType
    m, _, _ = make_test_assets(str(tmp_path), "tiny", FloatType.Q40, seq_len=64, seed=21, dim=8192, n_heads=64,
                               n_kv_heads=8, hidden_dim=2048, n_layers=1, vocab_size=1024)
    tokens = [5, 99, 300, 7]
    single = C.HipEngine(m, "q80", kv_bf16=False)
    ref = np.stack([single.forward([t], [p], [0])[0] for p, t in enumerate(tokens)])
    del single
    monkeypatch.setenv("DL_ATTN_BLOCK", "1")
    got, blocks = C.simulate_tp(m, "q80", 8, tokens, attn_block_flags=True)
    assert _rel(got, ref) < 3e-2
    assert all(blocks), blocks


@pytest.mark.gpu
def test_kv_cache_larger_than_hbm_is_refused(C):
    """64 slots x 131072 positions of bf16 KV for the 8B is ~1.1 TB: refused before allocating,
    with the numbers and what to lower, instead of an out-of-memory fault mid-load."""
    h = dict(dim=4096, hidden_dim=14336, n_layers=32, n_heads=32, n_kv_heads=8, vocab_size=128256,
             seq_len=131072, rope_theta=500000, weight_type=2)
    with pytest.raises(RuntimeError, match="does not fit on GPU.*--kv-pages"):
        C.HipEngine("", "q80", synthetic=h, max_seq_len=131072, n_slots=64, max_batch=1)
    # the same 64 slots of 128K context each over a shared pool of 131072 positions (paged KV)
    g = C.HipEngine("", "q80", synthetic=h, max_seq_len=131072, n_slots=64, max_batch=1, kv_pages=512,
                    kv_page_size=256)
    assert g.kv_pages_free == 512
    g.forward([1], [0], [63])
    assert g.kv_pages_free == 511


@pytest.mark.parametrize("n", [8, 32, 64, 200])
def test_engine_prefill_mfma_attention(C, medium, n, monkeypatch):
    """Batched forward with a bf16 cache (MFMA prefill attention over the chunk's rows, one slot) ==
    sequential decodes (per-row attention), and a second chunk on top of the first (keys of the
    earlier chunk + causal keys of its own). 200 rows: the wide GEMM over two token tiles in one
    launch with the fused residual + norm hand-off across them."""
    monkeypatch.setenv("DL_GEMM_MIN", "2")
    rng = np.random.default_rng(n)
    toks = [int(t) for t in rng.integers(0, 2048, 2 * n)]
    a = C.HipEngine(medium, "q80", kv_bf16=True, max_batch=256)
    b = C.HipEngine(medium, "q80", kv_bf16=True, max_batch=256)
    seq = _seq(a, toks)
    first = b.forward(toks[:n], list(range(n)), [0] * n)
    second = b.forward(toks[n:], list(range(n, 2 * n)), [0] * n)
    bat = np.concatenate([first, second])
    assert _rel(bat, seq) < 3e-2
    assert (bat.argmax(-1) == seq.argmax(-1)).mean() >= 0.85


def test_batched_path_outlier_residuals(C, tmp_path):
    """Real checkpoints carry "massive activation" channels in the residual stream (|x| of 1e3-1e4
    and more). The batched path hands x' * normW between GEMMs in f16 (EPI_RES): with outlier
    channels of 1.5e5 (x normW ~ 1.6e5 > the f16 maximum) it must stay finite and match the CPU
    reference (pre-scaled, saturating hand-off), like the per-row GEMV path."""
    import os
    from distributed_llama_multiusers_amd.models.synthetic import make_spec, random_tensors, make_tokenizer
    from distributed_llama_multiusers_amd.utils.mfile import FloatType, write_model
    spec = make_spec("tiny", FloatType.Q40, 128, dim=512, n_heads=8, n_kv_heads=4, hidden_dim=1024)
    t = random_tensors(spec, 21)
    emb = t[("embedding", -1)]
    emb[:, 7] = 1.5e5   # outlier channels on every token
    emb[:, 300] = -9e4
    m = os.path.join(str(tmp_path), "outlier.m")
    write_model(m, spec, t)
    cpu = C.cpu_backend(m, "q80", 4, max_batch=64)
    gpu = C.HipEngine(m, "q80", kv_bf16=False, max_batch=64)
    rng = np.random.default_rng(2)
    tokens = [int(x) for x in rng.integers(0, spec.vocab_size, 40)]
    ref = cpu.forward(tokens, list(range(40)), [0] * 40)
    got = gpu.forward(tokens, list(range(40)), [0] * 40)
    assert np.isfinite(got).all()
    assert _rel(got, ref) < 3e-2


@pytest.mark.parametrize("kv_bf16", [True, False])
def test_attn_block_matches_separate_kernels(C, assets, medium, monkeypatch, kv_bf16):
    """Single decode rows run the fused attention block (qkv GEMV + attention + wo GEMV as one
    launch with in-launch write-through hand-offs): same logits as the three separate launches
    (attention reduces in another order: tolerance), same greedy chain, over many forwards (the
    block's monotonic counters across layers, forwards and graph replays)."""
    for model in (assets["q40"], medium):
        monkeypatch.setenv("DL_ATTN_BLOCK", "0")
        ref = C.HipEngine(model, "q80", kv_bf16=kv_bf16, max_batch=8)
        monkeypatch.delenv("DL_ATTN_BLOCK")
        got = C.HipEngine(model, "q80", kv_bf16=kv_bf16, max_batch=8)
        assert got.attn_block and not ref.attn_block
        toks = [3, 17, 101, 7, 250, 9]
        a, b = _seq(ref, toks), _seq(got, toks)
        assert _rel(b, a) < 1e-3
        # a batched forward in between (no block; the block's epoch must not advance)
        ref.forward([5, 6, 7], [6, 7, 8], [0, 0, 0])
        got.forward([5, 6, 7], [6, 7, 8], [0, 0, 0])
        _, ca = ref.decode_greedy(24, [int(a[-1].argmax())], [9], [0])
        _, cb = got.decode_greedy(24, [int(b[-1].argmax())], [9], [0])
        assert list(ca) == list(cb)


@pytest.mark.parametrize("hq80", ["1", "0"])
@pytest.mark.parametrize("sync", ["q80", "f32"])
def test_prenorm_handoff_matches_norm_prologue(C, medium, monkeypatch, sync, hq80):
    """A TP rank's single decode rows with the pre-normalized hand-off (wo / w2 exchange tails apply
    the residual update and the next norm's weights and emit Q80 blocks + sums of squares; qkv,
    w13 and the logits GEMV only copy them and fold in 1 / rms) vs the norm prologues: the same
    shard logits up to Q80 rounding ties and the same greedy chain (rank in loopback). The f32
    exchange keeps 16-row workgroups, so the hand-off stays off there (same results both ways).
    Both w13 -> w2 hand-off types (DL_H_Q80: Q80 blocks / f32 rows that w2 quantizes): the default
    depends on the shard shape, so the pre-normalized rows run under either."""
    monkeypatch.setenv("DL_H_Q80", hq80)
    out = {}
    for on in ("1", "0"):
        monkeypatch.setenv("DL_PRENORM", on)
        e = C.HipEngine(medium, "q80", max_batch=8, rank=0, world=2, comm=C.ComputeOnlyComm(0, 2, 0),
                        sync_type=sync, kv_bf16=False)
        assert bool(e.prenorm) == (on == "1" and sync == "q80")
        v0 = e.header["vocab_size"] // 2
        toks = [3, 17, 101, 7, 250, 9]
        lg = np.stack([e.forward([t], [p], [0])[0][:v0] for p, t in enumerate(toks)])
        _, ch = e.decode_greedy(12, [int(lg[-1].argmax())], [len(toks)], [0])
        ids = [e.forward_argmax([t], [p], [0])[0] for p, t in enumerate(toks)]  # the EPI_ARGMAX consumer
        out[on] = (lg, list(ch), ids)
        del e
    assert np.isfinite(out["1"][0]).all()
    assert _rel(out["1"][0], out["0"][0]) < 2e-3
    assert sum(a == b for a, b in zip(out["1"][1], out["0"][1])) >= 10, (out["1"][1], out["0"][1])
    assert out["1"][2] == [int(i) for i in out["1"][0].argmax(-1)]


def test_engine_8b_shape_matches_cpu(C, tmp_path):
    """Llama-3.1-8B layer shapes (2 layers, 2048-token vocabulary, kvMul 4, head size 128): the
    fused attention block's decode logits against the CPU reference backend, token by token."""
    from distributed_llama_multiusers_amd.models.synthetic import make_test_assets
    from distributed_llama_multiusers_amd.utils.mfile import FloatType
    m, _, _ = make_test_assets(str(tmp_path), "tiny", FloatType.Q40, seq_len=128, seed=5, dim=4096,
                               hidden_dim=14336, n_heads=32, n_kv_heads=8, n_layers=2, vocab_size=2048)
    gpu = C.HipEngine(m, "q80", kv_bf16=False, max_batch=32)
    assert gpu.attn_block
    cpu = C.cpu_backend(m, "q80", 8, max_batch=32)
    toks = [1, 2, 3, 500, 1000, 7]
    assert _rel(_seq(gpu, toks), _seq(cpu, toks)) < 3e-2
    # batched rows on the MFMA GEMMs: 16-lane tilings (qkv, w13, logits) run the 16-block-chunk
    # kernel, wo / w2 the 8-block one; 8 and 24 rows (16- and 32-token tiles, split-K)
    rng = np.random.default_rng(3)
    for n in (8, 24):
        t = [int(x) for x in rng.integers(0, 2048, n)]
        got = gpu.forward(t, list(range(n)), [0] * n)
        ref = cpu.forward(t, list(range(n)), [0] * n)
        assert _rel(got, ref) < 3e-2, n


@pytest.mark.parametrize("shape", ["70b", "405b"])
def test_engine_big_model_shapes_match_cpu(C, tmp_path, shape):
    """BASELINE configs #4 / #5 layer shapes, one layer, 1024-token vocabulary, decode rows against
    the CPU reference backend: Llama-3.3-70B (dim 8192, 64 heads over 8 KV heads: kvMul 8, hidden
    28672) and Llama-3.1-405B attention (dim 16384, 128 heads over 8 KV heads: kvMul 16; hidden cut
    to 16384 to keep the synthetic file small). Checks the tilings, the attention block's
    workgroup plan at these widths and the kvMul 8 / 16 attention."""
    from distributed_llama_multiusers_amd.models.synthetic import make_test_assets
    from distributed_llama_multiusers_amd.utils.mfile import FloatType
    dims = {"70b": dict(dim=8192, hidden_dim=28672, n_heads=64, n_kv_heads=8),
            "405b": dict(dim=16384, hidden_dim=16384, n_heads=128, n_kv_heads=8)}[shape]
    m, _, _ = make_test_assets(str(tmp_path), "tiny", FloatType.Q40, seq_len=64, seed=21, n_layers=1,
                               vocab_size=1024, **dims)
    gpu = C.HipEngine(m, "q80", kv_bf16=False, max_batch=8)
    cpu = C.cpu_backend(m, "q80", 16)
    toks = [1, 2, 3, 500]
    assert _rel(_seq(gpu, toks), _seq(cpu, toks)) < 3e-2


@pytest.mark.parametrize("kv_bf16,page", [(True, 32), (False, 64)])
def test_paged_kv_cache_matches_contiguous(C, medium, kv_bf16, page):
    """Paged KV cache (page table per slot over a shared pool): the same forwards as the contiguous
    cache give bitwise the same logits - interleaved slots, a prefill chunk crossing page edges
    (MFMA path), single decode rows, a decode chain mapping pages ahead, a slot restarted at
    position 0 (its pages released and reused by another slot) - and the pool's free count follows."""
    seq = [int(t) for t in np.random.default_rng(5).integers(0, 2048, 200)]
    kw = dict(kv_bf16=kv_bf16, max_batch=64, n_slots=3)
    ref = C.HipEngine(medium, "q80", **kw)
    pg = C.HipEngine(medium, "q80", kv_pages=12, kv_page_size=page, **kw)
    assert pg.kv_pages_free == 12 and ref.kv_pages_free == -1

    def both(toks, pos, slots):
        a, b = ref.forward(toks, pos, slots), pg.forward(toks, pos, slots)
        assert np.array_equal(a, b)

    both(seq[:40], list(range(40)), [1] * 40)          # slot 1: 40 positions (pages 0..)
    both(seq[:3], [0, 1, 2], [2] * 3)                   # slot 2
    for p in range(40, 44):                             # interleaved single rows
        both([seq[p]], [p], [1])
        both([seq[p - 37]], [p - 37], [2])
    _, ca = ref.decode_greedy(20, [seq[44]], [44], [1])
    _, cb = pg.decode_greedy(20, [seq[44]], [44], [1])
    assert list(ca) == list(cb)
    used = 12 - pg.kv_pages_free
    assert used == -(-64 // page) + -(-7 // page)
    both(seq[100:110], list(range(10)), [1] * 10)       # slot 1 restarts: its pages are released
    assert 12 - pg.kv_pages_free == -(-10 // page) + -(-7 // page)
    both(seq[:64], list(range(64)), [0] * 64)           # slot 0 takes pages slot 1 gave back
    both([seq[64]], [64], [0])


def test_paged_kv_long_context_mfma_attention(C, tmp_path):
    """Paged KV at long context: decode rows at positions ~1500 of a 2048-position cache run the
    MFMA decode attention (bf16 cache >= 1024 positions), whose chunk page ids are looked up once
    per workgroup and shuffled to the key rows: bitwise the contiguous cache's logits, pages of 64
    and 128 positions."""
    from distributed_llama_multiusers_amd.models.synthetic import make_test_assets
    from distributed_llama_multiusers_amd.utils.mfile import FloatType
    m, _, _ = make_test_assets(str(tmp_path), "tiny", FloatType.Q40, seq_len=2048, seed=17, dim=1024,
                               hidden_dim=2816, n_heads=8, n_kv_heads=2, n_layers=2, vocab_size=1024)
    seq = [int(t) for t in np.random.default_rng(8).integers(0, 1024, 1504)]
    ref = C.HipEngine(m, "q80", kv_bf16=True, max_batch=256, n_slots=1)
    for page in (64, 128):
        pg = C.HipEngine(m, "q80", kv_bf16=True, max_batch=256, n_slots=1, kv_pages=2048 // page,
                         kv_page_size=page)
        for e in (ref, pg):
            for s0 in range(0, 1500, 250):
                e.forward_argmax(seq[s0:s0 + 250], list(range(s0, s0 + 250)), [0] * 250)
        for p in range(1500, 1504):
            a, b = ref.forward([seq[p]], [p], [0]), pg.forward([seq[p]], [p], [0])
            assert np.array_equal(a, b), (page, p)


def test_paged_kv_pool_exhaustion_raises(C, medium):
    """A forward that needs more pages than the pool has left fails with a clear error instead of
    writing through an unmapped page."""
    pg = C.HipEngine(medium, "q80", kv_bf16=True, max_batch=64, n_slots=2, kv_pages=2, kv_page_size=32)
    pg.forward(list(range(1, 41)), list(range(40)), [0] * 40)  # 2 pages
    with pytest.raises(RuntimeError, match="KV page pool exhausted"):
        pg.forward([5], [0], [1])


@pytest.mark.parametrize("sync", ["f32", "q80"])
def test_compute_only_rank_fused_matches_separate(C, medium, sync, monkeypatch):
    """bench.py --tp-rank-compute: a TP-2 rank with no peers (ComputeOnlyComm). The fused exchange
    in loopback (peers read as zeros) and the separate collectives (no-ops) must give the same
    shard logits: the timed kernels are the rank's real shard kernels, only the exchange removed."""
    tokens = [3, 17, 101, 7]
    out = {}
    for fused in (True, False):
        monkeypatch.setenv("DL_TP_FUSED", "1" if fused else "0")
        e = C.HipEngine(medium, "q80", max_batch=8, rank=0, world=2, comm=C.ComputeOnlyComm(0, 2, 0),
                        sync_type=sync)
        assert bool(e.tp_fused) == fused
        vocab0 = e.header["vocab_size"] // 2
        out[fused] = np.stack([e.forward([t], [p], [0])[0][:vocab0] for p, t in enumerate(tokens)])
        ids = e.forward_argmax(tokens, list(range(4)), [0] * 4)
        assert all(0 <= i < vocab0 for i in ids)
        del e
        # single-row greedy forwards (the argmax fused into the logits GEMV, or the separate argmax
        # + pick): the winner is this shard's own argmax (no phantom peer offering value 0 at index 0)
        e = C.HipEngine(medium, "q80", max_batch=8, rank=0, world=2, comm=C.ComputeOnlyComm(0, 2, 0),
                        sync_type=sync)
        ids1 = [e.forward_argmax([t], [p], [0])[0] for p, t in enumerate(tokens)]
        assert ids1 == [int(i) for i in out[fused].argmax(-1)], (ids1, out[fused].argmax(-1), out[fused].max(-1))
        del e
    assert np.isfinite(out[True]).all()
    if sync == "f32":
        assert np.array_equal(out[True], out[False])
    else:  # a Q80 rounding may flip by one step between the fused tail and the roundtrip kernel
        assert _rel(out[True], out[False]) < 2e-3
