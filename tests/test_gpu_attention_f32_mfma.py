"""attnDecodeF32MfmaKernel<KM,HS> (csrc/hip/attn_mfma_f32.hip): MFMA decode attention over an f32
KV cache against ops.ref_attention in float64. The arithmetic is f32 MFMAs, __expf and f32
reassociation, as test_attention_prefill_f32's, so its bound holds: relative L2 error < 1e-5, taken
per row so that one short row cannot hide behind its long neighbours. Tiles are 16 keys at head
size 128 and 32 at 64; a workgroup's 4 waves take tiles round-robin (a round is 64 / 128 keys)."""
import numpy as np
import pytest
import torch

import kernel_checks

pytestmark = pytest.mark.gpu

BOUND = 1e-5
LENS = {128: [1, 15, 16, 17, 63, 64, 65, 127, 128, 129], 64: [31, 32, 33, 127, 128, 129]}
SHAPES = [(hs, kvm) for hs in (128, 64) for kvm in (1, 2, 4, 8)]


@pytest.fixture(scope="module")
def ops():
    from distributed_llama_multiusers_amd import ops as o
    return o


def rel(got, want):
    """Largest relative L2 error over the rows."""
    g, w = got.double(), want.double()
    return float(((g - w).norm(dim=-1) / w.norm(dim=-1).clamp_min(1e-30)).max())


def setup(lens, hs, kvm, spot=None, seq=None):
    """q [B, H hs] (the heads of a KV group share a mean), k / v [B slots, seq, kv0] (row b on slot
    B - 1 - b, n_heads0 = 2 kv_mul) and the float64 reference. spot(len) -> key position: that key
    scores >= 25 above every other key of its row for all heads (asserted) and V is zero elsewhere,
    so the output is that V row."""
    from distributed_llama_multiusers_amd import ops as o
    B, H, kv0 = len(lens), 2 * kvm, 2 * hs
    g = torch.Generator().manual_seed(1000 * hs + 10 * kvm + len(lens))
    mu = torch.randn(2, 1, hs, generator=g)
    q = (torch.randn(B, 2, kvm, hs, generator=g) + 2 * mu).reshape(B, -1)
    k = torch.randn(B, seq or max(lens) + 7, kv0, generator=g)
    v = torch.randn(k.shape, generator=g)
    pos, slots = [n - 1 for n in lens], list(range(B))[::-1]
    for b, n in enumerate(lens if spot is not None else []):
        t, s = spot(n), slots[b]
        k[s, t] = 4 * mu.reshape(-1)
        sc = torch.einsum("tgd,gmd->gmt", k[s, :n].reshape(n, 2, hs), q[b].reshape(2, kvm, hs)) / hs ** 0.5
        others = [i for i in range(n) if i != t]
        assert n == 1 or float((sc[..., t:t + 1] - sc)[..., others].min()) >= 25
        row = v[s, t].clone()
        v[s] = 0
        v[s, t] = row
    return q, k, v, H, pos, slots, o.ref_attention(q, k, v, H, kvm, hs, pos, slots, dtype=torch.float64)


def run(ops, q, k, v, H, kvm, hs, pos, slots, **kw):
    r = ops.attention_launch(q, k, v, H, kvm, hs, pos, slots, kv_bf16=False, kernel="mfma", **kw)
    assert r["kernel"] == f"attnDecodeF32MfmaKernel<{kvm},{hs}>", r["kernel"]
    return r


@pytest.mark.parametrize("hs,kvm", SHAPES)
def test_tile_and_wave_edges(ops, hs, kvm):
    """One chunk: the first tile only, fewer tiles than waves, the exact round, one past it."""
    q, k, v, H, pos, slots, want = setup(LENS[hs], hs, kvm)
    r = run(ops, q, k, v, H, kvm, hs, pos, slots)
    assert all(ns == 1 for ns, _ in r["splits"])
    assert rel(r["out"], want) < BOUND, rel(r["out"], want)
    direct = ops.attention(q, k, v, H, kvm, hs, pos, slots, kv_bf16=False, impl="mfma")
    assert rel(direct, want) < BOUND, rel(direct, want)


@pytest.mark.parametrize("hs,kvm", SHAPES)
@pytest.mark.parametrize("where", ["first", "last", "tile_end"])
def test_spotlight_key(ops, hs, kvm, where):
    """One dominating key (position 0, the last one, the last key of the last whole tile), V zero
    elsewhere: a key order permuted between S^T and V^T would return another row's zeros."""
    tile = 2048 // hs
    spot = {"first": lambda n: 0, "last": lambda n: n - 1, "tile_end": lambda n: max(n // tile * tile - 1, 0)}[where]
    q, k, v, H, pos, slots, want = setup(LENS[hs], hs, kvm, spot=spot)
    for b, n in enumerate(LENS[hs]):  # the reference is the spotlit V row of each head's group
        assert torch.allclose(want[b].reshape(2, kvm, hs), v[slots[b], spot(n)].double().reshape(2, 1, hs).expand(2, kvm, hs), atol=1e-9)
    got = run(ops, q, k, v, H, kvm, hs, pos, slots)["out"]
    assert rel(got, want) < BOUND, rel(got, want)


@pytest.mark.parametrize("hs,kvm", [(128, 1), (128, 8), (64, 4)])
def test_split_and_combine(ops, hs, kvm):
    """split_grid forced to 4: rows one short of, at and one past a chunk edge of their own plan, next
    to a row of 40 keys whose later chunks return early. repeat=3: the op asserts that the launches
    agree bitwise and leave the arrival counters and the guarded scratch clean."""
    lens = [511, 512, 513, 40]
    q, k, v, H, pos, slots, want = setup(lens, hs, kvm)
    r = run(ops, q, k, v, H, kvm, hs, pos, slots, split_grid=4, repeat=3)
    assert [tuple(x) for x in r["splits"]] == [(2, 256), (2, 256), (3, 176), (1, 48)] and tuple(r["grid"]) == (2, 4, 4)
    assert rel(r["out"], want) < BOUND, rel(r["out"], want)


@pytest.mark.parametrize("kvm", [2, 4])
def test_paged_cache_is_bitwise_the_contiguous_one(ops, kvm):
    """Pages of 32 keys, shuffled pool pages, every page past a row's length unmapped (the poison
    page): the page ids only redirect the DMA, so the result is the contiguous launch's, bitwise."""
    hs, lens = 128, [129, 70]
    q, k, v, H, pos, slots, want = setup(lens, hs, kvm, seq=192)
    page_of = [[7, 2, 10, -1, -1, -1], [9, 0, 11, 4, 6, -1]]  # [slot][page]: the row of 70 keys is on slot 0
    poison = torch.full((2 * hs,), 1e4)
    flat = run(ops, q, k, v, H, kvm, hs, pos, slots)["out"]
    paged = run(ops, q, k, v, H, kvm, hs, pos, slots, page_size=32, page_of=page_of, poison_k=poison, poison_v=poison)["out"]
    assert torch.equal(paged, flat)
    assert rel(paged, want) < BOUND, rel(paged, want)


def test_outputs_and_strides(ops):
    """f16 and Q80 block outputs and ldq / ld_out beyond q0 (guards after every row's valid part)."""
    hs, kvm = 128, 4
    q, k, v, H, pos, slots, want = setup([129, 300, 17], hs, kvm)
    q0 = H * hs
    qw = torch.full((len(pos), q0 + 36), 1e4)
    qw[:, :q0] = q
    f32 = run(ops, q, k, v, H, kvm, hs, pos, slots)["out"]
    assert rel(f32, want) < BOUND, rel(f32, want)
    for out in ("f32", "f16", "q80"):
        r = run(ops, q, k, v, H, kvm, hs, pos, slots, out=out)
        wide = run(ops, qw, k, v, H, kvm, hs, pos, slots, out=out, ldq=q0 + 36, ld_out=q0 + 64)
        assert torch.equal(wide["out"], r["out"]), out
        if out == "f16":
            assert torch.equal(r["out"], f32.half().float())
        if out == "q80":
            kernel_checks.check_q80_row(r["out"].long(), r["scales"][..., 0], r["scales"][..., 1], want, "q80", kernel_bound=BOUND)


def test_engine_takes_the_kernel(C, tmp_path, monkeypatch):
    """An f32-KV engine (f32 weights, head size 128) under DL_ATTN_MFMA=1 runs 16 decode rows and a
    single row at position 1024 on the new kernel; under DL_ATTN_MFMA=0 the VALU kernel and the same
    GEMVs, so the logits differ by the attention's reassociation only. By default no f32 forward
    selects the kernel (it measured slower: profiles/attn_f32_mfma.md). DL_GEMM_MIN keeps the 16 rows
    on the GEMV path: the batched GEMM path hands the attention output on in f16, where a last-bit
    f32 difference flips a rounding (measured 2.9e-4 there against 2.8e-7 / 3.5e-7 here)."""
    from distributed_llama_multiusers_amd.models.synthetic import make_test_assets
    from distributed_llama_multiusers_amd.utils.mfile import FloatType
    m, _, _ = make_test_assets(str(tmp_path), "tiny", FloatType.F32, seq_len=1088, seed=5, dim=512, hidden_dim=1024,
                               n_heads=4, n_kv_heads=2, n_layers=2, vocab_size=512)
    toks = [int(t) for t in np.random.default_rng(3).integers(0, 512, 1100)]
    monkeypatch.setenv("DL_GEMM_MIN", "1000")
    monkeypatch.delenv("DL_ATTN_MFMA", raising=False)
    e = C.HipEngine(m, "f32", kv_bf16=False, max_batch=256, n_slots=16)
    assert e.decode_attn_kernel(16, 2) == e.decode_attn_kernel(1, 1024) == "attnKernel"
    del e
    logits = {}
    for mode, name in (("1", "attnDecodeF32MfmaKernel<2,128>"), ("0", "attnKernel")):
        monkeypatch.setenv("DL_ATTN_MFMA", mode)
        e = C.HipEngine(m, "f32", kv_bf16=False, max_batch=256, n_slots=16)
        assert e.decode_attn_kernel(16, 2) == e.decode_attn_kernel(1, 1024) == name
        for p in range(3):  # 16 decode rows, one per slot
            rows = e.forward(toks[16 * p:16 * p + 16], [p] * 16, list(range(16)))
        for p0 in range(3, 1024, 256):  # slot 0 up to position 1023
            n = min(256, 1024 - p0)
            e.forward_argmax(toks[48 + p0:48 + p0 + n], list(range(p0, p0 + n)), [0] * n)
        logits[mode] = (rows, e.forward([toks[-1]], [1024], [0]))
    errs = [float(np.abs(a - b).max() / np.abs(b).max()) for a, b in zip(logits["1"], logits["0"])]
    print("16 rows, row at 1024: max |logit difference| / max |logit|", errs)
    assert max(errs) < 1e-4, errs  # tests/test_gpu_engine.py:52, the f32-weight, f32-KV logits tolerance
