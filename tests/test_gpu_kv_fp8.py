"""The fp8 (e4m3) KV cache, `kv_dtype="fp8"`: the append rule bit for bit, attnDecodeFp8Kernel<KM,HS>
against float64 attention on the stored values, an engine end to end, and the refusals.

Rule: a rotated K or a V value x is stored as e4m3fn(clamp(x, -448, 448)), round to nearest even,
subnormals kept; torch's CPU conversion is that rounding (E4 below). Attention over an fp8 cache is
attention over the stored values with the bf16 MFMA kernels' arithmetic (fp8 -> bf16 is exact), so the
bound is their 1.2e-2 (test_gpu_attention_paths.py B_MFMA), on that file's metric and input recipe:
q scale 1 plus a per-KV-head offset, poison (a dominant K, the largest V) behind every row's last
position, in the slot no row addresses and in the unmapped page. The kernel's tile is 64 keys.

fp8 caches have no prefill kernel (attnPrefillSupported is false: prompt rows take the decode kernel),
so there is no prefill case here.
"""
import functools

import numpy as np
import pytest
import torch

import kernel_checks

pytestmark = pytest.mark.gpu

B_MFMA, MARGIN, TILE = 1.2e-2, 20.0, 64


def E4(x):
    return x.clamp(-448, 448).to(torch.float8_e4m3fn).float()


@pytest.fixture(scope="module")
def ops():
    from distributed_llama_multiusers_amd import ops as o
    return o


# ------------------------------------------------------------------------------------- 1. append
def _append(ops, op, hs, kv_dtype):
    """q0 = 2 heads, kv0 = 2 heads; weight row pairs scaled by 2^-14 .. 2^12 so the K / V rows span
    zero, the subnormals, the normals and the clamp."""
    g = torch.Generator().manual_seed(11 + hs)
    n, q0, kv0, seq = 256, 2 * hs, 2 * hs, 64
    rows = q0 + 2 * kv0
    scale = 2.0 ** ((torch.arange(rows) // 2) % 27 - 14).float()
    blocks = ops.quantize_q40(torch.randn(rows, n, generator=g) * scale[:, None])
    x, nw = torch.randn(4, n, generator=g), torch.rand(n, generator=g) + 0.5
    import distributed_llama_multiusers_amd as dl
    rope = torch.from_numpy(dl.native().cpu_ops.rope_table(dict(
        dim=32 * hs, hidden_dim=1, n_layers=1, n_heads=32, n_kv_heads=8, vocab_size=32, seq_len=seq,
        rope_theta=500000.0, rope_scaling_factor=8.0, rope_scaling_low_freq_factor=1.0,
        rope_scaling_high_freq_factor=4.0, rope_scaling_orig_max_seq_len=8192, rope_type=2)))
    pos = [5, 0, 63, 17]
    if op == "qkv_rope":
        _, k, v = ops.qkv_rope(blocks, q0, kv0, hs, n, x, nw, 1e-5, rope, seq, pos, False, kv_dtype=kv_dtype)
        return k, v
    r = ops.gemm(x, blocks=blocks, rows=rows, n=n, lanes=0, input="norm", norm_w=nw, epilogue="qkv", q0=q0, kv0=kv0,
                 head_size=hs, rope=rope, n_slots=2, pos=pos, slot=[1, 0, 1, 0], kv_bf16=False, kv_dtype=kv_dtype)
    return r["k"], r["v"]


@pytest.mark.parametrize("hs", [64, 128])
@pytest.mark.parametrize("op", ["qkv_rope", "gemm"])
def test_append_is_the_rule_bit_for_bit(ops, op, hs):
    """The same launch with an f32 cache (the very values the epilogue computed) and with an fp8 one:
    only the store differs, so the fp8 rows are the rule applied to the f32 rows, exactly."""
    k32, v32 = _append(ops, op, hs, "f32")
    k8, v8 = _append(ops, op, hs, "fp8")
    for x32, x8 in ((k32, k8), (v32, v8)):
        a = x32.abs()
        assert bool((a > 448).any()) and bool(((a < 2.0 ** -6) & (a >= 2.0 ** -10)).any()) and bool((a < 2.0 ** -10).any())
        assert torch.equal(x8, E4(x32))


# ------------------------------------------------------------------------------------- 2. decode
@functools.lru_cache(maxsize=4)
def _operands(pos, kvm, hs, seq=1088, seed=7):
    """(q, k, v, poison K row, poison V row, slots, n_slots): the recipe of test_gpu_attention_paths.py
    _base on e4m3 values; the margin of the poison score is asserted on the rounded values."""
    g = torch.Generator().manual_seed(seed)
    B, nkv = len(pos), 2
    slots, n_slots, kv0 = tuple(range(B))[::-1], B + 1, nkv * hs
    k, v = E4(torch.randn(n_slots, seq, kv0, generator=g)), E4(torch.randn(n_slots, seq, kv0, generator=g))
    mu = torch.randn(nkv, hs, generator=g)
    q = torch.randn(B, nkv, kvm, hs, generator=g) + mu[None, :, None, :]
    mq, qd = q.mean((0, 2)).double(), q.double()
    kd = k.double().reshape(n_slots, seq, nkv, hs)
    smax = torch.stack([torch.einsum("tkd,kmd->kmt", kd[s, :p + 1], qd[b]).amax((1, 2))
                        for b, (p, s) in enumerate(zip(pos, slots))]).amax(0) / hs ** 0.5
    dmin = (torch.einsum("bkmd,kd->bkm", qd, mq) / hs ** 0.5).amin((0, 2))
    assert bool((dmin > 0).all())
    pk = E4(((smax + MARGIN + 2.0) / dmin * 1.07)[:, None].float() * mq.float())  # 1.07: e4m3 rounds by up to 2^-4
    margin = torch.einsum("bkmd,kd->bkm", qd, pk.double()) / hs ** 0.5 - smax[None, :, None]
    assert float(margin.min()) >= MARGIN and float(pk.abs().max()) < 448
    pk, pv = pk.reshape(-1), torch.full((kv0,), 448.0)
    last = [-1] * n_slots
    for p, s in zip(pos, slots):
        last[s] = p
    for s in range(n_slots):
        k[s, last[s] + 1:], v[s, last[s] + 1:] = pk, pv
    return q.reshape(B, -1), k, v, pk, pv, list(slots), n_slots


def _page_map(pos, slots, n_slots, seq, page):
    """A shuffled, interleaved map of the pages the rows reach; the rest -1 (the poison page)."""
    pps = (seq + page - 1) // page
    po = [[-1] * pps for _ in range(n_slots)]
    for p, s in zip(pos, slots):
        for pg in range(p // page + 1):
            po[s][pg] = ((pg * n_slots + s) * 7 + 3) % (n_slots * pps)
    flat = [x for r in po for x in r if x >= 0]
    assert len(set(flat)) == len(flat)
    return po


# lengths 1, TILE - 1, TILE, TILE + 1; the batched plan's first chunk edge (256) - 1 / + 1 and 1025 keys
# (5 chunks); the single-row geometry's first edge (128) - 1 / + 1 and its 512 / 513 boundary
SHORT, LONG = (0, TILE - 2, TILE - 1, TILE), (254, 256, 1024)
CASES = [("tile edges", SHORT, 4, 128, {}),
         ("tile edges hs64 kvm8", SHORT, 8, 64, {}),
         ("chunk edges kvm1", LONG, 1, 128, {}),
         ("chunk edges hs64 kvm4", LONG, 4, 64, {}),
         ("kvm8 kernel named", LONG, 8, 128, {"kernel": "fp8"}),
         ("single row 127", (126,), 4, 128, {"single": True}),
         ("single row 129", (128,), 4, 128, {"single": True}),
         ("single row 513 hs64", (512,), 1, 64, {"single": True}),
         ("paged, 32-key pages", (300, 17, 600), 4, 128, {"page": 32}),
         ("paged hs64", (300, 17, 600), 8, 64, {"page": 32}),
         ("f16 writer", LONG, 4, 128, {"out": "f16"}),
         ("q80 writer", LONG, 4, 64, {"out": "q80"}),
         ("repeat", LONG + SHORT, 4, 128, {"repeat": 2})]


@pytest.mark.parametrize("name,pos,kvm,hs,kw", CASES, ids=[c[0] for c in CASES])
def test_decode_kernel_against_float64_on_the_stored_values(ops, name, pos, kvm, hs, kw):
    """repeat=2: the op itself requires the second launch on the same scratch to be bitwise equal and
    every arrival counter to be zero after each launch."""
    q, k, v, pk, pv, slots, n_slots = _operands(pos, kvm, hs)
    kw, H, seq = dict(kw), 2 * kvm, k.shape[1]
    page = kw.pop("page", 0)
    if page:
        kw.update(page_size=page, page_of=_page_map(pos, slots, n_slots, seq, page))
    r = ops.attention_launch(q, k, v, H, kvm, hs, pos, slots, kv_dtype="fp8", poison_k=pk, poison_v=pv, **kw)
    assert r["kernel"] == f"attnDecodeFp8Kernel<{kvm},{hs}>"
    if name.startswith("chunk edges"):
        assert [s[0] for s in r["splits"]] == [1, 2, 5]
    if name.startswith("single row"):
        assert r["splits"][0][0] == {126: 1, 128: 2, 512: 3}[pos[0]]
    want = ops.ref_attention(q, k, v, H, kvm, hs, pos, slots, dtype=torch.float64)
    if kw.get("out") == "q80":
        kernel_checks.check_q80_row(r["out"].long(), r["scales"][..., 0], r["scales"][..., 1], want, name, kernel_bound=B_MFMA)
        return
    got, w = r["out"].double().reshape(len(pos), H, hs), want.double().reshape(len(pos), H, hs)
    assert bool(torch.isfinite(got).all())
    rel = float(((got - w).norm(dim=-1) / w.norm(dim=-1)).max())
    print(f"{name}: worst (row, head) rel {rel:.3e} (bound {B_MFMA:.1e})")
    assert rel < B_MFMA


# ------------------------------------------------------------------------------------- 4. engine
MODELS = {128: dict(dim=1024, n_heads=8, n_kv_heads=2, hidden_dim=2048), 64: dict(dim=512, n_heads=8, n_kv_heads=2, hidden_dim=1024)}
N_PROMPT, N_DECODE = 40, 24


def _dev(a, b):
    return float(np.abs(a - b).max() / np.abs(b).max())


@pytest.mark.parametrize("hs", [128, 64])
def test_engine_tracks_the_e4m3_oracle(C, tmp_path, hs):
    """A 40-token prompt in one forward, then 24 single-row decode steps, against TorchLlama with the
    e4m3 rule as kv_round. d_fp8 / d_bf16: the oracle with that rounding / with bf16 rounding against
    the oracle without (what the cache type itself costs); the engine must track the e4m3 oracle within
    max(d_fp8 / 2, 3e-2), 3e-2 being test_gpu_engine.py's tolerance for its Q40, bf16-KV case.
    Measured (CPU oracles; engine on an MI355X), hs 128: d_fp8 2.08e-2, d_bf16 1.33e-2, engine 1.75e-2;
    hs 64: d_fp8 2.03e-2, d_bf16 1.53e-2, engine 1.72e-2 (the engine's distance is the Q40 / Q80
    quantisation noise both cache types share, so the 3e-2 term decides).
    Also: kv_bytes is a quarter of the f32 engine's, and a prefix copied into a second slot decodes
    bitwise the same row (the 1-byte copy path)."""
    from distributed_llama_multiusers_amd.models.llama import TorchLlama
    from distributed_llama_multiusers_amd.models.synthetic import make_test_assets
    from distributed_llama_multiusers_amd.utils.mfile import FloatType
    m, _, spec = make_test_assets(str(tmp_path), "tiny", FloatType.Q40, seq_len=128, seed=3, n_layers=2, vocab_size=2048, **MODELS[hs])
    toks = np.random.default_rng(5).integers(0, spec.vocab_size, N_PROMPT + N_DECODE).tolist()
    oracle = TorchLlama(m)

    def run(kv_round):
        kv = {}
        rows = [oracle.forward(toks[:N_PROMPT], 0, kv, kv_round=kv_round)[-1]]
        rows += [oracle.forward([toks[p]], p, kv, kv_round=kv_round)[0] for p in range(N_PROMPT, N_PROMPT + N_DECODE)]
        return torch.stack(rows).numpy()

    plain, want = run(None), run(E4)
    d_fp8, d_bf16 = _dev(want, plain), _dev(run(lambda x: x.bfloat16().float()), plain)
    eng = C.HipEngine(m, "q80", kv_dtype="fp8", max_batch=64, n_slots=2)
    assert eng.kv_bytes * 4 == C.HipEngine(m, "q80", kv_dtype="f32", max_batch=64, n_slots=2).kv_bytes
    got = [eng.forward(toks[:N_PROMPT], list(range(N_PROMPT)), [0] * N_PROMPT)[-1]]
    eng.copy_prefix(0, 1, N_PROMPT)
    assert np.array_equal(eng.forward([toks[N_PROMPT]], [N_PROMPT], [1])[0], eng.forward([toks[N_PROMPT]], [N_PROMPT], [0])[0])
    got += [eng.forward([toks[p]], [p], [0])[0] for p in range(N_PROMPT, N_PROMPT + N_DECODE)]
    d_gpu = _dev(np.stack(got), want)
    print(f"hs {hs}: d_fp8 {d_fp8:.3e} d_bf16 {d_bf16:.3e} engine vs e4m3 oracle {d_gpu:.3e}")
    assert d_gpu <= max(0.5 * d_fp8, 3e-2)


# ------------------------------------------------------------------------------------- 5. refusals
@pytest.mark.parametrize("H,kvm,hs", [(1, 1, 96), (3, 3, 128)])
def test_plan_refuses_unsupported_shapes(ops, H, kvm, hs):
    q, kv = torch.zeros(1, H * hs), torch.zeros(1, 64, hs)
    with pytest.raises(RuntimeError, match="fp8 KV caches need head size 64 or 128 and kvMul 1, 2, 4 or 8"):
        ops.attention_launch(q, kv, kv, H, kvm, hs, [3], [0], kv_dtype="fp8", plan_only=True)


def test_engine_refuses_batch_invariant(C, assets):
    with pytest.raises(RuntimeError, match="fp8 cannot be combined with --batch-invariant"):
        C.HipEngine(assets["q40"], "q80", kv_dtype="fp8", batch_invariant=True)
