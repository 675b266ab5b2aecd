"""attnPrefillFp8Kernel<KM,HS>: the prompt rows of an fp8 (e4m3) KV cache, against float64 attention on
the stored values, and an engine whose prompt chunks take it.

Metric and bound are test_gpu_kv_fp8.py's (worst (row, head) norm-relative error under B_MFMA = 1.2e-2:
the arithmetic is the bf16 MFMA kernels'), and so is the operand recipe: q scale 1 plus a per-KV-head
offset; the poison (a dominant K row, V = 448, margin >= 20 asserted on the rounded values) behind every
slot's last position, in a slot no row addresses and in the unmapped pages. Rows of a block share a
slot, so a causal mask wrong by one inside a block reaches a real neighbouring key, not the poison:
every case is also run with the dominant key at one spot position t and a small-integer V row there
(0, the first row's position + 1, a 32-key edge inside the block's positions, the chunk edge); rows at
or past t must follow it and rows before t must not, and the float64 reference decides both.

Measured on an MI355X, worst error per case: see profiles/kv_fp8.md ("Prefill" section).
"""
import functools

import numpy as np
import pytest
import torch

B_MFMA, MARGIN, SEQ = 1.2e-2, 20.0, 320


def E4(x):
    return x.clamp(-448, 448).to(torch.float8_e4m3fn).float()


@pytest.fixture(scope="module")
def ops():
    from distributed_llama_multiusers_amd import ops as o
    return o


def _r(a, b):
    return tuple(range(a, b + 1))


SPLIT = (_r(250, 265), (0,) * 16)
TWO = (_r(0, 15) + _r(250, 261), (1,) * 16 + (0,) * 12)
# name, positions, slot of every row, kvm, hs, launch keywords
CASES = [("first chunk", _r(0, 15), (0,) * 16, 4, 128, {}),
         ("tile edge in the block", _r(56, 71), (0,) * 16, 4, 128, {}),
         ("tile edge hs64 kvm8", _r(56, 63), (0,) * 8, 8, 64, {}),
         ("two blocks, two slots", *TWO, 4, 64, {}),
         ("split", *SPLIT, 4, 128, {}),
         ("scattered rows", (5, 40, 41, 100, 31, 32, 260), (0,) * 7, 8, 128, {}),
         ("kvm1", _r(200, 263), (0,) * 64, 1, 128, {}),
         ("kvm2 hs64", _r(120, 151), (0,) * 32, 2, 64, {}),
         ("paged split", *SPLIT, 4, 128, {"page": 32}),
         ("paged two slots", *TWO, 4, 64, {"page": 32}),
         ("f16 output", *SPLIT, 4, 128, {"out": "f16"}),
         ("scratch reuse", *SPLIT, 4, 128, {"repeat": 2})]


@functools.lru_cache(maxsize=4)
def _operands(pos, slots, kvm, hs):
    """(q, k, v, poison K row, poison V row, n_slots, last position per slot); slot n_slots - 1 is addressed by no row."""
    g = torch.Generator().manual_seed(7)
    B, nkv, n_slots = len(pos), 2, max(slots) + 2
    kv0 = nkv * hs
    k, v = E4(torch.randn(n_slots, SEQ, kv0, generator=g)), E4(torch.randn(n_slots, SEQ, kv0, generator=g))
    mu = torch.randn(nkv, hs, generator=g)
    q = torch.randn(B, nkv, kvm, hs, generator=g) + mu[None, :, None, :]
    mq, qd = q.mean((0, 2)).double(), q.double()
    kd = k.double().reshape(n_slots, SEQ, nkv, hs)
    smax = torch.stack([torch.einsum("tkd,kmd->kmt", kd[s, :p + 1], qd[b]).amax((1, 2))
                        for b, (p, s) in enumerate(zip(pos, slots))]).amax(0) / hs ** 0.5
    dmin = (torch.einsum("bkmd,kd->bkm", qd, mq) / hs ** 0.5).amin((0, 2))
    assert bool((dmin > 0).all())
    pk = E4(((smax + MARGIN + 2.0) / dmin * 1.07)[:, None].float() * mq.float())  # 1.07: e4m3 rounds by up to 2^-4
    margin = torch.einsum("bkmd,kd->bkm", qd, pk.double()) / hs ** 0.5 - smax[None, :, None]
    assert float(margin.min()) >= MARGIN and float(pk.abs().max()) < 448
    pk, pv = pk.reshape(-1), torch.full((kv0,), 448.0)
    last = [max([p for p, s in zip(pos, slots) if s == sl], default=-1) for sl in range(n_slots)]
    for s in range(n_slots):
        k[s, last[s] + 1:], v[s, last[s] + 1:] = pk, pv
    return q.reshape(B, -1), k, v, pk, pv, n_slots, last


def _page_map(last, page):
    """A shuffled, interleaved map of the pages the slots' rows reach; the rest -1 (the poison page)."""
    pps, n = (SEQ + page - 1) // page, len(last)
    po = [[((pg * n + s) * 7 + 3) % (n * pps) if pg <= last[s] // page and last[s] >= 0 else -1 for pg in range(pps)]
          for s in range(n)]
    flat = [x for r in po for x in r if x >= 0]
    assert len(set(flat)) == len(flat)
    return po


def _rel(got, want, B, H, hs):
    g, w = got.double().reshape(B, H, hs), want.double().reshape(B, H, hs)
    assert bool(torch.isfinite(g).all())
    return float(((g - w).norm(dim=-1) / w.norm(dim=-1)).max())


@pytest.mark.gpu
@pytest.mark.parametrize("name,pos,slots,kvm,hs,kw", CASES, ids=[c[0] for c in CASES])
def test_prefill_kernel_against_float64_on_the_stored_values(ops, name, pos, slots, kvm, hs, kw):
    """repeat=2: the op itself requires the second launch on the same scratch to be bitwise equal and
    every arrival counter to be zero after each launch."""
    q, k, v, pk, pv, n_slots, last = _operands(pos, slots, kvm, hs)
    kw, H, rpb = dict(kw), 2 * kvm, 64 // kvm
    page = kw.pop("page", 0)
    if page:
        kw.update(page_size=page, page_of=_page_map(last, page))
    kw.update(kv_dtype="fp8", prefill=True, poison_k=pk, poison_v=pv)
    plan = ops.attention_launch(q, k, v, H, kvm, hs, pos, slots, plan_only=True, **kw)
    if pos == SPLIT[0]:
        assert plan["splits"] == [(2, 160)]
    spot = {0, pos[0] + 1}
    for b0, (ns, ch) in zip(range(0, len(pos), rpb), plan["splits"]):
        lo, hi = min(pos[b0:b0 + rpb]), max(pos[b0:b0 + rpb])
        spot |= {t for t in range(32, hi + 1, 32) if lo < t}.union({ch} if ns > 1 else ())
    worst = 0.0
    for t in [None] + sorted(spot):
        ks, vs = k, v
        if t is not None:
            ks, vs = k.clone(), v.clone()
            for s in range(n_slots):
                if t <= last[s]:
                    ks[s, t], vs[s, t] = pk, ((torch.arange(v.shape[-1]) % 13) - 6).float()
        r = ops.attention_launch(q, ks, vs, H, kvm, hs, pos, slots, **kw)
        assert r["kernel"] == f"attnPrefillFp8Kernel<{kvm},{hs}>" and r["splits"] == plan["splits"]
        want = ops.ref_attention(q, ks, vs, H, kvm, hs, pos, slots, dtype=torch.float64)
        if kw.get("out") == "f16":
            r32 = ops.attention_launch(q, ks, vs, H, kvm, hs, pos, slots, **{**kw, "out": "f32"})
            assert torch.equal(r["out"], r32["out"].half().float())
        worst = max(worst, _rel(r["out"], want, len(pos), H, hs))
    print(f"{name}: spots {sorted(spot)}, worst (row, head) rel {worst:.3e} (bound {B_MFMA:.1e})")
    assert worst < B_MFMA


def test_plan_names_the_kernel_and_keeps_refusing(ops):
    def plan(H, kvm, hs, slots=(0, 0), **kw):
        q, kv = torch.zeros(len(slots), H * hs), torch.zeros(3, 64, H // kvm * hs)
        return ops.attention_launch(q, kv, kv, H, kvm, hs, [3] * len(slots), slots, kv_dtype="fp8", prefill=True,
                                    plan_only=True, **kw)
    for hs in (64, 128):
        for kvm in (1, 2, 4, 8):
            for kernel in ("auto", "prefill"):
                assert plan(2 * kvm, kvm, hs, kernel=kernel)["kernel"] == f"attnPrefillFp8Kernel<{kvm},{hs}>"
    for H, kvm, hs in ((1, 1, 96), (3, 3, 128)):
        with pytest.raises(RuntimeError, match="fp8 KV caches need head size 64 or 128 and kvMul 1, 2, 4 or 8"):
            plan(H, kvm, hs)
    with pytest.raises(RuntimeError, match="prefill row blocks must share a slot"):
        plan(8, 4, 128, slots=(0, 1))
    with pytest.raises(RuntimeError, match="no Q80 output"):
        plan(8, 4, 128, out="q80")


MODELS = {128: dict(dim=1024, n_heads=8, n_kv_heads=2, hidden_dim=2048), 64: dict(dim=512, n_heads=8, n_kv_heads=2, hidden_dim=1024)}
N_PROMPT, N_DECODE, CHUNK = 300, 8, 64


@pytest.mark.gpu
@pytest.mark.parametrize("hs", [128, 64])
def test_engine_prompt_takes_the_prefill_kernel(C, tmp_path, hs):
    """A 300-token prompt in forwards of 64 rows (the last chunks split at 256 keys), then 8 decode rows,
    against TorchLlama with the e4m3 rule as kv_round: within max(d_fp8 / 2, 3e-2), the rule and origin
    of test_gpu_kv_fp8.py's engine test (d_fp8: what the rounding itself costs the oracle)."""
    from distributed_llama_multiusers_amd.models.llama import TorchLlama
    from distributed_llama_multiusers_amd.models.synthetic import make_test_assets
    from distributed_llama_multiusers_amd.utils.mfile import FloatType
    m, _, spec = make_test_assets(str(tmp_path), "tiny", FloatType.Q40, seq_len=512, seed=3, n_layers=2, vocab_size=2048, **MODELS[hs])
    toks = np.random.default_rng(5).integers(0, spec.vocab_size, N_PROMPT + N_DECODE).tolist()
    oracle = TorchLlama(m)

    def run(kv_round):
        kv = {}
        rows = [oracle.forward(toks[:N_PROMPT], 0, kv, kv_round=kv_round)[-1]]
        rows += [oracle.forward([toks[p]], p, kv, kv_round=kv_round)[0] for p in range(N_PROMPT, N_PROMPT + N_DECODE)]
        return torch.stack(rows).numpy()

    def dev(a, b):
        return float(np.abs(a - b).max() / np.abs(b).max())

    plain, want = run(None), run(E4)
    eng = C.HipEngine(m, "q80", kv_dtype="fp8", max_batch=64, n_slots=2)
    assert eng.prefill_attn_kernel(CHUNK, N_PROMPT - 1) == f"attnPrefillFp8Kernel<4,{hs}>"
    for p0 in range(0, N_PROMPT, CHUNK):
        ps = list(range(p0, min(p0 + CHUNK, N_PROMPT)))
        got = [eng.forward([toks[p] for p in ps], ps, [0] * len(ps))[-1]]
    got += [eng.forward([toks[p]], [p], [0])[0] for p in range(N_PROMPT, N_PROMPT + N_DECODE)]
    d_fp8, d_gpu = dev(want, plain), dev(np.stack(got), want)
    print(f"hs {hs}: d_fp8 {d_fp8:.3e} engine vs e4m3 oracle {d_gpu:.3e}")
    assert d_gpu <= max(0.5 * d_fp8, 3e-2)
