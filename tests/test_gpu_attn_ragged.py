"""attnRaggedF32Kernel<KM,HS> (csrc/hip/attn_ragged.hip): decode rows and prompt chunks of several slots in one
launch against float64 attention, the host's plan of such a launch, and an engine's mixed forward.
Inputs: the recipe of test_gpu_kv_fp8.py _operands on unrounded f32 values (a dominant K and V = 1024 behind
every slot's last read position, in the slot no row addresses and in unmapped pages). Metric: worst (row,
head) relative L2. Bound: 1e-5, test_gpu_attention_paths.py's for attnPrefillF32Kernel (B_F32PF); the
key-split wave merge stays inside it (worst measured 9.8e-7). Schedules follow the kernel's rule, rows >
16 / kvMul: row-block, else key-split (so at kvMul 4 the 5-row tail of a 21-row chunk is row-block)."""
import functools

import numpy as np
import pytest
import torch

from test_gpu_kv_fp8 import MARGIN, MODELS, _page_map

gpu = pytest.mark.gpu
B_F32PF = 1e-5
SHAPES = [(4, 128), (8, 64), (1, 128), (2, 64)]


@pytest.fixture(scope="module")
def ops():
    from distributed_llama_multiusers_amd import ops as o
    return o


def _segments(slots, kvm):
    """Maximal runs of at most 64 / kvm consecutive rows of one slot: (first row, rows, schedule)."""
    out, b = [], 0
    while b < len(slots):
        e = b + 1
        while e < len(slots) and e - b < 64 // kvm and slots[e] == slots[b]:
            e += 1
        out.append((b, e - b, "row-block" if e - b > 16 // kvm else "key-split"))
        b = e
    return out


def _layout(name, kvm):
    rpb, rpw = 64 // kvm, 16 // kvm
    if name == "decode+chunk":  # 3 decode rows in 3 slots, then a 21-row chunk
        return (150, 40, 299) + tuple(range(130, 151)), (0, 1, 2) + (3,) * 21
    if name == "two chunks":  # rpb + a key-split tail from row 0, then another slot's chunk at an unaligned row
        n0, n1 = rpb + min(2, rpw), rpw + 1
        return tuple(range(200, 200 + n0)) + tuple(range(70, 70 + n1)), (1,) * n0 + (0,) * n1
    if name == "rows only":  # 1-row segments only
        return (0, 15, 16, 300, 63), (4, 3, 2, 1, 0)
    return tuple(range(100, 100 + rpb)), (0,) * rpb  # one full segment


@functools.lru_cache(maxsize=4)
def _operands(pos, slots, kvm, hs, seq=384, seed=7):
    g = torch.Generator().manual_seed(seed)
    B, nkv, n_slots = len(pos), 2, max(slots) + 2
    kv0 = nkv * hs
    k, v = torch.randn(n_slots, seq, kv0, generator=g), torch.randn(n_slots, seq, kv0, generator=g)
    mu = torch.randn(nkv, hs, generator=g)
    q = torch.randn(B, nkv, kvm, hs, generator=g) + mu[None, :, None, :]
    mq, qd = q.mean((0, 2)).double(), q.double()
    kd = k.double().reshape(n_slots, seq, nkv, hs)
    smax = torch.stack([torch.einsum("tkd,kmd->kmt", kd[s, :p + 1], qd[b]).amax((1, 2))
                        for b, (p, s) in enumerate(zip(pos, slots))]).amax(0) / hs ** 0.5
    dmin = (torch.einsum("bkmd,kd->bkm", qd, mq) / hs ** 0.5).amin((0, 2))
    assert bool((dmin > 0).all())
    pk = (((smax + MARGIN + 2.0) / dmin)[:, None] * mq).float()
    margin = torch.einsum("bkmd,kd->bkm", qd, pk.double()) / hs ** 0.5 - smax[None, :, None]
    assert float(margin.min()) >= MARGIN
    pk, pv = pk.reshape(-1), torch.full((kv0,), 1024.0)
    last = [max([p for p, t in zip(pos, slots) if t == s], default=-1) for s in range(n_slots)]
    for s in range(n_slots):
        k[s, last[s] + 1:], v[s, last[s] + 1:] = pk, pv
    return q.reshape(B, -1), k, v, pk, pv, n_slots


def _check(ops, name, pos, slots, kvm, hs, **kw):
    (q, k, v, pk, pv, n_slots), H = _operands(tuple(pos), tuple(slots), kvm, hs), 2 * kvm
    r = ops.attention_launch(q, k, v, H, kvm, hs, pos, slots, kv_dtype="f32", kernel="ragged", poison_k=pk, poison_v=pv, **kw)
    assert r["kernel"] == f"attnRaggedF32Kernel<{kvm},{hs}>" and r["segments"] == _segments(slots, kvm)
    want = ops.ref_attention(q, k, v, H, kvm, hs, pos, slots, dtype=torch.float64)
    got, w = r["out"].double().reshape(len(pos), H, hs), want.double().reshape(len(pos), H, hs)
    assert bool(torch.isfinite(got).all())
    rel = float(((got - w).norm(dim=-1) / w.norm(dim=-1)).max())
    print(f"{name}: worst (row, head) rel {rel:.3e} (bound {B_F32PF:.1e})")
    assert rel < B_F32PF
    return r


# ------------------------------------------------------------------------------- 1. kernel, float64
@gpu
@pytest.mark.parametrize("kvm,hs", SHAPES)
@pytest.mark.parametrize("layout", ["decode+chunk", "two chunks", "rows only", "full segment"])
def test_layouts_against_float64(ops, layout, kvm, hs):
    pos, slots = _layout(layout, kvm)
    r = _check(ops, f"{layout} kvm{kvm} hs{hs}", pos, slots, kvm, hs)
    assert {s[2] for s in r["segments"]} == {"decode+chunk": {"row-block", "key-split"}, "two chunks": {"row-block", "key-split"},
                      "rows only": {"key-split"}, "full segment": {"row-block"}}[layout]


@gpu
@pytest.mark.parametrize("kvm,hs", [(4, 128), (8, 64)])
@pytest.mark.parametrize("edge", [16, 32, 64, 256])
def test_rows_across_a_tile_or_split_edge(ops, edge, kvm, hs):
    """edge: a key-split wave's 16 keys, the row-block subtile, the 64-key tile, the first split (257 keys: two
    chunks). A 6-row and a 3-row chunk whose lengths straddle it, decode rows of edge and edge + 1 keys."""
    pos = tuple(range(edge - 3, edge + 3)) + tuple(range(edge - 2, edge + 1)) + (edge - 1, edge)
    r = _check(ops, f"edge {edge} kvm{kvm}", pos, (0,) * 6 + (1,) * 3 + (2, 3), kvm, hs)
    if edge == 256:
        assert [s[0] for s in r["splits"]] == [2, 2, 1, 2]


@gpu
def test_paged_cache_with_a_shuffled_map(ops):
    pos, slots = _layout("decode+chunk", 4)
    _check(ops, "paged", pos, slots, 4, 128, page_size=32, page_of=_page_map(pos, slots, max(slots) + 2, 384, 32))


@gpu
def test_second_launch_is_bitwise_equal(ops):
    """repeat=2: the op requires a bitwise equal second launch and zero counters; 257+ keys: the combine runs."""
    pos = (300, 280) + tuple(range(250, 271))
    _check(ops, "repeat", pos, (0, 1) + (2,) * 21, 4, 128, repeat=2)


# ------------------------------------------------------------------------------- 2. plan, no device
def test_plan_segments_and_surplus_workgroups(ops):
    z = torch.zeros
    for layout in ("decode+chunk", "two chunks", "rows only", "full segment"):
        for kvm, hs in SHAPES:
            pos, slots = _layout(layout, kvm)
            kv = z(max(slots) + 1, 384, 2 * hs)
            r = ops.attention_launch(z(len(pos), 2 * kvm * hs), kv, kv, 2 * kvm, kvm, hs, pos, slots, kv_dtype="f32",
                                     kernel="ragged", plan_only=True)
            assert r["kernel"] == f"attnRaggedF32Kernel<{kvm},{hs}>" and r["segments"] == _segments(slots, kvm)
            assert r["grid"] == (2 * len(pos), r["split_grid"], 1) and len(r["splits"]) == len(r["segments"])
            if layout != "rows only":  # fewer segments than the grid has room for: surplus workgroups exit
                assert len(r["segments"]) < len(pos)
    (pos, slots), kv = _layout("decode+chunk", 4), z(4, 384, 256)
    r = ops.attention_launch(z(24, 1024), kv, kv, 8, 4, 128, pos, slots, kv_dtype="f32", kernel="ragged", plan_only=True)
    assert r["segments"] == [(0, 1, "key-split"), (1, 1, "key-split"), (2, 1, "key-split"), (3, 16, "row-block"), (19, 5, "row-block")]
    pos, slots = _layout("two chunks", 4)
    r = ops.attention_launch(z(23, 1024), kv, kv, 8, 4, 128, pos, slots, kv_dtype="f32", kernel="ragged", plan_only=True)
    assert r["segments"] == [(0, 16, "row-block"), (16, 2, "key-split"), (18, 5, "row-block")]


@pytest.mark.parametrize("kw,H,kvm,hs,why", [(dict(kv_dtype="bf16"), 8, 4, 128, "f32 KV caches only"),
                                              (dict(kv_dtype="fp8"), 8, 4, 128, "f32 KV caches only"),
                                              (dict(kv_dtype="f32"), 16, 16, 128, "kvMul 1, 2, 4 or 8"),
                                              (dict(kv_dtype="f32"), 2, 2, 96, "head layout"),
                                              (dict(kv_dtype="f32", out="q80"), 8, 4, 128, "no Q80 output")])
def test_plan_refusals(ops, kw, H, kvm, hs, why):
    q, kv = torch.zeros(2, H * hs), torch.zeros(1, 64, H // kvm * hs)
    with pytest.raises(RuntimeError, match=why):
        ops.attention_launch(q, kv, kv, H, kvm, hs, [3, 4], [0, 0], kernel="ragged", plan_only=True, **kw)


# ------------------------------------------------------------------------------- 3. engine
TOL = 3e-2  # test_gpu_engine.py, Q40 weights with an f32 KV cache, on its metric (max |diff| / max |ref|)
LENS, P0, N_CHUNK, N_GREEDY = (9, 17, 5), 130, 40, 8


@gpu
def test_engine_mixed_forward(C, tmp_path, monkeypatch):
    """3 decode rows + rows 130..169 of a fourth slot in one forward (segments 1 + 1 + 1 + 16 + 16 + 8): every row
    against TorchLlama and against an engine with DL_ATTN_RAGGED=0 (test_gpu_engine.py scales no kernel bound to
    logits: the oracle tolerance), then 8 greedy steps where the oracle's top-2 gap exceeds it (asserted)."""
    from distributed_llama_multiusers_amd.models.llama import TorchLlama
    from distributed_llama_multiusers_amd.models.synthetic import make_test_assets
    from distributed_llama_multiusers_amd.utils.mfile import FloatType
    m, _, spec = make_test_assets(str(tmp_path), "tiny", FloatType.Q40, seq_len=256, seed=3, n_layers=2, vocab_size=2048, **MODELS[128])
    rng = np.random.default_rng(48)  # top-2 gaps of the 9 greedy rows: 3.9e-2 at the least
    prompts = [rng.integers(0, spec.vocab_size, n + 1).tolist() for n in LENS] + [rng.integers(0, spec.vocab_size, P0 + N_CHUNK).tolist()]
    oracle, kvs = TorchLlama(m), [{}, {}, {}, {}]
    for s, n in enumerate(LENS):
        oracle.forward(prompts[s][:n], 0, kvs[s])
    oracle.forward(prompts[3][:P0], 0, kvs[3])
    want = [oracle.forward([prompts[s][n]], n, kvs[s])[0] for s, n in enumerate(LENS)]
    want = torch.stack(want + list(oracle.forward(prompts[3][P0:], P0, kvs[3]))).numpy()
    chain, row = [], want[-1]
    for i in range(N_GREEDY + 1):
        top = np.sort(row)[-2:]
        assert top[1] - top[0] > TOL * np.abs(row).max(), (i, top)
        chain.append(int(row.argmax()))
        if i < N_GREEDY:
            row = oracle.forward([chain[-1]], P0 + N_CHUNK + i, kvs[3])[0].numpy()
    toks = [prompts[s][n] for s, n in enumerate(LENS)] + prompts[3][P0:]
    pos = list(LENS) + list(range(P0, P0 + N_CHUNK))
    slots = [0, 1, 2] + [3] * N_CHUNK
    got = {}
    for sw in ("1", "0"):
        monkeypatch.setenv("DL_ATTN_RAGGED", sw)
        eng = C.HipEngine(m, "q80", kv_dtype="f32", max_batch=64, n_slots=4)
        for s, n in enumerate(LENS):
            eng.forward(prompts[s][:n], list(range(n)), [s] * n)
        for c0 in range(0, P0, 64):
            c1 = min(P0, c0 + 64)
            eng.forward(prompts[3][c0:c1], list(range(c0, c1)), [3] * (c1 - c0))
        got[sw] = eng.forward(toks, pos, slots)
        assert np.array_equal(eng.forward(toks, pos, slots), got[sw]) and np.array_equal(eng.forward(toks, pos, slots), got[sw])
        if sw == "1":
            assert int(got[sw][-1].argmax()) == chain[0]
            for i in range(N_GREEDY):
                assert int(eng.forward([chain[i]], [P0 + N_CHUNK + i], [3])[0].argmax()) == chain[i + 1], i
    dev = lambda a, b: float(np.abs(a - b).max() / np.abs(b).max())  # noqa: E731
    print(f"ragged vs oracle {dev(got['1'], want):.3e}, ragged vs DL_ATTN_RAGGED=0 {dev(got['1'], got['0']):.3e}")
    assert dev(got["1"], want) < TOL and dev(got["0"], want) < TOL and dev(got["1"], got["0"]) < TOL
