"""The decode GEMVs per launch geometry: ring schedule, lanes per row, passes, row tails, prologue
paths and epilogues of the Q40 register-ring GEMV (csrc/hip/gemv_dev.h gemvQ40Body), the F32-weight
GEMV (gemv_inst.h gemvKernel), the host tiling, and the engine's default geometries pinned.

The single-kernel ops take `lanes` (L) and `passes` so a test reaches the launches a real model makes
(L = 16, K = ceil(n / 32 / L) of 8..100 ring steps per row pair, several passes, partial last
workgroups) at a few dozen rows. Notation: RP = 512 / L rows per pass, R = RP * passes rows per
workgroup, T = passes * K ring steps per workgroup, ring depth 4.

References are plain torch in float64 on the kernel's own operands (Q40 weights dequantized,
activations through the reference Q80 quantizer). Bounds are the project's: rel < 2e-4 for the Q40
GEMV against same-operand references (test_gpu_ops.py), 8e-3 for bf16 cache rows, 1e-5 for the
f32-only GEMV (test_gemm_f32_mfma, test_attention_prefill_f32). The ops guard every output buffer:
a store past the last valid row raises instead of passing.

Tests that need the device are marked `gpu` one by one; the tiling, the pinned defaults, the sweep
coverage and the refused launches run on the CPU.
"""
import functools

import numpy as np
import pytest
import torch

import kernel_checks

gpu = pytest.mark.gpu


@pytest.fixture(scope="module")
def ops():
    from distributed_llama_multiusers_amd import ops as o
    return o


def _ops():
    from distributed_llama_multiusers_amd import ops as o
    return o


def rel(a, b):
    return float((a.double() - b.double()).norm() / b.double().norm().clamp_min(1e-30))


def cdiv(a, b):
    return (a + b - 1) // b


# ------------------------------------------------------------------------------------ operands
@functools.lru_cache(maxsize=6)
def q40_weights(rows, n, seed=1):
    """(file-layout Q40 blocks, the same weights dequantized, float64)."""
    o = _ops()
    g = torch.Generator().manual_seed(seed)
    w = torch.randn(rows, n, generator=g) / n ** 0.5
    blocks = o.quantize_q40(w)
    return blocks, o.dequantize_q40(blocks, rows, n).double()


@functools.lru_cache(maxsize=6)
def f32_weights(rows, n, seed=3):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(rows, n, generator=g) / n ** 0.5


@functools.lru_cache(maxsize=16)
def activations(B, n, seed=2):
    """(x, residual, norm weights)."""
    g = torch.Generator().manual_seed(seed)
    return torch.randn(B, n, generator=g), torch.randn(B, n, generator=g), torch.rand(n, generator=g) + 0.5


def staged_q80(o, x, r, nw):
    """The Q80 image the norm prologue stages: (x + r) -> RMS norm -> reference Q80 round trip."""
    xs = x + r if r is not None else x
    return o.dequantize_q80(o.ref_rmsnorm(xs, nw)).double()


def check_rows(out, want, tol):
    """rel < tol, and every element within tol * max|want|: one wrong row cannot hide in the norm."""
    assert out.shape == want.shape
    err = (out.double() - want).abs()
    r = rel(out, want)
    worst = float(err.max() / want.abs().max())
    print(f"rel {r:.3e} worst row {worst:.3e}")
    assert r < tol, r
    assert worst <= tol, (worst, int(err.argmax()))  # NaN (a row never written) fails both


# ------------------------------------------------------------------------------------ geometry
def n_for(L, K):
    """Input width with K ring steps per row pair at L lanes and n / 32 no multiple of L."""
    return 32 * ((K - 1) * L + L // 2)


def rows_past(L, passes, odd=True):
    """Two workgroups; of the second only half of the first pass (+ 1 row) is live, so with
    passes > 1 its later passes lie wholly past `rows`. Odd: RP / 2 is even for every L."""
    RP = 512 // L
    return RP * passes + RP // 2 + (1 if odd else 0)


def rows_partial(L, passes, odd=True):
    """Two workgroups; the last pass of the second is half live."""
    RP = 512 // L
    return 2 * RP * passes - RP // 2 - (1 if odd else 0)


LANES = (16, 32, 64)

# a. ring schedule: (L, K, passes, rows rule, B). T = passes * K covers 1..10, 12, 14, 15, 18, 21, 27:
# fewer than one round (T < 4), exactly one (4), full rounds with remainders 1, 2, 3 and 0 (5, 6, 7, 8),
# and with K = 1, 2, 3, 5, 7 against ring depth 4 a row-pair boundary at every slot position.
RING_K = (1, 2, 3, 4, 5, 7, 9)
RING_CASES = [(L, K, p, "past", 1) for L in LANES for K in RING_K for p in (1, 2, 3)]
RING_CASES += [(L, K, p, "partial", 1) for L in LANES for K in RING_K for p in (2, 3)]
RING_CASES += [(L, K, p, "past", B) for L in LANES for K in (3, 5) for p in (1, 2) for B in (2, 4)]

# b. prologue paths at B = 1, at the op's default geometry ...
RESNORM_N = (1280, 2304, 4352, 8192, 8448)   # PK 1 clamped, PK 2, PK 4 last sweep clamped, PK 4 edge, late
Q80_N = (4352, 8448, 16384, 16416)           # PK 2, PK 4, PK 4 edge, late
# ... and (kind, n, L, passes): the widths, lanes and single / several passes of the model matrices
# of DEFAULTS below, one case per (L, K mod 4, passes > 1, prologue path) class, at a few dozen rows
MODEL_WIDTH_CASES = [
    ("res", 4096, 16, 1), ("res", 4096, 16, 2), ("res", 4096, 64, 1), ("res", 4096, 32, 2),
    ("res", 8192, 16, 1), ("res", 8192, 16, 2), ("res", 8192, 64, 1),
    ("res", 16384, 16, 1), ("res", 16384, 16, 2), ("res", 16384, 64, 1),
    ("q80", 512, 32, 1), ("q80", 1792, 32, 1), ("q80", 4096, 32, 1), ("q80", 14336, 32, 1),
    ("q80", 1024, 16, 1), ("q80", 2048, 16, 1), ("q80", 3584, 16, 1), ("q80", 6656, 16, 1),
    ("q80", 8192, 16, 1), ("q80", 16384, 16, 1), ("q80", 28672, 16, 1), ("q80", 53248, 16, 1),
]

# c. epilogues: (L, passes); SwiGLU -> Q80 needs whole 64-row blocks per workgroup
EPI_CASES = [(L, p) for L in LANES for p in (1, 2, 3)]
Q80_EPI_CASES = [(16, 2), (16, 4), (32, 4), (32, 8), (64, 8), (64, 16)]
EPI_K = 3


def prologue_path(kind, n):
    """The prologue instance gemvQ40Body takes at B = 1 (gemv_dev.h: unitsPerThread)."""
    units = cdiv(n, 2048 if kind == "res" else 4096)
    return (kind, "early1" if units <= 1 else "early2" if units <= 2 else "early4" if units <= 4 else "late")


def geometry_class(kind, n, L, passes):
    return (L, cdiv(n // 32, L) % 4, passes > 1, prologue_path(kind, n))


def swept_classes():
    """Classes of the B = 1 launches of sweeps a to c (default-geometry cases excluded: their L
    follows the heuristic under test)."""
    s = set()
    for L, K, p, _, B in RING_CASES:
        if B == 1:
            s.add(geometry_class("res", n_for(L, K), L, p))
    for kind, n, L, p in MODEL_WIDTH_CASES:
        s.add(geometry_class(kind, n, L, p))
    for L, p in EPI_CASES + Q80_EPI_CASES:
        s.add(geometry_class("res", n_for(L, EPI_K), L, p))
    return s


# ----------------------------------------------------------------------- a. ring schedule sweep
@gpu
@pytest.mark.parametrize("L,K,passes,tail,B", RING_CASES)
def test_ring_schedule(ops, L, K, passes, tail, B):
    """PRO_RESNORM + EPI_STORE over the ring's schedules: the full-round loop and its vmcnt wait
    (T > 4), the last round with 1..4 live slots, row-pair boundaries inside a round (passes > 1),
    the cLast clamp (later passes past the last row), the odd-row guard and a partial workgroup."""
    n = n_for(L, K)
    assert (n // 32) % L != 0 and cdiv(n // 32, L) == K
    rows = (rows_past if tail == "past" else rows_partial)(L, passes)
    R = 512 // L * passes
    assert rows % 2 == 1 and rows % R != 0 and rows > R
    blocks, wd = q40_weights(rows, n)
    x, r, nw = activations(B, n)
    out, xn = ops.gemv_q40(blocks, rows, n, x, r, nw, lanes=L, passes=passes)  # raises if a guard changed
    assert torch.equal(xn, x + r)
    check_rows(out, staged_q80(ops, x, r, nw) @ wd.T, 2e-4)


# ------------------------------------------------------------------------ b. prologue paths, B = 1
@gpu
@pytest.mark.parametrize("norm", [True, False])
@pytest.mark.parametrize("residual", [True, False])
@pytest.mark.parametrize("n", RESNORM_N)
def test_resnorm_prologue_paths(ops, n, residual, norm):
    """The early prologue's three instances (PK 1, 2, 4) with their clamped loads where n does not
    fill the last 256-thread sweep, and the late path beyond n = 8192; with and without the residual
    (xNext) and the norm weights."""
    rows = 97
    blocks, wd = q40_weights(rows, n)
    x, r, nw = activations(1, n)
    r, nw = (r if residual else None), (nw if norm else None)
    out, xn = ops.gemv_q40(blocks, rows, n, x, r, nw)
    if residual:
        assert torch.equal(xn, x + r)
    else:
        assert xn is None
    check_rows(out, staged_q80(ops, x, r, nw) @ wd.T, 2e-4)


@gpu
@pytest.mark.parametrize("n", Q80_N)
def test_q80_input_prologue_paths(ops, n):
    """The Q80 copy prologue at PK 2, PK 4, its edge and the late path (B = 1)."""
    rows = 97
    blocks, wd = q40_weights(rows, n)
    x = activations(1, n)[0]
    out = ops.gemv_q40_q80_in(blocks, rows, n, x)
    check_rows(out, ops.dequantize_q80(x).double() @ wd.T, 2e-4)


@gpu
@pytest.mark.parametrize("kind,n,L,passes", MODEL_WIDTH_CASES)
def test_model_width_geometries(ops, kind, n, L, passes):
    """The input widths of the 8B / 70B / 405B matrices (TP1 and TP8 shards) at the lanes per row
    the engine tiles them with, one pass or several: K up to 104 ring steps per row pair."""
    rows = rows_past(L, passes)
    blocks, wd = q40_weights(rows, n)
    x, r, nw = activations(1, n)
    if kind == "res":
        out, xn = ops.gemv_q40(blocks, rows, n, x, r, nw, lanes=L, passes=passes)
        assert torch.equal(xn, x + r)
        want = staged_q80(ops, x, r, nw) @ wd.T
    else:
        out = ops.gemv_q40_q80_in(blocks, rows, n, x, lanes=L, passes=passes)
        want = ops.dequantize_q80(x).double() @ wd.T
    check_rows(out, want, 2e-4)


# ----------------------------------------------------------------------------------- c. epilogues
def swiglu64(y):
    return torch.nn.functional.silu(y[..., 0::2]) * y[..., 1::2]


@gpu
@pytest.mark.parametrize("B", [1, 2])
@pytest.mark.parametrize("L,passes", EPI_CASES)
def test_swiglu_epilogue(ops, L, passes, B):
    n = n_for(L, EPI_K)
    rows = rows_past(L, passes, odd=False)  # interleaved (w1, w3) pairs: even, last workgroup partial
    blocks, wd = q40_weights(rows, n)
    x, _, nw = activations(B, n)
    out, _ = ops.gemv_q40(blocks, rows, n, x, None, nw, swiglu=True, lanes=L, passes=passes)
    check_rows(out, swiglu64(staged_q80(ops, x, None, nw) @ wd.T), 2e-4)


@functools.lru_cache(maxsize=1)
def llama31_rope(seq, hs):
    import distributed_llama_multiusers_amd as dl
    return torch.from_numpy(dl.native().cpu_ops.rope_table(dict(
        dim=32 * hs, hidden_dim=1, n_layers=1, n_heads=32, n_kv_heads=8, vocab_size=32, seq_len=seq,
        rope_theta=500000.0, rope_scaling_factor=8.0, rope_scaling_low_freq_factor=1.0,
        rope_scaling_high_freq_factor=4.0, rope_scaling_orig_max_seq_len=8192, rope_type=2)))


def rope64(x, rope, pos, hs):
    """Adjacent pairs (i, i + 1) of every head rotated by the table row at `pos`, in float64."""
    v = x.double().reshape(-1, hs // 2, 2)
    c, s = rope[pos, :, 0].double(), rope[pos, :, 1].double()
    return torch.stack([v[..., 0] * c - v[..., 1] * s, v[..., 0] * s + v[..., 1] * c], dim=-1).reshape(x.shape)


@gpu
@pytest.mark.parametrize("kv_bf16", [True, False])
@pytest.mark.parametrize("hs", [64, 128])
@pytest.mark.parametrize("L,passes,pos", [(L, p, pos) for L in LANES for p, pos in ((1, [37]), (3, [37]), (2, [5, 63]))])
def test_qkv_rope_epilogue(ops, L, passes, pos, hs, kv_bf16):
    """RoPE + KV append across L and passes, one row (early prologue) and two (late): workgroup
    boundaries fall inside the K and the V rows, the last workgroup is partial where R allows. The
    op presets both caches to a pattern: any element changed besides the appended rows raises."""
    n, seq = n_for(L, EPI_K), 64
    q0, kv0 = 2 * hs, 3 * hs
    rows, R = q0 + 2 * kv0, 512 // L * passes
    inside = lambda lo, hi: any(lo < k * R < hi for k in range(1, rows // R + 1))
    assert inside(q0, q0 + kv0) and inside(q0 + kv0, rows)
    assert passes != 3 or rows % R != 0
    blocks, wd = q40_weights(rows, n)
    B = len(pos)
    x, _, nw = activations(B, n)
    rope = llama31_rope(seq, hs)
    q, k, v = ops.qkv_rope(blocks, q0, kv0, hs, n, x, nw, 1e-5, rope, seq, pos, kv_bf16, lanes=L, passes=passes)
    y = staged_q80(ops, x, None, nw) @ wd.T
    tol = 8e-3 if kv_bf16 else 2e-4  # bf16 cache rows
    for b, p in enumerate(pos):
        check_rows(q[b], rope64(y[b, :q0], rope, p, hs), 2e-4)
        check_rows(k[b], rope64(y[b, q0:q0 + kv0], rope, p, hs), tol)
        check_rows(v[b], y[b, q0 + kv0:], tol)


def swiglu_q80_case(L, passes, B):
    """Operands and the float64 SwiGLU row h of a SwiGLU -> Q80 case (shared with the CPU check of
    the bound)."""
    o = _ops()
    n, R = n_for(L, EPI_K), 512 // L * passes
    rows = R + 64 if R > 64 else 2 * R  # whole 64-row blocks; R > 64: the last workgroup is partial
    blocks, wd = q40_weights(rows, n)
    x, r, nw = activations(B, n)
    return n, rows, blocks, x, r, nw, swiglu64(staged_q80(o, x, r, nw) @ wd.T)


def check_q80_row(codes, d, sums, h, what):
    """The hand-off's contract (kernel_checks.check_q80_row, shared with the attention suite) with the
    GEMV's own bound of 2e-4 * max|h|."""
    kernel_checks.check_q80_row(codes, d, sums, h, what, kernel_bound=2e-4)


def test_host_q80_meets_handoff_bound(C):
    """CPU: the host Q80 quantizer alone, fed the float64 SwiGLU rows of every SwiGLU -> Q80 case,
    meets the bound those cases assert of the kernel (so the bound asks nothing the format cannot
    give)."""
    for L, passes in Q80_EPI_CASES:
        for B in (1, 2):
            h = swiglu_q80_case(L, passes, B)[-1]
            raw = np.asarray(C.quantize_q80(h.float().numpy().reshape(-1))).reshape(-1, 34)  # f16 d + 32 int8
            d = torch.from_numpy(raw[:, :2].copy().view(np.float16).astype(np.float64)).reshape(h.shape[0], -1)
            codes = torch.from_numpy(raw[:, 2:].copy().view(np.int8).astype(np.int64)).reshape(h.shape)
            check_q80_row(codes, d, codes.reshape(h.shape[0], -1, 32).sum(-1), h, f"host L{L} p{passes} B{B}")


@gpu
@pytest.mark.parametrize("B", [1, 2])
@pytest.mark.parametrize("L,passes", Q80_EPI_CASES)
def test_swiglu_q80_epilogue(ops, L, passes, B):
    """EPI_ACT_Q80, the w13 hand-off of every default decode step."""
    n, rows, blocks, x, r, nw, h = swiglu_q80_case(L, passes, B)
    codes, scales = ops.gemv_q40(blocks, rows, n, x, r, nw, epilogue="swiglu_q80", lanes=L, passes=passes)
    assert codes.shape == (B, rows // 2) and scales.shape == (B, rows // 64, 2)
    check_q80_row(codes, scales[..., 0], scales[..., 1], h, f"L{L} p{passes} B{B}")


# -------------------------------------------------------------------------------- d. fused argmax
def lowest_argmax(row):
    return int((row == row.max()).nonzero()[0])


@gpu
@pytest.mark.parametrize("vocab_start", [0, 1000])
@pytest.mark.parametrize("rows,L,passes", [(1000, 0, 0), (1000, 16, 3), (1000, 64, 1), (4099, 16, 1), (4099, 32, 2),
                                           (4099, 0, 0)])
def test_fused_argmax(ops, rows, L, passes, vocab_start):
    """EPI_ARGMAX against the argmax of the EPI_STORE logits of the same geometry, a planted
    three-way tie across workgroups (the lowest row wins), and a second launch on the same scratch
    (the arrival counter resets itself; the op checks it is back to zero)."""
    n = 1280
    blocks, _ = q40_weights(rows, n)
    x, r, nw = activations(1, n)
    geom = dict(lanes=L, passes=passes)
    logits, _ = ops.gemv_q40(blocks, rows, n, x, r, nw, **geom)
    want = lowest_argmax(logits[0])
    assert ops.gemv_q40_argmax(blocks, rows, n, x, r, nw, vocab_start=vocab_start, **geom) == vocab_start + want
    assert ops.gemv_q40_argmax(blocks, rows, n, x, r, nw, vocab_start=vocab_start, repeat=2, **geom) == vocab_start + want
    # the winner's weight row copied to a lower and two higher rows of other workgroups
    rb = np.array(blocks, copy=True).reshape(rows, -1)
    spots = [i for i in (5, rows // 2 + 1, rows - 2) if i != want]
    for i in spots:
        rb[i] = rb[want]
    tied = rb.reshape(-1)
    logits2, _ = ops.gemv_q40(tied, rows, n, x, r, nw, **geom)
    top = logits2[0].max()
    assert all(logits2[0, i] == top for i in spots + [want])  # a real tie, bitwise
    low = min(spots + [want])
    assert lowest_argmax(logits2[0]) == low
    assert ops.gemv_q40_argmax(tied, rows, n, x, r, nw, vocab_start=vocab_start, repeat=2, **geom) == vocab_start + low


# ----------------------------------------------------------------------------------- e. F32 GEMV
# (prologue, norm weights, residual, SwiGLU). PRO_GLOBAL + EPI_ACT is no engine launch (the F32 w13
# GEMV always normalizes) and has no kernel instance: the op refuses it (test_impossible_launches_refused).
F32_VARIANTS = [("resnorm", True, True, False), ("resnorm", True, False, True), ("resnorm", False, False, True),
                ("resnorm", False, True, False), ("global", False, False, False)]


@gpu
@pytest.mark.parametrize("prologue,norm,residual,act", F32_VARIANTS)
@pytest.mark.parametrize("n", [1024, 2560, 8448])
@pytest.mark.parametrize("L", LANES)
@pytest.mark.parametrize("B", [1, 2, 4])
def test_gemv_f32(ops, B, L, n, prologue, norm, residual, act):
    """gemvKernel (F32 weights): f32 reassociation only. One row per lane group (256 / L rows per
    pass); passes 1, 3 and 2 go with B = 1, 2 and 4; the last workgroup is partial."""
    passes = {1: 1, 2: 3, 4: 2}[B]
    RP = 256 // L
    rows = RP * passes + RP // 2 + (0 if act else 1)
    assert rows % (RP * passes) != 0 and rows % 2 == (0 if act else 1)
    w = f32_weights(rows, n)
    x, r, nw = activations(B, n)
    r, nw = (r if residual else None), (nw if norm else None)
    out, xn = ops.gemv_f32(w, x, r, nw, prologue=prologue, swiglu=act, lanes=L, passes=passes)
    if residual:
        assert torch.equal(xn, x + r)
    xs = (x + r if residual else x).double()
    if norm:
        xs = nw.double() * (xs * torch.rsqrt(xs.pow(2).mean(-1, keepdim=True) + 1e-5))
    y = xs @ w.double().T
    check_rows(out, (swiglu64(y) if act else y).float().double(), 1e-5)


# ---------------------------------------------------------------- f. the default geometries, pinned
# (model, TP ranks, matrix, rows, n, epilogue, lanes per row, passes) as gemvLanesPerRow /
# gemvDefaultPasses choose them for one decode row. A change of either heuristic changes this
# table, and a new (L, K mod 4, passes > 1, prologue path) class has to be added to the sweeps.
DEFAULTS = [
    ("8b", 1, "qkv", 6144, 4096, "qkv", 16, 1),
    ("8b", 1, "wo", 4096, 4096, "store", 32, 1),
    ("8b", 1, "w13", 28672, 4096, "swiglu_q80", 16, 2),
    ("8b", 1, "w2", 4096, 14336, "store", 32, 1),
    ("8b", 1, "logits", 128256, 4096, "store", 16, 8),
    ("8b", 8, "qkv", 768, 4096, "qkv", 64, 1),
    ("8b", 8, "wo", 4096, 512, "store", 32, 1),
    ("8b", 8, "w13", 3584, 4096, "swiglu_q80", 32, 4),
    ("8b", 8, "w2", 4096, 1792, "store", 32, 1),
    ("8b", 8, "logits", 16032, 4096, "store", 16, 1),
    ("70b", 1, "qkv", 10240, 8192, "qkv", 16, 1),
    ("70b", 1, "wo", 8192, 8192, "store", 16, 1),
    ("70b", 1, "w13", 57344, 8192, "swiglu_q80", 16, 4),
    ("70b", 1, "w2", 8192, 28672, "store", 16, 1),
    ("70b", 1, "logits", 128256, 8192, "store", 16, 8),
    ("70b", 8, "qkv", 1280, 8192, "qkv", 64, 1),
    ("70b", 8, "wo", 8192, 1024, "store", 16, 1),
    ("70b", 8, "w13", 7168, 8192, "swiglu_q80", 16, 2),
    ("70b", 8, "w2", 8192, 3584, "store", 16, 1),
    ("70b", 8, "logits", 16032, 8192, "store", 16, 1),
    ("405b", 1, "qkv", 18432, 16384, "qkv", 16, 2),
    ("405b", 1, "wo", 16384, 16384, "store", 16, 1),
    ("405b", 1, "w13", 106496, 16384, "swiglu_q80", 16, 8),
    ("405b", 1, "w2", 16384, 53248, "store", 16, 1),
    ("405b", 1, "logits", 128256, 16384, "store", 16, 8),
    ("405b", 8, "qkv", 2304, 16384, "qkv", 64, 1),
    ("405b", 8, "wo", 16384, 2048, "store", 16, 1),
    ("405b", 8, "w13", 13312, 16384, "swiglu_q80", 16, 2),
    ("405b", 8, "w2", 16384, 6656, "store", 16, 1),
    ("405b", 8, "logits", 16032, 16384, "store", 16, 1),
]
MODELS = {"8b": (4096, 14336, 32, 8), "70b": (8192, 28672, 64, 8), "405b": (16384, 53248, 128, 8)}  # dim, hidden, heads, KV heads
VOCAB = 128256


def test_default_geometries_pinned(ops):
    shapes = set()
    for name, (dim, hidden, heads, kv) in MODELS.items():
        hs = dim // heads
        for tp in (1, 8):
            shapes |= {(name, tp, "qkv", (dim + 2 * kv * hs) // tp, dim), (name, tp, "wo", dim, dim // tp),
                       (name, tp, "w13", 2 * hidden // tp, dim), (name, tp, "w2", dim, hidden // tp),
                       (name, tp, "logits", VOCAB // tp, dim)}
    assert shapes == {d[:5] for d in DEFAULTS}  # the table is the models' matrices, all of them
    for name, tp, mat, rows, n, epi, L, passes in DEFAULTS:
        assert tuple(ops.gemv_defaults(rows, n, 1, True, epi)) == (L, passes), (name, tp, mat)


def test_default_geometries_are_swept():
    """Every (L, K mod 4, passes > 1, prologue path) class a model matrix launches is one that
    sweeps a to c run against a reference."""
    swept = swept_classes()
    for name, tp, mat, rows, n, epi, L, passes in DEFAULTS:
        kind = "q80" if mat in ("wo", "w2") else "res"  # wo / w2 read Q80 activations, the rest normalize
        assert geometry_class(kind, n, L, passes) in swept, (name, tp, mat, geometry_class(kind, n, L, passes))


def test_impossible_launches_refused(ops):
    """Refused on the host, before anything touches the device."""
    rows, n = 64, 256
    blocks, _ = q40_weights(rows, n)
    x = activations(1, n)[0]
    with pytest.raises(Exception, match="lanes"):
        ops.gemv_q40(blocks, rows, n, x, lanes=8)
    with pytest.raises(Exception, match="lanes"):
        ops.gemv_q40_q80_in(blocks, rows, n, x, lanes=48)
    with pytest.raises(Exception, match="passes"):
        ops.gemv_q40(blocks, rows, n, x, passes=-1)
    with pytest.raises(Exception, match="multiple of 64"):  # L = 16, one pass: 32-row workgroups
        ops.gemv_q40(blocks, rows, n, x, epilogue="swiglu_q80", lanes=16, passes=1)
    with pytest.raises(Exception, match="multiple of 64"):  # L = 64, 3 passes: 24-row workgroups
        ops.gemv_q40(blocks, rows, n, x, epilogue="swiglu_q80", lanes=64, passes=3)
    wide = 32 * 5000  # 160000 int8 + 40000 bytes of scales: beyond the CU's 160 KB
    with pytest.raises(Exception, match="LDS"):
        ops.gemv_q40(np.zeros(2 * wide // 32 * 18, np.uint8), 2, wide, torch.zeros(1, wide), lanes=64, passes=1)
    with pytest.raises(Exception, match="no SwiGLU instance"):  # F32 GEMV: PRO_GLOBAL + EPI_ACT is never launched
        ops.gemv_f32(torch.zeros(4, 64), torch.zeros(1, 64), prologue="global", swiglu=True)
    with pytest.raises(Exception, match="LDS"):  # F32 GEMV: 4 rows of 16384 floats staged in LDS
        ops.gemv_f32(torch.zeros(4, 16384), torch.zeros(4, 16384), lanes=64, passes=1)


# --------------------------------------------------------------------------- host tiling (CPU)
def expected_tiling(blocks, rows, n, L):
    """The tiled image as the Q40Tiling comment of csrc/hip/kernels.h documents it:
    chunk c = g * K + k; nibbles at ((c * 2 + r) * 256 + tid) * 16 for tid = gi * L + li, holding
    block j = li + k * L of row 2 * (g * NG + gi) + r; scales at c * 256 + tid, low half the even
    row's f16, high half the odd row's; padding (rows past the end, j >= n / 32) zero."""
    nb, NG = n // 32, 256 // L
    K, G = cdiv(nb, L), cdiv(rows, 2 * NG)
    b = np.asarray(blocks, np.uint8).reshape(rows, nb, 18)
    qs = np.zeros((G * K, 2, 256, 16), np.uint8)
    d = np.zeros((G * K, 256), np.uint32)
    for row in range(rows):
        g, gi, r = row // (2 * NG), (row // 2) % NG, row % 2
        for j in range(nb):
            k, li = j // L, j % L
            qs[g * K + k, r, gi * L + li] = b[row, j, 2:]
            scale = int(b[row, j, 0]) | (int(b[row, j, 1]) << 8)
            d[g * K + k, gi * L + li] |= np.uint32(scale << (16 * r))
    return qs.reshape(-1), d.reshape(-1)


@pytest.mark.parametrize("L,rows,n", [
    (16, 33, 32 * 7), (16, 33, 32 * 40),   # n / 32 below L; not a multiple of L
    (32, 17, 32 * 9), (32, 49, 32 * 80),
    (64, 5, 32 * 3), (64, 13, 32 * 100),
    (64, 67, 32 * 70),                     # 9 pass groups: the writers split them over threads
    (16, 301, 32 * 24),                    # 10 pass groups at L = 16
])
def test_host_tiling_layout(ops, L, rows, n):
    """tileQ40 and tileQ40AoS: every block at its documented offset, all padding zero, and the two
    writers byte for byte the same (the binding presets the buffers to a non-zero pattern, so
    padding a writer skipped would show)."""
    assert rows % 2 == 1 and (n // 32) % L != 0
    g = torch.Generator().manual_seed(7)
    blocks = ops.quantize_q40(torch.randn(rows, n, generator=g))
    want_qs, want_d = expected_tiling(blocks, rows, n, L)
    for aos in (False, True):
        qs, d = ops.tile_q40(blocks, rows, n, L, aos=aos)
        assert qs.shape == want_qs.shape and d.shape == want_d.shape
        assert np.array_equal(qs, want_qs), aos
        assert np.array_equal(d, want_d), aos
