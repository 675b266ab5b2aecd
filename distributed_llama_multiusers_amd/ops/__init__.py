"""Kernel-level access to the gfx950 HIP kernels, plus plain PyTorch fp32 references of the same ops.

Each `*` function runs exactly one kernel of `csrc/hip/kernels.hip` the way the engine launches it
(same weight tiling, fused prologue / epilogue) through `_C.ops` (csrc/hip/ops.cpp); each `ref_*`
is the textbook fp32 definition. They exist for numerics tests (tests/test_gpu_ops.py) and for
experiments; the inference hot path never goes through Python.

Reference semantics: OP_MATMUL Q80 x Q40 (nn-cpu-ops.cpp:222-440), RMS norm
(nn-cpu-ops.cpp:105-166), RoPE over adjacent pairs (nn-cpu-ops.cpp:1090-1120), multi-head attention
with GQA (nn-cpu-ops.cpp:749-784), SiLU (nn-cpu-ops.cpp:453-491), embedding (nn-cpu-ops.cpp:880-892).
"""
from __future__ import annotations

import numpy as np
import torch

from .. import native


def _np(x, dtype=np.float32):
    if x is None:
        return None
    if isinstance(x, torch.Tensor):
        x = x.detach().cpu().numpy()
    return np.ascontiguousarray(x, dtype=dtype)


# ---------------------------------------------------------------------------------------- codecs
def quantize_q40(w: torch.Tensor) -> np.ndarray:
    """[rows, n] float -> Q40 blocks in file layout (uint8, rows * n/32 * 18 bytes)."""
    return native().quantize_q40(_np(w).reshape(-1))


def dequantize_q40(blocks: np.ndarray, rows: int, n: int) -> torch.Tensor:
    return torch.from_numpy(native().dequantize_q40(blocks).reshape(rows, n))


def dequantize_q80(x: torch.Tensor) -> torch.Tensor:
    """Round trip through the reference Q80 quantizer (what a Q80 hand-off between kernels does)."""
    C = native()
    flat = _np(x).reshape(-1)
    return torch.from_numpy(C.dequantize_q80(C.quantize_q80(flat)).reshape(x.shape))


# ------------------------------------------------------------------------------- HIP kernels
def gemv_q40(blocks, rows: int, n: int, x, residual=None, norm_w=None, eps: float = 1e-5, swiglu: bool = False,
             epilogue: str | None = None, lanes: int = 0, passes: int = 0):
    """Decode GEMV (1, 2 or 4 rows): (x + residual) -> RMS norm (norm_w) -> Q80 -> W.x.
    swiglu (or epilogue="swiglu"): rows are interleaved (w1, w3) pairs and the result is
    silu(w1.x) * (w3.x). Returns (out [B, rows or rows/2], x + residual or None).
    epilogue="swiglu_q80": the SwiGLU row quantized to Q80 as the w13 hand-off of a decode step
    stores it; returns (int8 codes [B, rows/2], (d, sum of codes) pairs [B, rows/64, 2]).
    lanes (0, 16, 32, 64) / passes (0, >= 1) force the launch geometry (0: the engine's choice);
    every output buffer is guarded, a store past its valid part raises."""
    epilogue = epilogue or ("swiglu" if swiglu else "store")
    if epilogue == "swiglu_q80":
        codes, scales = native().ops.gemv_q40_swiglu_q80(_np(blocks, np.uint8), rows, n, _np(x), _np(residual),
                                                         _np(norm_w), eps, lanes, passes)
        return torch.from_numpy(codes), torch.from_numpy(scales)
    out, xn = native().ops.gemv_q40(_np(blocks, np.uint8), rows, n, _np(x), _np(residual), _np(norm_w), eps,
                                    {"store": 0, "swiglu": 1}[epilogue], lanes, passes)
    return torch.from_numpy(out), (torch.from_numpy(xn) if xn is not None else None)


def gemv_q40_q80_in(blocks, rows: int, n: int, x, lanes: int = 0, passes: int = 0) -> torch.Tensor:
    """Decode GEMV on activations handed over as Q80 blocks (the wo / w2 path)."""
    return torch.from_numpy(native().ops.gemv_q40_q80_in(_np(blocks, np.uint8), rows, n, _np(x), lanes, passes))


def gemv_q40_argmax(blocks, rows: int, n: int, x, residual=None, norm_w=None, eps: float = 1e-5,
                    vocab_start: int = 0, lanes: int = 0, passes: int = 0, repeat: int = 1) -> int:
    """Fused greedy logits GEMV (one row): vocab_start + argmax of W.x without storing the logits,
    ties to the lowest row. repeat > 1 launches again on the same scratch; all ids must agree."""
    return native().ops.gemv_q40_argmax(_np(blocks, np.uint8), rows, n, _np(x), _np(residual), _np(norm_w), eps,
                                        vocab_start, lanes, passes, repeat)


def gemv_f32(w, x, residual=None, norm_w=None, eps: float = 1e-5, prologue: str = "resnorm", swiglu: bool = False,
             lanes: int = 0, passes: int = 0):
    """F32-weight decode GEMV (1, 2 or 4 rows), w [rows, n]. prologue "resnorm": (x + residual) ->
    RMS norm (norm_w) staged in LDS; "global": x read straight from global memory. Returns
    (out [B, rows or rows/2], x + residual or None)."""
    rows, n = w.shape
    out, xn = native().ops.gemv_f32(_np(w), rows, n, _np(x), _np(residual), _np(norm_w), eps,
                                    {"global": 0, "resnorm": 1}[prologue], 1 if swiglu else 0, lanes, passes)
    return torch.from_numpy(out), (torch.from_numpy(xn) if xn is not None else None)


def gemv_defaults(rows: int, n: int, batch: int = 1, q40: bool = True, epilogue: str = "store"):
    """(lanes per row, passes) the engine takes for a matrix of this shape (host only)."""
    epi = {"store": 0, "swiglu": 1, "qkv": 2, "swiglu_q80": 3, "argmax": 7}[epilogue]
    return native().ops.gemv_defaults(rows, n, batch, q40, epi)


def tile_q40(blocks, rows: int, n: int, lanes: int, aos: bool = False):
    """Tiled device image of file-layout Q40 blocks (host only): (uint8 nibble bytes, uint32 scale
    pairs), written by tileQ40 (aos=False) or tileQ40AoS (aos=True)."""
    return native().ops.tile_q40(_np(blocks, np.uint8), rows, n, lanes, aos)


def gemm_q40(blocks, rows: int, n: int, x, residual=None, norm_w=None, eps: float = 1e-5,
             splits: int = 0) -> torch.Tensor:
    """Batched (MFMA) matmul for 1..2048 tokens: (x + residual) -> RMS norm -> f16 -> W.x (f32
    accumulate); narrow 64-row tiles up to 64 tokens, 128 x 128 wide tiles above. `splits` > 0
    forces the K split (a divisor of n / 32)."""
    return torch.from_numpy(native().ops.gemm_q40(_np(blocks, np.uint8), rows, n, _np(x), _np(residual),
                                                  _np(norm_w), eps, splits))


def gemm_f32(w, x, norm_w=None, eps: float = 1e-5) -> torch.Tensor:
    """Batched (MFMA, v_mfma_f32_16x16x4_f32) matmul for F32 weights [rows][n], 1..256 tokens:
    x -> RMS norm -> f16 -> W.x (weights exact in f32, f32 accumulate)."""
    rows, n = w.shape
    return torch.from_numpy(native().ops.gemm_f32(_np(w), rows, n, _np(x), _np(norm_w), eps))


GEMM_INPUTS = {"norm": 0, "f16": 1, "prenorm": 2}
GEMM_EPILOGUES = {"store": 0, "qkv": 2, "swiglu_f16": 4, "res": 6}


def gemm(x, blocks=None, w=None, rows: int = 0, n: int = 0, lanes: int = 0, input: str = "norm", residual=None,
         norm_w=None, eps: float = 1e-5, ss=None, ld_ss: int = 0, epilogue: str = "store", res_in=None, res_w=None,
         q0: int = 0, kv0: int = 0, head_size: int = 0, rope=None, n_slots: int = 0, pos=(), slot=(),
         kv_bf16: bool = True, splits: int = 0, fixed: bool = False, chunk: int = 0, plan_only: bool = False) -> dict:
    """One batched GEMM of the forward schedule, launched as the engine launches it (ops::gemmBatched,
    csrc/hip/ops.h): Q40 `blocks` [rows][n/32] tiled at `lanes` (0: the GEMV's choice; 16 / 32 / 64) or
    F32 `w` [rows, n]; x [M, n].
    input "norm": (x + residual) -> RMS norm (norm_w) -> f16 by the norm kernel; "f16": x rounded to
    f16 on the host; "prenorm": x = x' * w / 32 rows and ss = [ss_tiles, ld_ss] partial sums of squares.
    epilogue "store" -> out [M, rows]; "swiglu_f16" -> out [M, rows/2] (f16 values); "res" (res_in
    [M, rows], res_w [rows], ld_ss) -> out (= resOut), res_x (f16 values), ss_out [ceil(rows/64), ld_ss];
    "qkv" (q0, kv0, head_size, rope [seq_len, hs/2, 2], pos, slot, n_slots) -> out (= q [M, q0]), k, v.
    splits 0: the launcher's choice; fixed: the batch-invariant narrow launch; chunk: tokens per launch
    (0: the engine's rule). Outputs are guarded: a store outside their valid part raises. Returns a
    dict with the outputs and "launches": [{c0, tokens, kernel, splits, grid}] ("narrow", "l16",
    "wide", "f32"). plan_only: just the launches and the refusals, no device needed."""
    if w is not None:
        rows, n = w.shape
    ss_np = _np(ss)
    rope_np = _np(rope)
    r = native().ops.gemm(_np(blocks, np.uint8), _np(w), rows, n, lanes, GEMM_INPUTS[input], _np(x), _np(residual),
                          _np(norm_w), eps, ss_np, 0 if ss_np is None else ss_np.shape[0], ld_ss,
                          GEMM_EPILOGUES[epilogue], _np(res_in), _np(res_w), q0, kv0, head_size, rope_np,
                          0 if rope_np is None else rope_np.shape[0], n_slots, [int(p) for p in pos],
                          [int(s) for s in slot], kv_bf16, splits, 1 if fixed else 0, chunk, plan_only)
    return {k: (torch.from_numpy(v) if isinstance(v, np.ndarray) else v) for k, v in r.items()}


def gemm_splits(rows: int, n: int, tokens: int, lanes: int = 0) -> int:
    """K splits the launcher takes for a launch of `tokens` on a matrix tiled at `lanes` (host only)."""
    return native().ops.gemm_splits(rows, n, tokens, lanes)


def qkv_rope(blocks, q0: int, kv0: int, head_size: int, n: int, x, norm_w, eps: float, rope, seq_len: int,
             pos, kv_bf16: bool = True, lanes: int = 0, passes: int = 0):
    """QKV GEMV with the RoPE + KV-cache-append epilogue. Returns (q rotated, k row, v row)."""
    q, k, v = native().ops.qkv_rope(_np(blocks, np.uint8), q0, kv0, head_size, n, _np(x), _np(norm_w), eps,
                                    _np(rope), seq_len, [int(p) for p in pos], kv_bf16, lanes, passes)
    return torch.from_numpy(q), torch.from_numpy(k), torch.from_numpy(v)


def attention(q, k_cache, v_cache, n_heads0: int, kv_mul: int, head_size: int, pos, slot,
              kv_bf16: bool = True, prefill: bool = False, impl: str = "auto") -> torch.Tensor:
    """Decode attention. k_cache / v_cache: [slots, seq_len, kv0]; q: [B, n_heads0 * head_size].
    prefill=True (impl "prefill"): the MFMA prefill kernel (bf16 MFMAs for a bf16 cache, f32 MFMAs
    for an f32 one; row blocks of 64 / kv_mul rows share a slot). impl "valu" / "mfma": force the VALU or the MFMA decode kernel ("auto": the
    engine's choice, MFMA for bf16 caches of >= 1024 positions)."""
    n_slots, seq_len, _ = k_cache.shape
    code = {"auto": 0, "prefill": 1, "valu": 2, "mfma": 3}["prefill" if prefill else impl]
    return torch.from_numpy(native().ops.attention(_np(q), _np(k_cache), _np(v_cache), n_slots, seq_len, n_heads0,
                                                   kv_mul, head_size, [int(p) for p in pos], [int(s) for s in slot],
                                                   kv_bf16, code))


ATTN_KERNELS = {"auto": 0, "valu": 1, "mfma": 2, "prefill": 3}
ATTN_OUTPUTS = {"f32": 0, "f16": 1, "q80": 2}


def attention_launch(q, k_cache, v_cache, n_heads0: int, kv_mul: int, head_size: int, pos, slot,
                     kv_bf16: bool = True, kernel: str = "auto", prefill: bool = False, single: bool = False,
                     split_grid: int = 0, head_group: int = 0, out: str = "f32", ldq: int = 0, ld_out: int = 0,
                     page_size: int = 0, page_of=None, poison_k=None, poison_v=None, repeat: int = 1,
                     warm_pos=None, plan_only: bool = False) -> dict:
    """One attention launch set up as the engine sets it up (ops::attentionLaunch, csrc/hip/ops.h).
    q [B, ldq or q0], k_cache / v_cache [slots, seq_len, kv0]. kernel "auto" / "valu" / "mfma" /
    "prefill"; prefill: prefill rows (row blocks share a slot). single: the engine's single-row split
    geometry; split_grid > 0 forces the grid. head_group 0 / 1 / 2 / 4 / 8. out "f32" / "f16" / "q80".
    page_size > 0: a paged cache, page_of [slots, ceil(seq_len / page_size)] pool pages (-1: not mapped:
    the poison page, which holds poison_k / poison_v [kv0] at every position). repeat: launches on
    the same scratch, which must agree bitwise and leave the counters zero; warm_pos [B]: one launch at these
    positions runs first on that scratch and output (its partials stay behind). Outputs and scratch are
    guarded: a store outside their valid part raises. Returns {"kernel", "hg", "grid", "split_grid",
    "chunk_max", "short_len", "splits": [(nSplit, ch) per decode row, or per prefill row block], "out" [B, q0] (f32, the f16
    values or the Q80 codes), "scales" [B, q0 / 32, 2] (Q80: d, sum of codes)}. plan_only: just the
    plan and the refusals, no device needed."""
    n_slots, seq_len, _ = k_cache.shape
    po = [] if page_of is None else [int(p) for p in np.asarray(page_of).reshape(-1)]
    r = native().ops.attention_launch(_np(q), _np(k_cache), _np(v_cache), n_slots, seq_len, n_heads0, kv_mul,
                                      head_size, [int(p) for p in pos], [int(s) for s in slot], kv_bf16,
                                      ATTN_KERNELS["prefill" if prefill and kernel == "auto" else kernel],
                                      1 if prefill else 0, single, split_grid, head_group, ATTN_OUTPUTS[out], ldq,
                                      ld_out, page_size, po, _np(poison_k), _np(poison_v), repeat,
                                      [] if warm_pos is None else [int(p) for p in warm_pos], plan_only)
    return {k: (torch.from_numpy(v) if isinstance(v, np.ndarray) else v) for k, v in r.items()}


def sample(logits, temperatures, topps, coins) -> list:
    """Device sampler: per row softmax(logits / T) then multinomial (top-p >= 1) or nucleus draw."""
    x = _np(logits)
    B = x.shape[0] if x.ndim == 2 else 1
    spec = np.stack([np.asarray(temperatures, np.float32), np.asarray(topps, np.float32),
                     np.asarray(coins, np.float32), np.zeros(B, np.float32)], axis=1)
    return native().ops.sample(x, B, spec)


def logprobs(logits, ids, top_logprobs, targets=None, warm=None):
    """Device log-probabilities (launchLogprobs) of [B, vocab] logits: log_softmax of the raw logits.
    ids[b] is the row's chosen token, top_logprobs[b] = -1 (no request) or k in 0..20. Returns
    (float32 [B, 21] logprobs, int32 [B, 21] token ids): slot 0 the chosen token, slots 1..k the k
    best by (logit descending, id ascending), unused slots id -1. Rows without a request are not
    written and keep the fill (0, -2). warm=(logits, ids): an earlier call of the same shape and
    requests run first on the same scratch and output buffers. targets[b] >= 0: the row scores that
    given token in slot 0 instead of ids[b] (prompt scoring); None or -1: ids[b]."""
    x = _np(logits)
    x = x.reshape(1, -1) if x.ndim == 1 else x
    req = [0 if int(k) < 0 else 1 + int(k) for k in top_logprobs]
    wl, wi = (None, None) if warm is None else (_np(warm[0]), np.asarray(warm[1], np.int32))
    tg = None if targets is None else np.asarray(targets, np.int32)
    return native().ops.logprobs(x, [int(i) for i in ids], req, wl, wi, tg)


MAX_LOGIT_BIAS = 300


def _bias_tables(bias, n_slots):
    """bias: None or one {token id: value} dict (or None) per slot -> ([S, 300] ids, [S, 300] values, [S] counts)."""
    ids = np.zeros((n_slots, MAX_LOGIT_BIAS), np.int32)
    vals = np.zeros((n_slots, MAX_LOGIT_BIAS), np.float32)
    nb = [0] * n_slots
    for s, d in enumerate(bias or []):
        items = list((d or {}).items())
        if len(items) > MAX_LOGIT_BIAS:
            raise ValueError("at most 300 logit_bias entries per slot")
        nb[s] = len(items)
        for j, (t, v) in enumerate(items):
            ids[s, j], vals[s, j] = int(t), float(v)
    return ids, vals, nb


def logit_proc(logits, temperatures, slots, active, presence, frequency, counts, bias=None, fill=float("nan")):
    """Device logit processors (launchLogitProc) of [B, vocab] logits, OpenAI's formula in separate f32
    steps: for an active row b on slot s = slots[b], x[t] = logits[b, t]; where counts[s, t] > 0,
    x[t] -= frequency[b] * float(counts[s, t]) and then x[t] -= presence[b]; where t is a key of
    bias[s], x[t] += bias[s][t]. Rows with temperatures[b] >= 0 that are not active are copied; rows
    with temperatures[b] < 0 are not written and keep `fill`. counts is uint32 [slots, vocab], bias
    None or one {token id: value} dict (or None) per slot. Returns float32 [B, vocab]."""
    x = _np(logits)
    x = x.reshape(1, -1) if x.ndim == 1 else x
    c = np.ascontiguousarray(np.asarray(counts, np.uint32))
    c = c.reshape(1, -1) if c.ndim == 1 else c
    ids, vals, nb = _bias_tables(bias, c.shape[0])
    return native().ops.logit_proc(x, [float(t) for t in temperatures], [int(s) for s in slots],
                                   [int(bool(a)) for a in active], [float(p) for p in presence],
                                   [float(f) for f in frequency], c, ids, vals, nb, float(fill))


def logit_proc_count(counts, ids, slots, active):
    """Device count update (launchLogitProcCount): counts[slots[b], ids[b]] += 1 for the active rows
    with ids[b] >= 0 (at most one active row per slot). Returns the uint32 [slots, vocab] table after."""
    c = np.ascontiguousarray(np.asarray(counts, np.uint32))
    c = c.reshape(1, -1) if c.ndim == 1 else c
    return native().ops.logit_proc_count(c, c.shape[0], [int(i) for i in ids], [int(s) for s in slots],
                                         [int(bool(a)) for a in active])


def logit_filter(logits, temperatures, top_k, delta, active, fill=None):
    """Device candidate filter (launchLogitFilter) of [B, vocab] logits. For an active row b with
    temperatures[b] > 0: thr = max(the top_k[b]-th largest value of the row (1 <= top_k[b] < vocab,
    else -inf), max of the row + delta[b] (delta = cpu_ops.min_p_delta(T, min_p); -inf: off)), and
    every element below thr (float32 comparison) becomes -inf; survivors keep their bits. The kernel
    works in place and neither reads nor writes any other row: with `fill`, those rows hold `fill`
    instead of their logits when the kernel runs, and must hold it afterwards. Returns float32
    [B, vocab], the buffer after the launch."""
    x = _np(logits)
    x = (x.reshape(1, -1) if x.ndim == 1 else x).copy()
    temps = [float(t) for t in temperatures]
    act = [int(bool(a)) for a in active]
    if fill is not None:
        for b in range(x.shape[0]):
            if not (act[b] and temps[b] > 0):
                x[b] = fill
    return native().ops.logit_filter(x, temps, [int(k) for k in top_k], [float(d) for d in delta], act)


POOL_TAKE, POOL_FIRST, POOL_LAST, POOL_MODE_LAST = 1, 2, 4, 8


def pool(launches, norm_w, eps, n_slots, out=None, acc=None):
    """Device pooling (launchPool): the L2-normalised mean (or last row) of the rows' final-norm hidden
    states, per slot. `launches` is a list of launches run in order on one per-slot state; each is a
    dict with x [B, dim] (the residual rows), add (None or [B, dim], summed to x first), slots [B] and,
    per row, take / first / last (does the row take part, is it its request's first / last row),
    count (the request's row count N, read at its last row) and mode ("mean" | "last"). For a
    taking-part row: h = norm_w * rmsnorm(x + add); mean: acc[slot] = h if first else acc[slot] + h;
    at the last row out[slot] = p / |p| with p = acc[slot] / N (mean) or h (last). Rows that do not
    take part are neither read nor written. out / acc ([n_slots, dim], default zeros) are the buffers'
    contents before the first launch. Returns float32 (out, acc) after the last one."""
    w = _np(norm_w).reshape(-1)
    dim = w.shape[0]
    ls = []
    for l in launches:
        x = _np(l["x"]).reshape(-1, dim)
        B = x.shape[0]
        flags = [(POOL_TAKE if l["take"][b] else 0) | (POOL_FIRST if l["first"][b] else 0) |
                 (POOL_LAST if l["last"][b] else 0) | (POOL_MODE_LAST if l["mode"][b] == "last" else 0) for b in range(B)]
        ls.append({"x": x, "add": None if l.get("add") is None else _np(l["add"]).reshape(-1, dim),
                   "slots": [int(s) for s in l["slots"]], "flags": flags, "counts": [int(c) for c in l["count"]]})
    o = np.zeros((n_slots, dim), np.float32) if out is None else _np(out).reshape(n_slots, dim)
    a = np.zeros((n_slots, dim), np.float32) if acc is None else _np(acc).reshape(n_slots, dim)
    return native().ops.pool(ls, dim, int(n_slots), w, float(eps), o, a)


def ref_pool(x, norm_w, eps, mode="mean", add=None) -> np.ndarray:
    """float64 reference of one request's pooled vector: x [N, dim] (+ add) -> [dim]."""
    xs = np.asarray(_np(x), np.float64)
    if add is not None:
        xs = (_np(x) + _np(add)).astype(np.float64)  # the f32 sum the kernel and the host form first
    h = np.asarray(_np(norm_w), np.float64) * (xs / np.sqrt((xs * xs).mean(-1, keepdims=True) + float(eps)))
    p = h.mean(0) if mode == "mean" else h[-1]
    ss = float((p * p).sum())
    return p / np.sqrt(ss) if ss > 0 else np.zeros_like(p)


def json_mask(logits, temperatures, on, table, states, fill=None):
    """Device JSON token mask (launchJsonMask) of [B, vocab] logits. `table` is a `JsonTable` of the
    vocabulary, states[b] row b's automaton state (4 words, as `cpu_ops.json_walk` returns). For a
    row b with on[b] and temperatures[b] >= 0 every token that is not allowed in states[b] becomes
    -inf; the others keep their bits. The kernel works in place and neither reads nor writes any
    other row: with `fill`, those rows hold `fill` instead of their logits when the kernel runs, and
    must hold it afterwards. Returns float32 [B, vocab], the buffer after the launch."""
    x = _np(logits)
    x = (x.reshape(1, -1) if x.ndim == 1 else x).copy()
    temps = [float(t) for t in temperatures]
    flags = [int(bool(a)) for a in on]
    if fill is not None:
        for b in range(x.shape[0]):
            if not (flags[b] and temps[b] >= 0):
                x[b] = fill
    return native().ops.json_mask(x, temps, flags, table, [[int(w) for w in s] for s in states])


def json_advance(temperatures, on, ids, table, states):
    """Device automaton advance (launchJsonAdvance): states[b] stepped by the bytes of token ids[b]
    for every row with on[b] and temperatures[b] >= 0; a token that is not allowed, and every other
    row, leaves the state as it is. Returns the states after the launch (lists of 4 words)."""
    return native().ops.json_advance([float(t) for t in temperatures], [int(bool(a)) for a in on],
                                     [int(i) for i in ids], table, [[int(w) for w in s] for s in states])


ROW_KINDS = {"none": 0, "json": 1, "grammar": 2}


def grammar_mask(logits, temperatures, kinds, table, grammars, states, slots=None, fill=None):
    """Device grammar token mask (launchGrammarMask) of [B, vocab] logits. `table` is the `JsonTable`
    of the vocabulary; slot s holds `grammars[s]` (a `Grammar`, or None for an empty slot) in state
    `states[s]`; row b is of kind `kinds[b]` ("none", "json" or "grammar") and sits in slot
    `slots[b]` (default: b). For a grammar row with temperatures[b] >= 0 every token that is not
    allowed in its slot's state becomes -inf; the others keep their bits. The kernel works in place
    and neither reads nor writes any other row, a JSON-mode row included: with `fill`, those rows hold
    `fill` instead of their logits when the kernel runs, and must hold it afterwards. Returns float32
    [B, vocab], the buffer after the launch."""
    x = _np(logits)
    x = (x.reshape(1, -1) if x.ndim == 1 else x).copy()
    temps = [float(t) for t in temperatures]
    codes = [ROW_KINDS[k] for k in kinds]
    slots = list(range(x.shape[0])) if slots is None else [int(s) for s in slots]
    if fill is not None:
        for b in range(x.shape[0]):
            if not (codes[b] == 2 and temps[b] >= 0):
                x[b] = fill
    return native().ops.grammar_mask(x, temps, codes, slots, table, list(grammars), [int(s) for s in states])


def grammar_advance(temperatures, kinds, ids, table, grammars, states, slots=None):
    """Device grammar advance (launchGrammarAdvance): the state of slot slots[b] stepped by token
    ids[b] for every grammar row with temperatures[b] >= 0; a token that is not allowed, an id
    outside the vocabulary and every other row leave the state as it is. Returns the slots' states."""
    slots = list(range(len(ids))) if slots is None else [int(s) for s in slots]
    return native().ops.grammar_advance([float(t) for t in temperatures], [ROW_KINDS[k] for k in kinds], slots,
                                        [int(i) for i in ids], table, list(grammars), [int(s) for s in states])


def argmax(logits) -> list:
    x = _np(logits)
    return native().ops.argmax(x, x.shape[0] if x.ndim == 2 else 1)


def embedding(table, tokens) -> torch.Tensor:
    t = _np(table)
    return torch.from_numpy(native().ops.embedding(t, t.shape[0], t.shape[1], [int(x) for x in tokens]))


# --------------------------------------------------------------------------- fp32 references
def ref_rmsnorm(x: torch.Tensor, w: torch.Tensor | None, eps: float = 1e-5) -> torch.Tensor:
    x = x.float()
    if w is None:
        return x
    return w.float() * (x * torch.rsqrt(x.pow(2).mean(-1, keepdim=True) + eps))


def ref_swiglu(y: torch.Tensor) -> torch.Tensor:
    """Interleaved (w1, w3) rows -> silu(w1 x) * (w3 x)."""
    return torch.nn.functional.silu(y[..., 0::2]) * y[..., 1::2]


def ref_rope(x: torch.Tensor, rope: torch.Tensor, pos: int, head_size: int) -> torch.Tensor:
    """Rotate adjacent pairs (i, i+1) of every head by the table row at `pos` ([seq_len, hs/2, 2])."""
    v = x.float().reshape(-1, head_size // 2, 2)
    cs = rope[pos].float()
    c, s = cs[:, 0], cs[:, 1]
    out = torch.stack([v[..., 0] * c - v[..., 1] * s, v[..., 0] * s + v[..., 1] * c], dim=-1)
    return out.reshape(x.shape)


def ref_rope_table(seq_len: int, head_size: int, theta: float = 10000.0) -> torch.Tensor:
    i = torch.arange(0, head_size, 2, dtype=torch.float64) / head_size
    freq = 1.0 / (theta ** i)
    ang = torch.arange(seq_len, dtype=torch.float64)[:, None] * freq[None, :]
    return torch.stack([torch.cos(ang), torch.sin(ang)], dim=-1).float()


def ref_attention(q: torch.Tensor, k_cache: torch.Tensor, v_cache: torch.Tensor, n_heads0: int, kv_mul: int,
                  head_size: int, pos, slot, dtype=torch.float32) -> torch.Tensor:
    out = torch.zeros(q.shape[0], n_heads0 * head_size, dtype=dtype)
    for b in range(q.shape[0]):
        for h in range(n_heads0):
            kvh = h // kv_mul
            qh = q[b, h * head_size:(h + 1) * head_size].to(dtype)
            K = k_cache[slot[b], :pos[b] + 1, kvh * head_size:(kvh + 1) * head_size].to(dtype)
            V = v_cache[slot[b], :pos[b] + 1, kvh * head_size:(kvh + 1) * head_size].to(dtype)
            p = torch.softmax(K @ qh / head_size ** 0.5, dim=0)
            out[b, h * head_size:(h + 1) * head_size] = p @ V
    return out


__all__ = [n for n in dir() if not n.startswith("_") and n not in ("annotations", "np", "torch", "native")]
