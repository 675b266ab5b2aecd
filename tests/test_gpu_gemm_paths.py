"""The batched GEMMs per kernel, tiling, tile edge, input mode and fused epilogue: gemmQ40Kernel
("narrow": 64-row tiles, 16..128-token tiles), gemmQ40L16Kernel ("l16": 16-lane tilings at <= 16
tokens), gemmWideKernel ("wide": 128 x 128 tiles from 65 tokens) and gemmF32Kernel ("f32"), through
`ops.gemm`, which launches them as the engine's gemmBatched does and reports the kernel of every launch
by the launcher's own predicates (csrc/hip/ops.h gemmBatched).

The (epilogue, input mode) pairs gemmBatched launches (engine_forward.cpp enqueueQkv .. enqueueLogits),
each on all four kernels; test_every_launchable_triple runs every one and asserts the reported kernel:

    epilogue      input     launch of the forward
    qkv           norm      qkv behind a norm kernel (first layer, or no fused norm)
    qkv           prenorm   qkv after a fused-norm w2
    res           f16       wo, w2 with the fused residual + norm
    store         f16       wo, w2 without it
    swiglu_f16    norm      w13 behind a norm kernel
    swiglu_f16    prenorm   w13 after a fused-norm wo
    store         norm      logits behind a norm kernel
    store         prenorm   logits after a fused-norm w2

The sweep is NOT complete over the compiled instances: EPI_ACT and EPI_ACT_Q80 exist for every GEMM
kernel, but the engine launches neither on a GEMM (they are GEMV hand-offs), and the tensor-parallel
tile exchange (GemmArgs::tpx) needs peers; none of them is run here.

References are float64 torch on the operands the kernel sees (Q40 weights dequantized, activations
rounded to f16 where the kernel rounds them). Bounds, norm-relative per token row against that
reference: 5e-4 for Q40 weights (test_gemm_q40_mfma), 1e-5 for F32 weights (test_gemm_f32_mfma); f16
outputs and bf16 cache rows add one rounding of that type (2^-11, 2^-8). Where the error of the
accumulation is amplified (SwiGLU, the producer -> consumer chain) the bound is 4 x the error of the
reference path itself: the same operation in f32 torch with the kernel's roundings against float64
(ref_path_error; measured on the CPU at the shapes below, largest token row: SwiGLU 4.0e-4 .. 6.1e-4 for Q40 and
2.2e-4 .. 3.2e-4 for F32 weights, the chain 3.4e-4 .. 3.5e-4). Never from the kernel's output.

The op guards every output (after each token row, after the last token, ssOut past column M, the
caches outside the appended rows): a store out of bounds raises instead of passing.

A model whose w2 input width (hidden_dim per rank) is no multiple of 64 used to reach
launchGemmWide's `bad K split` in the middle of a forward of >= 65 tokens: batchedPath asks only for
multiples of 32, dim and q0 are multiples of the head size (64 / 128) but hidden_dim is free. Such a
width now stays on narrow launches (kernels.h gemmChunkTokens); test_engine_hidden_not_multiple_of_64
runs the smallest such model.
"""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

gpu = pytest.mark.gpu

EPS = 1e-5
F16_EPS = 2.0 ** -11
BF16_EPS = 2.0 ** -8


def _ops():
    from distributed_llama_multiusers_amd import ops as o
    return o


def cdiv(a, b):
    return (a + b - 1) // b


def rel_rows(a, b):
    """Largest norm-relative error of a token row: one wrong token cannot hide among the others."""
    a, b = a.double(), b.double()
    return float(((a - b).norm(dim=-1) / b.norm(dim=-1).clamp_min(1e-30)).max())


def rel_all(a, b):
    return float((a.double() - b.double()).norm() / b.double().norm().clamp_min(1e-30))


def check(name, got, want, tol, whole=False):
    """whole: the norm over all tokens, as test_gemm_q40_mfma / test_gemm_f32_mfma take it. For rows that
    went through the norm kernel only: its f32 sum of squares is ordered differently from torch's, so a
    few of a row's f16 roundings may fall the other way (one flip in a row of 1056 is 1.5e-5 of that
    row's output, above the F32 bound of 1e-5 per row, while over all tokens it is far below it)."""
    assert got.shape == want.shape, (name, got.shape, want.shape)
    assert bool(torch.isfinite(got).all()), f"{name}: unwritten or non-finite elements"
    r = rel_all(got, want) if whole else rel_rows(got, want)
    print(f"{name}: rel {r:.3e} (bound {tol:.3e})")
    assert r < tol, (name, r, tol)
    return r


# ------------------------------------------------------------------------------------ operands
@functools.lru_cache(maxsize=8)
def q40_weights(rows, n, seed=1):
    """(file-layout Q40 blocks, the same weights dequantized, float64)."""
    o = _ops()
    g = torch.Generator().manual_seed(seed)
    w = torch.randn(rows, n, generator=g) / n ** 0.5
    blocks = o.quantize_q40(w)
    return blocks, o.dequantize_q40(blocks, rows, n).double()


@functools.lru_cache(maxsize=8)
def f32_weights(rows, n, seed=3):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(rows, n, generator=g) / n ** 0.5


@functools.lru_cache(maxsize=4)
def rope_table(seq, hs):
    """The engines' Llama-3.1-scaled table, as test_qkv_rope_kv_append."""
    import distributed_llama_multiusers_amd as dl
    return torch.from_numpy(dl.native().cpu_ops.rope_table(dict(
        dim=32 * hs, hidden_dim=1, n_layers=1, n_heads=32, n_kv_heads=8, vocab_size=32, seq_len=seq,
        rope_theta=500000.0, rope_scaling_factor=8.0, rope_scaling_low_freq_factor=1.0,
        rope_scaling_high_freq_factor=4.0, rope_scaling_orig_max_seq_len=8192, rope_type=2)))


def silu64(y):
    return y / (1.0 + torch.exp(-y))


def rope64(y, rope, pos, hs):
    """ops.ref_rope in float64: adjacent pairs of every head rotated by the table row at pos."""
    v = y.double().reshape(-1, hs // 2, 2)
    c, s = rope[pos].double()[:, 0], rope[pos].double()[:, 1]
    return torch.stack([v[..., 0] * c - v[..., 1] * s, v[..., 0] * s + v[..., 1] * c], dim=-1).reshape(y.shape)


def prenorm_operands(xp, nw, ld_ss):
    """The EPI_RES producer's outputs for residual rows xp: f16(x' w / 32) rows and the per-64-column
    partial sums of squares as [tiles][ld_ss] (columns past M: NaN, never read)."""
    M, n = xp.shape
    rows16 = (xp * nw / 32).half()
    tiles = cdiv(n, 64)
    ss = torch.full((tiles, ld_ss), float("nan"))
    for j in range(tiles):
        ss[j, :M] = xp[:, 64 * j:64 * j + 64].double().pow(2).sum(-1).float()
    return rows16, ss


def prenorm_input64(rows16, ss, M, n):
    """What the consumer multiplies: rows * 32 / sqrt(sum(ss) / n + eps), float64."""
    return rows16.double() * 32 / torch.sqrt(ss[:, :M].double().sum(0) / n + EPS)[:, None]


class Case:
    """Operands, the op's result and the float64 references of one ops.gemm call."""

    def __init__(self, kind, L, M, rows, n, inp, epi, seed=5, hs=64, kv_bf16=True, token_scale=False, splits=0,
                 fixed=False, x=None, nw=None, **extra):
        o = _ops()
        self.kind, self.M, self.rows, self.n, self.inp, self.epi = kind, M, rows, n, inp, epi
        self.hs, self.kv_bf16 = hs, kv_bf16
        g = torch.Generator().manual_seed(seed + 31 * M)
        kw = dict(input=inp, epilogue=epi, splits=splits, fixed=fixed, eps=EPS, **extra)
        if kind == "f32":
            w = f32_weights(rows, n)
            self.wd, self.w16 = w.double(), w
            kw["w"] = w
        else:
            blocks, self.wd = q40_weights(rows, n)
            self.w16 = self.wd.half().float()  # the kernel dequantizes (q - 8) * d to f16
            kw.update(blocks=blocks, rows=rows, n=n, lanes=L)
        x = torch.randn(M, n, generator=g) if x is None else x
        if token_scale:  # every token its own RMS: a scale applied to the wrong token is off by a factor
            x = x * (1 + torch.arange(M, dtype=torch.float32))[:, None]
        if inp == "norm":
            r, nw = torch.randn(M, n, generator=g), torch.rand(n, generator=g) + 0.5
            kw.update(residual=r, norm_w=nw)
            self.xk = o.ref_rmsnorm(x + r, nw, EPS).half().double()
            xin = x
        elif inp == "f16":
            self.xk, xin = x.half().double(), x
        else:
            nw = torch.rand(n, generator=g) + 0.5 if nw is None else nw
            ld_ss = M + 5
            rows16, ss = prenorm_operands(x, nw, ld_ss)
            kw.update(ss=ss, ld_ss=ld_ss)
            self.xk, xin = prenorm_input64(rows16, ss, M, n), rows16.float()
        self.y = self.xk @ self.wd.T  # float64 [M, rows]
        if epi == "res":
            self.res_in, self.res_w = torch.randn(M, rows, generator=g), torch.rand(rows, generator=g) + 0.5
            self.ld_ss = kw.setdefault("ld_ss", M + 3)
            kw.update(res_in=self.res_in, res_w=self.res_w)
        if epi == "qkv":
            self.seq, self.kv0 = 128, hs
            self.q0 = rows - 2 * hs
            self.rope = rope_table(self.seq, hs)
            # non-monotonic positions, two slots in use, no (slot, position) twice
            perm = torch.randperm(2 * self.seq, generator=g)[:M]
            self.pos, self.slot = [int(p) % self.seq for p in perm], [int(p) // self.seq for p in perm]
            kw.update(q0=self.q0, kv0=self.kv0, head_size=hs, rope=self.rope, n_slots=2, pos=self.pos,
                      slot=self.slot, kv_bf16=kv_bf16)
        self.kw, self.xin = kw, xin
        self.res = None

    def run(self):
        self.res = _ops().gemm(self.xin, **self.kw)
        return self.res

    def kernels(self):
        return [l["kernel"] for l in self.res["launches"]]

    def base_tol(self):
        return 1e-5 if self.kind == "f32" else 5e-4

    def ref_path_error(self, want64, fn32):
        """Error of the reference path itself: fn32 of the f32 product of the kernel's f16 operands
        (f32 torch, the kernel's roundings) against the float64 reference."""
        y32 = self.xk.float() @ self.w16.T
        return (rel_all if self.inp == "norm" else rel_rows)(fn32(y32), want64)

    def verify(self):
        """Every output of the epilogue against float64; returns the errors by name."""
        res, tol, M, rows = self.res, self.base_tol(), self.M, self.rows
        errs = {}
        whole = self.inp == "norm"  # see check()
        if self.epi == "store":
            errs["out"] = check("out", res["out"], self.y, tol, whole)
        elif self.epi == "swiglu_f16":
            want = silu64(self.y[:, 0::2]) * self.y[:, 1::2]
            path = self.ref_path_error(want, lambda y: (torch.nn.functional.silu(y[:, 0::2]) * y[:, 1::2]).half())
            print(f"reference path error {path:.3e}")
            errs["out"] = check("swiglu", res["out"], want, 4 * path, whole)
        elif self.epi == "res":
            out, rx, ss = res["out"], res["res_x"], res["ss_out"]
            errs["product"] = check("resOut - resIn", out.double() - self.res_in.double(), self.y, tol)
            # the hand-off from the RETURNED resOut: at most one f16 rounding
            want_x = (out * self.res_w / 32).clamp(-65504, 65504)
            ulp = torch.exp2(torch.floor(torch.log2(want_x.abs().clamp_min(2.0 ** -14))) - 10)
            assert bool(((rx - want_x).abs() <= ulp).all()), float(((rx - want_x).abs() / ulp).max())
            tiles = cdiv(rows, 64)
            assert ss.shape == (tiles, self.ld_ss)
            got = ss[:, :M]
            assert bool(torch.isfinite(got).all()), "an ssOut slot of a valid (tile, token) was not written"
            want_ss = torch.stack([out[:, 64 * j:64 * j + 64].double().pow(2).sum(-1) for j in range(tiles)])
            worst = float(((got.double() - want_ss).abs() / want_ss).max())
            print(f"ssOut worst rel {worst:.3e}")
            assert worst < 1e-5, worst
            errs["ss"] = worst
        else:
            q0, kv0, hs = self.q0, self.kv0, self.hs
            ctol = tol + (BF16_EPS if self.kv_bf16 else 0)
            wq = torch.stack([rope64(self.y[t, :q0], self.rope, self.pos[t], hs) for t in range(M)])
            wk = torch.stack([rope64(self.y[t, q0:q0 + kv0], self.rope, self.pos[t], hs) for t in range(M)])
            errs["q"] = check("q", res["out"], wq, tol, whole)
            errs["k"] = check("k rows", res["k"], wk, ctol, whole)
            errs["v"] = check("v rows", res["v"], self.y[:, q0 + kv0:], ctol, whole)
        return errs


# ------------------------------------------------------------------------------------ shapes
ALIGNED = (256, 2048)
EDGES = (200, 32 * 72)   # partial 64- and 128-row tiles, rows < 2 NG groups at L = 16; n / 32 = 72: no multiple
                         # of 64 or 16 (tiling padding, partial last K chunks), even and a multiple of 8 (wide)
THIN = (200, 32 * 33)    # narrow only: partial last chunk and tiling padding at every L
TOKENS = (1, 16, 17, 32, 33, 64, 65, 128, 129, 200)


def expected_kernel(L, M, n):
    if M >= 65:
        return "wide"
    return "l16" if L == 16 and M <= 16 and (n // 32) % 16 == 0 else "narrow"


STORE_CASES = [(s, L, M) for s in (ALIGNED, EDGES) for L in (16, 32, 64) for M in TOKENS]
STORE_CASES += [(THIN, L, M) for L in (32, 64) for M in TOKENS if M <= 64]


def test_store_sweep_reaches_every_kernel():
    """The sweep's expectations cover l16, narrow at L = 16 for both reasons (n / 32 % 16, 17 tokens) and wide."""
    exp = {(s, L, M): expected_kernel(L, M, s[1]) for s, L, M in STORE_CASES}
    assert exp[(ALIGNED, 16, 16)] == exp[(ALIGNED, 16, 1)] == "l16"
    assert exp[(ALIGNED, 16, 17)] == exp[(EDGES, 16, 16)] == "narrow"
    assert all(k == "wide" for (s, L, M), k in exp.items() if M >= 65)
    assert {k for k in exp.values()} == {"l16", "narrow", "wide"}


@pytest.mark.parametrize("shape,L,M", STORE_CASES, ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else str(v))
def test_kernel_selection_query(shape, L, M):
    """Host only: the kernel the op reports (hipk::gemmKernelFor, the launcher's dispatch) per sweep case."""
    rows, n = shape
    c = Case("q40", L, M, rows, n, "f16", "store", plan_only=True)
    launches = c.run()["launches"]
    assert [l["kernel"] for l in launches] == [expected_kernel(L, M, n)]
    assert launches[0]["tokens"] == M and launches[0]["splits"] == _ops().gemm_splits(rows, n, M, L)


@gpu
@pytest.mark.parametrize("shape,L,M", STORE_CASES, ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else str(v))
def test_store_kernel_tiling_tokens(shape, L, M):
    """EPI_STORE on f16 rows: kernel x tiling x token tile, aligned and with every edge at once."""
    rows, n = shape
    c = Case("q40", L, M, rows, n, "f16", "store")
    c.run()
    assert c.kernels() == [expected_kernel(L, M, n)]
    c.verify()


@gpu
@pytest.mark.parametrize("shape", [ALIGNED, EDGES], ids=["aligned", "edges"])
@pytest.mark.parametrize("L,M", [(16, 16), (16, 40), (64, 64), (32, 130)])
def test_forced_splits(shape, L, M):
    """Forced K splits: within f32 reassociation of one split, and bitwise equal over three runs."""
    rows, n = shape
    one = Case("q40", L, M, rows, n, "f16", "store", splits=1).run()["out"]
    for splits in (2, 4):
        assert (n // 32) % splits == 0
        c = Case("q40", L, M, rows, n, "f16", "store", splits=splits)
        runs = [c.run()["out"] for _ in range(3)]
        assert c.res["launches"][0]["splits"] == splits
        assert torch.equal(runs[0], runs[1]) and torch.equal(runs[0], runs[2])
        assert rel_rows(runs[0], one) < 1e-5
        c.verify()


@gpu
@pytest.mark.parametrize("shape,splits,grid", [(ALIGNED, 4, 24), (ALIGNED, 1, 6), (EDGES, 2, 12), (EDGES, 4, 24)])
def test_wide_grid_mapping(shape, splits, grid):
    """The wide kernel's two grid mappings: XCD-aware when row tiles x token tiles x splits is a
    multiple of 8, identity otherwise. 300 tokens: three token tiles, the last one partial."""
    rows, n = shape
    c = Case("q40", 32, 300, rows, n, "f16", "store", splits=splits)
    c.run()
    l, = c.res["launches"]
    assert (l["kernel"], l["splits"], l["grid"]) == ("wide", splits, grid)
    assert l["grid"] == cdiv(rows, 128) * 3 * splits
    c.verify()


# (kind, L, M, n): one launch geometry per kernel at rows = 200 / 192
KERNEL_GEOM = {"narrow": ("q40", 32, 40, 2048), "l16": ("q40", 16, 16, 2048), "wide": ("q40", 16, 130, 2048),
               "f32": ("f32", 0, 40, 32 * 33)}
TRIPLES = [("qkv", "norm"), ("qkv", "prenorm"), ("res", "f16"), ("store", "f16"), ("swiglu_f16", "norm"),
           ("swiglu_f16", "prenorm"), ("store", "norm"), ("store", "prenorm")]


@gpu
@pytest.mark.parametrize("kernel", list(KERNEL_GEOM))
@pytest.mark.parametrize("epi,inp", TRIPLES)
def test_every_launchable_triple(kernel, epi, inp):
    """Every (kernel, epilogue, input mode) gemmBatched can launch (the table above), kernel asserted."""
    kind, L, M, n = KERNEL_GEOM[kernel]
    rows = 256 if epi == "qkv" else 200
    c = Case(kind, L, M, rows, n, inp, epi, token_scale=inp == "prenorm")
    c.run()
    assert set(c.kernels()) == {kernel}
    c.verify()


@gpu
@pytest.mark.parametrize("kernel", ["narrow", "l16", "wide"])
def test_swiglu_f16(kernel):
    """EPI_ACT_F16: out[t][i] = f16(silu(y[2i]) * y[2i + 1]) over interleaved (w1, w3) rows; 200 rows end
    both the 64- and the 128-row kernels on a partial tile. Bound: 4 x the reference path's own error
    (f32 torch on the f16-rounded operands, SiLU and product in f32, one f16 rounding; measured
    4.0e-4 .. 6.1e-4 against float64 on the largest token row, so the bound is 1.6e-3 .. 2.4e-3)."""
    kind, L, M, n = KERNEL_GEOM[kernel]
    c = Case(kind, L, M, 200, n, "f16", "swiglu_f16")
    c.run()
    assert set(c.kernels()) == {kernel}
    c.verify()
    # a swapped (w1, w3) pair would give silu(y[2i + 1]) * y[2i]
    swapped = silu64(c.y[:, 1::2]) * c.y[:, 0::2]
    assert rel_rows(c.res["out"], swapped) > 0.5


@gpu
@pytest.mark.parametrize("rows", [192, 200])
@pytest.mark.parametrize("kernel", list(KERNEL_GEOM))
def test_residual_norm_producer(kernel, rows):
    """EPI_RES: resOut = resIn + product, resX = f16(resOut * resW / 32) from the returned resOut, one
    sum of squares per (64-row tile, token) of the returned resOut (the partial last tile sums its
    valid rows only), every slot written, ldSS = M + 3 (the op guards the columns past M)."""
    kind, L, M, n = KERNEL_GEOM[kernel]
    c = Case(kind, L, M, rows, n, "f16", "res")
    c.run()
    assert set(c.kernels()) == {kernel} and c.ld_ss == M + 3
    c.verify()
    out = c.res["out"]
    assert torch.equal(c.res_in + (out - c.res_in), out)


@gpu
def test_residual_saturation():
    """One residual channel at 1e7 with resW = 1: resX stores 65504, never inf; resOut stays unclipped."""
    kind, L, M, n = KERNEL_GEOM["narrow"]
    c = Case(kind, L, M, 200, n, "f16", "res")
    c.res_in[:, 5] = 1e7
    c.res_in[0, 7] = -1e7
    c.res_w[5] = c.res_w[7] = 1.0
    c.run()
    out, rx = c.res["out"], c.res["res_x"]
    assert bool((rx[:, 5] == 65504).all()) and float(rx[0, 7]) == -65504 and bool(torch.isfinite(rx).all())
    assert bool((out[:, 5] > 9.99e6).all()) and float(out[0, 7]) < -9.99e6
    keep = [i for i in range(200) if i not in (5, 7)]
    check("product", (out.double() - c.res_in.double())[:, keep], c.y[:, keep], 5e-4)


@gpu
@pytest.mark.parametrize("ss_tiles", [1, 3, 16, 33])
@pytest.mark.parametrize("kernel,M", [("narrow", 40), ("wide", 200)])
@pytest.mark.parametrize("epi", ["store", "swiglu_f16", "qkv"])
def test_prenorm_consumer(epi, kernel, M, ss_tiles):
    """The consumer of a fused residual + norm: rows f16(x' w / 32), ssTiles partial sums per token below,
    at and above gemmRowScales' threads per token (16 / 8 / 4 / 2), ldSS > M; token t's x' scaled by
    1 + t. Wide at 200 tokens: token tile 1 reads its scales at offset T0 = 128."""
    n = 64 * ss_tiles
    rows = 256 if epi == "qkv" else 200
    c = Case("q40", 32, M, rows, n, "prenorm", epi, token_scale=True)
    assert c.kw["ss"].shape == (ss_tiles, M + 5)
    c.run()
    assert set(c.kernels()) == {kernel}
    c.verify()


@gpu
@pytest.mark.parametrize("kernel,M", [("narrow", 40), ("wide", 150)])
def test_producer_consumer_chain(kernel, M):
    """wo -> w13 hand-off: the EPI_RES outputs (resX, ssOut with its ldSS = M + 3) fed unchanged into a
    prenorm EPI_STORE launch on a second matrix; reference rmsnorm(resIn + y1, resW) @ W2^T in float64.
    Bound: 4 x the reference path's own error (f32 torch with the kernels' roundings: f16 operands,
    f32 products, f32 resOut, f16(resOut * resW / 32), f32 sums of squares; measured 3.4e-4 (40 tokens) and
    3.5e-4 (150) against float64, so the bound is 1.4e-3)."""
    rows1, n1, rows2 = 192, 2048, 200
    p = Case("q40", 32, M, rows1, n1, "f16", "res")
    p.run()
    assert set(p.kernels()) == {kernel}
    blocks2, wd2 = q40_weights(rows2, rows1, seed=9)
    res = _ops().gemm(p.res["res_x"], blocks=blocks2, rows=rows2, n=rows1, lanes=32, input="prenorm",
                      ss=p.res["ss_out"], ld_ss=M + 3, eps=EPS)
    assert {l["kernel"] for l in res["launches"]} == {kernel}
    x1 = p.res_in.double() + p.y
    want = (x1 * torch.rsqrt(x1.pow(2).mean(-1, keepdim=True) + EPS) * p.res_w.double()) @ wd2.T
    # the reference path in f32
    o32 = p.res_in + p.xk.float() @ p.w16.T
    rx32 = (o32 * p.res_w / 32).half()
    ss32 = torch.stack([o32[:, 64 * j:64 * j + 64].pow(2).sum(-1) for j in range(rows1 // 64)])
    y32 = (rx32.float() @ wd2.half().float().T) * (32 / torch.sqrt(ss32.sum(0) / rows1 + EPS))[:, None]
    path = rel_rows(y32, want)
    print(f"reference path error {path:.3e}")
    check("chain", res["out"], want, 4 * path)


@gpu
@pytest.mark.parametrize("kv_bf16", [True, False], ids=["bf16", "f32"])
@pytest.mark.parametrize("hs", [64, 128])
@pytest.mark.parametrize("kernel,M", [("narrow", 20), ("wide", 130)])
def test_qkv_rope_kv_append(kernel, M, hs, kv_bf16):
    """EPI_QKV from a GEMM tile: q and the appended K / V rows against ref_rope of the float64 product,
    non-monotonic positions over two slots; the op checks that every other cache element kept the guard."""
    rows = 128 + 2 * hs
    c = Case("q40", 32, M, rows, 1024, "norm", "qkv", hs=hs, kv_bf16=kv_bf16)
    assert len(set(c.slot)) == 2 and c.pos != sorted(c.pos) and len(set(zip(c.slot, c.pos))) == M
    c.run()
    assert set(c.kernels()) == {kernel}
    c.verify()


@gpu
@pytest.mark.parametrize("M", [5, 40, 100])
@pytest.mark.parametrize("n", [32 * 33, 32 * 3], ids=["8steps+1", "remainder-only"])
@pytest.mark.parametrize("epi,inp", [("store", "f16"), ("swiglu_f16", "norm"), ("res", "f16"), ("qkv", "prenorm")])
def test_f32_gemm(epi, inp, n, M):
    """gemmF32Kernel: the four epilogues at 5 / 40 / 100 tokens (100: a second launch at c0 = 64), the
    remainder loop after 8 unrolled steps and alone, 200 rows (partial last tile)."""
    rows = 256 if epi == "qkv" else 200
    c = Case("f32", 0, M, rows, n, inp, epi, token_scale=inp == "prenorm")
    c.run()
    assert c.kernels() == ["f32"] * cdiv(M, 64)
    assert [l["c0"] for l in c.res["launches"]] == list(range(0, M, 64))
    c.verify()


@gpu
def test_fixed_launch_is_batch_invariant():
    """GemmArgs::fixed: the first 3 output rows are bitwise equal whatever the launch's token count (the
    narrow kernel, the 16-token split count, two threads per token in gemmRowScales); 200 tokens run
    two narrow launches, never the wide kernel."""
    rows, n = 200, 2048
    g = torch.Generator().manual_seed(77)
    head, nw = torch.randn(3, n, generator=g), torch.rand(n, generator=g) + 0.5
    splits = _ops().gemm_splits(rows, n, 16, 0)
    outs = {}
    for M in (3, 40, 128, 200):
        x = torch.cat([head, torch.randn(M - 3, n, generator=g)])
        c = Case("q40", 16, M, rows, n, "prenorm", "store", fixed=True, splits=splits, x=x, nw=nw)
        c.run()
        assert c.kernels() == ["narrow"] * cdiv(M, 128)
        assert all(l["splits"] == splits for l in c.res["launches"])
        c.verify()
        outs[M] = c.res["out"][:3]
    for M in (40, 128, 200):
        assert torch.equal(outs[M], outs[3]), M


# ------------------------------------------------------------------------------------ refusals (no device)
def test_refusals():
    """What the launchers refuse raises before any device work (these run without a GPU)."""
    o = _ops()
    with pytest.raises(RuntimeError, match="even rows"):
        Case("q40", 32, 8, 201, 2048, "f16", "res").run()
    with pytest.raises(RuntimeError, match="bad K split"):  # one launch of all 100 tokens forced
        Case("q40", 32, 100, 200, 32 * 33, "f16", "store", chunk=100).run()
    with pytest.raises(RuntimeError, match="splits must divide"):
        Case("q40", 32, 8, 200, 32 * 33, "f16", "store", splits=2).run()
    with pytest.raises(RuntimeError, match="ldSS"):
        Case("q40", 32, 8, 200, 2048, "f16", "res", ld_ss=7).run()
    c = Case("q40", 32, 8, 200, 2048, "prenorm", "store")
    c.kw.update(ss=c.kw["ss"][:, :7], ld_ss=7)
    with pytest.raises(RuntimeError, match="ldSS"):
        c.run()
    with pytest.raises(RuntimeError, match="more than 128 tokens"):
        Case("q40", 32, 200, 200, 2048, "f16", "store", fixed=True, chunk=200).run()
    # the engine's rule keeps a width the wide kernel cannot take on narrow launches
    plan = Case("q40", 32, 100, 200, 32 * 33, "f16", "store", plan_only=True).run()["launches"]
    assert [(l["kernel"], l["c0"], l["tokens"]) for l in plan] == [("narrow", 0, 64), ("narrow", 64, 36)]
    assert o.gemm_splits(200, 2048, 16, 16) >= 1


# ------------------------------------------------------------------------------------ engine
@gpu
def test_engine_hidden_not_multiple_of_64(tmp_path):
    """The smallest model whose w2 input width (hidden_dim 96) is a multiple of 32 but not of 64: a
    forward of 100 tokens takes narrow launches on w2 (it used to throw `bad K split` in
    launchGemmWide) and matches the CPU backend."""
    import distributed_llama_multiusers_amd as dl
    from distributed_llama_multiusers_amd.models.synthetic import make_test_assets
    from distributed_llama_multiusers_amd.utils.mfile import FloatType
    C = dl.native()
    m, _, _ = make_test_assets(str(tmp_path), "tiny", FloatType.Q40, seq_len=128, seed=4, dim=128, hidden_dim=96,
                               n_heads=2, n_kv_heads=1, n_layers=2, vocab_size=512)
    rng = np.random.default_rng(3)
    toks = [int(t) for t in rng.integers(0, 512, 100)]
    eng = C.HipEngine(m, "q80", kv_bf16=False, max_batch=128)
    got = eng.forward(toks, list(range(100)), [0] * 100)
    ref = C.cpu_backend(m, "q80", 2, max_batch=128).forward(toks, list(range(100)), [0] * 100)
    assert np.isfinite(got).all()
    assert float(np.linalg.norm(got - ref) / np.linalg.norm(ref)) < 3e-2


# ------------------------------------------------------------------------------------ compiled instances
# DL_GEMM_RT1/2/4, DL_GEMM_STG1/2/4 and DL_GEMM_L16 are read once per process: one fresh child per
# setting, each an instance set that exists in launchGemmQ40's DL_GEMM_CASES list
# (token tiles, stages, row tiles): (1,2,2) (2,2,2) (4,1,2) | (1,3,1) (2,3,1) (4,3,1) | (1,4,1) (2,4,1) (4,2,1) |
# (1,2,1) at L = 16 with the l16 kernel off, (2,1,1)
INSTANCE_SETTINGS = {
    "rt2": dict(DL_GEMM_RT1="2", DL_GEMM_RT2="2", DL_GEMM_RT4="2"),
    "stg3": dict(DL_GEMM_STG1="3", DL_GEMM_STG2="3", DL_GEMM_STG4="3"),
    "stg4-4-2": dict(DL_GEMM_STG1="4", DL_GEMM_STG2="4", DL_GEMM_STG4="2"),
    "l16off-stg2=1": dict(DL_GEMM_L16="0", DL_GEMM_STG2="1"),
}
ABSENT = dict(DL_GEMM_RT1="2", DL_GEMM_STG1="3")  # (1, 3, 2) is not compiled


def child_main(mode):
    """Runs in the child: the narrow EPI_STORE cases of the sweep and one EPI_RES case; prints the
    largest errors (the parent asserts them) or, mode "absent", the launcher's error."""
    if mode == "absent":
        try:
            Case("q40", 32, 8, 200, 2048, "f16", "store").run()
        except RuntimeError as e:
            print("REFUSED", e)
            return
        print("LAUNCHED")
        return
    worst = 0.0
    for shape, L, M in STORE_CASES:
        if M > 64:
            continue
        c = Case("q40", L, M, shape[0], shape[1], "f16", "store")
        c.run()
        want = expected_kernel(L, M, shape[1])
        if os.environ.get("DL_GEMM_L16") == "0" or os.environ.get("DL_GEMM_RT1") == "2":
            want = "narrow"  # the l16 kernel is off, or not eligible at two row tiles per workgroup
        assert c.kernels() == [want], (shape, L, M, c.kernels())
        worst = max(worst, rel_rows(c.res["out"], c.y))
    c = Case("q40", 32, 40, 200, 2048, "f16", "res")
    c.run()
    errs = c.verify()
    print(f"MAXERR store {worst:.6e} product {errs['product']:.6e} ss {errs['ss']:.6e}")


def run_child(mode, env):
    repo = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    full = dict(os.environ, PYTHONPATH=repo, **env)
    return subprocess.run([sys.executable, os.path.abspath(__file__), mode], env=full, capture_output=True, text=True,
                          timeout=240)


@gpu
@pytest.mark.parametrize("setting", list(INSTANCE_SETTINGS))
def test_non_default_instances(setting):
    out = run_child("sweep", INSTANCE_SETTINGS[setting])
    assert out.returncode == 0, out.stdout[-1500:] + out.stderr[-1500:]
    line = [l for l in out.stdout.splitlines() if l.startswith("MAXERR")][-1].split()
    store, product, ss = float(line[2]), float(line[4]), float(line[6])
    assert store < 5e-4 and product < 5e-4 and ss < 1e-5, line


@gpu
def test_absent_instance_is_refused():
    """A stage / row-tile combination that is not compiled gives the launcher's clean error."""
    out = run_child("absent", ABSENT)
    assert out.returncode == 0, out.stdout[-1500:] + out.stderr[-1500:]
    assert "REFUSED" in out.stdout and "no narrow kernel instance" in out.stdout, out.stdout[-1500:]


if __name__ == "__main__":
    child_main(sys.argv[1])
