"""F16-weight kernels and engine on the GPU: gemvF16wKernel and gemmF16wKernel against float64
references over the exact f16 weight values, and a tiny F16 model against the CPU backend.

The decode GEMV multiplies f32(w) by f32 activations, one f32 FMA per term: against float64 over the
same operands the bound is that of an any-order f32 sum of n once-rounded terms, (n + 8) * 2^-24 *
sum_k |w x|, elementwise. Behind the norm prologue the reference normalises in its own order, so those
cases take the tolerances the norm-prologue cases of test_gpu_gemv_paths.py / test_gpu_q80_weights.py
take (2e-4 of the output's norm and of its largest element; 8e-3 for bf16 cache rows). The batched GEMM
rounds activations to f16 once; products are exact and accumulate in f32: gemm_bound."""
import numpy as np
import pytest
import torch

from distributed_llama_multiusers_amd import ops
from distributed_llama_multiusers_amd.models.synthetic import make_test_assets
from distributed_llama_multiusers_amd.utils.mfile import FloatType

pytestmark = pytest.mark.gpu


def f16_weights(rows, n, seed=1):
    """([rows, n] float16 array, the same values as a float64 tensor)"""
    w = (np.random.default_rng(seed).standard_normal((rows, n)) / n ** 0.5).astype(np.float16)
    return w, torch.from_numpy(w.astype(np.float64))


def activations(B, n, seed=2):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(B, n, generator=g), torch.randn(B, n, generator=g), torch.rand(n, generator=g) + 0.5


def check(out, want, tol):
    err = (out.double() - want).abs()
    assert float(err.norm() / want.norm()) < tol and float(err.max() / want.abs().max()) <= tol


def swiglu64(y):
    return torch.nn.functional.silu(y[:, 0::2]) * y[:, 1::2]


# (B, L, n, rows, passes). n / 8 = 32 units (fewer than 64 lanes; one unguarded iteration at 16) or 68
# (a partial last step: behind a whole iteration at 16 lanes, alone at 32 / 64); rows = one workgroup's
# rows (2 * 256 / L * passes) + 2, or an odd count over several workgroups
@pytest.mark.parametrize("B,L,n,rows,passes", [(1, 16, 544, 34, 1), (2, 16, 256, 66, 2), (4, 32, 544, 19, 1),
                                               (2, 64, 256, 27, 3), (1, 64, 544, 10, 1)])
def test_gemv_global_prologue(B, L, n, rows, passes):
    w, w64 = f16_weights(rows, n)
    x = activations(B, n)[0]
    out = ops.gemv_f16w(w, x, prologue="global", lanes=L, passes=passes)["out"].double()
    bound = (n + 8) * 2.0 ** -24 * (x.double().abs() @ w64.abs().T)
    assert bool(((out - x.double() @ w64.T).abs() <= bound).all())


@pytest.mark.parametrize("B,L,n,rows,passes,epi", [(1, 16, 256, 34, 1, "store"), (4, 16, 544, 33, 2, "store"),
                                                   (2, 64, 544, 10, 1, "swiglu"), (1, 32, 256, 66, 2, "swiglu")])
def test_gemv_norm_prologue(B, L, n, rows, passes, epi):
    w, w64 = f16_weights(rows, n)
    x, r, nw = activations(B, n)
    got = ops.gemv_f16w(w, x, r, nw, epilogue=epi, lanes=L, passes=passes)
    assert torch.equal(got["x_next"], x + r)
    y = ops.ref_rmsnorm(x + r, nw).double() @ w64.T
    check(got["out"], y if epi == "store" else swiglu64(y), 2e-4)


@pytest.mark.parametrize("B,L,passes,kv_dtype", [(1, 16, 1, "bf16"), (2, 32, 3, "f32"), (4, 64, 2, "bf16")])
def test_gemv_qkv_epilogue(B, L, passes, kv_dtype):
    n, hs, seq, pos = 256, 64, 32, [17, 5, 0, 31][:B]
    q0, kv0 = 2 * hs, hs
    rows = q0 + 2 * kv0
    w, w64 = f16_weights(rows, n)
    x, _, nw = activations(B, n)
    ang = torch.outer(torch.arange(seq).double(), 10000.0 ** (-torch.arange(0, hs, 2).double() / hs))
    rope = torch.stack([ang.cos(), ang.sin()], -1).float()
    got = ops.gemv_f16w(w, x, None, nw, epilogue="qkv", lanes=L, passes=passes, q0=q0, kv0=kv0, hs=hs, rope=rope, pos=pos,
                        kv_dtype=kv_dtype)
    y = ops.ref_rmsnorm(x, nw).double() @ w64.T

    def rot(v, p):
        v = v.reshape(-1, hs // 2, 2)
        c, s = rope[p, :, 0].double(), rope[p, :, 1].double()
        return torch.stack([v[..., 0] * c - v[..., 1] * s, v[..., 0] * s + v[..., 1] * c], -1).reshape(-1)

    tol = 8e-3 if kv_dtype == "bf16" else 2e-4
    for b, p in enumerate(pos):
        check(got["out"][b], rot(y[b, :q0], p), 2e-4)
        check(got["k"][b], rot(y[b, q0:q0 + kv0], p), tol)
        check(got["v"][b], y[b, q0 + kv0:], tol)


def gemm_bound(w64, x16, n):
    return (n + 8) * 2.0 ** -24 * (x16.abs() @ w64.abs().T)


# n = 256: four 64-k steps (one whole group), or two per split; 288: a 32-k remainder behind them (9
# blocks: the launcher takes no split in two, K per split must be whole 32-k blocks); 320 in two splits:
# 160 per split, the remainder behind a partial group
@pytest.mark.parametrize("n,splits", [(256, 1), (256, 2), (288, 1), (320, 2)])
@pytest.mark.parametrize("M", [1, 16, 17, 64])
def test_gemm_store(M, n, splits):
    rows = 80  # 64 + 16: a tile edge
    w, w64 = f16_weights(rows, n)
    x16 = activations(M, n)[0].half()
    got = ops.gemm_f16w(w, x16.float(), splits=splits)
    assert got["splits"] == [splits]
    x16 = x16.double()
    assert bool(((got["out"].double() - x16 @ w64.T).abs() <= gemm_bound(w64, x16, n)).all())


@pytest.mark.parametrize("M,splits", [(17, 1), (64, 2)])
def test_gemm_res_and_consumer(M, splits):
    """EPI_RES producer (residual update, f16 hand-off rows, per-tile sums of squares), then a GEMM
    that consumes the hand-off and scales each token by its RMS factor."""
    rows, n = 96, 256  # 64 + 32: a tile edge; the consumer's K = 96 is one 64-k step and the remainder
    w, w64 = f16_weights(rows, n)
    x, res_in, res_w = activations(M, n)[0], activations(M, rows, seed=5)[0], activations(1, rows, seed=6)[2]
    x16 = x.half().double()
    p = ops.gemm_f16w(w, x, splits=splits, epilogue="res", res_in=res_in, res_w=res_w)
    xn = res_in.double() + x16 @ w64.T
    bound = gemm_bound(w64, x16, n) + 2.0 ** -24 * xn.abs()
    assert bool(((p["out"].double() - xn).abs() <= bound).all())
    hand = xn * res_w.double() / 32
    assert bool(((p["res_x"].double() - hand).abs() <= 2.0 ** -10 * hand.abs() + bound).all())  # one f16 rounding
    ss = torch.stack([xn[:, :64].pow(2).sum(-1), xn[:, 64:].pow(2).sum(-1)])
    assert torch.allclose(p["ss"].double(), ss, rtol=1e-5, atol=0)
    w2, w2_64 = f16_weights(48, rows, seed=4)  # consumer: a second matrix over the `rows` hand-off columns
    c = ops.gemm_f16w(w2, p["res_x"], ss=p["ss"], eps=1e-5)
    scale = 32.0 / torch.sqrt(p["ss"].double().sum(0) / rows + 1e-5)
    want = (p["res_x"].double() @ w2_64.T) * scale[:, None]
    bound = (rows + 12) * 2.0 ** -24 * (p["res_x"].double().abs() @ w2_64.abs().T) * scale[:, None]
    assert bool(((c["out"].double() - want).abs() <= bound).all())


# ---------------------------------------------------------------------------------------- engine
@pytest.fixture(scope="module")
def f16_model(tmp_path_factory):
    d = str(tmp_path_factory.mktemp("f16w_gpu"))
    return make_test_assets(d, "tiny", FloatType.F16, seq_len=128, seed=9, dim=512, n_heads=8, n_kv_heads=4,
                            hidden_dim=1024, vocab_size=1024)[0]


def _rel(a, b):
    return float(np.abs(a - b).max() / np.abs(b).max())


# the F32-model tolerances of test_gpu_engine.py: single rows 1e-4 at f32 KV, 2e-2 at bf16 KV; batched 1e-2
@pytest.mark.parametrize("n,kv_bf16,tol", [(1, False, 1e-4), (1, True, 2e-2), (24, False, 1e-2)])
def test_engine_matches_cpu_and_replays(C, f16_model, n, kv_bf16, tol):
    """Rows one at a time (GEMVs) or 24 per forward (batched GEMMs) against the CPU backend, then the
    same forward twice more: the captured graph and its replay equal the eager run bitwise."""
    tokens = [(7 * i + 3) % 1024 for i in range(24)]
    cpu = C.cpu_backend(f16_model, "f32", 4)
    ref = np.stack([cpu.forward([t], [p], [0])[0] for p, t in enumerate(tokens)])
    gpu = C.HipEngine(f16_model, "f32", kv_bf16=kv_bf16, max_batch=32)
    pos = list(range(24))
    if n == 1:  # every single-row forward shares one graph: the eager value comes from a graph-free engine
        got = np.stack([gpu.forward([t], [p], [0])[0] for p, t in enumerate(tokens)])
        eager = C.HipEngine(f16_model, "f32", kv_bf16=kv_bf16, max_batch=32, use_graphs=False)
        first = np.stack([eager.forward([t], [p], [0])[0] for p, t in enumerate(tokens)])
        assert np.array_equal(got, first)  # row 0 eager, row 1 the capture, rows 2.. replays
        last = lambda: gpu.forward(tokens[-1:], [23], [0])
        first = first[-1:]
    else:
        got = gpu.forward(tokens, pos, [0] * 24)
        last = lambda: gpu.forward(tokens, pos, [0] * 24)
        first = got
    assert _rel(got, ref) < tol
    for _ in range(2):
        assert np.array_equal(last(), first)


def test_engine_refuses_q80_buffers(C, f16_model):
    with pytest.raises(Exception, match="F16 weights require --buffer-float-type f32"):
        C.HipEngine(f16_model, "q80")


def test_simulated_tp2_matches_single(C, f16_model):
    """Two simulated ranks against one engine: the split sums differ by f32 reassociation only, the
    f32-KV single-row tolerance of F32 models."""
    tokens = [5, 99, 300, 7, 1000, 2]
    single = C.HipEngine(f16_model, "f32", kv_bf16=False)
    ref = np.stack([single.forward([t], [p], [0])[0] for p, t in enumerate(tokens)])
    got = C.simulate_tp(f16_model, "f32", 2, tokens)
    assert _rel(got, ref) < 1e-4
    assert (got.argmax(-1) == ref.argmax(-1)).all()
