"""Q80-weight kernels and engine on the GPU: gemvQ80wKernel and gemmQ80wKernel against float64
references of the same operands, and a tiny Q80 model against the CPU backend.

GEMV references use the exact Q80 codes of both operands. With the producer's blocks (global
prologue) the bound is the kernel's own arithmetic: (nb + 4) * 2^-24 * sum_j |term_j| for any-order
f32 sums of nb exact block terms and the scale roundings. Behind the norm prologue a 1-ulp difference
in the normalised input can move a Q80 code, so those cases take the bound the Q40 norm-prologue cases
of test_gpu_gemv_paths.py take against their float64 reference (2e-4 of the output's norm and of its
largest element; 8e-3 for bf16 cache rows)."""
import numpy as np
import pytest
import torch

from distributed_llama_multiusers_amd import ops
from distributed_llama_multiusers_amd.models.synthetic import make_test_assets
from distributed_llama_multiusers_amd.utils.mfile import FloatType, quantize_q80

pytestmark = pytest.mark.gpu


def q80_weights(rows, n, seed=1):
    """(file-layout blocks as bytes, codes float64 [rows, nb, 32], scales float64 [rows, nb])"""
    w = np.random.default_rng(seed).standard_normal((rows, n)).astype(np.float32) / n ** 0.5
    b = quantize_q80(w.reshape(-1)).reshape(rows, n // 32)
    return b.view(np.uint8).reshape(-1), b["qs"].astype(np.float64), b["d"].astype(np.float64)


def activations(B, n, seed=2):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(B, n, generator=g), torch.randn(B, n, generator=g), torch.rand(n, generator=g) + 0.5


def check(out, want, tol):
    err = (out.double() - want).abs()
    assert float(err.norm() / want.norm()) < tol and float(err.max() / want.abs().max()) <= tol


def swiglu64(y):
    return torch.nn.functional.silu(y[:, 0::2]) * y[:, 1::2]


# (B, L, n, rows, passes): n = 256 (fewer blocks than lanes) and 544 (17 blocks: a second, partial step);
# rows = one workgroup's rows + 2 (2 * 256 / L * passes + 2) or an odd count
@pytest.mark.parametrize("B,L,n,rows,passes", [(1, 16, 256, 34, 1), (2, 16, 544, 66, 2), (4, 32, 256, 19, 1),
                                               (1, 64, 544, 27, 3)])
def test_gemv_global_prologue(B, L, n, rows, passes):
    blocks, wq, wd = q80_weights(rows, n)
    x = activations(B, n)[0]
    xb = quantize_q80(x.numpy().reshape(-1)).reshape(B, n // 32)
    terms = wd[None] * xb["d"].astype(np.float64)[:, None] * np.einsum("rji,bji->brj", wq, xb["qs"].astype(np.float64))
    out = ops.gemv_q80w(blocks, rows, n, x, prologue="global", lanes=L, passes=passes)["out"].numpy()
    bound = (n // 32 + 4) * 2.0 ** -24 * np.abs(terms).sum(-1)
    assert (np.abs(out - terms.sum(-1)) <= bound).all()


@pytest.mark.parametrize("B,L,n,rows,passes,epi", [
    (1, 16, 256, 34, 1, "store"), (4, 16, 544, 33, 2, "store"), (2, 64, 544, 10, 1, "swiglu"),
    (1, 32, 256, 66, 2, "swiglu"), (2, 16, 544, 128, 2, "swiglu_q80"), (1, 32, 256, 192, 4, "swiglu_q80")])
def test_gemv_norm_prologue(B, L, n, rows, passes, epi):
    blocks, wq, wd = q80_weights(rows, n)
    w64 = torch.from_numpy((wq * wd[..., None]).reshape(rows, n))
    x, r, nw = activations(B, n)
    got = ops.gemv_q80w(blocks, rows, n, x, r, nw, epilogue=epi, lanes=L, passes=passes)
    assert torch.equal(got["x_next"], x + r)
    y = ops.dequantize_q80(ops.ref_rmsnorm(x + r, nw)).double() @ w64.T
    if epi == "store":
        check(got["out"], y, 2e-4)
    elif epi == "swiglu":
        check(got["out"], swiglu64(y), 2e-4)
    else:  # the hand-off row: code * d within half a step, the f16 rounding of d and the GEMV's bound
        h = swiglu64(y).reshape(B, -1, 32)
        d, sums = got["scales"][..., 0].double(), got["scales"][..., 1].double()
        codes = got["codes"].double().reshape(h.shape)
        bound = d[..., None] / 2 + h.abs().amax(-1, keepdim=True) * 2.0 ** -10 + 2e-4 * h.abs().max()
        assert bool(((codes * d[..., None] - h).abs() <= bound).all())
        assert torch.equal(sums, codes.sum(-1)) and torch.equal(d.float().half().double(), d)


@pytest.mark.parametrize("B,L,passes,kv_bf16", [(1, 16, 1, True), (2, 32, 3, False)])
def test_gemv_qkv_epilogue(B, L, passes, kv_bf16):
    n, hs, seq, pos = 256, 64, 32, [17, 5][:B]
    q0, kv0 = 2 * hs, hs
    rows = q0 + 2 * kv0
    blocks, wq, wd = q80_weights(rows, n)
    w64 = torch.from_numpy((wq * wd[..., None]).reshape(rows, n))
    x, _, nw = activations(B, n)
    ang = torch.outer(torch.arange(seq).double(), 10000.0 ** (-torch.arange(0, hs, 2).double() / hs))
    rope = torch.stack([ang.cos(), ang.sin()], -1).float()
    got = ops.gemv_q80w(blocks, rows, n, x, None, nw, epilogue="qkv", lanes=L, passes=passes, q0=q0, kv0=kv0, hs=hs,
                        rope=rope, pos=pos, kv_bf16=kv_bf16)
    y = ops.dequantize_q80(ops.ref_rmsnorm(x, nw)).double() @ w64.T

    def rot(v, p):
        v = v.reshape(-1, hs // 2, 2)
        c, s = rope[p, :, 0].double(), rope[p, :, 1].double()
        return torch.stack([v[..., 0] * c - v[..., 1] * s, v[..., 0] * s + v[..., 1] * c], -1).reshape(-1)

    for b, p in enumerate(pos):
        check(got["out"][b], rot(y[b, :q0], p), 2e-4)
        check(got["k"][b], rot(y[b, q0:q0 + kv0], p), 8e-3 if kv_bf16 else 2e-4)
        check(got["v"][b], y[b, q0 + kv0:], 8e-3 if kv_bf16 else 2e-4)


def gemm_bound(w64, x16, n):
    return (n + 8) * 2.0 ** -24 * (x16.abs() @ w64.abs().T)


@pytest.mark.parametrize("fetch", [8, 16])
@pytest.mark.parametrize("splits", [1, 2])
@pytest.mark.parametrize("M", [1, 16, 17, 64])
def test_gemm_store(M, splits, fetch):
    rows, n = 80, 256  # 64 + 16: a tile edge
    blocks, wq, wd = q80_weights(rows, n)
    w64 = torch.from_numpy((wq * wd[..., None]).reshape(rows, n))
    x = activations(M, n)[0]
    x16 = x.half().double()
    got = ops.gemm_q80w(blocks, rows, n, x, lanes=16, splits=splits, fetch=fetch)
    assert got["splits"] == [splits]
    assert bool(((got["out"].double() - x16 @ w64.T).abs() <= gemm_bound(w64, x16, n)).all())


@pytest.mark.parametrize("M,splits", [(17, 1), (64, 2)])
def test_gemm_res_and_consumer(M, splits):
    """EPI_RES producer (residual update, f16 hand-off rows, per-tile sums of squares), then a GEMM
    that consumes the hand-off and scales each token by its RMS factor."""
    rows, n = 96, 256  # 64 + 32: a tile edge, and whole Q80 blocks for the consumer's input width
    blocks, wq, wd = q80_weights(rows, n)
    w64 = torch.from_numpy((wq * wd[..., None]).reshape(rows, n))
    x, res_in, res_w = activations(M, n)[0], activations(M, rows, seed=5)[0], activations(1, rows, seed=6)[2]
    x16 = x.half().double()
    p = ops.gemm_q80w(blocks, rows, n, x, lanes=32, splits=splits, epilogue="res", res_in=res_in, res_w=res_w)
    xn = res_in.double() + x16 @ w64.T
    bound = gemm_bound(w64, x16, n) + 2.0 ** -24 * xn.abs()
    assert bool(((p["out"].double() - xn).abs() <= bound).all())
    hand = xn * res_w.double() / 32
    assert bool(((p["res_x"].double() - hand).abs() <= 2.0 ** -10 * hand.abs() + bound).all())  # one f16 rounding
    ss = torch.stack([xn[:, :64].pow(2).sum(-1), xn[:, 64:].pow(2).sum(-1)])
    assert torch.allclose(p["ss"].double(), ss, rtol=1e-5, atol=0)
    # consumer: a second matrix over the `rows` hand-off columns
    rows2 = 48
    blocks2, wq2, wd2 = q80_weights(rows2, rows, seed=4)
    w2 = torch.from_numpy((wq2 * wd2[..., None]).reshape(rows2, rows))
    c = ops.gemm_q80w(blocks2, rows2, rows, p["res_x"], lanes=16, ss=p["ss"], eps=1e-5)
    scale = 32.0 / torch.sqrt(p["ss"].double().sum(0) / rows + 1e-5)
    want = (p["res_x"].double() @ w2.T) * scale[:, None]
    assert bool(((c["out"].double() - want).abs() <= (rows + 12) * 2.0 ** -24 * (p["res_x"].double().abs() @ w2.abs().T) * scale[:, None]).all())


# ---------------------------------------------------------------------------------------- engine
@pytest.fixture(scope="module")
def q80_model(tmp_path_factory):
    d = str(tmp_path_factory.mktemp("q80w_gpu"))
    return make_test_assets(d, "tiny", FloatType.Q80, seq_len=128, seed=9, dim=512, n_heads=8, n_kv_heads=4,
                            hidden_dim=1024, vocab_size=1024)[0]


def _rel(a, b):
    return float(np.abs(a - b).max() / np.abs(b).max())


@pytest.mark.parametrize("n", [1, 24])
@pytest.mark.parametrize("kv_bf16", [True, False])
def test_engine_matches_cpu_and_replays(C, q80_model, kv_bf16, n):
    """Rows one at a time (GEMVs) or 24 per forward (batched GEMMs) against the CPU backend, then the
    same forward twice more: the captured graph and its replay equal the eager run bitwise."""
    tokens = [(7 * i + 3) % 1024 for i in range(24)]
    cpu = C.cpu_backend(q80_model, "q80", 4)
    ref = np.stack([cpu.forward([t], [p], [0])[0] for p, t in enumerate(tokens)])
    gpu = C.HipEngine(q80_model, "q80", kv_bf16=kv_bf16, max_batch=32)
    pos = list(range(24))
    if n == 1:  # every single-row forward shares one graph: the eager value comes from a graph-free engine
        got = np.stack([gpu.forward([t], [p], [0])[0] for p, t in enumerate(tokens)])
        eager = C.HipEngine(q80_model, "q80", kv_bf16=kv_bf16, max_batch=32, use_graphs=False)
        first = np.stack([eager.forward([t], [p], [0])[0] for p, t in enumerate(tokens)])
        assert np.array_equal(got, first)  # row 0 eager, row 1 the capture, rows 2.. replays
        last = lambda: gpu.forward(tokens[-1:], [23], [0])
        first = first[-1:]
    else:
        got = gpu.forward(tokens, pos, [0] * 24)
        last = lambda: gpu.forward(tokens, pos, [0] * 24)
        first = got
    assert _rel(got, ref) < 3e-2
    for _ in range(2):
        assert np.array_equal(last(), first)
    with pytest.raises(Exception, match="Q80 sync type"):
        C.HipEngine(q80_model, "f32")


def test_simulated_tp2_matches_single(C, q80_model):
    tokens = [5, 99, 300, 7, 1000, 2]
    single = C.HipEngine(q80_model, "q80", kv_bf16=False)
    ref = np.stack([single.forward([t], [p], [0])[0] for p, t in enumerate(tokens)])
    got = C.simulate_tp(q80_model, "q80", 2, tokens)
    assert _rel(got, ref) < 3e-2
    assert (got.argmax(-1) == ref.argmax(-1)).all()
