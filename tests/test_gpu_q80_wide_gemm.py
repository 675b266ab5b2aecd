"""gemmQ80wWideKernel (128 x 128 tiles, Q80 weights staged in LDS) against float64 references of the
same operands, and a Q80 engine forward of 150 rows (two token tiles, every fused epilogue) against
the CPU backend.

The store bound is the any-order f32 bound of the narrow kernel's test: int8 -> f16 and the block
products are exact in the MFMA's f32 accumulator up to its roundings, so n products and the scale
steps give (n + 8) * 2^-24 * (|x16| @ |w64|.T) for any split and stage order; a q * d rounded to f16
(2^-11 per weight) would exceed it."""
import numpy as np
import pytest
import torch

from distributed_llama_multiusers_amd import ops
from distributed_llama_multiusers_amd.models.synthetic import make_test_assets
from distributed_llama_multiusers_amd.utils.mfile import FloatType, quantize_q80

pytestmark = pytest.mark.gpu


def q80_weights(rows, n, seed=1):
    """(file-layout blocks as bytes, the weights they encode as float64 [rows, n])"""
    w = np.random.default_rng(seed).standard_normal((rows, n)).astype(np.float32) / n ** 0.5
    b = quantize_q80(w.reshape(-1)).reshape(rows, n // 32)
    w64 = b["qs"].astype(np.float64) * b["d"].astype(np.float64)[..., None]
    return b.view(np.uint8).reshape(-1), torch.from_numpy(w64.reshape(rows, n))


def activations(M, n, seed=2):
    return torch.randn(M, n, generator=torch.Generator().manual_seed(seed))


def gemm_bound(w64, x16, n):
    return (n + 8) * 2.0 ** -24 * (x16.abs() @ w64.abs().T)


# rows = 144: a full 128-row tile and a 16-row one (clamped rows). (n, splits): a split shorter than the
# pipeline, steady state with wrapping stage buffers, the combine over two full splits. M: a ragged
# token tile, an exact one, a second tile of one token. lanes: both address forms of the tiling.
@pytest.mark.parametrize("lanes", [16, 32])
@pytest.mark.parametrize("M", [65, 128, 129])
@pytest.mark.parametrize("n,splits", [(256, 2), (512, 1), (512, 2)])
def test_wide_store(n, splits, M, lanes):
    rows = 144
    blocks, w64 = q80_weights(rows, n)
    x = activations(M, n)
    x16 = x.half().double()
    got = ops.gemm_q80w(blocks, rows, n, x, lanes=lanes, splits=splits, wide=True)
    assert got["kernels"] == ["wide"] and got["splits"] == [splits]
    assert bool(((got["out"].double() - x16 @ w64.T).abs() <= gemm_bound(w64, x16, n)).all())


@pytest.mark.parametrize("splits", [1, 2])
def test_wide_res_and_consumer(splits):
    """EPI_RES producer over two token tiles, then a consumer that scales each token by its RMS factor
    (gemmRowScales at T0 > 0): the bounds of test_gpu_q80_weights.test_gemm_res_and_consumer."""
    rows, n, M = 192, 256, 130
    blocks, w64 = q80_weights(rows, n)
    x, res_in, res_w = activations(M, n), activations(M, rows, seed=5), torch.rand(rows, generator=torch.Generator().manual_seed(6)) + 0.5
    x16 = x.half().double()
    p = ops.gemm_q80w(blocks, rows, n, x, lanes=32, splits=splits, epilogue="res", res_in=res_in, res_w=res_w, wide=True)
    assert p["kernels"] == ["wide"] and p["splits"] == [splits]
    xn = res_in.double() + x16 @ w64.T
    bound = gemm_bound(w64, x16, n) + 2.0 ** -24 * xn.abs()
    assert bool(((p["out"].double() - xn).abs() <= bound).all())
    hand = xn * res_w.double() / 32
    assert bool(((p["res_x"].double() - hand).abs() <= 2.0 ** -10 * hand.abs() + bound).all())  # one f16 rounding
    ss = torch.stack([xn[:, i:i + 64].pow(2).sum(-1) for i in range(0, rows, 64)])
    assert torch.allclose(p["ss"].double(), ss, rtol=1e-5, atol=0)
    rows2 = 48  # consumer: a second matrix over the 192 hand-off columns
    blocks2, w2 = q80_weights(rows2, rows, seed=4)
    c = ops.gemm_q80w(blocks2, rows2, rows, p["res_x"], lanes=16, ss=p["ss"], eps=1e-5, wide=True)
    assert c["kernels"] == ["wide"]
    scale = 32.0 / torch.sqrt(p["ss"].double().sum(0) / rows + 1e-5)
    hx = p["res_x"].double()
    want = (hx @ w2.T) * scale[:, None]
    assert bool(((c["out"].double() - want).abs() <= (rows + 12) * 2.0 ** -24 * (hx.abs() @ w2.abs().T) * scale[:, None]).all())


# ---------------------------------------------------------------------------------------- engine
N_ROWS = 150
TOKENS = [(7 * i + 3) % 1024 for i in range(N_ROWS + 1)]


@pytest.fixture(scope="module")
def q80_model(tmp_path_factory):
    d = str(tmp_path_factory.mktemp("q80w_wide"))
    return make_test_assets(d, "tiny", FloatType.Q80, seq_len=192, seed=9, dim=512, n_heads=8, n_kv_heads=4,
                            hidden_dim=1024, vocab_size=1024)[0]


@pytest.fixture(scope="module")
def cpu_rows(C, q80_model):
    cpu = C.cpu_backend(q80_model, "q80", 4)
    return np.stack([cpu.forward([t], [p], [0])[0] for p, t in enumerate(TOKENS)])


def _rel(a, b):
    return float(np.abs(a - b).max() / np.abs(b).max())


@pytest.mark.parametrize("kv_bf16", [True, False])
def test_engine_wide_forward(C, q80_model, cpu_rows, kv_bf16):
    """150 rows in one forward: QKV + RoPE + KV append, SwiGLU -> f16, the residual hand-off and the
    logits on the wide kernel with a ragged second token tile; its replays; then a decode row that
    reads the KV the wide QKV epilogue appended."""
    gpu = C.HipEngine(q80_model, "q80", kv_bf16=kv_bf16, max_batch=160)
    pos = list(range(N_ROWS))
    got = gpu.forward(TOKENS[:N_ROWS], pos, [0] * N_ROWS)
    for r in range(N_ROWS):
        assert _rel(got[r], cpu_rows[r]) < 3e-2, r
    for _ in range(2):
        assert np.array_equal(gpu.forward(TOKENS[:N_ROWS], pos, [0] * N_ROWS), got)
    assert _rel(gpu.forward(TOKENS[N_ROWS:], [N_ROWS], [0])[0], cpu_rows[N_ROWS]) < 3e-2
