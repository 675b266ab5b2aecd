"""gemmF16wWideKernel (128 x 128 tiles, F16 weights and activations staged in LDS as one image) against
float64 references of the same operands, and an F16 engine forward of 150 rows (two token tiles, every
fused epilogue) against the CPU backend.

The store bound is the any-order f32 bound of the narrow kernel's test: f16 x f16 products are exact
in the MFMA's f32 accumulator, so n products give (n + 8) * 2^-24 * (|x16| @ |w64|.T) for any split and
stage order. The engine tolerances are the batched F16 / F32-model ones of test_gpu_f16_weights.py
(1e-2 of the largest logit; 2e-2 for a single row over a bf16 cache): the wide kernel only
reassociates the narrow kernel's f32 sums."""
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


def activations(M, n, seed=2):
    return torch.randn(M, n, generator=torch.Generator().manual_seed(seed))


def gemm_bound(w64, x16, n):
    return (n + 8) * 2.0 ** -24 * (x16.abs() @ w64.abs().T)


# rows = 144: a full 128-row tile and a 16-row one (clamped rows). (n, splits): one stage per split
# (shorter than any pipeline depth), eight stages (steady state with wrapping stage buffers), the
# combine over two four-stage splits. M: a ragged token tile, an exact one, a second tile of one token.
@pytest.mark.parametrize("M", [65, 128, 129])
@pytest.mark.parametrize("n,splits", [(128, 2), (512, 1), (512, 2)])
def test_wide_store(n, splits, M):
    rows = 144
    w, w64 = f16_weights(rows, n)
    x = activations(M, n)
    x16 = x.half().double()
    got = ops.gemm_f16w(w, x, splits=splits, wide=True)
    assert got["kernels"] == ["wide"] and got["splits"] == [splits]
    assert bool(((got["out"].double() - x16 @ w64.T).abs() <= gemm_bound(w64, x16, n)).all())


@pytest.mark.parametrize("splits", [1, 2])
def test_wide_res_and_consumer(splits):
    """EPI_RES producer over two token tiles, then a consumer that scales each token by its RMS factor
    (gemmRowScales at T0 > 0): the bounds of test_gpu_f16_weights.test_gemm_res_and_consumer."""
    rows, n, M = 192, 256, 130
    w, w64 = f16_weights(rows, n)
    x, res_in, res_w = activations(M, n), activations(M, rows, seed=5), torch.rand(rows, generator=torch.Generator().manual_seed(6)) + 0.5
    x16 = x.half().double()
    p = ops.gemm_f16w(w, x, splits=splits, epilogue="res", res_in=res_in, res_w=res_w, wide=True)
    assert p["kernels"] == ["wide"] and p["splits"] == [splits]
    xn = res_in.double() + x16 @ w64.T
    bound = gemm_bound(w64, x16, n) + 2.0 ** -24 * xn.abs()
    assert bool(((p["out"].double() - xn).abs() <= bound).all())
    hand = xn * res_w.double() / 32
    assert bool(((p["res_x"].double() - hand).abs() <= 2.0 ** -10 * hand.abs() + bound).all())  # one f16 rounding
    ss = torch.stack([xn[:, i:i + 64].pow(2).sum(-1) for i in range(0, rows, 64)])
    assert torch.allclose(p["ss"].double(), ss, rtol=1e-5, atol=0)
    rows2 = 48  # consumer: a second matrix over the 192 hand-off columns
    w2, w2_64 = f16_weights(rows2, rows, seed=4)
    c = ops.gemm_f16w(w2, p["res_x"], ss=p["ss"], eps=1e-5, wide=True)
    assert c["kernels"] == ["wide"]
    scale = 32.0 / torch.sqrt(p["ss"].double().sum(0) / rows + 1e-5)
    hx = p["res_x"].double()
    want = (hx @ w2_64.T) * scale[:, None]
    assert bool(((c["out"].double() - want).abs() <= (rows + 12) * 2.0 ** -24 * (hx.abs() @ w2_64.abs().T) * scale[:, None]).all())


def test_chunking():
    """wide=None follows the engine: a width that is no multiple of 64 stays on narrow launches (and
    the wide kernel refuses it), 64 rows are one narrow launch."""
    rows, n, M = 80, 288, 70
    w, w64 = f16_weights(rows, n)
    x = activations(M, n)
    x16 = x.half().double()
    got = ops.gemm_f16w(w, x, wide=None)
    assert got["kernels"] == ["narrow", "narrow"]
    assert bool(((got["out"].double() - x16 @ w64.T).abs() <= gemm_bound(w64, x16, n)).all())
    with pytest.raises(Exception, match="whole 64-k stages"):
        ops.gemm_f16w(w, x, wide=True)
    assert ops.gemm_f16w(f16_weights(rows, 256)[0], activations(64, 256), wide=None)["kernels"] == ["narrow"]


# ---------------------------------------------------------------------------------------- engine
N_ROWS = 150
TOKENS = [(7 * i + 3) % 1024 for i in range(N_ROWS + 1)]


@pytest.fixture(scope="module")
def f16_model(tmp_path_factory):
    d = str(tmp_path_factory.mktemp("f16w_wide"))
    return make_test_assets(d, "tiny", FloatType.F16, seq_len=192, seed=9, dim=512, n_heads=8, n_kv_heads=4,
                            hidden_dim=1024, vocab_size=1024)[0]


@pytest.fixture(scope="module")
def cpu_rows(C, f16_model):
    cpu = C.cpu_backend(f16_model, "f32", 4)
    return np.stack([cpu.forward([t], [p], [0])[0] for p, t in enumerate(TOKENS)])


def _rel(a, b):
    return float(np.abs(a - b).max() / np.abs(b).max())


@pytest.mark.parametrize("kv_bf16", [True, False])
def test_engine_wide_forward(C, f16_model, cpu_rows, kv_bf16):
    """150 rows in one forward: QKV + RoPE + KV append, SwiGLU -> f16, the residual hand-off and the
    logits on the wide kernel with a ragged second token tile; its replays; then a decode row that
    reads the KV the wide QKV epilogue appended."""
    gpu = C.HipEngine(f16_model, "f32", kv_bf16=kv_bf16, max_batch=160)
    pos = list(range(N_ROWS))
    got = gpu.forward(TOKENS[:N_ROWS], pos, [0] * N_ROWS)
    for r in range(N_ROWS):
        assert _rel(got[r], cpu_rows[r]) < 1e-2, r
    for _ in range(2):
        assert np.array_equal(gpu.forward(TOKENS[:N_ROWS], pos, [0] * N_ROWS), got)
    assert _rel(gpu.forward(TOKENS[N_ROWS:], [N_ROWS], [0])[0], cpu_rows[N_ROWS]) < (2e-2 if kv_bf16 else 1e-2)
