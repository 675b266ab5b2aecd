"""Q80-weight models on the CPU backend: the Q80 x Q80 matmul, the device tiling (host side) and a
tiny model against the PyTorch oracle and against the same tensors written as q40 and f32."""
import numpy as np
import pytest

from distributed_llama_multiusers_amd import ops
from distributed_llama_multiusers_amd.models.llama import TorchLlama
from distributed_llama_multiusers_amd.models.synthetic import make_test_assets
from distributed_llama_multiusers_amd.utils.mfile import FloatType, Q80_DTYPE, quantize_q80

TOKENS = [3, 17, 101, 7, 250, 9, 44, 300]


def _q80(x):
    """x [r, c] -> (Q80 blocks [r, c/32], codes int64 [r, c/32, 32], scales float64 [r, c/32])"""
    b = quantize_q80(np.ascontiguousarray(x, dtype=np.float32).reshape(-1)).reshape(x.shape[0], -1)
    return b, b["qs"].astype(np.int64), b["d"].astype(np.float64)


@pytest.fixture(scope="module")
def models(tmp_path_factory):
    d = str(tmp_path_factory.mktemp("q80w"))
    return {k: make_test_assets(d, "tiny", t, seq_len=128, seed=1)[0]
            for k, t in (("q80", FloatType.Q80), ("q40", FloatType.Q40), ("f32", FloatType.F32))}


def _logits(C, path, buf):
    be = C.cpu_backend(path, buf, 2)
    return np.stack([be.forward([t], [p], [0])[0] for p, t in enumerate(TOKENS)])


def test_matmul_q80_q80(C):
    rows, n, B = 64, 256, 3
    g = np.random.default_rng(0)
    wb, wq, wd = _q80(g.standard_normal((rows, n)) * 0.05)
    x = g.standard_normal((B, n)).astype(np.float32)
    _, xq, xd = _q80(x)
    terms = wd[None] * xd[:, None] * np.einsum("rji,bji->brj", wq, xq)  # [B, rows, nb], float64
    got = C.cpu_ops.matmul_q80_q80(wb.view(np.uint8).reshape(-1), rows, n, x)
    bound = (n // 32 + 4) * 2.0 ** -24 * np.abs(terms).sum(-1)
    assert (np.abs(got - terms.sum(-1)) <= bound).all()


@pytest.mark.parametrize("rows,n,L,c0,nc", [(40, 256, 16, 0, 0), (66, 160, 32, 0, 0), (9, 256, 64, 64, 96)])
def test_tile_q80_round_trip(rows, n, L, c0, nc):
    """Every block of the (sliced) matrix at its documented offset, everything else zero: rows that
    are no multiple of the pass (2 * 256 / L), block counts that are no multiple of L, a column slice."""
    g = np.random.default_rng(1)
    wb, wq, _ = _q80(g.standard_normal((rows, n)))
    q, d = ops.tile_q80(wb.view(np.uint8).reshape(-1), rows, n, L, c0, nc)
    nbs = (nc or n - c0) // 32
    NG, K = 256 // L, -(-nbs // L)
    assert q.size == -(-rows // (2 * NG)) * K * 4 * 256 * 16 and d.size * 16 * 4 == q.size
    q = q.view(np.int8).reshape(-1, 2, 2, 256, 16)  # [chunk][row of the pair][half][thread][16]
    d16 = d.view(np.float16).reshape(-1, 256, 2)
    seen_q, seen_d = np.zeros(q.shape, bool), np.zeros(d16.shape, bool)
    for r in range(rows):
        for j in range(nbs):
            c, tid = (r // (2 * NG)) * K + j // L, (r % (2 * NG)) // 2 * L + j % L
            assert (q[c, r & 1, :, tid].reshape(32) == wq[r, c0 // 32 + j]).all()
            assert d16[c, tid, r & 1] == wb["d"][r, c0 // 32 + j]
            seen_q[c, r & 1, :, tid] = True
            seen_d[c, tid, r & 1] = True
    assert not q[~seen_q].any() and not d16[~seen_d].view(np.uint16).any()


def test_q80_model_matches_oracle(C, models):
    got = _logits(C, models["q80"], "q80")
    ref = TorchLlama(models["q80"]).forward(TOKENS).numpy()
    assert np.abs(got - ref).max() / np.abs(ref).max() < 2e-2  # test_cpu_backend's Q40 tolerance
    assert (got.argmax(-1) == ref.argmax(-1)).mean() >= 0.75
    with pytest.raises(Exception, match="Q80 sync type"):
        C.cpu_backend(models["q80"], "f32", 1)


def test_q80_model_closer_to_f32_than_q40(C, models):
    f32 = _logits(C, models["f32"], "f32")
    e80 = np.abs(_logits(C, models["q80"], "q80") - f32).max()
    e40 = np.abs(_logits(C, models["q40"], "q80") - f32).max()
    assert e80 < e40, (e80, e40)
