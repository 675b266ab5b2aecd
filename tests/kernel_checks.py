"""Assertions shared by the kernel suites (test_gpu_gemv_paths.py, test_gpu_attention_paths.py)."""
import torch


def check_q80_row(codes, d, sums, h, what, kernel_bound=2e-4):
    """The contract of a Q80 hand-off row. codes [B, H] int, d / sums [B, H / 32], h [B, H] float64
    (the reference row).
    |code * d - h| <= d / 2 (rounding half-step) + A * 2^-10 (f16 rounding of the scale, A the
    block's largest |h|, a factor 2 of slack) + kernel_bound * max|h| (the producing kernel's own
    bound: 2e-4 for the GEMV); d is an f16 value, the sum field is the sum of the codes, |code| <= 127."""
    Bn, H = h.shape
    codes, d, sums = codes.double().reshape(Bn, H // 32, 32), d.double(), sums.double()
    hb = h.reshape(Bn, H // 32, 32)
    A = hb.abs().amax(-1, keepdim=True)
    bound = d[..., None] / 2 + A * 2.0 ** -10 + kernel_bound * h.abs().max()
    err = (codes * d[..., None] - hb).abs()
    print(f"{what}: worst error / bound {float((err / bound).max()):.3f}")
    assert bool((err <= bound).all()), float((err / bound).max())
    assert torch.equal(d.float().half().float().double(), d)  # the scale is an f16 value
    assert torch.equal(sums, codes.sum(-1))
    assert int(codes.abs().max()) <= 127
