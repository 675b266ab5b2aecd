"""The micro-benchmark entry points (`ops.bench_*`, `bench_*`, `trace_*`) that scripts/bench_*.py and
the figures under profiles/ go through: every one runs, returns finite positive times and traces of
the documented length, can be called again in the same process, and refuses bad arguments without
spoiling the next call. They share one timing harness (csrc/hip/host_harness.h).

Shapes: the row benches at 2 rows of 517 logits (no multiple of the 256-thread workgroup), the JSON
mask at the smallest table of test_gpu_json_mode.py, the kernel benches at the smallest launch of
test_gpu_gemv_paths.py (RING_CASES[0]: L 16, K 1, 1 pass), test_gpu_gemm_paths.py (ALIGNED, 1
token) and test_gpu_attention_paths.py (test_auto_runs_mfma_at_1024: the MFMA decode kernel, the
one that writes a trace). 2 operand copies, 3 launches per timed window."""
import math

import numpy as np
import pytest
import torch

from test_gpu_gemm_paths import ALIGNED
from test_gpu_gemv_paths import RING_CASES, n_for, rows_past
from test_gpu_json_mode import make_pieces

from distributed_llama_multiusers_amd import ops

pytestmark = pytest.mark.gpu

B, VOCAB, DIM, SLOTS, ITERS, COPIES = 2, 517, 64, 2, 3, 2
PRO_RESNORM, EPI_STORE = 1, 0

GEMV_L, GEMV_K, GEMV_PASSES = RING_CASES[0][:3]
GEMV = dict(rows=rows_past(GEMV_L, GEMV_PASSES), n=n_for(GEMV_L, GEMV_K), pro=PRO_RESNORM, epi=EPI_STORE, batch=1,
            lanes=GEMV_L, passes=GEMV_PASSES, copies=COPIES, iters=ITERS)
GEMM = dict(rows=ALIGNED[0], n=ALIGNED[1], tokens=1, epi=EPI_STORE, copies=COPIES, iters=ITERS)
ATTN = dict(n_heads0=4, kv_mul=4, head_size=128, seq_len=1024, pos=700, batch=2, copies=COPIES, iters=ITERS)


@pytest.fixture(scope="module")
def json_table(C):
    pieces, bos_id, eos = make_pieces(261)
    return C.JsonTable(pieces, bos_id, eos)


def check_times(name, times):
    times = tuple(np.atleast_1d(times))
    print(name, [round(float(t), 3) for t in times], "us")
    for t in times:
        assert math.isfinite(t) and t > 0, (name, times)


def check_trace(name, trace, words):
    trace = np.asarray(trace, dtype=np.uint64)
    print(name, trace.size, "words,", int(np.count_nonzero(trace)), "non-zero")
    assert trace.size == words, (name, trace.size, words)
    assert np.any(trace != 0), name


def filter_bench(C, batch=B):
    return C.ops.bench_logit_filter(batch, VOCAB, 40, float("-inf"), ITERS)


def test_row_benches(C, json_table):
    x = (np.random.default_rng(0).standard_normal((B, VOCAB)) * 6).astype(np.float32)
    check_times("bench_logprobs", C.ops.bench_logprobs(x, B, 5, ITERS))
    check_times("bench_logit_proc", C.ops.bench_logit_proc(B, VOCAB, 3, ITERS))
    check_times("bench_logit_filter", filter_bench(C))
    check_times("bench_json_mask", C.ops.bench_json_mask(B, json_table, C.cpu_ops.json_walk(b""), ITERS))
    check_times("bench_pool", C.ops.bench_pool(B, DIM, SLOTS, True, ITERS))


def test_kernel_benches(C):
    check_times("bench_gemv_q40", C.bench_gemv_q40(**GEMV))
    check_times("bench_gemm_q40", C.bench_gemm_q40(**GEMM))
    check_times("bench_attention", C.bench_attention(**ATTN))
    check_times("bench_memcpy_d2d", C.bench_memcpy_d2d(B * VOCAB * 4, ITERS))


def test_trace_variants(C):
    """8 u64 per workgroup (kernels.h GemvArgs::trace, gemm_dev.h gemmTrace, AttnArgs::trace): the GEMV
    stamps every launch of the graph, the GEMM and the attention one launch after the timing."""
    us, t = C.trace_gemv_q40(**GEMV)
    check_times("trace_gemv_q40", us)
    wg_rows = 512 // GEMV_L * GEMV_PASSES
    check_trace("trace_gemv_q40", t, ITERS * ((GEMV["rows"] + wg_rows - 1) // wg_rows) * 8)
    us, t, splits = C.trace_gemm_q40(**GEMM)
    check_times("trace_gemm_q40", us)
    assert splits >= 1
    check_trace("trace_gemm_q40", t, 8 * ((GEMM["rows"] + 63) // 64) * splits)
    us, t = C.trace_attention(**ATTN)
    check_times("trace_attention", us)
    n_kv, rows = ATTN["n_heads0"] // ATTN["kv_mul"], ATTN["batch"]
    cache = torch.zeros(rows, ATTN["seq_len"], n_kv * ATTN["head_size"])
    plan = ops.attention_launch(torch.zeros(rows, ATTN["n_heads0"] * ATTN["head_size"]), cache, cache, ATTN["n_heads0"],
                                ATTN["kv_mul"], ATTN["head_size"], [ATTN["pos"]] * rows, list(range(rows)), plan_only=True)
    assert plan["kernel"].startswith("attnDecodeMfmaKernel")
    check_trace("trace_attention", t, 8 * n_kv * plan["split_grid"] * rows)


def test_bench_twice_in_one_process(C):
    """The second call meets whatever the first one's teardown left of its stream, events and graph."""
    for _ in range(2):
        check_times("bench_gemv_q40", C.bench_gemv_q40(**GEMV))
        check_times("bench_logit_filter", filter_bench(C))


def test_refused_arguments_leave_the_next_call_intact(C):
    with pytest.raises(Exception, match="bench_logit_filter arguments"):
        filter_bench(C, batch=0)
    check_times("bench_logit_filter", filter_bench(C))
