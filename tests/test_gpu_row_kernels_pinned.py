"""The device sampler (`ops.sample`) and the logprobs kernel (`ops.logprobs`) pinned against recorded
outputs: token ids exactly, logprob floats bit for bit. The sampler's other tests accept any draw
that is valid within 2e-4 of cumulative mass, so a changed summation order of its histograms would
pass them; here it does not.

The fixture tests/golden/row_kernels_pinned.npz holds ids and 21-entry logprob records only; the
inputs are regenerated from the seeds below. It was recorded on an MI355X from the build of the
commit before the row kernels' building blocks moved to row_dev.h, and is re-recorded only by a
pull request that changes the kernels' arithmetic on purpose:

    DLLAMA_RECORD_PINNED=1 python tests/test_gpu_row_kernels_pinned.py --record

Every recorded sampler id is also checked to be a valid draw (`_draw_ok`), so a bad recording cannot
pin a wrong answer."""
import itertools
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "row_kernels_pinned.npz")
F32 = np.float32
# sampleGroups at its cap (1 and 5 rows) and at 16 (64 rows); one tile, the scalar tails 517 % 4 and
# 8193 % 4, and the full vocabulary
SHAPES = [(517, 1), (517, 5), (517, 64), (8193, 1), (8193, 5), (8193, 64), (128256, 1), (128256, 64)]
# (temperature, top-p), top-p outermost: rows 1 and 2 of a launch are multinomial draws
COMBOS = [(t, p) for p, t in itertools.product((0.0, 0.5, 0.95, 1.0), (0.0, 0.6, 1.3))]
ONE_ROW = {517: 4, 8193: 11, 128256: 7}  # the single row's combination: nucleus, multinomial, nucleus
TOP = (20, 1, 0)
BELOW_ONE = float(np.nextafter(F32(1), F32(0)))


def case(vocab, rows):
    """Quarter-step rounded normals (ties occur); every fourth row masked to -inf on its first three
    quarters, as the candidate filter leaves rows; coins 0.0 and just below 1 on a multinomial and on
    a nucleus row each."""
    rng = np.random.default_rng(100000 * rows + vocab)
    x = (np.round(rng.standard_normal((rows, vocab)) * 12) / 4).astype(F32)
    coins = rng.random(rows).astype(F32)
    for b, coin in ((1, 0.0), (2, BELOW_ONE), (4, 0.0), (5, BELOW_ONE)):
        if b < rows:
            coins[b] = coin
    start = ONE_ROW[vocab] if rows == 1 else 0
    specs = [COMBOS[(start + b) % len(COMBOS)] for b in range(rows)]
    for b in range(3, rows, 4):
        x[b, :3 * vocab // 4] = -np.inf
    chosen = [int(i) for i in rng.integers(0, vocab, rows)]
    top = [TOP[b % 3] for b in range(rows)]
    return x, specs, [float(c) for c in coins], chosen, top


def run(ops, vocab, rows):
    x, specs, coins, chosen, top = case(vocab, rows)
    ids = ops.sample(x, [s[0] for s in specs], [s[1] for s in specs], coins)
    vals, tok = ops.logprobs(x, chosen, top)
    return np.asarray(ids, np.int32), np.asarray(vals, F32), np.asarray(tok, np.int32)


def recorded_draw_ok(logits, temp, topp, coin, tok, tol=2e-4):
    """`_draw_ok` at the granularity the sampler draws with. A multinomial row is drawn by index and
    `_draw_ok` applies as it is. A nucleus row is cut and drawn by key (phases 1-6), and phase 7
    returns the lowest index that holds the drawn key. With tied logits (these inputs have them,
    `_draw_ok`'s other callers do not) a class of equal logits therefore counts as one candidate:
    the nucleus ends with the whole class that crosses top-p, `tok` is the lowest index of its
    class, and the coin falls in the class's run of `_draw_ok`'s stable order. Same f64 arithmetic
    and `tol`; on a row without ties this is `_draw_ok` term for term."""
    from test_gpu_sampling_filters import _draw_ok
    if topp <= 0.0 or topp >= 1.0:
        return _draw_ok(logits, temp, topp, coin, tok, tol)
    tied = np.nonzero(logits == logits[tok])[0]
    if tied[0] != tok:
        return False
    x = logits.astype(np.float64)
    with np.errstate(over="ignore", invalid="ignore"):
        p = np.exp(x / temp - (x / temp).max())
    p /= p.sum()
    cand = np.nonzero(p >= (1.0 - topp) / (len(p) - 1) * (1 - 1e-5))[0]
    order = cand[np.argsort(-p[cand], kind="stable")]
    cum = np.cumsum(p[order])
    last = min(int(np.searchsorted(cum, topp, side="right")), len(order) - 1)
    last = int(np.nonzero(logits[order] == logits[order[last]])[0][-1])  # the end of that class
    run_ =np.nonzero(np.isin(order, tied))[0]
    if len(run_) == 0 or run_[0] > last + 1:
        return False
    lo = cum[run_[0] - 1] if run_[0] > 0 else 0.0
    return lo - tol <= coin * cum[last] <= cum[run_[-1]] + tol


@pytest.fixture(scope="module")
def ops():
    from distributed_llama_multiusers_amd import ops
    return ops


@pytest.fixture(scope="module")
def golden():
    with np.load(GOLDEN) as z:
        return {k: z[k] for k in z.files}


@pytest.mark.parametrize("vocab,rows", SHAPES)
def test_sampler_ids_pinned(ops, golden, vocab, rows):
    x, specs, coins, _, _ = case(vocab, rows)
    want = golden[f"sample_{vocab}_{rows}"]
    for b, (temp, topp) in enumerate(specs):  # the recording itself is a valid draw
        if temp == 0.0:
            assert want[b] == int(np.argmax(x[b])), (b, want[b])
        else:
            assert recorded_draw_ok(x[b], temp, topp, coins[b], int(want[b])), (b, specs[b], coins[b], want[b])
    got = ops.sample(x, [s[0] for s in specs], [s[1] for s in specs], coins)
    assert [int(i) for i in got] == [int(i) for i in want]


@pytest.mark.parametrize("vocab,rows", SHAPES)
def test_logprobs_records_pinned(ops, golden, vocab, rows):
    x, _, _, chosen, top = case(vocab, rows)
    vals, tok = ops.logprobs(x, chosen, top)
    want_v, want_i = golden[f"logprob_{vocab}_{rows}"], golden[f"logprob_id_{vocab}_{rows}"]
    assert np.asarray(tok, np.int32).tolist() == want_i.tolist()
    assert np.asarray(vals, F32).tobytes() == want_v.tobytes()


if __name__ == "__main__":
    if "--record" not in sys.argv or os.environ.get("DLLAMA_RECORD_PINNED") != "1":
        sys.exit("recording needs --record and DLLAMA_RECORD_PINNED=1 (see the module docstring)")
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    from distributed_llama_multiusers_amd import ops as _ops
    out = {}
    for _vocab, _rows in SHAPES:
        _ids, _vals, _tok = run(_ops, _vocab, _rows)
        again = run(_ops, _vocab, _rows)
        assert all(a.tobytes() == b.tobytes() for a, b in zip((_ids, _vals, _tok), again)), (_vocab, _rows)
        out[f"sample_{_vocab}_{_rows}"] = _ids
        out[f"logprob_{_vocab}_{_rows}"] = _vals
        out[f"logprob_id_{_vocab}_{_rows}"] = _tok
    _path = sys.argv[sys.argv.index("--record") + 1] if len(sys.argv) > sys.argv.index("--record") + 1 else GOLDEN
    np.savez_compressed(_path, **out)
    print("recorded", _path, os.path.getsize(_path), "bytes")
