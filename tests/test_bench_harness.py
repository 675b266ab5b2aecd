"""bench.py's multi-GPU contract (the driver's scaling runs depend on it): `--gpus N` without a
launcher spawns its own N ranks, refuses to fake a scaling point when fewer GPUs are visible, and a
same-GPU rehearsal is labelled as one (n_gpus 1, same_gpu_rehearsal, no vs_baseline)."""
import json
import os
import subprocess
import sys

import pytest

from conftest import REPO, gpu_available

BENCH = os.path.join(REPO, "bench.py")


@pytest.mark.skipif(gpu_available(), reason="checks the no-GPU refusal path")
def test_gpus_n_without_enough_devices_refuses():
    env = dict(os.environ)
    env.pop("WORLD_SIZE", None)
    env.pop("DL_BENCH_SAME_GPU", None)
    r = subprocess.run([sys.executable, BENCH, "--gpus", "2", "--steps", "2", "--warmup", "1"], capture_output=True,
                       text=True, timeout=300, env=env)
    assert r.returncode == 2, r.stdout + r.stderr
    assert "GPU(s) visible" in r.stderr and "DL_BENCH_SAME_GPU" in r.stderr
    assert not [l for l in r.stdout.splitlines() if l.startswith("{")]  # no result line at all


def test_help_names_full_and_dump_outputs():
    r = subprocess.run([sys.executable, BENCH, "--help"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "--full" in r.stdout and "--dump-outputs" in r.stdout


@pytest.mark.gpu
def test_plain_run_is_headline_only_and_dumps_the_same_outputs_twice(tmp_path):
    """A plain run times the headline alone (every extra point of `config` is absent), `--steps` is the
    number of timed decode steps, and two runs with the same arguments dump identical arrays."""
    import numpy as np
    steps, prompt = 6, 32
    dumps = []
    for name in ("a", "b"):
        d = tmp_path / name
        r = subprocess.run([sys.executable, BENCH, "--gpus", "1", "--shape", "llama3_2_1b", "--steps", str(steps),
                            "--warmup", "2", "--prompt", str(prompt), "--max-seq-len", "128", "--dump-outputs", str(d)],
                           capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, r.stderr[-3000:]
        lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
        assert len(lines) == 1, r.stdout
        res = json.loads(lines[0])
        assert res["steps"] == steps and res["ms_per_step"] > 0 and res["value"] > 0
        cfg = res["config"]
        # the host window around the timed call encloses the device events around its `steps` steps
        # (1 % for the two clocks), and adds one launch and one synchronise: 20 ms covers a busy host
        dev_ms, host_ms = cfg["device_ms_per_step"] * steps, res["ms_per_step"] * steps
        assert 0.99 * dev_ms <= host_ms <= dev_ms + 20.0, (dev_ms, host_ms)
        assert abs(cfg["pred_ms_per_token"] - res["ms_per_step"]) < 1e-9
        for k in ("long_ctx_pred_ms_per_token", "cap131072_pred_ms_per_token", "prompt_4k_eval_ms_per_token",
                  "prompt_4k_eval_big_chunk_ms_per_token", "tp_f32_pred_ms_per_token"):
            assert cfg[k] is None, k
        assert not [k for k in cfg if k.startswith(("bf16_kv_", "cli_", "tp2_", "tp4_", "tp8_"))]
        out = {f: np.load(d / f) for f in sorted(os.listdir(d))}
        assert sorted(out) == ["eval_tokens.npy", "next_logits.npy", "pred_tokens.npy"]
        assert all(a.dtype == np.float32 for a in out.values())
        assert out["pred_tokens.npy"].shape == (steps, 1) and out["eval_tokens.npy"].shape == (1, prompt)
        assert out["next_logits.npy"].shape == (1, 128256) and np.isfinite(out["next_logits.npy"]).all()
        assert 0 <= out["pred_tokens.npy"].min() and out["pred_tokens.npy"].max() < 128256
        dumps.append(out)
    for f in dumps[0]:
        assert np.array_equal(dumps[0][f], dumps[1][f]), f


@pytest.mark.gpu
def test_dump_outputs_batch_2_rows_are_steps_columns_are_sequences(C, tmp_path):
    """`--batch 2`: pred_tokens.npy is [steps, batch]. The reference decodes the same engine one step
    per call (a one-step call returns one token per sequence, so its layout cannot be mistaken) and
    feeds each step's tokens to the next; next_logits.npy continues from the last row. Every sequence
    gets the same prompt, so the columns are equal, and random-init weights mostly repeat one token:
    an 8-token prompt without warmup is a case whose chain changes from step to step, which a
    [batch, steps] buffer read as [steps, batch] would not reproduce."""
    import numpy as np
    import bench
    from distributed_llama_multiusers_amd.models.synthetic import LLAMA_SHAPES
    steps, warmup, n_prompt, B, seq = 5, 0, 8, 2, 128
    r = subprocess.run([sys.executable, BENCH, "--gpus", "1", "--shape", "llama3_2_1b", "--batch", str(B), "--steps",
                        str(steps), "--warmup", str(warmup), "--prompt", str(n_prompt), "--max-seq-len", str(seq),
                        "--dump-outputs", str(tmp_path)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-3000:]
    pred = np.load(tmp_path / "pred_tokens.npy")
    assert pred.shape == (steps, B) and np.load(tmp_path / "eval_tokens.npy").shape == (B, n_prompt)

    shape = dict(bench.LLAMA31_8B, **LLAMA_SHAPES["llama3_2_1b"])
    eng = C.HipEngine("", "q80", max_seq_len=seq, max_batch=32, n_slots=B, kv_bf16=False, gpu_index=0,
                      synthetic=dict(shape, seq_len=seq), seed=1234, sync_type="q80")
    prompt = [(i * 7919 + 13) % 128000 for i in range(n_prompt)]
    slots = list(range(B))
    for b in slots:
        eng.forward_argmax(prompt, list(range(n_prompt)), [b] * n_prompt)
    p1, toks, want = n_prompt + warmup, [prompt[-1]] * B, []
    for s in range(steps):
        _, toks = eng.decode_greedy(1, toks, [p1 + s] * B, slots)
        want.append(list(toks))
    assert len({t for row in want for t in row}) > 1, f"pick a case whose tokens vary: {want}"
    assert np.array_equal(pred, np.asarray(want, dtype=np.float32)), (pred, want)
    logits = eng.forward(want[-1], [p1 + steps] * B, slots)
    assert np.array_equal(np.load(tmp_path / "next_logits.npy"), logits)


@pytest.mark.gpu
def test_same_gpu_rehearsal_self_launch_is_labelled():
    env = dict(os.environ, DL_BENCH_SAME_GPU="1", HSA_ENABLE_IPC_MODE_LEGACY="0")
    env.pop("WORLD_SIZE", None)
    r = subprocess.run([sys.executable, BENCH, "--gpus", "2", "--shape", "llama3_2_1b", "--steps", "8", "--warmup", "2",
                        "--prompt", "32", "--full", "--long-ctx", "0", "--no-altkv", "--no-cli"],
                       capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, r.stdout
    res = json.loads(lines[0])
    assert res["n_gpus"] == 1 and res["same_gpu_rehearsal"] is True and res["vs_baseline"] is None
    cfg = res["config"]
    assert cfg["tp_ranks"] == 2 and cfg["tp_sync"] == "q80" and cfg["parallelism"] == "tp2"
    assert cfg["tp_f32_pred_ms_per_token"] > 0 and res["value"] > 0
    # ranks reach their first forward seconds apart: the fused exchange's self-test must wait for them
    assert cfg["tp_fused_exchange"] is True and "self-test failed" not in r.stderr, r.stderr[-3000:]
    assert cfg["prompt_4k_eval_ms_per_token"] > 0
