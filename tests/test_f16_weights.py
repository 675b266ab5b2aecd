"""F16-weight models on the CPU backend: the weights are widened to f32 once at load, so an F16 file
computes bit for bit what an F32 file holding the same f16-representable values computes."""
import dataclasses

import numpy as np
import pytest

from distributed_llama_multiusers_amd.models.synthetic import make_spec, random_tensors
from distributed_llama_multiusers_amd.utils.mfile import FloatType, write_model

TOKENS = [3, 17, 101, 7, 250, 9]


@pytest.fixture(scope="module")
def models(tmp_path_factory):
    d = tmp_path_factory.mktemp("f16w")
    spec = make_spec("tiny", FloatType.F16, seq_len=128)
    t = random_tensors(spec, seed=1)
    for k, v in t.items():  # the matmul weights at f16 precision; embedding and norms stay f32 in both files
        if k[0] != "embedding" and not k[0].startswith("rms"):
            t[k] = v.astype(np.float16).astype(np.float32)
    paths = {"f16": str(d / "tiny_f16.m"), "f32": str(d / "tiny_f32.m")}
    write_model(paths["f16"], spec, t)
    write_model(paths["f32"], dataclasses.replace(spec, weights_float_type=FloatType.F32), t)
    return paths


def _logits(C, path):
    be = C.cpu_backend(path, "f32", 2)
    return np.stack([be.forward([t], [p], [0])[0] for p, t in enumerate(TOKENS)])


def test_f16_file_equals_f32_file_bitwise(C, models):
    got = _logits(C, models["f16"])
    assert np.isfinite(got).all() and np.array_equal(got, _logits(C, models["f32"]))


def test_f16_model_refuses_q80_buffers(C, models):
    with pytest.raises(Exception, match="F16 weights require --buffer-float-type f32"):
        C.cpu_backend(models["f16"], "q80", 1)
