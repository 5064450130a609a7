"""bench.py --dump-outputs on CPU: what the last timed step returned (a SeparationResult) lands in DIR as float32 .npy files,
whole when it fits, as the same seeded positions from run to run when it does not, and never over the 64 MB bound; the
prompt tokenizer gives the same ids in every process."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import bench
from sam_audio_amd.model import SeparationResult

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _result(clips, n, rows_t, seed=0):
    g = torch.Generator().manual_seed(seed)
    return SeparationResult(target=[torch.randn(1, n, generator=g) for _ in range(clips)],
                            residual=[torch.randn(1, n, generator=g) for _ in range(clips)],
                            noise=torch.randn(clips, rows_t, 256, generator=g))


def _load(d):
    return {f[:-4]: np.load(os.path.join(d, f)) for f in sorted(os.listdir(d))}


def test_small_result_is_written_whole(tmp_path):
    res = _result(2, 4800, 3)
    bench.dump_outputs(res, str(tmp_path))
    got = _load(tmp_path)
    assert sorted(got) == ["noise", "residual", "target"]
    assert all(a.dtype == np.float32 for a in got.values())
    assert np.array_equal(got["target"], torch.stack(res.target).numpy())
    assert np.array_equal(got["residual"], torch.stack(res.residual).numpy())
    assert np.array_equal(got["noise"], res.noise.numpy())


def test_large_result_is_a_seeded_sample_within_the_bound(tmp_path, monkeypatch):
    monkeypatch.setattr(bench, "DUMP_BYTES", 400_000)   # the default workload's 131 MB against 64 MB, scaled down
    res = _result(4, 48_000, 25)
    a, b = tmp_path / "a", tmp_path / "b"
    bench.dump_outputs(res, str(a))
    bench.dump_outputs(res, str(b))
    got, again = _load(a), _load(b)
    assert sum(os.path.getsize(a / f) for f in os.listdir(a)) <= bench.DUMP_BYTES
    for name, full in (("target", torch.stack(res.target)), ("residual", torch.stack(res.residual)), ("noise", res.noise)):
        assert np.array_equal(got[name], again[name])
        assert 0 < got[name].size < full.numel()
        assert np.isin(got[name], full.numpy().reshape(-1)).all()


def test_steps_must_be_positive():
    with pytest.raises(SystemExit):
        bench.parse(["--steps", "0"])
    assert bench.parse(["--steps", "7", "--dump-outputs", "d"]).steps == 7


def test_prompt_ids_do_not_depend_on_the_process():
    code = "import bench; print(bench._HashTokenizer()(['a dog barking', 'rain'])['input_ids'].tolist())"
    outs = {subprocess.run([sys.executable, "-c", code], cwd=ROOT, capture_output=True, text=True, check=True,
                           env=dict(os.environ, PYTHONHASHSEED=str(seed))).stdout for seed in (1, 2)}
    assert len(outs) == 1, outs
