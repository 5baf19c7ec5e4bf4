"""bench.dump_outputs (--dump-outputs DIR): float32 .npy files, whole arrays under the cap, a fixed seeded sample of them past it."""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402


def test_dump_outputs_writes_float32_arrays(tmp_path):
    x = torch.randn(1, 4, 3, 5, 6, dtype=torch.float64)
    bench.dump_outputs(str(tmp_path / "d"), dict(latent=x))
    assert os.listdir(tmp_path / "d") == ["latent.npy"]
    a = np.load(tmp_path / "d" / "latent.npy")
    assert a.dtype == np.float32 and a.shape == tuple(x.shape)
    assert np.array_equal(a, x.float().numpy())


def test_dump_outputs_samples_past_the_cap_the_same_way_every_time(tmp_path, monkeypatch):
    monkeypatch.setattr(bench, "DUMP_CAP_BYTES", 4 * 1000)
    x = torch.arange(10000, dtype=torch.float32).reshape(10, 1000)
    bench.dump_outputs(str(tmp_path / "a"), dict(latent=x))
    bench.dump_outputs(str(tmp_path / "b"), dict(latent=x))
    assert os.listdir(tmp_path / "a") == ["latent_sample.npy"]
    a, b = np.load(tmp_path / "a" / "latent_sample.npy"), np.load(tmp_path / "b" / "latent_sample.npy")
    assert a.dtype == np.float32 and a.size == 1000 and a.nbytes <= bench.DUMP_CAP_BYTES
    assert np.array_equal(a, b) and (np.diff(a) > 0).all() and len(np.unique(a)) == a.size
