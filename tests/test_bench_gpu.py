"""A plain `python bench.py` run (no --full) times the headline steps and nothing else; --dump-outputs writes the latent the last timed
step left, and two runs with the same arguments write the same bytes (the path has no atomics: run-to-run bitwise determinism)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bench(out_dir, steps):
    env = dict(os.environ)
    for k in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_PORT"):
        env.pop(k, None)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", str(steps), "--warmup", "1",
                        "--latent", "16x16", "--frames", "4", "--dump-outputs", str(out_dir)],
                       cwd=ROOT, env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    return json.loads(lines[0])


@pytest.mark.gpu
def test_plain_bench_dumps_the_last_step_and_repeats_it_exactly(tmp_path):
    a = _bench(tmp_path / "a", 3)
    b = _bench(tmp_path / "b", 3)
    for d in (a, b):
        assert d["steps"] == 3 and d["warmup"] == 1 and d["finite"] and d["unit"] == "denoise-steps/s" and d["higher_is_better"]
        assert abs(d["value"] - 1000.0 / d["ms_per_step"]) < 1e-2 * d["value"]
        # nothing beyond the headline ran
        for k in ("roofline", "reference_shape", "prompt_batch", "sample_24view", "clip_towers", "lgm_refined_sample", "i2vgen",
                  "frame_parallel", "simulated_rank", "cpu_baseline"):
            assert d[k] is None, k
    assert sorted(os.listdir(tmp_path / "a")) == ["latent.npy"]
    xa, xb = np.load(tmp_path / "a" / "latent.npy"), np.load(tmp_path / "b" / "latent.npy")
    assert xa.dtype == np.float32 and xa.shape == (1, 4, 4, 16, 16) and np.isfinite(xa).all()
    assert np.array_equal(xa, xb)
    # the dump is the last TIMED step's result: one more step gives another latent
    c = _bench(tmp_path / "c", 4)
    assert c["steps"] == 4 and not np.array_equal(np.load(tmp_path / "c" / "latent.npy"), xa)
