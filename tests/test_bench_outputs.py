"""bench.py --dump-outputs DIR: the frame of the last timed step as DIR/frame.npy (float32), a fixed seeded sample of it beyond the
64 MB budget; and a plain run (no --full) prints the headline line without the separately reported figures."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT

sys.path.insert(0, ROOT)
import bench  # noqa: E402


def test_dump_outputs_writes_float32_within_the_budget(tmp_path):
    a = np.random.default_rng(1).random((30, 40, 3))
    bench.dump_outputs(str(tmp_path / "full"), {"frame": a})
    got = np.load(tmp_path / "full" / "frame.npy")
    assert got.dtype == np.float32 and np.array_equal(got, a.astype(np.float32))
    limit = 4096 + 100 * 12                               # room for 100 pixels of 3 floats
    for d in ("s1", "s2"):
        bench.dump_outputs(str(tmp_path / d), {"frame": a}, limit=limit)
    s1, s2 = np.load(tmp_path / "s1" / "frame_sample.npy"), np.load(tmp_path / "s2" / "frame_sample.npy")
    assert s1.shape == (100, 3) and s1.dtype == np.float32 and np.array_equal(s1, s2)   # the same pixels every run
    assert os.path.getsize(tmp_path / "s1" / "frame_sample.npy") <= limit
    assert not os.path.exists(tmp_path / "s1" / "frame.npy")
    px = a.astype(np.float32).reshape(-1, 3)
    assert all(any(np.array_equal(row, p) for p in px) for row in s1[:5])   # pixels of the frame, not something else


@pytest.mark.gpu
def test_plain_bench_dumps_the_timed_frame(native, renderer, samples, tmp_path):
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1", "--width", "96",
                        "--height", "80", "--dump-outputs", str(tmp_path)], capture_output=True, text=True, timeout=600, env=env)
    assert p.returncode == 0, p.stderr[-2000:]
    lines = [ln for ln in p.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1
    d = json.loads(lines[0])
    assert d["steps"] == 3 and d["warmup"] == 1 and d["ms_per_step"] > 0 and d["value"] > 0 and d["unit"] == "rays/s"
    assert d["dtype"] == "f32" and d["higher_is_better"] is True and "roofline" in d
    assert "cpu_baseline" not in d and not [k for k in d if k.startswith("extra_")]   # those need --full
    frame = np.load(tmp_path / "frame.npy")
    cam = native.camera_from_samples(samples, 96, 80, 64)
    ref = native.render_image(renderer.coarse, renderer.fine, cam, 128, seed=0)
    assert frame.dtype == np.float32 and frame.shape == (80, 96, 3)
    assert np.array_equal(frame, ref)
