"""bench.py's plain run (no --full): the line of the headline figure, --steps timed steps, and --dump-outputs writing the frame
of the last timed step -- the frame the same workload renders through the library directly, bit for bit."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from bibim_renderer_amd import Renderer, configs, textures
from bibim_renderer_amd import scene as S

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bench(*args):
    p = subprocess.run([sys.executable, "bench.py", "--gpus", "1"] + list(args), cwd=ROOT, capture_output=True, text=True,
                       timeout=600)
    assert p.returncode == 0, p.stderr[-3000:]
    lines = [l for l in p.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, p.stdout[-2000:]
    return json.loads(lines[0])


def _direct_frame(workload):
    cfg = configs.CONFIGS[workload]
    r = Renderer(cfg.width, cfg.height)
    material = r.upload_material(textures.make_material(cfg.texture_size))
    scene, cam, settings = S.config_scene(r, cfg, S.load_shaderball_vertices())
    S.draw_frame(r, scene, cam, settings, material)
    frame = r.read_framebuffer()
    scene.close(); r.close()
    return frame


def _plain_line(d, steps, warmup, width, height):
    for k in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step"):
        assert k in d, k
    assert d["steps"] == steps and d["warmup"] == warmup and d["unit"] == "Mpixels/s" and d["higher_is_better"] is True
    assert d["dtype"] == "f32" and d["ms_per_step"] > 0
    assert abs(d["value"] - width * height / (d["ms_per_step"] * 1e-3) / 1e6) / d["value"] < 1e-3
    assert d["roofline"] is None and d["cpu_baseline"] is None and "also" not in d and "parity_vs_oracle" not in d


def test_plain_run_dumps_the_whole_1080p_frame(tmp_path):
    d = _bench("--workload", "c2", "--steps", "7", "--warmup", "3", "--dump-outputs", str(tmp_path))
    _plain_line(d, 7, 3, 1920, 1080)
    assert sorted(os.listdir(tmp_path)) == ["frame.npy"]
    got = np.load(tmp_path / "frame.npy")
    assert got.dtype == np.float32 and got.shape == (1080, 1920, 4)
    # (the scene is static: every step renders this frame, so this shows the dump is a correct frame of the workload, not
    #  that it came from the last timed step rather than another frame slot)
    assert np.array_equal(got.view(np.uint32), _direct_frame("c2").view(np.uint32))


def test_plain_run_dumps_a_fixed_sample_of_the_4k_frame(tmp_path):
    d = _bench("--steps", "5", "--warmup", "2", "--dump-outputs", str(tmp_path))
    _plain_line(d, 5, 2, 3840, 2160)
    assert sorted(os.listdir(tmp_path)) == ["frame_sample.npy", "sample_pixels.npy"]
    assert sum(os.path.getsize(tmp_path / n) for n in os.listdir(tmp_path)) <= 64e6
    idx = np.load(tmp_path / "sample_pixels.npy").astype(np.int64)
    got = np.load(tmp_path / "frame_sample.npy")
    assert got.dtype == np.float32 and got.shape == (idx.size, 4)
    want = _direct_frame("c3").reshape(-1, 4)[idx]
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
