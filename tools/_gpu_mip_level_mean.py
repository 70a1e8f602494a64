"""Diagnostic: mean level of detail per shaded pixel of a workload under option "mip_levels" (bbr_read_surface slots 28 / 29:
d and delta of the packed set), for each max_anisotropy given.  usage: _gpu_mip_level_mean.py workload [max_anisotropy ...]"""
import os, sys
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from bibim_renderer_amd import configs, textures, Renderer
from bibim_renderer_amd import scene as S
cfg = configs.CONFIGS[sys.argv[1]]
r = Renderer(cfg.width, cfg.height)
r.set_option("mip_levels", 15)
material = r.upload_material(textures.make_material(cfg.texture_size))
scene, cam, settings = S.config_scene(r, cfg)
for aniso in [int(x) for x in sys.argv[2:]] or [1, 16]:
    r.set_option("max_anisotropy", aniso)
    S.draw_frame(r, scene, cam, settings, material)
    s = r.read_surface().reshape(-1, 32)
    at = np.flatnonzero(s[:, 22] > 0)
    d, delta, n = s[at, 28].astype(np.float64), s[at, 29].astype(np.float64), s[at, 22].astype(np.float64)
    hist = np.bincount(d.astype(np.int64), minlength=12)
    print(f"{sys.argv[1]} mip_levels=15 max_anisotropy={aniso}: {len(at)} shaded pixels, mean d {d.mean():.3f}, mean d + delta {(d + delta).mean():.3f}, "
          f"delta != 0 on {(delta != 0).mean():.3f}, mean taps {n.mean():.2f}, pixels per level {hist.tolist()}", flush=True)
    del s
scene.close(); r.close()
