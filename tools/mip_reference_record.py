"""Rewrites tests/golden/mip_reference.json: a record (not a test bound) of how far the level rule of option "mip_levels"
stands from lambda = 1/2 log2 P on frames the GPU rendered.  Needs a GPU.

  python tools/mip_reference_record.py [--out PATH]

Population: every covered pixel of the perspective quad of tests/test_gpu_aniso.py (scene Q: footprints of every tap count)
and of the three scenes of tests/mip_reference.py, 64^2 maps, both passes, max_anisotropy 1 and 16, mip_levels 15, whose
level was chosen by the rule's live branch (finite differences, P > 1, not clamped to the last level).  P is recomputed
in binary64 from the dumped differences and the dumped tap count; d + delta is what the kernel dumped in slots 28 / 29."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
PATH = os.path.join(ROOT, "tests", "golden", "mip_reference.json")


def main(out):
    import mip_reference as M
    import test_gpu_aniso as GA
    import torch
    from bibim_renderer_amd import Renderer
    device = torch.cuda.get_device_name(0)
    w = h = 64
    levels = M.level_count(w, h, 15)
    cases = [("Q", GA.scene("Q"))] + [(name, M.scene(name, (M.maps64(),))) for name in M.SCENES]
    low = high = 0.0
    pixels = 0
    mean_d = {}
    for name, sc in cases:
        for deferred in (0, 1):
            for max_aniso in (1, 16):
                r = Renderer(sc.width, sc.height)
                for k, v in (("render_pass", deferred), ("max_anisotropy", max_aniso), ("mip_levels", 15)):
                    r.set_option(k, v)
                r.render_scene(sc)
                surf = r.read_surface()
                r.close()
                rec = surf[surf[..., 22] > 0].astype(np.float64)
                mean_d[f"{name} pass {deferred} max_anisotropy {max_aniso}"] = round(float((rec[:, 28] + rec[:, 29]).mean()), 4)
                with np.errstate(all="ignore"):
                    px2 = (rec[:, 2] * w) ** 2 + (rec[:, 3] * h) ** 2
                    py2 = (rec[:, 4] * w) ** 2 + (rec[:, 5] * h) ** 2
                    P = np.maximum(px2, py2) / rec[:, 22] ** 2
                    live = np.isfinite(rec[:, 2:6]).all(1) & (P > 1.0 + 1e-5) & (rec[:, 28] < levels - 1)
                    err = 0.5 * np.log2(P[live]) - (rec[live, 28] + rec[live, 29])
                if len(err):
                    low, high, pixels = max(low, float(err.max())), max(high, float(-err.min())), pixels + len(err)
    rec = {"rule": "d + delta against 1/2 log2 P (binary64, from the dumped differences and tap count)",
           "derived_bound_low": M.LEVEL_BOUND, "gpu": {"worst_low": low, "worst_high": high, "pixels": pixels,
                                                       "mean_d_plus_delta": mean_d, "device": device}}
    with open(out, "w") as f:
        json.dump(rec, f, indent=1)
        f.write("\n")
    print(json.dumps(rec["gpu"]))


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=PATH)
    main(ap.parse_args().out)
