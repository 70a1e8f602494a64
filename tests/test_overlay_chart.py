"""The oracle's overlay subpass (bbo_overlay: light markers + corner gizmo) against tests/overlay_chart.py, a model written
from the Vulkan rules and the four shader files and evaluated by the exact rasteriser of tests/raster_reference.py.

  1  on every pixel the model decides, the oracle's image is the model's: unchanged pixels are the presented base, changed ones
     carry a byte whose linear interval is within the derived tolerance of the exact colour; at most 1 % of a frame is undecided
  2  the census: every class of every case has the pixels it exists for (overlay_chart.CLASSES), printed with -s
  3  properties that need no model: hostile lights change nothing for the others, NumLights is clamped to 0..100, 99 lights at
     one position leave the last one's colour
  4  the refactored raster_reference.rasterise returns what it returned before (digest recorded before the refactoring)

Measured (recorded in tests/golden/overlay_chart.json by `python tests/test_overlay_chart.py --write`): per case the largest
colour error / tolerance and the undecided pixels."""
import hashlib
import json
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
if __name__ == "__main__":   # run as a script (--write): what tests/conftest.py does for pytest
    sys.path.insert(0, os.path.dirname(HERE))

from oracle import bbo, scenes
import overlay_chart as OC
import raster_reference as RR

RECORD = os.path.join(HERE, "golden", "overlay_chart.json")
_measured = {}


@pytest.mark.parametrize("name", OC.modelled())
def test_1_oracle_is_the_model_on_every_decided_pixel(name):
    o = OC.oracle_frame(name)
    ratio = OC.check_image(name, o.want, o.base, "oracle, ")
    mo = OC.model(name)
    _measured[name] = {"colour_ratio": round(ratio, 4), "undecided": int((mo.kind == OC.UNDECIDED).sum())}
    print(f"\n{name}: colour error / tolerance {ratio:.4f}, undecided {_measured[name]['undecided']} of {OC.W * OC.H}")
    assert ratio <= 1.0


@pytest.mark.parametrize("name", OC.modelled())
def test_2_census(name):
    c = OC.census(name)
    print(f"\n{name}:")
    for cls, n in c.items():
        print(f"    {cls:18s} {n}")
    assert c["frame"]["undecided"] <= OC.MAX_UNDECIDED * OC.W * OC.H


def test_2_every_class_is_in_a_case():
    seen = {cls for c in OC.cases().values() for cls in c.classes}
    assert seen == set(OC.CLASSES), seen ^ set(OC.CLASSES)
    extents = {c.extent for c in OC.cases().values() if c.gizmo}
    assert {1, 33, 100, 150, 200} <= extents
    assert {c.view for c in OC.cases().values() if c.gizmo == "reference"} == set(OC.VIEWS)


def test_3_hostile_lights_leave_the_others_alone():
    o, c = OC.oracle_frame("nonfinite"), OC.cases()["nonfinite"]
    finite = [l for i, l in enumerate(c.lights) if i not in c.classes["nonfinite"]]
    alone, _ = bbo.overlay(scenes.frame_uniforms(finite), o.scene.view, o.depth, o.base)
    assert np.array_equal(alone, o.want) and (o.want != o.base).any()


def test_3_num_lights_is_clamped():
    o = {n: OC.oracle_frame(f"count {n}") for n in (0, -4, 100, 250)}
    assert np.array_equal(o[0].want, o[0].base) and np.array_equal(o[-4].want, o[-4].base)
    assert o[0].stats["n_prims"] == o[-4].stats["n_prims"] == 0
    assert o[100].stats["n_prims"] == o[250].stats["n_prims"] == 100 * 480
    assert np.array_equal(o[100].want, o[250].want) and (o[100].want != o[100].base).any()


def test_3_ninety_nine_lights_at_one_position_show_the_last():
    o, c = OC.oracle_frame("many"), OC.cases()["many"]
    assert o.stats["n_prims"] == 99 * 480
    changed = (o.want != o.base).any(-1)
    last = bbo.present(np.array([[*c.lights[-1]["color"], 1.0]], np.float32), 0, 1.0, hdr16=False)[0]
    assert changed.sum() > 150 and (o.want[changed] == last).all()


def digest(res):
    h = hashlib.sha256()
    for a in (res.winner, res.decided, res.depth, res.depth_tol, res.uv, res.uv_tol):
        h.update(np.ascontiguousarray(a).tobytes())
    return h.hexdigest()


def test_4_refactored_rasterise_returns_what_it_returned():
    from test_raster_reference import soup_scene
    res = RR.rasterise(soup_scene(333, 207, 1))
    assert digest(res) == json.load(open(RECORD))["rasterise soup 333x207 before the refactoring"]
    assert res.not_all_in > 0 and (res.winner != RR.NONE).sum() > 1000


def _write_record():
    rec = json.load(open(RECORD)) if os.path.exists(RECORD) else {}
    for name in OC.modelled():
        test_1_oracle_is_the_model_on_every_decided_pixel(name)
    rec["oracle against the model"] = _measured
    json.dump(rec, open(RECORD, "w"), indent=1, sort_keys=True)
    print("wrote", RECORD)


if __name__ == "__main__":
    if "--write" in sys.argv:
        bbo.build()
        _write_record()
