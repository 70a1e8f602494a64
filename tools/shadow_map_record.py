"""Rewrites the `census` block of tests/golden/shadow_map.json, the record of the shadow scenes (tests/shadow_scenes.py): for
every kind x map side >= 33 the shares of LIT, SHADOWED and OUTSIDE pixels a factor 2 clear of their thresholds at bias 2^-8, the
pixels behind the light, and at bias 0 the pixels whose map texel is their own depth -- all on the oracle's maps (CPU only).

  python tools/shadow_map_record.py

Other blocks of the file are kept as they stand."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
PATH = os.path.join(ROOT, "tests", "golden", "shadow_map.json")


def census():
    import shadow_scenes as SS
    from test_shadow_reference import SIDES, census_pair
    out = {}
    for kind in SS.KINDS:
        for side in SIDES:
            c_bias, c_zero = census_pair(kind, side)
            SS.check_census(kind, side, c_bias, c_zero)
            out[f"{kind} {side}"] = {"bias": {k: round(v, 4) for k, v in c_bias.items()},
                                     "zero": {k: round(v, 4) for k, v in c_zero.items()}}
    return {"frame": list(SS.FRAME_SMALL), "sides": list(SS.SIDES), "biases": list(SS.BIASES), "caster": SS.CASTER,
            "minima": {"share": SS.MIN_SHARE, "behind": SS.MIN_BEHIND, "self": SS.MIN_SELF}, "census": out}


if __name__ == "__main__":
    rec = json.load(open(PATH)) if os.path.exists(PATH) else {}
    rec.update(census())
    with open(PATH, "w") as f:
        json.dump(rec, f, indent=1)
        f.write("\n")
