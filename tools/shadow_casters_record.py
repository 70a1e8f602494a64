"""Writes tests/golden/shadow_casters.json, the record of the casters scenes (tests/shadow_casters_scenes.py): for every kind x
frame size x map side the census of tests/shadow_casters_scenes.census -- shares and counts of pixels a factor 2 clear of their
thresholds, in binary64 on the oracle's maps (CPU only).

  python tools/shadow_casters_record.py"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
PATH = os.path.join(ROOT, "tests", "golden", "shadow_casters.json")


def record():
    import shadow_casters_scenes as CS
    from test_shadow_casters_reference import recorded
    out = {}
    for kind in CS.KINDS:
        for size in (CS.FRAME_SMALL, CS.FRAME_DUMP):
            for side in CS.SIDES:
                c = CS.census(kind, side, size)
                CS.check_census(kind, c, side)
                out[f"{kind} {size[0]}x{size[1]} {side}"] = recorded(kind, c)
    return {"sides": list(CS.SIDES), "bias": CS.BIAS, "blocks": [list(b) for b in CS.BLOCKS],
            "casters": {kind: [[c["slot"], c["light"], len(c["views"])] for c in CS.casters(kind)] for kind in CS.KINDS},
            "minima": {"share": CS.MIN_SHARE, "both": CS.MIN_BOTH, "pair": CS.MIN_PAIR, "partial_both": CS.MIN_PARTIAL_BOTH,
                       "eight": CS.MIN_EIGHT, "partial_side_max": CS.PARTIAL_SIDE_MAX},
            "census": out}


if __name__ == "__main__":
    with open(PATH, "w") as f:
        json.dump(record(), f, indent=1)
        f.write("\n")
