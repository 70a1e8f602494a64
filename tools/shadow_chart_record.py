"""Writes tests/golden/shadow_chart.json, the record of the shadow chart (tests/shadow_chart.py): for every chart x light x map
side the census (pixels on each boundary of the shadow test's comparisons, pixels whose map texel is within one ulp of their
own depth, pixels per cube face, quads of mixed faces, the model's classes) and the number of classes every model mutant changes
at every bias, on the oracle's maps (CPU only).  tests/test_shadow_chart.py compares the chart with it.

  python tools/shadow_chart_record.py"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
PATH = os.path.join(ROOT, "tests", "golden", "shadow_chart.json")


if __name__ == "__main__":
    from test_shadow_chart import measured
    with open(PATH, "w") as f:
        json.dump(measured(), f, indent=1)
        f.write("\n")
