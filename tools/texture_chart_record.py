"""Rewrites tests/golden/texture_chart.json, the record of the texture charts (tests/texture_chart.py).

  python tools/texture_chart_record.py                 seeds, layouts, census counts per layout and point chart (on the oracle's
                                                       FLAG_OUTPUT_UV frame) and the oracle's and the model's worst error /
                                                       tolerance against binary64 per layout (CPU only)
  python tools/texture_chart_record.py --gpu-log LOG   also the `gpu` block, from the output of
                                                       python -m pytest tests/test_gpu_texture_chart.py tests/test_gpu_aniso.py -m gpu -q -s --durations=0 > LOG
                                                       (the lines "5: <layout> | <chart> | <pass>: ...", the durations and the closing "N passed in T s")
A `gpu` block that is not rewritten is kept as it stands."""
import argparse
import json
import os
import re
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
PATH = os.path.join(ROOT, "tests", "golden", "texture_chart.json")


def cpu_side():
    import aniso_reference as A
    import texture_chart as TC
    from test_oracle_contract import np_bilinear
    from test_texture_chart import all_pairs, oracle_sample
    from oracle import bbo
    census, model, oracle = {}, {}, {}
    for layout in TC.LAYOUTS:
        for chart in TC.POINT_CHARTS:
            uv = bbo.render(TC.scene(layout, chart), flags=bbo.FLAG_OUTPUT_UV)[0][..., :2]
            census[f"{layout} {chart}"] = TC.check_census(layout, chart, uv)
        uv = all_pairs(layout)
        fp = np.concatenate([uv, np.zeros((len(uv), 4), np.float32)], 1)
        wm = wo = 0.0
        for maps in TC.materials(layout):
            wm = max(wm, TC.check_values(maps, uv, A.filter_maps(maps, fp, 1, True, 1), True, np_bilinear, layout))
            got = np.zeros((len(uv), 10), np.float32)
            for name, col, chans in TC.COLUMNS:
                t = oracle_sample(A.texture_of(maps.get(name), name), name, uv)[:, :len(chans)]
                got[:, col:col + len(chans)] = A.fmaf(t, np.float32(2.0), np.float32(-1.0)) if name == "normal" else t
            wo = max(wo, TC.check_values(maps, uv, got, True, np_bilinear, layout))
        model[layout], oracle[layout] = round(wm, 4), round(wo, 4)
    return {"seeds": TC.SEEDS, "frame": [TC.W, TC.H], "layouts": TC.LAYOUTS, "minimums": {"class": TC.MIN_CLASS, "pair": TC.MIN_PAIR},
            "census": census,
            "model": {"worst_error_over_tolerance": model, "population": "every planted pair as it arrives on flat and steep, one tap"},
            "oracle": {"worst_error_over_tolerance": oracle, "population": "the same pairs through bbo_sample, one call each"},
            "tolerance": "4 eps32 (1 + max(|u| w, |v| h)) + 1e-7 where both |u| w and |v| h are below 2^20"}


def gpu_side(log):
    text = open(log).read()
    lines = re.findall(r"(?:^|[.FEsx])5: (.+?) \| (\w+) \| (forward|deferred): worst error / tolerance against binary64 ([0-9.e+-]+)", text, flags=re.M)
    # (under -q a test's output follows the progress dot of the test before it on the same line)
    done = re.search(r"(\d+) passed.* in ([0-9.]+)s", text)
    if not lines or not done or " failed" in done.group(0):
        raise SystemExit(f"{log}: not the output of a passing run with -s")
    worst = {}
    for layout, chart, p, w in lines:
        k = f"{layout} {p}"
        worst[k] = max(worst.get(k, 0.0), float(w))
    wall = {"test_gpu_texture_chart.py": 0.0, "test_gpu_aniso.py": 0.0}
    count = dict.fromkeys(wall, 0)
    for secs, phase, test in re.findall(r"^([0-9.]+)s (call|setup|teardown)\s+tests/(\S+?)::", text, flags=re.M):
        if test in wall:
            wall[test] += float(secs)
            count[test] += phase == "call"
    return {"worst_error_over_tolerance": worst, "tests": count["test_gpu_texture_chart.py"],
            "wall_time_s": {k: round(v, 2) for k, v in wall.items()}, "tests_of_test_gpu_aniso": count["test_gpu_aniso.py"],
            "whole_call": {"passed": int(done.group(1)), "wall_time_s": float(done.group(2))},
            "population": "the values the kernel dumped (bbr_read_surface) at max_anisotropy 1, every chart, MI355X"}


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpu-log")
    a = ap.parse_args()
    rec = json.load(open(PATH)) if os.path.exists(PATH) else {}
    rec.update(cpu_side())
    if a.gpu_log:
        rec["gpu"] = gpu_side(a.gpu_log)
    with open(PATH, "w") as f:
        json.dump(rec, f, indent=1)
        f.write("\n")
