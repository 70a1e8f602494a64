"""Rewrites tests/golden/surface_chart.json, the record of the surface charts (tests/surface_chart.py).

  python tools/surface_chart_record.py                 seeds, census counts and the oracle's worst error / bound (CPU only)
  python tools/surface_chart_record.py --gpu-log LOG   also the `gpu` block, from the output of
                                                       python -m pytest tests/test_gpu_surface_chart.py -m gpu -q -s > LOG
                                                       (the lines "3: <chart> <pass>: ..." and the closing "N passed in T s")
A `gpu` block that is not rewritten is kept as it stands."""
import argparse
import json
import os
import re
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
PATH = os.path.join(ROOT, "tests", "golden", "surface_chart.json")
CENSUS_KEYS = {"a": ["roughness_0", "ndv_negative", "ndl_negative_some_light"], "d": ["d2_denormal", "d2_normal"],
               "e": ["d2_finite", "d2_overflows"], "g unknown first": ["roughness_0", "ndv_negative", "ndl_negative_some_light"]}


def oracle_side():
    import surface_chart as SC
    from test_oracle_contract import BOUND_EPS, conditioning, glsl_f64_light_loop, rel_err
    from test_surface_chart import static_case
    from oracle import bbo
    census, worst = {}, {}
    for name in SC.CHARTS:
        for case, keys in CENSUS_KEYS.items():
            sc, lights, view, s = static_case(case, name)
            c = SC.census(SC.model_surface(sc, bbo.render(sc)[1], s), lights, view)
            census[f"{name} {case}"] = {k: (np.round(c[k], 4).tolist() if isinstance(c[k], list) else round(c[k], 4)) for k in keys}
        sc, lights, view, _ = static_case("a", name)
        surf = SC.f32(SC.model_surface(sc, bbo.render(sc)[1]))
        args = SC.glsl_args(lights, view, surf)
        want = glsl_f64_light_loop(*args)
        bound = 1e-5 + BOUND_EPS / conditioning(args[0], args[1], args[2], args[3], args[6])
        worst[name] = round(max(float((rel_err(bbo.light_surface(sc.frame, sc.view, surf, literal=lit)[:, :3].astype(np.float64), want)
                                       / bound).max()) for lit in (True, False)), 4)
    return {"seeds": SC.SEEDS, "frame": [SC.W, SC.H], "census": census,
            "oracle": {"worst_error_over_bound": worst,
                       "population": "the charts' surface modelled in binary64 (surface_chart.model_surface), set a, literal and contract form"}}


def gpu_side(log):
    text = open(log).read()
    lines = re.findall(r"3: (\w+) (forward|deferred): .*?worst well-conditioned error ([0-9.e+-]+), worst error / bound ([0-9.e+-]+)", text)
    done = re.search(r"(\d+) passed in ([0-9.]+)s", text)
    if len(lines) != 8 or not done or " failed" in text.splitlines()[-1]:
        raise SystemExit(f"{log}: not the output of a passing run with -s")
    return {"worst_error_over_bound": {f"{n} {p}": float(w) for n, p, _, w in lines},
            "worst_well_conditioned_error": max(float(e) for _, _, e, _ in lines), "tests": int(done.group(1)),
            "wall_time_s": float(done.group(2)),
            "population": "the inputs the kernel dumped (bbr_read_surface / bbr_read_gbuffer), set a, MI355X"}


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpu-log")
    a = ap.parse_args()
    rec = json.load(open(PATH)) if os.path.exists(PATH) else {}
    rec.update(oracle_side())
    if a.gpu_log:
        rec["gpu"] = {**{k: v for k, v in rec.get("gpu", {}).items() if k.startswith(("whole_", "test_gpu_parity"))}, **gpu_side(a.gpu_log)}
    with open(PATH, "w") as f:
        json.dump(rec, f, indent=1)
        f.write("\n")
