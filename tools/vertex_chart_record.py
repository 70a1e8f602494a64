"""Rewrites tests/golden/vertex_chart.json, the record of the vertex chart (tests/vertex_chart.py).

  python tools/vertex_chart_record.py                 seeds, the census of visible primitives per category and pass, the
                                                      oracle's worst error / bound per instance class and pass (CPU only)
  python tools/vertex_chart_record.py --gpu-log LOG   also the `gpu` block, from the output of
                                                      python -m pytest tests/test_gpu_vertex_chart.py -m gpu -q -s > LOG
                                                      (the lines "records <view> <pass> tile_mode <m>: ..." and the closing
                                                      "N passed in T s")
A `gpu` block that is not rewritten is kept as it stands."""
import argparse
import json
import os
import re
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
PATH = os.path.join(ROOT, "tests", "golden", "vertex_chart.json")


def oracle_side():
    import vertex_chart as VC
    worst, left_out = VC.oracle_worst()
    return {"seeds": VC.SEEDS, "frame": [VC.W, VC.H], "primitives": len(VC.plan().cells),
            "census": {"forward": VC.census(0), "deferred": VC.census(1)},
            "oracle": {"worst_error_over_bound": {k: round(v, 4) for k, v in worst.items()}, "share_left_out": round(left_out, 4),
                       "population": "the cells whose six squared lengths are normal numbers, bbo.vertex_stage against the GLSL in binary64"}}


def gpu_side(log):
    text = open(log).read()
    lines = re.findall(r"records (\w+) (forward|deferred) tile_mode (\d): (\d+) inspected, (\d+) unclipped, (\d+) clipped", text)
    done = re.search(r"(\d+) passed[^\n]* in ([0-9.]+)s", text)
    if len(lines) != 8 or not done or " failed" in text.splitlines()[-1]:
        raise SystemExit(f"{log}: not the output of a passing run with -s")
    return {"records": {f"{v} {p} tile_mode {m}": {"inspected": int(i), "unclipped": int(u), "clipped": int(c)} for v, p, m, i, u, c in lines},
            "tests": int(done.group(1)), "wall_time_s": float(done.group(2)),
            "population": "every record bbr_read_records returns for a primitive that wins a pixel, survives or is clipped, MI355X"}


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpu-log")
    a = ap.parse_args()
    rec = json.load(open(PATH)) if os.path.exists(PATH) else {}
    rec.update(oracle_side())
    if a.gpu_log:
        rec["gpu"] = gpu_side(a.gpu_log)
    with open(PATH, "w") as f:
        json.dump(rec, f, indent=1)
        f.write("\n")
