"""What a shadow caster that moves every frame costs (profiles/shadow_queue.txt): the C3 scene at 3840 x 2160, three frames in
flight, light 0 the caster, its view blocks new every frame (bb::cubeShadowViews at a position that moves on a small circle).

  arm "queue"   bbr_queue_shadow_caster inside every frame
  arm "sync"    bbr_render_shadow_caster directly in front of every bbr_end_frame (the only form an older tree has: --root)
  arm "static"  the maps rendered once, then plain frames

Per arm: us per frame over --frames timed frames between two synchronisations (after --warmup frames), --reps times, and
bbr_host_timing's submit and blocked time per frame over the timed frames; arm "queue" also bbr_shadow_queue_counts.  The frames
are recorded through the Python binding (begin_frame, two draws, the call, end_frame), the same way in every arm.
Every case runs in a process of its own under a time limit; the first case that fails ends the run.

usage: shadow_queue_cost.py [--root TREE] [--arms queue,sync,static] [--cases 2048x1x0,...] [--reps 3] [--frames 200] [--warmup 60] [--out FILE]"""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

CHILD = r'''
import sys, time, gc, json, math
import numpy as np
sys.path.insert(0, %(oracle_root)r)
sys.path.insert(0, %(root)r)
from bibim_renderer_amd import configs, textures, Renderer
from bibim_renderer_amd import scene as S
from oracle import bbo, scenes
ARM, SIDE, FACES, RADIUS, REPS, FRAMES, WARMUP = %(arm)r, %(side)d, %(faces)d, %(radius)d, %(reps)d, %(frames)d, %(warmup)d
cfg = configs.C3
r = Renderer(cfg.width, cfg.height)
r.set_option("frames_in_flight", 3)
r.set_option("shadow_map", SIDE)
r.set_option("shadow_filter", RADIUS)
sc = scenes.shaderball_scene(cfg, bbo.MaterialData(textures.make_material(cfg.texture_size)))
h = r.render_scene(sc); r.synchronize()          # the first frame sizes the capacities
draws = [(h["mesh"][id(d.vertices)], h["mat"][id(d.material)], d.instances) for d in sc.draws]
p0 = np.asarray(cfg.lights[0].pos, np.float64)
views = [np.ascontiguousarray(S.cube_shadow_views(p0 + 0.25 * np.array([math.cos(k * math.pi / 8), 0.0, math.sin(k * math.pi / 8)]), 96.0, 0.1, 1000.0)[:FACES])
         for k in range(16)]
BIAS = 2.0 ** -10
r.render_shadow_caster(0, 0, views[0], BIAS)      # (may grow a capacity: not timed)
cast = {"queue": getattr(r, "queue_shadow_caster", None), "sync": r.render_shadow_caster, "static": None}[ARM]
def frame(k):
    r.begin_frame()
    for mesh, mat, inst in draws: r.draw(mesh, mat, inst)
    if cast: cast(0, 0, views[k %% 16], BIAS)
    r.end_frame()
r.set_frame_uniforms(sc.frame); r.set_view_uniforms(sc.view)
gc.collect(); gc.disable()
for k in range(WARMUP): frame(k)
r.synchronize()
out = dict(period_us=[], submit_us=[], blocked_us=[])
for rep in range(REPS):
    for k in range(10): frame(k)
    r.synchronize(); r.host_timing_reset()
    t0 = time.perf_counter()
    for k in range(FRAMES): frame(k)
    r.synchronize()
    out["period_us"].append((time.perf_counter() - t0) / FRAMES * 1e6)
    ht = r.host_timing()
    out["submit_us"].append(ht["submit_ns"] / max(ht["frames"], 1) / 1e3)
    out["blocked_us"].append(ht["blocked_ns"] / max(ht["frames"], 1) / 1e3)
out["counts"] = list(r.shadow_queue_counts()) if hasattr(r, "shadow_queue_counts") else None
print("RESULT", json.dumps(out), flush=True)
r.close()
'''


def run(tag, **kw):
    p = subprocess.run([sys.executable, "-c", CHILD % kw], capture_output=True, text=True, timeout=240)
    if p.returncode:
        raise SystemExit(f"{tag}: FAILED rc={p.returncode}\n{p.stderr[-2000:]}")
    line = [l for l in p.stdout.splitlines() if l.startswith("RESULT ")][-1]
    return json.loads(line[7:])


def fmt(xs):
    return " ".join(f"{x:7.1f}" for x in xs)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--root", default=ROOT, help="the tree whose package and library are measured (the scene data come from this one)")
    ap.add_argument("--arms", default="queue,sync,static")
    ap.add_argument("--cases", default="2048x1x0,2048x1x1,1024x6x0,1024x6x1", help="SxFxR: the side, the faces, the filter radius")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--frames", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=60)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    say(f"# tree {os.path.relpath(a.root, ROOT)}: C3 (3840 x 2160), three frames in flight, light 0 moves every frame; us per frame over {a.frames} frames "
        f"({a.reps} runs) | host submit us per frame | host blocked us per frame | (queued passes, drains)")
    for side, faces, radius in (tuple(int(x) for x in case.split("x")) for case in a.cases.split(",")):
        for arm in a.arms.split(","):
            o = run(f"{arm} S {side} F {faces} R {radius}", root=a.root, oracle_root=ROOT, arm=arm, side=side, faces=faces, radius=radius,
                    reps=a.reps, frames=a.frames, warmup=a.warmup)
            say(f"S {side:4d} F {faces} R {radius} {arm:<6s} {fmt(o['period_us'])} | {fmt(o['submit_us'])} | {fmt(o['blocked_us'])} | {o['counts']}")
    if a.out:
        with open(a.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
