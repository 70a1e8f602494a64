"""What option "shadow_map" costs (profiles/shadow_map.txt): the C3 scene, light 0 the caster, a 120 degree frustum from the light
towards the middle of the ball grid.

  the synchronous pass alone   bbr_render_shadow_map at side S, wall time per call (the call drains, uploads the draws, runs
                               k_geometry and k_raster at S x S, and waits)
  the pipelined frame          three frames in flight, frame period with the map in use, beside the same tree's default frame
                               (k_shade) and its max_anisotropy = 2 frame (k_shade_aniso, the neighbour k_shade_shadow is built on)

Every case runs in a process of its own under a time limit; the first case that fails ends the run.
usage: shadow_map_cost.py [--reps 3] [--frames 300] [--side 2048] [--out FILE]"""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

CHILD = r'''
import sys, time, gc, json
import ctypes as C
import numpy as np
sys.path.insert(0, %(root)r)
from bibim_renderer_amd import configs, textures, Renderer
from bibim_renderer_amd._capi import lib
from bibim_renderer_amd import scene as S
SIDE, ANISO, REPS, FRAMES, CALLS = %(side)d, %(aniso)d, %(reps)d, %(frames)d, %(calls)d
cfg = configs.C3
r = Renderer(cfg.width, cfg.height)
r.set_option("frames_in_flight", 3)
r.set_option("max_anisotropy", ANISO)
r.set_option("shadow_map", SIDE)
material = r.upload_material(textures.make_material(cfg.texture_size))
scene, cam, settings = S.config_scene(r, cfg)
frame = S.frame_call(r, scene, cam, settings, material)
frame(); r.synchronize()                      # the first frame sizes the capacities
out = dict(pass_us=[], classes=[])
if SIDE:
    light = np.zeros(144, np.uint8)
    view, proj = np.zeros((4, 4), np.float32), np.zeros((4, 4), np.float32)
    p = lambda a: np.asarray(a, np.float32).ctypes.data_as(C.c_void_p)
    eye, target, up = np.asarray(cfg.lights[0].pos, np.float32), np.asarray((0.0, -1.0, 5.0), np.float32), np.asarray((0.0, 1.0, 0.0), np.float32)
    lib().bbs_mat4_look_at(p(eye), p(target), p(up), p(view))
    lib().bbs_mat4_perspective(120.0, 1.0, 0.1, 1000.0, p(proj))
    light[:64], light[64:128] = view.view(np.uint8).ravel(), proj.view(np.uint8).ravel()
    r.render_shadow_map(0, light, 2.0 ** -10)     # (may grow a capacity: not timed)
    for rep in range(REPS):
        t0 = time.perf_counter()
        for _ in range(CALLS): r.render_shadow_map(0, light, 2.0 ** -10)
        out["pass_us"].append((time.perf_counter() - t0) / CALLS * 1e6)
    frame(); r.synchronize()
    out["classes"] = (np.bincount(r.read_shadow_mask().ravel(), minlength=4) / float(cfg.width * cfg.height)).tolist()
    out["map_covered"] = float((r.read_shadow_map() != 0).mean())
gc.collect(); gc.disable()
for _ in range(60): frame()
r.synchronize()
out["period_us"] = []
for rep in range(REPS):
    for _ in range(10): frame()
    t0 = time.perf_counter()
    for _ in range(FRAMES): frame()
    r.synchronize()
    out["period_us"].append((time.perf_counter() - t0) / FRAMES * 1e6)
print("RESULT", json.dumps(out), flush=True)
scene.close(); r.close()
'''


def run(tag, **kw):
    args = dict(root=ROOT, side=0, aniso=1, calls=20)
    args.update(kw)
    p = subprocess.run([sys.executable, "-c", CHILD % args], capture_output=True, text=True, timeout=240)
    if p.returncode:
        raise SystemExit(f"{tag}: FAILED rc={p.returncode}\n{p.stderr[-2000:]}")
    line = [l for l in p.stdout.splitlines() if l.startswith("RESULT ")][-1]
    return json.loads(line[7:])


def fmt(xs):
    return " ".join(f"{x:8.1f}" for x in xs)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--frames", type=int, default=300)
    ap.add_argument("--side", type=int, default=2048)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    common = dict(reps=a.reps, frames=a.frames)
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    say(f"# C3 scene (3840 x 2160), three frames in flight: frame period, us per frame ({a.frames} frames between two synchronisations, {a.reps} runs)")
    say(f"default (k_shade)                                  {fmt(run('default', **common)['period_us'])}")
    say(f"max_anisotropy 2 (k_shade_aniso)                   {fmt(run('aniso 2', aniso=2, **common)['period_us'])}")
    s = run("shadow", side=a.side, **common)
    say(f"shadow_map {a.side:<5d} (k_shade_shadow)                {fmt(s['period_us'])}")
    s2 = run("shadow + aniso 2", side=a.side, aniso=2, **common)
    say(f"shadow_map {a.side:<5d} + max_anisotropy 2              {fmt(s2['period_us'])}")
    say(f"# the frame's pixels by class (not covered, lit, shadowed, outside): {' '.join('%.3f' % x for x in s['classes'])}; covered texels of the map: {s['map_covered']:.3f}")
    say()
    say(f"# bbr_render_shadow_map alone, side {a.side}: wall time per call, us (20 calls back to back, {a.reps} runs)")
    say(f"the synchronous pass                               {fmt(s['pass_us'])}")
    small = run("shadow 256", side=256, **common)
    say(f"the same at side 256 (the call's fixed part)       {fmt(small['pass_us'])}")
    if a.out:
        with open(a.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
