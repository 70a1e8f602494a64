"""What option "shadow_filter" costs (profiles/shadow_filter.txt): the C3 scene at 3840 x 2160, light 0 the caster, three frames
in flight, frame period.

  one face    tools/shadow_map_cost.py's 120 degree frustum, S = 2048, with R = 0 (k_shade_shadow), 1 and 2 (k_shade_shadow_pcf:
              9 and 25 taps)
  six faces   tools/shadow_faces_cost.py's cube at 96 degrees, S = 1024, with R = 0 (k_shade_shadow_faces) and 1
  beside them the default frame (k_shade), and, with --parent ROOT (the parent commit's tree, built), that tree's default frame
              and its S = 2048 frame: the unchanged paths, alternated with this tree's in the same call
  classes     the share of the frame's pixels by class (0 not covered, LIT, SHADOWED, OUTSIDE, PARTIAL), bbr_read_shadow_mask

Every case runs in a process of its own under a time limit; the first case that fails ends the run.
usage: shadow_filter_cost.py [--reps 3] [--frames 300] [--rounds 2] [--parent ROOT] [--out FILE]"""
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
SIDE, FACES, RADIUS, REPS, FRAMES = %(side)d, %(faces)d, %(radius)d, %(reps)d, %(frames)d
cfg = configs.C3
r = Renderer(cfg.width, cfg.height)
r.set_option("frames_in_flight", 3)
r.set_option("shadow_map", SIDE)
if RADIUS:
    r.set_option("shadow_filter", RADIUS)
material = r.upload_material(textures.make_material(cfg.texture_size))
scene, cam, settings = S.config_scene(r, cfg)
frame = S.frame_call(r, scene, cam, settings, material)
frame(); r.synchronize()                      # the first frame sizes the capacities
out = dict(classes=[])
if SIDE:
    if FACES > 1:
        r.render_shadow_faces(0, S.cube_shadow_views(cfg.lights[0].pos, 96.0, 0.1, 1000.0)[:FACES], 2.0 ** -10)
    else:
        light = np.zeros(144, np.uint8)
        view, proj = np.zeros((4, 4), np.float32), np.zeros((4, 4), np.float32)
        p = lambda a: np.asarray(a, np.float32).ctypes.data_as(C.c_void_p)
        eye, target, up = np.asarray(cfg.lights[0].pos, np.float32), np.asarray((0.0, -1.0, 5.0), np.float32), np.asarray((0.0, 1.0, 0.0), np.float32)
        lib().bbs_mat4_look_at(p(eye), p(target), p(up), p(view))
        lib().bbs_mat4_perspective(120.0, 1.0, 0.1, 1000.0, p(proj))
        light[:64], light[64:128] = view.view(np.uint8).ravel(), proj.view(np.uint8).ravel()
        r.render_shadow_map(0, light, 2.0 ** -10)
    frame(); r.synchronize()
    out["classes"] = (np.bincount(r.read_shadow_mask().ravel(), minlength=5) / float(cfg.width * cfg.height)).tolist()
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
    args = dict(root=ROOT, side=0, faces=1, radius=0)
    args.update(kw)
    p = subprocess.run([sys.executable, "-c", CHILD % args], capture_output=True, text=True, timeout=240)
    if p.returncode:
        raise SystemExit(f"{tag}: FAILED rc={p.returncode}\n{p.stderr[-2000:]}")
    line = [l for l in p.stdout.splitlines() if l.startswith("RESULT ")][-1]
    return json.loads(line[7:])


def fmt(xs):
    return " ".join(f"{x:8.1f}" for x in xs)


def median(xs):
    return sorted(xs)[len(xs) // 2]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--frames", type=int, default=300)
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--parent", default=None, help="root of the parent commit's tree, built: its default and S = 2048 frames are timed too")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    common = dict(reps=a.reps, frames=a.frames)
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    cases = [("default (k_shade)", dict()),
             ("S = 2048, R = 0 (k_shade_shadow)", dict(side=2048)),
             ("S = 2048, R = 1 (k_shade_shadow_pcf, 9 taps)", dict(side=2048, radius=1)),
             ("S = 2048, R = 2 (k_shade_shadow_pcf, 25 taps)", dict(side=2048, radius=2)),
             ("six faces of S = 1024, R = 0 (k_shade_shadow_faces)", dict(side=1024, faces=6)),
             ("six faces of S = 1024, R = 1 (k_shade_shadow_pcf)", dict(side=1024, faces=6, radius=1))]
    if a.parent:
        parent = os.path.abspath(a.parent)
        cases[1:1] = [("the parent's default", dict(root=parent))]
        cases[2:2] = [("the parent's S = 2048", dict(root=parent, side=2048))]
    say(f"# C3 scene (3840 x 2160), light 0 the caster, three frames in flight: frame period, us per frame ({a.frames} frames between two "
        f"synchronisations, {a.reps} runs), the cases alternated, {a.rounds} rounds")
    last = {}
    for rnd in range(a.rounds):
        say(f"round {rnd + 1}")
        for name, kw in cases:
            last[name] = run(name, **kw, **common)
            say(f"{name:54s} {fmt(last[name]['period_us'])}")
        m = {name: median(res["period_us"]) for name, res in last.items()}
        say(f"by the medians: R = 1 : R = 0  {m[cases[-4][0]] / m[cases[-5][0]]:.3f}   R = 2 : R = 0  {m[cases[-3][0]] / m[cases[-5][0]]:.3f}   "
            f"six faces, R = 1 : R = 0  {m[cases[-1][0]] / m[cases[-2][0]]:.3f}")
    say()
    say("# share of the frame's pixels by class: not covered, LIT, SHADOWED, OUTSIDE, PARTIAL (bbr_read_shadow_mask; the last round)")
    for name, _ in cases:
        if last[name]["classes"]:
            say(f"{name:54s} {' '.join('%.4f' % x for x in last[name]['classes'])}")
    if a.out:
        with open(a.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
