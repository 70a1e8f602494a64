"""What several shadow casters cost (profiles/shadow_casters.txt): the C3 scene at 3840 x 2160, three frames in flight, frame
period over 200 timed frames after the steady warm-up.  A caster is tools/shadow_faces_cost.py's cube: six faces of 96 degrees
at the light's position, S = 1024.

  (a)  the default frame (k_shade) and the frame with light 0 a caster in slot 0: the cube's first face alone (k_shade_shadow),
       the cube (k_shade_shadow_faces), the cube at R = 1 (k_shade_shadow_pcf)
  (b)  the same caster in slot 1 (k_shade_shadow_casters) against slot 0: the price of the general kernel
  (c)  all four lights of C3 as cube casters, at R = 0 and R = 1
  (d)  the wall time of the four bbr_render_shadow_caster calls of (c)

With --parent ROOT (the parent commit's tree, built) every case runs on both trees, alternated in the same call: each of the four
shadow kernels against its parent.  Per case the difference of the two medians is set against the parent's own spread (max - min
over its repetitions).
Every case runs in a process of its own under a time limit, behind bench.py's steady warm-up rule; the first case that fails
ends the run.
usage: shadow_casters_cost.py [--reps 3] [--frames 200] [--rounds 2] [--parent ROOT] [--out FILE]"""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PARENT = "parent: "

CHILD = r'''
import sys, time, gc, json
import numpy as np
sys.path.insert(0, %(root)r)
from bibim_renderer_amd import configs, textures, Renderer
from bibim_renderer_amd import scene as S
SLOTS, FACES, RADIUS, REPS, FRAMES = %(slots)r, %(faces)d, %(radius)d, %(reps)d, %(frames)d
cfg = configs.C3
r = Renderer(cfg.width, cfg.height)
r.set_option("frames_in_flight", 3)
r.set_option("shadow_map", 1024 if SLOTS else 0)
if RADIUS:
    r.set_option("shadow_filter", RADIUS)
material = r.upload_material(textures.make_material(cfg.texture_size))
scene, cam, settings = S.config_scene(r, cfg)
frame = S.frame_call(r, scene, cam, settings, material)
frame(); r.synchronize()                      # the first frame sizes the capacities
out = dict(shadowed=[], cast_ms=[])
for slot, light in SLOTS:
    views = S.cube_shadow_views(cfg.lights[light].pos, 96.0, 0.1, 1000.0)[:FACES]
    t0 = time.perf_counter()
    if slot is None:
        r.render_shadow_faces(light, views, 2.0 ** -10)        # (slot 0)
    else:
        r.render_shadow_caster(slot, light, views, 2.0 ** -10)
    out["cast_ms"].append((time.perf_counter() - t0) * 1e3)
if SLOTS:
    frame(); r.synchronize()
    for slot, light in SLOTS:
        mask = r.read_shadow_mask() if slot is None else r.read_shadow_caster_mask(slot)
        out["shadowed"].append(float(np.isin(mask, (2, 4)).sum()) / float(cfg.width * cfg.height))
gc.collect(); gc.disable()
# the steady warm-up, bench.py's rule: blocks of 50 frames until two consecutive blocks agree within 1 %% (at least 3 blocks, at
# most 2 s) -- with a fixed 60 frames the first timed window of a process was the slow one in either tree
blocks, t_start = [], time.perf_counter()
while True:
    t0 = time.perf_counter()
    for _ in range(50): frame()
    r.synchronize()
    blocks.append(time.perf_counter() - t0)
    if len(blocks) >= 3 and abs(blocks[-1] - blocks[-2]) <= 0.01 * blocks[-2]: break
    if time.perf_counter() - t_start > 2.0: break
out["warm_blocks"] = len(blocks)
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
    args = dict(root=ROOT, slots=[], faces=6, radius=0)
    args.update(kw)
    p = subprocess.run([sys.executable, "-c", CHILD % args], capture_output=True, text=True, timeout=240)
    if p.returncode:
        raise SystemExit(f"{tag}: FAILED rc={p.returncode}\n{p.stderr[-2000:]}")
    line = [l for l in p.stdout.splitlines() if l.startswith("RESULT ")][-1]
    return json.loads(line[7:])


def fmt(xs, form="%8.1f"):
    return " ".join(form % x for x in xs)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--frames", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--parent", default=None, help="root of the parent commit's tree, built: every case is timed on it too")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    common = dict(reps=a.reps, frames=a.frames)
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    four = [(s, s) for s in range(4)]
    own = [("(a) default (k_shade)", dict()),
           ("(a) first face in slot 0 (k_shade_shadow)", dict(slots=[(None, 0)], faces=1)),
           ("(a) cube caster in slot 0 (k_shade_shadow_faces)", dict(slots=[(None, 0)])),
           ("(a) cube caster in slot 0, R = 1 (k_shade_shadow_pcf)", dict(slots=[(None, 0)], radius=1)),
           ("(b) the same caster in slot 1 (k_shade_shadow_casters)", dict(slots=[(1, 0)])),
           ("(c) four cube casters, R = 0 (k_shade_shadow_casters)", dict(slots=four)),
           ("(c) four cube casters, R = 1 (k_shade_shadow_casters)", dict(slots=four, radius=1))]
    cases = []
    for name, kw in own:
        cases.append((name, kw))
        if a.parent:
            cases.append((PARENT + name, dict(kw, root=os.path.abspath(a.parent))))
    say(f"# C3 scene (3840 x 2160), three frames in flight: frame period, us per frame ({a.frames} frames between two synchronisations, "
        f"{a.reps} runs per process), the cases alternated, {a.rounds} rounds: {a.reps * a.rounds} repetitions each")
    seen = {name: [] for name, _ in cases}
    cast, last = [], {}
    for rnd in range(a.rounds):
        say(f"round {rnd + 1}")
        for name, kw in cases:
            last[name] = run(name, **kw, **common)
            seen[name] += last[name]["period_us"]
            say(f"{name:66s} {fmt(last[name]['period_us'])}")
            if len(kw.get("slots", [])) == 4:
                cast.append((name, last[name]["cast_ms"]))
    say()
    say("# range over all repetitions, us per frame")
    for name, _ in cases:
        say(f"{name:66s} {min(seen[name]):8.1f} .. {max(seen[name]):8.1f}")
    say()
    if a.parent:
        say("# median of this tree, of the parent, their difference, the parent's spread (max - min); inside: |difference| <= spread")
        for name, _ in own:
            new, old = statistics.median(seen[name]), statistics.median(seen[PARENT + name])
            spread = max(seen[PARENT + name]) - min(seen[PARENT + name])
            say(f"{name:66s} {new:8.1f} {old:8.1f} {new - old:+8.1f} {spread:8.1f}   {'inside' if abs(new - old) <= spread else 'OUTSIDE'}")
        say()
    say("# (d) wall time of the four bbr_render_shadow_caster calls (six faces of S = 1024 each; the first also makes the pass's buffers), ms")
    for name, ms in cast:
        say(f"{name:66s} {fmt(ms, '%8.2f')}   sum {sum(ms):8.2f}")
    say()
    say("# share of the frame's pixels SHADOWED or PARTIAL, per caster (the last round)")
    for name, _ in cases:
        if last[name]["shadowed"]:
            say(f"{name:66s} {fmt(last[name]['shadowed'], '%.4f')}")
    if a.out:
        with open(a.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
