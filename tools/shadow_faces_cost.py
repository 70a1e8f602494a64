"""What a cube shadow map costs (profiles/shadow_faces.txt): the C3 scene, light 0 the caster, the six faces of
bb::cubeShadowViews at the light's position (96 degrees), S = 1024.

  the synchronous pass alone   bbr_render_shadow_faces with F = 6 and F = 1 and bbr_render_shadow_map, wall time per call: how
                               much of the call is paid once (the drain, the uploads, the wait, the counter read) and how much
                               per face
  the pipelined frame          three frames in flight, frame period with six faces (k_shade_shadow_faces), with the first face
                               alone (k_shade_shadow), by default (k_shade) and at max_anisotropy 2 without a map (k_shade_aniso),
                               alternated
  who decides                  the share of the covered pixels each face decides, from bbr_read_shadow_face_index on a frame of a
                               quarter of the extent each way (the same view)

Every case runs in a process of its own under a time limit; the first case that fails ends the run.
usage: shadow_faces_cost.py [--reps 3] [--frames 300] [--side 1024] [--rounds 2] [--out FILE]"""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

CHILD = r'''
import sys, time, gc, json
import numpy as np
sys.path.insert(0, %(root)r)
from bibim_renderer_amd import configs, textures, Renderer
from bibim_renderer_amd import scene as S
SIDE, FACES, ANISO, REPS, FRAMES, CALLS, SMALL = %(side)d, %(faces)d, %(aniso)d, %(reps)d, %(frames)d, %(calls)d, %(small)d
cfg = configs.C3
if SMALL:
    cfg = cfg.scaled(cfg.width // 4, cfg.height // 4, cfg.texture_size)
r = Renderer(cfg.width, cfg.height)
r.set_option("frames_in_flight", 3)
r.set_option("max_anisotropy", ANISO)
r.set_option("shadow_map", SIDE)
material = r.upload_material(textures.make_material(cfg.texture_size))
scene, cam, settings = S.config_scene(r, cfg)
frame = S.frame_call(r, scene, cam, settings, material)
frame(); r.synchronize()                      # the first frame sizes the capacities
out = dict(pass_us=[], pass_map_us=[], classes=[], faces=[])
if SIDE:
    views = S.cube_shadow_views(cfg.lights[0].pos, 96.0, 0.1, 1000.0)[:FACES]
    r.render_shadow_faces(0, views, 2.0 ** -10)     # (may grow a capacity: not timed)
    for rep in range(REPS):
        t0 = time.perf_counter()
        for _ in range(CALLS): r.render_shadow_faces(0, views, 2.0 ** -10)
        out["pass_us"].append((time.perf_counter() - t0) / CALLS * 1e6)
    if FACES == 1:
        for rep in range(REPS):
            t0 = time.perf_counter()
            for _ in range(CALLS): r.render_shadow_map(0, views[0], 2.0 ** -10)
            out["pass_map_us"].append((time.perf_counter() - t0) / CALLS * 1e6)
        r.render_shadow_faces(0, views, 2.0 ** -10)
    frame(); r.synchronize()
    if SMALL:
        mask, face = r.read_shadow_mask(), r.read_shadow_face_index()
        covered = float((mask != 0).sum())
        out["classes"] = [float((mask == k).sum()) / covered for k in (1, 2, 3)]
        out["faces"] = [float(((face == f) & (mask != 0)).sum()) / covered for f in range(FACES)]
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
    args = dict(root=ROOT, side=0, faces=1, aniso=1, calls=20, small=0)
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
    ap.add_argument("--side", type=int, default=1024)
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    common = dict(reps=a.reps, frames=a.frames)
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    say(f"# C3 scene (3840 x 2160), three frames in flight: frame period, us per frame ({a.frames} frames between two synchronisations, "
        f"{a.reps} runs), the cases alternated, {a.rounds} rounds")
    six = one = None
    for rnd in range(a.rounds):
        say(f"round {rnd + 1}")
        say(f"default (k_shade)                                  {fmt(run('default', **common)['period_us'])}")
        say(f"max_anisotropy 2, no map (k_shade_aniso)           {fmt(run('aniso 2', aniso=2, **common)['period_us'])}")
        one = run("one face", side=a.side, faces=1, **common)
        say(f"shadow_map {a.side:<5d} one face  (k_shade_shadow)       {fmt(one['period_us'])}")
        six = run("six faces", side=a.side, faces=6, **common)
        say(f"shadow_map {a.side:<5d} six faces (k_shade_shadow_faces) {fmt(six['period_us'])}")
        say(f"six faces : one face, by the medians                {sorted(six['period_us'])[len(six['period_us']) // 2] / sorted(one['period_us'])[len(one['period_us']) // 2]:8.3f}")
    say()
    say(f"# the synchronous pass alone, side {a.side}: wall time per call, us (20 calls back to back, {a.reps} runs; the last round's processes)")
    say(f"bbr_render_shadow_faces, F = 6                     {fmt(six['pass_us'])}")
    say(f"bbr_render_shadow_faces, F = 1                     {fmt(one['pass_us'])}")
    say(f"bbr_render_shadow_map                              {fmt(one['pass_map_us'])}")
    say()
    small = run("small", side=a.side, faces=6, small=1, reps=1, frames=20)
    say("# who decides: a frame of a quarter of the extent each way, the same view (bbr_read_shadow_mask, bbr_read_shadow_face_index)")
    say(f"covered pixels lit, shadowed, outside every face:  {' '.join('%.3f' % x for x in small['classes'])}")
    say(f"covered pixels decided by face 0 .. 5:             {' '.join('%.3f' % x for x in small['faces'])}")
    if a.out:
        with open(a.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
