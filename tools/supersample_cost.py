"""What option "supersample" costs (profiles/r07_supersample.txt): the C3 scene on a 3840 x 2160 context with supersample 2
against the same scene on a 7680 x 4320 context with supersample 1 (the difference of the frame periods is the resolve),
k_resolve against k_present as streaming kernels (bbr_resolve_timing / bbr_present_timing, one frame in flight so that each
runs alone), and k_resolve's PRESENT form against the fp32 form followed by k_present.

Every case runs in a process of its own under a time limit; the first case that fails ends the run.
usage: supersample_cost.py [--reps 3] [--frames 120] [--out FILE]"""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HBM_BYTES_PER_S = 8e12          # the MI355X's nominal HBM bandwidth: what a streaming kernel is held against

CHILD = r'''
import sys, time, gc, json
sys.path.insert(0, %(root)r)
from bibim_renderer_amd import configs, textures, Renderer
from bibim_renderer_amd import scene as S
W, H, N, FIF, REPS, FRAMES = %(w)d, %(h)d, %(n)d, %(fif)d, %(reps)d, %(frames)d
FUSED, PRESENT, TIMING = %(fused)d, %(present)d, %(timing)d
cfg = configs.C3.scaled(W, H)
r = Renderer(W, H)
r.set_option("frames_in_flight", FIF)
r.set_option("supersample", N)
r.set_option("present_fused", FUSED)
material = r.upload_material(textures.make_material(cfg.texture_size))
scene, cam, settings = S.config_scene(r, cfg)
def frame():
    S.draw_frame(r, scene, cam, settings, material)
    if PRESENT: r.present()
frame(); r.synchronize()                      # the first frame sizes the capacities
gc.collect(); gc.disable()
for _ in range(30): frame()
r.synchronize()
if TIMING:
    r.set_option("timing", 2)
    frame(); r.synchronize()
period, resolve, present = [], [], []
for rep in range(REPS):
    if TIMING: r.timing_reset()
    t0 = time.perf_counter()
    for _ in range(FRAMES): frame()
    r.synchronize()
    period.append((time.perf_counter() - t0) / FRAMES * 1e6)
    if TIMING:
        resolve.append(r.resolve_timing()[1] * 1e3 if N > 1 else 0.0)
        present.append(r.present_timing()[1] * 1e3 if PRESENT and not FUSED else 0.0)
print("RESULT", json.dumps(dict(period_us=period, resolve_us=resolve, present_us=present)), flush=True)
scene.close(); r.close()
'''


def run(tag, **kw):
    args = dict(root=ROOT, fused=0, present=0, timing=0, fif=3)
    args.update(kw)
    p = subprocess.run([sys.executable, "-c", CHILD % args], capture_output=True, text=True, timeout=240)
    if p.returncode:
        raise SystemExit(f"{tag}: FAILED rc={p.returncode}\n{p.stderr[-2000:]}")
    line = [l for l in p.stdout.splitlines() if l.startswith("RESULT ")][-1]
    return json.loads(line[7:])


def fmt(xs):
    return " ".join(f"{x:8.1f}" for x in xs)


def med(xs):
    return sorted(xs)[len(xs) // 2]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--frames", type=int, default=120)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    common = dict(reps=a.reps, frames=a.frames)
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    px = 3840 * 2160
    say("# C3 scene, three frames in flight: frame period, us per frame (%d frames between two synchronisations, %d runs)" % (a.frames, a.reps))
    ss = run("ss2", w=3840, h=2160, n=2, **common)
    say(f"3840 x 2160, supersample 2 (fine 7680 x 4320 + k_resolve)   {fmt(ss['period_us'])}")
    big = run("8k", w=7680, h=4320, n=1, **common)
    say(f"7680 x 4320, supersample 1 (the fine frame alone)            {fmt(big['period_us'])}")
    say(f"difference of the medians: the resolve in the pipelined frame  {med(ss['period_us']) - med(big['period_us']):8.1f}")
    say()
    say("# the kernels alone, one frame in flight, HIP events around each launch: us, GB/s by the algorithmic bytes, fraction of 8 TB/s")
    k = run("kernels", w=3840, h=2160, n=2, fif=1, present=1, timing=1, **common)
    for name, us, nbytes in (("k_resolve<2> fp32 form, 16 * (4 + 1) B per output pixel", k["resolve_us"], 80 * px),
                             ("k_present at 3840 x 2160, 16 + 4 B per pixel", k["present_us"], 20 * px)):
        rate = [nbytes / (u * 1e-6) for u in us]
        say(f"{name:58s} {fmt(us)}   GB/s {fmt([x / 1e9 for x in rate])}   of 8 TB/s {' '.join('%.3f' % (x / HBM_BYTES_PER_S) for x in rate)}")
    f = run("fused kernel", w=3840, h=2160, n=2, fif=1, fused=1, present=1, timing=1, **common)
    rate = [68 * px / (u * 1e-6) for u in f["resolve_us"]]
    say(f"{'k_resolve<2> PRESENT form, 16 * 4 + 4 B per output pixel':58s} {fmt(f['resolve_us'])}   GB/s {fmt([x / 1e9 for x in rate])}   of 8 TB/s {' '.join('%.3f' % (x / HBM_BYTES_PER_S) for x in rate)}")
    say(f"fp32 form + k_present, sum of the medians {med(k['resolve_us']) + med(k['present_us']):8.1f} us;  PRESENT form alone {med(f['resolve_us']):8.1f} us")
    say()
    say("# presented frames, three frames in flight: frame period, us per frame")
    unfused = run("present", w=3840, h=2160, n=2, present=1, **common)
    fused = run("present fused", w=3840, h=2160, n=2, present=1, fused=1, **common)
    say(f"supersample 2, k_resolve fp32 form + k_present             {fmt(unfused['period_us'])}")
    say(f"supersample 2, present_fused (k_resolve PRESENT form)      {fmt(fused['period_us'])}")
    if a.out:
        with open(a.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
