"""What option "sample_shading" 0 buys (profiles/r08_sample_shading.txt): the C3 scene on a 3840 x 2160 context, three
frames in flight, frame period of
  supersample 2, per-sample shading, on the parent commit's tree (--parent DIR, built; skipped without it)
  the same on this tree
  supersample 2, sample_shading 0
  supersample 4, sample_shading 0 (tile_mode 0: a fine frame of 15360 x 8640 has more 32 x 32 tiles than launch slots)
alternated; and the two kernels of the option alone, one frame in flight so that each runs by itself: k_resolve_merged by its
own HIP events (bbr_resolve_timing), k_sample_merge as the difference of the raster interval (k_raster + k_sample_merge +
k_shade_items, option "timing" 1) between the merged frame and the per-sample frame, both against their algorithmic bytes.

Every case runs in a process of its own under a time limit; the first case that fails ends the run.
usage: sample_shading_cost.py [--parent DIR] [--rounds 3] [--frames 120] [--out FILE]"""
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
W, H, N, SHADING, TILE_MODE, FIF, REPS, FRAMES, TIMING = %(w)d, %(h)d, %(n)d, %(shading)d, %(tile_mode)d, %(fif)d, %(reps)d, %(frames)d, %(timing)d
cfg = configs.C3.scaled(W, H)
r = Renderer(W, H)
r.set_option("frames_in_flight", FIF)
r.set_option("tile_mode", TILE_MODE)
if SHADING != 1: r.set_option("sample_shading", SHADING)      # (the parent's tree does not know the option)
r.set_option("supersample", N)
material = r.upload_material(textures.make_material(cfg.texture_size))
scene, cam, settings = S.config_scene(r, cfg)
def frame():
    S.draw_frame(r, scene, cam, settings, material)
frame(); r.synchronize()                      # the first frame sizes the capacities
gc.collect(); gc.disable()
for _ in range(30): frame()
r.synchronize()
if TIMING:
    r.set_option("timing", 1)
    frame(); r.synchronize()
period, resolve, raster, shade = [], [], [], []
for rep in range(REPS):
    if TIMING: r.timing_reset()
    t0 = time.perf_counter()
    for _ in range(FRAMES): frame()
    r.synchronize()
    period.append((time.perf_counter() - t0) / FRAMES * 1e6)
    if TIMING:
        resolve.append(r.resolve_timing()[1] * 1e3)
        s = r.timing_summary()
        raster.append(s[3] * 1e3); shade.append(s[4] * 1e3)
print("RESULT", json.dumps(dict(period_us=period, resolve_us=resolve, raster_us=raster, shade_us=shade,
                                n_shaded=int(r.stats()["n_shaded"]))), flush=True)
scene.close(); r.close()
'''


def run(tag, root=ROOT, **kw):
    args = dict(root=root, w=3840, h=2160, shading=1, tile_mode=1, timing=0, fif=3, reps=1)
    args.update(kw)
    p = subprocess.run([sys.executable, "-c", CHILD % args], capture_output=True, text=True, timeout=300, cwd=root)
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
    ap.add_argument("--parent", default=None, help="the parent commit's tree, built")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--frames", type=int, default=120)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)
        if a.out:                                  # (rewritten as the run goes: a case that fails leaves what came before it)
            with open(a.out, "w") as fh:
                fh.write("\n".join(lines) + "\n")

    px = 3840 * 2160
    cases = [("this tree, supersample 2, per-sample", dict(n=2)),
             ("this tree, supersample 2, sample_shading 0", dict(n=2, shading=0)),
             ("this tree, supersample 4, sample_shading 0, tile_mode 0", dict(n=4, shading=0, tile_mode=0))]
    if a.parent:
        cases.insert(0, ("parent's tree, supersample 2, per-sample", dict(n=2, root=os.path.abspath(a.parent))))
    say("# C3 scene at 3840 x 2160, three frames in flight: frame period, us per frame (%d frames between two synchronisations), %d rounds alternated"
        % (a.frames, a.rounds))
    period = {name: [] for name, _ in cases}
    for _ in range(a.rounds):
        for name, kw in cases:
            period[name] += run(name, frames=a.frames, **kw)["period_us"]
    for name, _ in cases:
        say(f"{name:58s} {fmt(period[name])}   median {med(period[name]):8.1f}")
    if a.parent:
        p, m = period[cases[0][0]], period[cases[2][0]]
        say(f"parent's min - max spread {max(p) - min(p):.1f} us; parent's median - merged n = 2 median {med(p) - med(m):.1f} us; "
            f"ratio of the medians {med(p) / med(m):.3f}")
    say()
    say("# the kernels alone, one frame in flight, option timing 1: us; GB/s by the algorithmic bytes; fraction of 8 TB/s")
    k = {}
    for tag, kw in (("per-sample n = 2", dict(n=2)), ("merged n = 2", dict(n=2, shading=0)),
                    ("merged n = 4", dict(n=4, shading=0, tile_mode=0))):
        k[tag] = run(tag, fif=1, timing=1, reps=3, frames=a.frames, **kw)
        say(f"{tag:18s} raster interval {fmt(k[tag]['raster_us'])}   shade interval {fmt(k[tag]['shade_us'])}   resolve {fmt(k[tag]['resolve_us'])}"
            f"   n_shaded {k[tag]['n_shaded']}")
    covered, reps = k["per-sample n = 2"]["n_shaded"], k["merged n = 2"]["n_shaded"]
    merge_us = med(k["merged n = 2"]["raster_us"]) - med(k["per-sample n = 2"]["raster_us"])
    merge_bytes = 8 * covered + 8 * reps + 2 * px
    say(f"k_sample_merge<32, 32, 2> = difference of the raster intervals {merge_us:8.1f} us; {covered} covered samples, {reps} representatives: "
        f"{merge_bytes / 1e6:.1f} MB, {merge_bytes / (merge_us * 1e-6) / 1e9:.1f} GB/s, {merge_bytes / (merge_us * 1e-6) / HBM_BYTES_PER_S:.3f} of 8 TB/s")
    for tag, n, word in (("merged n = 2", 2, 2), ("merged n = 4", 4, 8)):
        # the map word, 16 B per distinct representative of a pixel (an uncovered sample is its own), the store
        cov = covered if n == 2 else None
        us = med(k[tag]["resolve_us"])
        if cov is None:
            say(f"k_resolve_merged<{n}> {us:8.1f} us ({k[tag]['n_shaded']} representatives; the covered samples at n = 4 were not counted on the GPU)")
            continue
        nbytes = word * px + 16 * (k[tag]["n_shaded"] + n * n * px - cov) + 16 * px
        say(f"k_resolve_merged<{n}> {us:8.1f} us; {nbytes / 1e6:.1f} MB, {nbytes / (us * 1e-6) / 1e9:.1f} GB/s, {nbytes / (us * 1e-6) / HBM_BYTES_PER_S:.3f} of 8 TB/s"
            f"   (k_resolve<{n}> in the per-sample frame: {med(k['per-sample n = 2']['resolve_us']):.1f} us)")


if __name__ == "__main__":
    main()
