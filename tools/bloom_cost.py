"""Measurement: what option "bloom" costs a pipelined frame (profiles/bloom.txt).  Every case runs in its own process: warm-up,
then N frames between two synchronisations, `reps` times; with present=1 every frame is followed by bbr_present.  Other
trees (the parent commit's package with its library built; this tree's sources built with a diagnostic macro) alternate with this
one within one call.

usage: bloom_cost.py [--reps 3] [--rounds 2] [--parent DIR] [--variant DIR] [--chain] CASE [CASE ...]
       CASE = workload[:name=value ...]   names: fif (frames in flight, default 3), present (0 | 1), every option of bbr_set_option
       --parent DIR   run every case without a bloom option on DIR's tree too, before this tree's, in every round
       --variant DIR  run every case WITH a bloom option on DIR's tree too (this tree's sources built with another EXTRA=-D...),
                      behind this tree's, in every round and in the --chain part: an A/B
       --chain        afterwards, per bloom case: the chain's own interval (bbr_bloom_timing) and k_present_bloom's
                      (bbr_present_timing) over 200 timed frames, one frame in flight, and the chain's algorithmic bytes"""
import argparse
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHILD = r'''
import sys, time, gc
sys.path.insert(0, %(root)r)
from bibim_renderer_amd import configs, textures, Renderer
from bibim_renderer_amd import scene as S
cfg = configs.CONFIGS[%(workload)r]
r = Renderer(cfg.width, cfg.height)
r.set_option("frames_in_flight", %(fif)d)
for k, v in %(opts)r: r.set_option(k, v)
material = r.upload_material(textures.make_material(cfg.texture_size))
scene, cam, settings = S.config_scene(r, cfg)
settings.enable_tone_mapping = 1
def frame():
    S.draw_frame(r, scene, cam, settings, material)
    if %(present)d: r.present()
frame(); r.synchronize()
gc.collect(); gc.disable()
if %(chain)d:
    r.set_option("timing", 2)
    for _ in range(20): frame()
    r.timing_reset()
    for _ in range(200): frame()
    n, chain_ms = r.bloom_timing()
    m, present_ms = r.present_timing()
    levels = r.get_bloom()[0]
    w, h = [cfg.width], [cfg.height]
    for k in range(levels):
        w.append((w[-1] + 1) >> 1); h.append((h[-1] + 1) >> 1)
    # k_bloom_first reads the frame and writes D_1; each k_bloom_down reads a level and writes the next; each k_bloom_up reads the
    # coarser level and reads and writes its own: 16 bytes a texel
    moved = 16 * (w[0] * h[0] + w[1] * h[1] + sum(w[k] * h[k] + w[k + 1] * h[k + 1] for k in range(1, levels))
                  + sum(w[k + 1] * h[k + 1] + 2 * w[k] * h[k] for k in range(1, levels)))
    print("%(tag)-40s chain  n=%%d  %%7.1f us   %%6.1f MB  %%5.2f of 8 TB/s     k_present_bloom  n=%%d  %%7.1f us"
          %% (n, chain_ms * 1e3, moved / 1e6, moved / (chain_ms * 1e-3) / 8e12, m, present_ms * 1e3), flush=True)
else:
    for _ in range(60): frame()
    r.synchronize()
    out = []
    for rep in range(%(reps)d):
        for _ in range(10): frame()
        t0 = time.perf_counter()
        for _ in range(%(frames)d): frame()
        r.synchronize()
        out.append((time.perf_counter() - t0) / %(frames)d * 1e6)
    print("%(tag)-40s us/frame " + " ".join("%%7.1f" %% x for x in out), flush=True)
scene.close(); r.close()
'''


def run(case, root, reps, chain, label):
    parts = case.split(":")
    workload, fif, present, opts = parts[0], 3, 0, []
    for p in parts[1:]:
        k, v = p.split("=")
        if k == "fif":
            fif = int(v)
        elif k == "present":
            present = int(v)
        else:
            opts.append((k, int(v)))
    if chain:
        fif, present = 1, 1
    frames = {"c2": 600, "c3": 300, "c5": 80}[workload]
    code = CHILD % dict(root=root, workload=workload, opts=opts, frames=frames, fif=fif, present=present, reps=reps, chain=int(chain),
                        tag=f"{label} {case}")
    p = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=300)
    sys.stdout.write(p.stdout)
    if p.returncode:
        sys.stdout.write(f"{label} {case}: FAILED rc={p.returncode}\n{p.stderr[-1500:]}\n")
    sys.stdout.flush()
    return p.returncode


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--parent", default="")
    ap.add_argument("--variant", default="")
    ap.add_argument("--chain", action="store_true")
    ap.add_argument("cases", nargs="+")
    a = ap.parse_args()
    for rnd in range(1, a.rounds + 1):
        for case in a.cases:
            if a.parent and "bloom=" not in case:
                if run(case, os.path.abspath(a.parent), a.reps, False, f"parent r{rnd}"):
                    return 1               # (a failed process: nothing more is started on the GPU)
            if run(case, ROOT, a.reps, False, f"this   r{rnd}"):
                return 1
            if a.variant and "bloom=" in case and run(case, os.path.abspath(a.variant), a.reps, False, f"variant r{rnd}"):
                return 1
    if a.chain:
        for case in a.cases:
            if "bloom=" in case and run(case, ROOT, a.reps, True, "this     "):
                return 1
            if a.variant and "bloom=" in case and run(case, os.path.abspath(a.variant), a.reps, True, "variant  "):
                return 1
    return 0


if __name__ == "__main__":
    sys.exit(main())
