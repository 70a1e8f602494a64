"""Measurement: what option "auto_exposure" costs a pipelined frame, and what k_luminance costs by itself
(profiles/auto_exposure.txt).  The method of tools/bloom_cost.py: every case runs in its own process -- warm-up, then N frames
between two synchronisations, `reps` times; with present=1 every frame is followed by bbr_present.  Other trees (the parent
commit's package with its library built; this tree's sources built with another BB_LUMA_FORM) alternate with this one within
one call.

usage: auto_exposure_cost.py [--reps 3] [--rounds 2] [--parent DIR] [--variant NAME=DIR ...] [--kernel] CASE [CASE ...]
       CASE = workload[:name=value ...]   names: fif (frames in flight, default 3), present (0 | 1), every option of bbr_set_option
       --parent DIR        run every case without auto_exposure on DIR's tree too, before this tree's, in every round
       --variant NAME=DIR  run every case WITH auto_exposure on DIR's tree too (this tree's sources built with
                           make EXTRA=-DBB_LUMA_FORM=n), behind this tree's, in every round and in the --kernel part: an A/B
       --kernel            afterwards, per tree: k_luminance's own interval (bbr_luminance_timing) beside the present kernel's
                           (bbr_present_timing) over 200 timed frames, one frame in flight, option "timing" 2 -- on the case's
                           frame through bbr_present, and on a constant 3840 x 2160 frame through bbr_present_buffer_auto"""
import argparse
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHILD = r'''
import sys, time, gc
sys.path.insert(0, %(root)r)
if %(kernel)d:
    import torch
    torch.cuda.init()        # (first: initialised behind the library it found no device in this process)
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
def share(nbytes, ms): return nbytes / (ms * 1e-3) / 8e12 if ms else 0.0
frame(); r.synchronize()
gc.collect(); gc.disable()
if %(kernel)d:
    px = cfg.width * cfg.height
    r.set_option("timing", 2)
    for _ in range(20): frame()
    r.timing_reset()
    for _ in range(200): frame()
    n, luma_ms = r.luminance_timing()
    m, present_ms = r.present_timing()
    print("%(tag)-44s frame     k_luminance n=%%d %%6.1f us %%5.2f of 8 TB/s (16 B/px)    present kernel n=%%d %%6.1f us %%5.2f (20 B/px)"
          %% (n, luma_ms * 1e3, share(16 * px, luma_ms), m, present_ms * 1e3, share(20 * px, present_ms)), flush=True)
    w, h = 3840, 2160
    src = torch.empty((h, w, 4), dtype=torch.float32, device="cuda")
    src[..., 0], src[..., 1], src[..., 2], src[..., 3] = 0.5, 0.4, 0.3, 1.0
    out = torch.zeros(h * w, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    call = lambda: r.present_buffer_auto(src.data_ptr(), out.data_ptr(), w, h, 1, 1.0)
    for _ in range(20): call()
    r.timing_reset()
    for _ in range(200): call()
    n, luma_ms = r.luminance_timing()
    m, present_ms = r.present_timing()
    rec = r.read_exposure(1)
    assert int(rec["hist"].max()) == w * h, "the constant frame fell into more than one bin"
    print("%(tag)-44s constant  k_luminance n=%%d %%6.1f us %%5.2f of 8 TB/s (16 B/px)    present kernel n=%%d %%6.1f us %%5.2f (20 B/px)"
          %% (n, luma_ms * 1e3, share(16 * w * h, luma_ms), m, present_ms * 1e3, share(20 * w * h, present_ms)), flush=True)
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
    print("%(tag)-44s us/frame " + " ".join("%%7.1f" %% x for x in out), flush=True)
scene.close(); r.close()
'''


def run(case, root, reps, kernel, label):
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
    if kernel:
        fif, present = 1, 1
    frames = {"c2": 600, "c3": 300, "c5": 80}[workload]
    code = CHILD % dict(root=root, workload=workload, opts=opts, frames=frames, fif=fif, present=present, reps=reps, kernel=int(kernel),
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
    ap.add_argument("--variant", action="append", default=[], metavar="NAME=DIR")
    ap.add_argument("--kernel", action="store_true")
    ap.add_argument("cases", nargs="+")
    a = ap.parse_args()
    variants = [v.split("=", 1) for v in a.variant]
    for rnd in range(1, a.rounds + 1):
        for case in a.cases:
            auto = "auto_exposure=1" in case
            if a.parent and not auto:
                if run(case, os.path.abspath(a.parent), a.reps, False, f"parent r{rnd}"):
                    return 1               # (a failed process: nothing more is started on the GPU)
            if run(case, ROOT, a.reps, False, f"this   r{rnd}"):
                return 1
            for name, d in variants if auto else []:
                if run(case, os.path.abspath(d), a.reps, False, f"{name:6s} r{rnd}"):
                    return 1
    if a.kernel:
        for case in a.cases:
            if "auto_exposure=1" not in case:
                continue
            for name, d in [("this", ROOT)] + variants:
                if run(case, os.path.abspath(d), a.reps, True, f"{name:6s}   "):
                    return 1
    return 0


if __name__ == "__main__":
    sys.exit(main())
