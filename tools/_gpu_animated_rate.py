"""Diagnostic: pipelined frame period of a workload whose instances MOVE every frame (every instance block of both draws differs
from the one the frame slot saw last), through the plain C API: bbr_begin_frame / bbr_draw / bbr_end_frame.  Option
"static_records" never finds a repeated key in such a sequence: the figure shows what an animated scene pays for the comparison.
--still: the same loop with the instances left alone (the draws go to the light path).  Each case runs in its own process.
--camera: the CAMERA moves instead (implies --still): sixteen views, a quarter of a degree of yaw and an eighth of pitch apart, one
per frame in turn, so every frame's view differs from the one its slot saw last.  What option "sky_keep" keeps of such a
sequence is printed as the share of background tiles kept, summed over the last frame of every slot.
--every N (with --camera): the view changes with every N-th frame only, the frames between repeat it.
--lights: the camera stands still and LIGHT 0 moves instead (implies --still): eight positions a millimetre apart, one per frame in
turn -- what the application does between two inputs.  Every frame has its slot's view and draws and new shading inputs: what
option "view_keep" keeps of a sequence is printed as the share of frames kept (bbr_view_keep_counts, the whole run).
--forget: bbr_framebuffer_device_ptr in front of every frame: every frame slot forgets what option "sky_keep" remembers and no
tile is ever kept (the call waits for nothing; on a tree without the option it only returns the pointer).
usage: _gpu_animated_rate.py [--root TREE] [--reps 3] [--still] [--camera [--every N]] [--lights] [--forget] workload[:fif=3][:name=value ...] ..."""
import argparse, os, subprocess, sys

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHILD = r'''
import sys, time, gc, dataclasses
sys.path.insert(0, %(root)r)
import numpy as np
from bibim_renderer_amd import configs, textures, Renderer
from bibim_renderer_amd import scene as S
cfg = configs.CONFIGS[%(workload)r]
r = Renderer(cfg.width, cfg.height)
r.set_option("frames_in_flight", %(fif)d)
for k, v in %(opts)r: r.set_option(k, v)
material = r.upload_material(textures.make_material(cfg.texture_size))
scene, cam, settings = S.config_scene(None, cfg)
fb, vb = scene.fill_uniforms(cam, settings, cfg.width, cfg.height)
balls, ground = scene.instances(0), scene.instances(1)
plane = np.zeros((4, 11), np.float32)
plane[:, 0:3] = [(-0.5, 0, -0.5), (-0.5, 0, 0.5), (0.5, 0, 0.5), (0.5, 0, -0.5)]
plane[:, 3:5] = [(0, 0), (0, 1), (1, 1), (1, 0)]
plane[:, 5:8], plane[:, 8:11] = (0, 1, 0), (1, 0, 0)
m_ball = r.upload_mesh(S.load_shaderball_vertices())
m_plane = r.upload_mesh(plane, np.array([0, 1, 2, 2, 3, 0], np.uint32))
# eight sets of instance blocks, a hair apart (the translation column of every model matrix): consecutive frames of a slot differ
sets = []
for k in range(1 if %(still)r else 8):
    b, g = balls.copy(), ground.copy()
    b[:, 0, 3, 1] += 1e-4 * k
    g[:, 0, 3, 1] -= 1e-4 * k
    sets.append((np.ascontiguousarray(b).view(np.uint8).reshape(-1), np.ascontiguousarray(g).view(np.uint8).reshape(-1)))
r.set_frame_uniforms(fb)
r.set_view_uniforms(vb)
views = []
if %(camera)r:
    for k in range(16):
        step = min(k, 16 - k)   # there and back
        views.append(scene.fill_uniforms(dataclasses.replace(cam, yaw=cam.yaw + 0.25 * step, pitch=cam.pitch + 0.125 * step), settings,
                                         cfg.width, cfg.height)[1])
frame_blocks = []
if %(lights)r:
    for k in range(8):
        f = fb.copy()
        f[16:20].view(np.float32)[0] += 1e-3 * k   # lights[0].pos.x
        frame_blocks.append(f)
n = [0]
def frame():
    b, g = sets[n[0] %% len(sets)]
    if views: r.set_view_uniforms(views[(n[0] // %(every)d) %% len(views)])
    if frame_blocks: r.set_frame_uniforms(frame_blocks[n[0] %% len(frame_blocks)])
    if %(forget)r and n[0]: r.framebuffer_device_ptr()   # (there is no frame in front of the first)
    n[0] += 1
    r.begin_frame(); r.draw(m_ball, material, b); r.draw(m_plane, material, g); r.end_frame()
frame(); r.synchronize()
gc.collect(); gc.disable()
for _ in range(60): frame()
r.synchronize()
out = []
for rep in range(%(reps)d):
    for _ in range(10): frame()
    t0 = time.perf_counter()
    for _ in range(%(frames)d): frame()
    r.synchronize()
    out.append((time.perf_counter() - t0) / %(frames)d * 1e6)
counts = r.static_record_counts() if hasattr(r, "static_record_counts") else None
sky = ""
if hasattr(r, "read_sky_tiles"):
    kept = filled = 0
    for _ in range(%(fif)d):   # (one frame at a time: the report is the last frame's)
        frame()
        t = r.read_sky_tiles()
        kept, filled = kept + int((t == 2).sum()), filled + int((t == 1).sum())
    sky = "   background tiles kept: %%d of %%d" %% (kept, kept + filled)
if hasattr(r, "view_keep_counts"):
    c = r.view_keep_counts()
    sky += "   frames kept: %%d of %%d" %% (c["kept"], c["kept"] + c["full"])
print("%(tag)-40s us/frame " + " ".join("%%7.1f" %% x for x in out) + "   static records: %%s" %% (counts,) + sky, flush=True)
scene.close(); r.close()
'''
ap = argparse.ArgumentParser()
ap.add_argument("--root", default=HERE, help="the tree whose package and library are used (another checkout, for A/B timing)")
ap.add_argument("--reps", type=int, default=3)
ap.add_argument("--still", action="store_true")
ap.add_argument("--camera", action="store_true")
ap.add_argument("--every", type=int, default=1)
ap.add_argument("--lights", action="store_true")
ap.add_argument("--forget", action="store_true")
ap.add_argument("cases", nargs="+")
a = ap.parse_args()
rc = 0
for case in a.cases:
    parts = case.split(":")
    workload = parts[0]
    fif, opts = (4 if workload == "c2" else 3), []
    for p in parts[1:]:
        k, v = p.split("=")
        if k == "fif":
            fif = int(v)
        else:
            opts.append((k, int(v)))
    frames = {"c2": 600, "c3": 300, "c5": 80}[workload]
    tag = ("lights " if a.lights else (f"camera/{a.every} " if a.every > 1 else "camera ") if a.camera else "still " if a.still else "moving ") + ("forget " if a.forget else "") + case + (" [" + os.path.basename(os.path.abspath(a.root)) + "]" if a.root != HERE else "")
    code = CHILD % dict(root=os.path.abspath(a.root), workload=workload, opts=opts, frames=frames, fif=fif, reps=a.reps, tag=tag, still=a.still or a.camera or a.lights,
                        camera=a.camera, forget=a.forget, lights=a.lights, every=max(a.every, 1))
    p = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=300)
    sys.stdout.write(p.stdout)
    if p.returncode:
        sys.stdout.write(f"{case}: FAILED rc={p.returncode}\n{p.stderr[-1500:]}\n"); rc = 1
    sys.stdout.flush()
sys.exit(rc)
