"""GPU: option "static_records" -- the camera-independent part of a draw's records is written once per frame slot
(k_record_static) and k_geometry stores only what follows the camera (its light path).

Every sequence below runs twice on fresh contexts, with "static_records" 1 and 0, and everything read back is compared bit for
bit between the two and, wherever the oracle reaches, with the oracle.  The host's counters (static_record_counts: fills
queued, draws submitted on the light path) say which path a frame took: every test asserts that its frames did leave the full
path, and when.  Frames are 160 x 90 (15 tiles of 32 x 32, partial at the bottom edge) with 2 x 80 + 2 primitives.

The scene: two small spheres side by side (one draw, two instances: closed convex meshes, so what does not win a pixel of an
unoccluded sphere faces away from the camera and is culled) over a ground quad (an indexed draw).  The user moves the camera,
not the instances (the reference's ShaderBallScene::updateScene rebuilds the same matrices every call)."""
import functools
import os

import numpy as np
import pytest

import resolve_reference as RR
import test_gpu_late_clip_slot as LC
from conftest import GOLDEN
from bibim_renderer_amd import Renderer, textures
from bibim_renderer_amd import partition as P
from oracle import bbo, scenes

F = np.float32
W, H = 160, 90
NO = bbo.NO_PRIM
FILL = 0xFFFFFFFF
N_SPHERE = 80                      # primitives of one sphere
N_DRAWS = 2


def bits(a):
    return np.ascontiguousarray(a, F).view(np.uint32)


def same(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


# ---- the scene ----
@functools.lru_cache(None)
def sphere_mesh(n_lon=8, n_lat=6, radius=0.8):
    """a UV sphere, non-indexed: 2 * n_lon * (n_lat - 1) triangles"""
    def vert(i, j):
        th, ph = 2 * np.pi * i / n_lon, np.pi * j / n_lat
        n = np.array([np.sin(ph) * np.cos(th), np.cos(ph), np.sin(ph) * np.sin(th)])
        return radius * n, (i / n_lon, j / n_lat), n, (-np.sin(th), 0.0, np.cos(th))
    tris = []
    for j in range(n_lat):
        for i in range(n_lon):
            a, b, c, d = vert(i, j), vert(i + 1, j), vert(i + 1, j + 1), vert(i, j + 1)
            if j > 0:
                tris += [a, b, c]
            if j < n_lat - 1:
                tris += [a, c, d]
    v = np.zeros(len(tris), bbo.VERTEX_DTYPE)
    for k, (pos, uv, nrm, tng) in enumerate(tris):
        v[k]["pos"], v[k]["uv"], v[k]["normal"], v[k]["tangent"] = pos, uv, nrm, tng
    assert len(v) == 3 * N_SPHERE
    return v


@functools.lru_cache(None)
def materials():
    rng = np.random.default_rng(5)
    m = textures.make_material(16)
    other = {k: rng.integers(30, 256, (8, 8, 4), dtype=np.uint8) for k in ("albedo", "metallic", "roughness", "ao", "normal")}
    mixed = dict(m, roughness=rng.integers(40, 256, (8, 8, 4), dtype=np.uint8), normal=rng.integers(100, 156, (10, 12, 4), dtype=np.uint8))
    return {"packed": bbo.MaterialData(m), "other": bbo.MaterialData(other), "mixed": bbo.MaterialData(mixed)}


def sphere_instances(offsets=((-1.0, 0.0, 0.0), (1.0, 0.0, 0.0)), turn=0.0):
    inst = np.zeros(len(offsets), bbo.INSTANCE_DTYPE)
    for i, o in enumerate(offsets):
        inst[i] = scenes.instance(bbo.mat_mul(bbo.mat_translate(*[float(x) for x in o]), bbo.mat_rotate_y(float(turn) if i == len(offsets) - 1 else 0.0)))
    return inst


@functools.lru_cache(None)
def base_draws(ground=12.0):
    pv, pi = scenes.plane_mesh()
    g = np.zeros(1, bbo.INSTANCE_DTYPE)
    g[0] = scenes.instance(bbo.mat_mul(bbo.mat_translate(0.0, -1.0, 0.0), bbo.mat_scale(float(ground))))
    return (bbo.DrawData(sphere_mesh(), None, sphere_instances(), materials()["packed"]), bbo.DrawData(pv, pi, g, materials()["packed"]))


LIGHTS = [scenes.light(0, pos=(0.5, 3.0, -2.0), color=(1.0, 0.9, 0.8), intensity=30.0),
          scenes.light(0, pos=(-1.0, 2.0, 4.0), color=(0.7, 0.8, 1.0), intensity=25.0)]


def view(eye, target=(0.0, 0.0, 0.0), w=W, h=H):
    vu = scenes.view_uniforms(eye, 0.0, 0.0, w, h, 1)
    vu["view"] = bbo.mat_look_at(eye, target)
    return vu


def scene_of(draws, eye, target=(0.0, 0.0, 0.0), w=W, h=H):
    return bbo.Scene(scenes.frame_uniforms(LIGHTS, 1, 1.1), view(eye, target, w, h), list(draws), w, h, f"static records {eye}")


def walk_eye(k, n):
    """a camera that walks round the spheres: a few degrees a frame in front of them (z < 0), the last two frames behind them"""
    a = np.radians(4.0 * k + (0.0 if k < n - 2 else 180.0))
    return (float(5.0 * np.sin(a)), 0.6 + 0.1 * k, float(-5.0 * np.cos(a)))


N_WALK = 10


@functools.lru_cache(None)
def walk_scene(k):
    return scene_of(base_draws(), walk_eye(k, N_WALK))


@functools.lru_cache(None)
def near_scene(k):
    """even k: the camera stands on the ground quad, which crosses the near plane; odd k: it sees all of it"""
    return scene_of(base_draws(), (0.3, 0.5, -3.0) if k % 2 == 0 else (0.0, 6.0, -14.0))


@functools.lru_cache(None)
def late_scene(k):
    """test_gpu_late_clip_slot's 48 triangles on one tile: every one of them crosses the near plane seen from the origin
    (96 clipped sub-triangles, more than kClipRefs = 32), fewer seen from four units further back"""
    sc = LC.scene()
    vu = sc.view if k % 2 == 0 else view((0.0, 0.0, -4.0), (0.0, 0.0, 1.0), LC.W, LC.H)
    return bbo.Scene(sc.frame, vu, sc.draws, LC.W, LC.H, f"late clip {k % 2}")


@functools.lru_cache(None)
def oracle(sc_fn, k):
    frame, prim, depth, stats = bbo.render(sc_fn(k))
    for a in (frame, prim, depth):
        a.setflags(write=False)
    return frame, prim, depth, stats


# ---- the harness ----
def run(script, static, fif=2, w=W, h=H):
    """`script(r, h)` on a fresh context -> (what it returns, the counters at the end); h: the handles of render_scene"""
    r = Renderer(w, h)
    r.set_option("frames_in_flight", fif)
    r.set_option("static_records", static)
    assert r.static_record_counts() == {"fills": 0, "light_draws": 0}
    out = script(r, {"mesh": {}, "mat": {}})
    counts = r.static_record_counts()
    r.close()
    return out, counts


def both(script, fif=2, w=W, h=H):
    """the script with "static_records" 1 and 0: the same bits; 0 never leaves the full path.  Returns the run with 1."""
    out1, c1 = run(script, 1, fif, w, h)
    out0, c0 = run(script, 0, fif, w, h)
    assert c0 == {"fills": 0, "light_draws": 0}
    assert len(out1) == len(out0)
    for i, (a, b) in enumerate(zip(out1, out0)):
        assert same(a, b), f"item {i}: static_records 1 and 0 differ"
    return out1, c1


def delta(r, before):
    c = r.static_record_counts()
    return (c["fills"] - before["fills"], c["light_draws"] - before["light_draws"])


# ---- on the oracle alone: the scenes reach what the tests are about ----
def test_the_scenes_reach_their_cases():
    # the walk: many of the spheres' primitives that win pixels in the last frame win none before every slot has been filled
    # (a facet of an unoccluded convex mesh that wins no pixel faces away from the camera, a sliver aside: it was culled then)
    early = set()
    for k in range(N_WALK - 2):
        early |= set(np.unique(oracle(walk_scene, k)[1]).tolist())
    late = set(np.unique(oracle(walk_scene, N_WALK - 1)[1]).tolist()) - {NO}
    late_spheres = {p for p in late if p < 2 * N_SPHERE}
    assert len(late_spheres - early) >= 30
    # the near-plane walk: the ground is clipped in the even frames only
    assert oracle(near_scene, 0)[3]["n_clipped_prims"] == 2 and oracle(near_scene, 1)[3]["n_clipped_prims"] == 0
    assert (oracle(near_scene, 0)[1] >= 2 * N_SPHERE).sum() > 1000 and (oracle(near_scene, 1)[1] == 2 * N_SPHERE).sum() > 100
    # the late route: 96 clipped sub-triangles on the one tile, and a view in which some of the 48 are not clipped
    a, b = oracle(late_scene, 0)[3], oracle(late_scene, 1)[3]
    assert a["n_clipped_prims"] == LC.N_TRI and a["n_raster_tris"] > 32
    assert b["n_clipped_prims"] < LC.N_TRI and (oracle(late_scene, 1)[1] != NO).sum() > 100


# ---- camera walk ----
@pytest.mark.gpu
@pytest.mark.parametrize("fif", [1, 2, 3, 4])
def test_camera_walk(fif):
    """fixed instances, a camera that walks round them: slot s is filled in frame fif + s, exactly once, and every frame from
    frame fif on is on the light path; the last two frames see the spheres from behind"""
    def script(r, h):
        out, per_frame = [], []
        for k in range(N_WALK):
            c = r.static_record_counts()
            r.render_scene(walk_scene(k), h)
            per_frame.append(delta(r, c))
            out.append(r.read_framebuffer())
        if r.static_record_counts()["fills"]:
            want = [(0, 0)] * fif + [(N_DRAWS, N_DRAWS)] * fif + [(0, N_DRAWS)] * (N_WALK - 2 * fif)
            assert per_frame == want, per_frame
        return out
    out, counts = both(script, fif)
    assert counts == {"fills": N_DRAWS * fif, "light_draws": N_DRAWS * (N_WALK - fif)}
    for k in range(N_WALK):
        assert np.array_equal(bits(out[k]), bits(oracle(walk_scene, k)[0])), f"frame {k}"


# ---- near-plane walk ----
@pytest.mark.gpu
@pytest.mark.parametrize("fif", [1, 3])
def test_near_plane_walk(fif):
    """the ground quad is clipped in the even frames and not in the odd ones: with one or three frames in flight every slot
    sees clipped -> unclipped -> clipped, so clip_base goes kNotClipped -> arena slot -> kNotClipped on the light path"""
    n = 4 * fif + 2
    def script(r, h):
        out = []
        for k in range(n):
            r.render_scene(near_scene(k), h)
            out += [r.read_framebuffer(), *r.read_visibility()]
        return out
    out, counts = both(script, fif)
    # (read_visibility renders its frame again in the same slot: a repeated key, so the slots are filled early)
    assert counts["fills"] == N_DRAWS * fif and counts["light_draws"] >= N_DRAWS * (n - fif)
    for k in range(n):
        frame, prim, depth, _ = oracle(near_scene, k)
        assert np.array_equal(bits(out[3 * k]), bits(frame)), f"frame {k}"
        assert np.array_equal(out[3 * k + 1], prim) and np.array_equal(bits(out[3 * k + 2]), bits(depth)), f"visibility {k}"


@pytest.mark.gpu
def test_near_plane_walk_late_clip_route():
    """more than kClipRefs clipped sub-triangles on a tile: the fragments of the later ones find their arena slot through
    recs[prim].clip_base, which the light path stores (kNotClipped) and the clipper patches every frame"""
    n = 6
    def script(r, h):
        out = []
        for k in range(n):
            r.render_scene(late_scene(k), h)
            out.append(r.read_framebuffer())
        return out
    out, counts = both(script, 1, LC.W, LC.H)
    assert counts == {"fills": 1, "light_draws": n - 1}
    for k in range(n):
        assert np.array_equal(bits(out[k]), bits(oracle(late_scene, k)[0])), f"frame {k}"


# ---- changing instances ----
@functools.lru_cache(None)
def turned_scene(turn):
    d = base_draws()
    return scene_of((bbo.DrawData(sphere_mesh(), None, sphere_instances(turn=turn), materials()["packed"]), d[1]), (1.0, 1.5, -5.0))


@pytest.mark.gpu
def test_changing_instances():
    """two frames in flight.  Frames 0..5: nothing moves.  Frame 6: one instance matrix of the first draw changes and stays: the
    draw leaves the light path at once, in both slots, with no fill, and comes back (one fill per slot) when its key has
    repeated; the ground draw stays on the light path throughout.  Frames 12..17: the instance turns every frame: no fill."""
    turns = [0.0] * 6 + [30.0] * 6 + [35.0 + 5.0 * i for i in range(6)]
    want = ([(0, 0)] * 2 + [(2, 2)] * 2 + [(0, 2)] * 2 +        # full, filled, light
            [(0, 1)] * 2 + [(1, 2)] * 2 + [(0, 2)] * 2 +        # the first draw: full (no fill), filled again, light
            [(0, 1)] * 6)                                       # ... full every frame, the ground light
    def script(r, h):
        out, per_frame = [], []
        for t in turns:
            c = r.static_record_counts()
            r.render_scene(turned_scene(t), h)
            per_frame.append(delta(r, c))
            out.append(r.read_framebuffer())
        if r.static_record_counts()["fills"]:
            assert per_frame == want, per_frame
        return out
    out, counts = both(script, 2)
    assert counts == {"fills": 6, "light_draws": sum(w[1] for w in want)}
    for k, t in enumerate(turns):
        assert np.array_equal(bits(out[k]), bits(bbo.render(turned_scene(t))[0])), f"frame {k}"


# ---- reused handles ----
@pytest.mark.gpu
def test_reused_handles():
    """one frame in flight, three frames per step (full, filled, light): a mesh freed and uploaded again with other vertices
    (the allocator may hand out the old address), a material uploaded again packed and with maps of different sizes, the
    draws in the other order, another instance count.  Every step starts on the full path and shows its own scene."""
    small = sphere_mesh(8, 6, 0.5)
    eye = (0.5, 1.2, -5.0)
    def draws(mesh, mat, order=(0, 1), n_inst=2):
        offs = ((-1.0, 0.0, 0.0), (1.0, 0.0, 0.0), (0.0, 0.9, 0.5))[:n_inst]
        d = (bbo.DrawData(mesh, None, sphere_instances(offs), mat), bbo.DrawData(*scenes.plane_mesh(), base_draws()[1].instances, mat))
        return [d[i] for i in order]
    m = materials()
    steps = [("first", sphere_mesh(), m["packed"], (0, 1), 2, False),
             ("mesh again, other vertices", small, m["packed"], (0, 1), 2, True),
             ("material again, packed", small, m["other"], (0, 1), 2, True),
             ("material again, maps of different sizes", small, m["mixed"], (0, 1), 2, True),
             ("draw order swapped", small, m["mixed"], (1, 0), 2, False),
             ("three instances", small, m["mixed"], (1, 0), 3, False)]
    wanted = [bbo.render(scene_of(draws(*s[1:5]), eye))[0] for s in steps]
    def script(r, h):
        out, mesh_h, mat_h = [], {}, None
        for name, mesh, mat, order, n_inst, free_first in steps:
            if free_first:                                         # the handles of the step before go; their memory may come back
                for k in list(mesh_h):
                    r.free_mesh(mesh_h.pop(k))
                r.free_material(mat_h)
                mat_h = None
            for d in draws(mesh, mat):
                key = d.indices is None
                if key not in mesh_h:
                    mesh_h[key] = r.upload_mesh(d.vertices, d.indices)
            if mat_h is None:
                mat_h = r.upload_material(mat.maps)
            sc = scene_of(draws(mesh, mat, order, n_inst), eye)
            r.set_frame_uniforms(sc.frame)
            r.set_view_uniforms(sc.view)
            per_frame = []
            for _ in range(3):
                c = r.static_record_counts()
                r.begin_frame()
                for d in sc.draws:
                    r.draw(mesh_h[d.indices is None], mat_h, d.instances)
                r.end_frame()
                per_frame.append(delta(r, c))
                out.append(r.read_framebuffer())
            if r.static_record_counts()["fills"] or per_frame[1] != (0, 0):
                assert per_frame == [(0, 0), (2, 2), (0, 2)], (name, per_frame)
        return out
    out, counts = both(script, 1)
    assert counts == {"fills": 2 * len(steps), "light_draws": 4 * len(steps)}
    for i, want in enumerate(wanted):
        for j in range(3):
            assert np.array_equal(bits(out[3 * i + j]), bits(want)), (steps[i][0], j)


# ---- read-backs and context changes ----
@pytest.mark.gpu
def test_read_backs_and_context_changes():
    """two frames in flight, the near-plane scene (half of each sphere is culled).  bbr_read_records between light-path frames:
    culled primitives keep the fill -- a fill of the static part, or a light-path record, would show -- and the next frames are
    right; then read_visibility, a resize, tile_mode 0, supersample 2 and a shadow-map pass, each followed by two frames."""
    w2, h2 = 120, 68
    def frames(r, h, sc, n=2):
        out = []
        for _ in range(n):
            r.render_scene(sc, h)
            out.append(r.read_framebuffer())
        return out
    def script(r, h):
        sc = near_scene(0)
        out = frames(r, h, sc, 5)                                  # (frames 2.. are on the light path)
        c = r.static_record_counts()
        recs, tris = r.read_records()
        assert delta(r, c) == (0, 0)                               # the dump itself: the full path, no fill
        culled = recs["material"] == FILL
        assert 60 <= culled.sum() <= 2 * N_SPHERE and (recs[culled].view(np.uint32) == FILL).all() and (tris[culled].view(np.uint32) == FILL).all()
        out += [recs, tris]
        out += frames(r, h, sc, 3)
        out += list(r.read_visibility())
        out += frames(r, h, sc)
        r.resize(w2, h2)
        out += frames(r, h, scene_of(base_draws(), (0.3, 0.5, -3.0), w=w2, h=h2))
        r.resize(W, H)
        r.set_option("tile_mode", 0)
        out += frames(r, h, sc)
        r.set_option("tile_mode", 1)
        r.set_option("supersample", 2)
        out += frames(r, h, scene_of(base_draws(), (0.3, 0.5, -3.0), w=2 * W, h=2 * H))
        r.set_option("supersample", 1)
        r.set_option("shadow_map", 64)
        r.render_scene(sc, h)
        lv = scenes.view_uniforms((0.5, 3.0, -2.0), 0.0, 0.0, 64, 64, 0, fov=90.0)
        lv["view"] = bbo.mat_look_at((0.5, 3.0, -2.0), (0.0, 0.0, 0.0))
        c = r.static_record_counts()
        r.render_shadow_map(0, lv, 0.002)
        assert delta(r, c) == (0, 0)                               # the map pass writes whole records into its own buffers
        out.append(r.read_shadow_map())
        c = r.static_record_counts()
        out += frames(r, h, sc)
        if c["fills"]:
            assert delta(r, c)[1] == 2 * N_DRAWS                   # both still on the light path
        return out
    out, counts = both(script, 2)
    assert counts["fills"] >= 2 * N_DRAWS and counts["light_draws"] >= 30, counts
    want = oracle(near_scene, 0)
    for i in (0, 1, 2, 3, 4, 7, 8, 9, 12, 13, 16, 17):
        assert np.array_equal(bits(out[i]), bits(want[0])), f"item {i}"
    assert np.array_equal(out[10], want[1]) and np.array_equal(bits(out[11]), bits(want[2]))
    small = bbo.render(scene_of(base_draws(), (0.3, 0.5, -3.0), w=w2, h=h2))[0]
    assert np.array_equal(bits(out[14]), bits(small)) and np.array_equal(bits(out[15]), bits(small))
    fine = bbo.render(scene_of(base_draws(), (0.3, 0.5, -3.0), w=2 * W, h=2 * H))[0]
    assert np.array_equal(bits(out[18]), bits(RR.resolve(fine, 2))) and np.array_equal(bits(out[19]), bits(RR.resolve(fine, 2)))
    assert len(np.unique(out[20])) > 10                            # (the map holds the spheres and the ground)


# ---- partition, overlay, deferred ----
@pytest.mark.gpu
@pytest.mark.parametrize("world", [2, 3])
def test_partition(world):
    """every rank rehearsed on the one device, bands of 32 rows (3 bands): the static part is written for every primitive,
    whichever rank owns it, and the shards of the light-path frames reassemble to the oracle's frames"""
    n, band = 5, 32
    shards = [[] for _ in range(n)]
    for rank in range(world):
        def script(r, h):
            r.set_partition(rank, world, band)
            out = []
            for k in range(n):
                r.render_scene(walk_scene(N_WALK - n + k), h)
                out.append(r.read_shard())
            return out
        out, counts = both(script, 1)
        assert counts == {"fills": N_DRAWS, "light_draws": N_DRAWS * (n - 1)}
        for k in range(n):
            shards[k].append(out[k])
    for k in range(n):
        frame = P.unpack_gathered(np.stack(shards[k]), H, band)
        assert np.array_equal(bits(frame), bits(oracle(walk_scene, N_WALK - n + k)[0])), f"frame {k}"


@pytest.mark.gpu
def test_overlay_pass_behind_a_light_path_frame():
    g = np.load(os.path.join(GOLDEN, "gizmo.npz"))
    gv = np.zeros(len(g["vertices"]), bbo.GIZMO_VERTEX_DTYPE)
    gv["pos"], gv["color"], gv["normal"] = g["vertices"][:, 0:3], g["vertices"][:, 3:6], g["vertices"][:, 6:9]
    n = 4
    def script(r, h):
        r.set_option("overlays", 1)
        r.upload_gizmo(g["vertices"], g["indices"])
        out = []
        for k in range(n):
            r.render_scene(walk_scene(k), h)
            r.present()
            r.draw_overlays(32)                                    # (the overlay pass: whole records into its own buffers)
            out += [r.read_presented(), r.read_framebuffer()]
        return out
    out, counts = both(script, 2)
    assert counts == {"fills": 2 * N_DRAWS, "light_draws": N_DRAWS * (n - 2)}
    for k in range(n):
        sc = walk_scene(k)
        frame, _, depth, _ = oracle(walk_scene, k)
        base = bbo.present(frame, int(sc.frame["enable_tone_mapping"]), float(sc.frame["exposure"]))
        want, _ = bbo.overlay(sc.frame, sc.view, depth, base, gv, g["indices"], 32)
        assert (want != base).any(axis=2).sum() > 50
        assert np.array_equal(out[2 * k], want) and np.array_equal(bits(out[2 * k + 1]), bits(frame)), f"frame {k}"


@pytest.mark.gpu
def test_deferred_pass():
    n = 5
    def script(r, h):
        r.set_option("render_pass", 1)
        out = []
        for k in range(n):
            r.render_scene(near_scene(k), h)
            out.append(r.read_framebuffer())
        out.append(r.read_gbuffer())
        return out
    out, counts = both(script, 2)
    assert counts["fills"] == 2 * N_DRAWS and counts["light_draws"] >= N_DRAWS * (n - 2)
    for k in range(n):
        assert np.array_equal(bits(out[k]), bits(bbo.render_deferred(near_scene(k))[0])), f"frame {k}"
    assert np.array_equal(bits(out[n]), bits(bbo.render_deferred(near_scene(n - 1))[1]))
