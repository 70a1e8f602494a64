"""GPU: option "surface_keep" -- under a kept view a frame slot stores its shaded surface once (k_surface_store) and the frames
behind it run the light loop alone on it (k_shade_lit; include/bibim_hip.h).

The frames, scenes, oracle and visibility model of tests/test_gpu_view_keep.py: 96 x 64 and 100 x 70, one small triangle per
named tile, on the long route ("no_tail_items" 0).  Every sequence runs on two contexts, "surface_keep" n and 0, both with
"view_keep" 1.  Every frame is read back and compared bit for bit with the CPU oracle and with the other context's frame,
bbr_get_stats and bbr_view_keep_counts with the other context's (a lit frame is a kept frame), and bbr_surface_keep_counts with
a host-side model of what each frame slot holds:

    run      the slot's kept frames in a row that could be lit (the plain shading kernel, the long route), under the normal-map
             switch of the slot's last frame; a full frame, a kept frame that could not be lit and one under another switch
             start it again, and so does whatever makes the slot forget its visibility
    stored   the frame that makes the run n long; it and every frame of the run behind it are lit

The context with the option at 0 counts (0, 0) throughout."""
import functools

import numpy as np
import pytest

import test_gpu_late_clip_slot as LC
import test_gpu_view_keep as VK
from bibim_renderer_amd import Renderer
from bibim_renderer_amd._capi import BibimError
from bibim_renderer_amd.renderer import live_resources
from oracle import bbo, scenes

pytestmark = pytest.mark.gpu

SIZES = VK.SIZES
ONE, TWO = VK.ONE, VK.TWO
L0, L1, L2 = VK.L0, VK.L1, VK.L2


def bits(a):
    """bit for bit; a NaN by its place (a light on a surface point makes some)"""
    a = np.ascontiguousarray(a, np.float32)
    return np.where(np.isnan(a), np.uint32(0x7FC00000), a.view(np.uint32))


LONG = {"no_tail_items": 0}
NO_PIXEL = 0xFFFFFFFF


class SurfaceModel:
    def __init__(self, fif, n):
        self.fif, self.n = fif, n
        self.run, self.valid, self.normal_map = [0] * fif, [False] * fif, [0] * fif

    def forget(self):
        self.run, self.valid = [0] * self.fif, [False] * self.fif

    def frame(self, slot, kept, could, normal_map):
        """(stored, lit) of the next frame of `slot`"""
        out = (0, 0)
        if not (kept and could and self.n > 0) or normal_map != self.normal_map[slot]:
            self.run[slot], self.valid[slot] = 0, False
        elif self.valid[slot]:
            out = (0, 1)
        else:
            self.run[slot] += 1
            if self.run[slot] >= self.n:
                self.valid[slot], out = True, (1, 1)
        self.normal_map[slot] = normal_map
        return out


class Pair:
    """the same calls on a context with "surface_keep" n and one with 0, the visibility model of both and the surface model of
    the first"""

    def __init__(self, w, h, fif, n, **options):
        self.w, self.h = w, h
        self.r = [Renderer(w, h), Renderer(w, h)]
        self.handles = [{"mesh": {}, "mat": {}}, {"mesh": {}, "mat": {}}]
        self.vis, self.surf = VK.Model(fif), SurfaceModel(fif, n)
        self.stored = self.lit = 0
        for keep, r in zip((n, 0), self.r):
            r.set_option("frames_in_flight", fif)
            for name, value in {**LONG, **options}.items():
                r.set_option(name, value)
            r.set_option("surface_keep", keep)

    def both(self, call):
        for r in self.r:
            call(r)

    def set_n(self, n):
        """the option itself: the slots keep their visibility and forget their surfaces"""
        self.r[0].set_option("surface_keep", n)
        self.r[1].set_option("surface_keep", 0)
        self.surf.forget()
        self.surf.n = n

    def forget(self):
        self.vis.forget()
        self.surf.forget()

    def frame(self, key, what="", could=True, scene=None, want=None, **model):
        """one frame of VK.scene(*key) (or `scene`, with `want` its oracle frame) on both -> (frame, (stored, lit))"""
        c0, s0 = self.r[0].view_keep_counts(), self.r[0].surface_keep_counts()
        for r, handles in zip(self.r, self.handles):
            r.render_scene(VK.scene(*key) if scene is None else scene, handles)
        got = [r.read_framebuffer() for r in self.r]
        kept = self.vis.frame(key, **model)
        normal_map = int((VK.scene(*key) if scene is None else scene).view["enable_normal_map"])
        expect = self.surf.frame(self.vis.last, kept, could, normal_map)
        c1, s1 = self.r[0].view_keep_counts(), self.r[0].surface_keep_counts()
        assert (c1["kept"] - c0["kept"], c1["full"] - c0["full"]) == ((1, 0) if kept else (0, 1)), f"{what}: view counters {c0} -> {c1}, model kept={kept}"
        assert (s1["stored"] - s0["stored"], s1["lit"] - s0["lit"]) == expect, f"{what}: surface counters {s0} -> {s1}, model {expect}"
        assert np.array_equal(bits(got[0]), bits(VK.oracle(*key) if want is None else want)), f"{what}: pixels differ from the oracle"
        assert np.array_equal(bits(got[0]), bits(got[1])), f"{what}: surface_keep n and 0 differ"
        assert self.r[0].stats() == self.r[1].stats(), f"{what}: statistics differ"
        assert self.r[1].view_keep_counts() == c1, f"{what}: a lit frame is a kept frame"
        assert self.r[1].surface_keep_counts() == {"stored": 0, "lit": 0}
        self.stored += expect[0]
        self.lit += expect[1]
        return got[0], expect

    def settle(self, key, what="settling"):
        """until every slot's frame is lit (n >= 1)"""
        for k in range((3 + self.surf.n) * self.surf.fif):
            _, e = self.frame(key, f"{what}, frame {k}")
        assert e == (0, 1), (what, e)

    def close(self, used=True):
        assert not used or (self.stored > 0 and self.lit > self.stored), (self.stored, self.lit)
        for r in self.r:
            r.close()


# ---- 1. identical frames ----
@pytest.mark.parametrize("layout", [0, 1, 2])
@pytest.mark.parametrize("fif", [1, 2, 3, 4])
def test_identical_frames_store_on_the_nth_kept_frame_and_are_lit_behind_it(fif, layout):
    w, h = SIZES[fif % 2]
    p = Pair(w, h, fif, 1, stream_layout=layout)
    key = (w, h, TWO)
    for k in range(2 * fif):
        assert p.frame(key, f"frame {k}")[1] == (0, 0)
    for n in (1, 2, 3):
        if n > 1:
            p.set_n(n)     # (every slot's next frame is still a kept one)
        for k in range((n + 2) * fif):
            _, e = p.frame(key, f"n = {n}, frame {k}")
            assert e == ((0, 0) if k < (n - 1) * fif else (1, 1) if k < n * fif else (0, 1)), (n, k, e)
    p.close()


# ---- 2. lit frames under new lights and shading parameters ----
def world(w, h, px, py, z):
    """the point at depth z that the camera of VK.scene sees at pixel position (px, py) (SK.mesh's: the projection turns y over)"""
    return ((px / (w / 2) - 1.0) * VK.SK.TAN * (w / h) * z, (1.0 - py / (h / 2)) * VK.SK.TAN * z, z)


@functools.lru_cache(None)
def lights_scene(w, h, which, tone=0, exposure=1.0):
    """VK.scene(w, h, TWO) under light sets VK.scene cannot name"""
    base = VK.scene(w, h, TWO)
    covered = bbo.render(base)[1] != bbo.NO_PRIM
    y, x = np.argwhere(covered)[len(np.argwhere(covered)) // 2]
    on_surface = world(w, h, x + 0.5, y + 0.5, 2.0)   # the triangles stand at z = 2 (SK.mesh): a covered pixel's centre on that plane
    sets = {
        "spot": [scenes.light(1, pos=(0.2, 0.3, 0.0), dir=(-0.1, -0.1, 1.0), color=(1.0, 0.5, 0.2), intensity=20.0, inner=0.95, outer=0.6)],
        "directional": [scenes.light(2, dir=(0.3, 0.4, -0.8), color=(0.3, 0.8, 1.0), intensity=3.0)],
        "unknown type": [scenes.light(7, pos=(0.0, 0.0, 0.5), color=(1.0, 1.0, 1.0), intensity=5.0), scenes.light(0, pos=L1[0], color=L1[1], intensity=L1[2])],
        "on the surface": [scenes.light(0, pos=tuple(float(v) for v in on_surface), color=(1.0, 1.0, 1.0), intensity=2.0)],
    }
    fu = scenes.frame_uniforms(sets[which], tone, exposure)
    sc = bbo.Scene(fu, base.view, base.draws, w, h, f"surface keep, {which}")
    frame = bbo.render(sc)[0]
    frame.setflags(write=False)
    return sc, frame


@pytest.mark.parametrize("layout", [0, 1, 2])
def test_lights_exposure_and_tone_mapping_change_under_a_lit_run(layout):
    w, h = SIZES[1]
    fif = 2
    p = Pair(w, h, fif, 1, stream_layout=layout)
    p.settle((w, h, TWO))
    moved = ((0.1, 0.4, 0.3),) + L0[1:]
    recoloured = (moved[0], (0.1, 0.2, 1.0), 11.0)
    for lights in [(moved,), (recoloured,), (recoloured, L1, L2), (), (L2,), (L2, L0), (L1, L0)]:
        assert p.frame((w, h, TWO, lights), f"{len(lights)} lights")[1] == (0, 1)
    for which in ("spot", "directional", "unknown type", "on the surface"):
        for tone, exposure in ((0, 1.0), (1, 1.7)):
            sc, want = lights_scene(w, h, which, tone, exposure)
            assert p.frame((w, h, TWO), f"{which}, tone mapping {tone}", scene=sc, want=want)[1] == (0, 1)
    assert p.frame((w, h, TWO, (L1,), 0.0, 1, 0.0, False, 1, 1.7), "tone mapping")[1] == (0, 1)
    p.close()


# ---- 3. the normal-map switch ----
@pytest.mark.parametrize("n", [1, 2])
def test_the_normal_map_switch_starts_the_run_again(n):
    w, h = SIZES[0]
    fif = 2
    p = Pair(w, h, fif, n)
    p.settle((w, h, TWO))
    for normal_map in (0, 1, 0):
        key = (w, h, TWO, (L0, L1), 0.0, normal_map)
        history = [p.frame(key, f"normal map {normal_map}, frame {k}")[1] for k in range((n + 2) * fif)]
        assert history == [(0, 0)] * (n * fif) + [(1, 1)] * fif + [(0, 1)] * fif, history   # kept and not lit, stored after n, lit
    p.close()


# ---- 4. forgetting ----
def ev_camera_step(p, key):
    return key[:3] + ((L0,), 0.25)


def ev_instance_matrix(p, key):
    return key[:3] + ((L0,), 0.0, 1, 0.01)


def ev_material_upload(p, key):
    p.both(lambda r: r.upload_material(VK.other_material().maps))
    p.vis.forget_statics()
    return key


def ev_resize_and_back(p, key):
    p.both(lambda r: r.resize(SIZES[1][0], SIZES[1][1]))
    p.both(lambda r: r.resize(p.w, p.h))
    p.forget()
    return key


def ev_read_surface(p, key):
    for r in p.r:
        r.read_surface()
    p.forget()
    p.vis.frame(key, slot=p.vis.last)   # the diagnostic re-render: a full frame in the last frame's slot, and one to keep behind
    return key


def ev_surface_keep_itself(p, key):
    p.set_n(p.surf.n)
    return key


def option_event(name, value):
    def ev(p, key):
        p.both(lambda r: r.set_option(name, value))
        p.forget()
        return key
    ev.__name__ = f"ev_{name}"
    return ev


def ev_mip_levels(p, key):
    """the one option of the FULL column that leaves the visibility: an accepted value starts a new resource epoch, so the draws
    are new ones -- two frames in full per slot, as behind a material upload"""
    p.both(lambda r: r.set_option("mip_levels", 1))
    p.vis.forget_statics()
    return key


# test_gpu_option_chart.py's FULL column, each set to the value it has ("mip_levels": above)
FULL_OPTIONS = [("frames_in_flight", 2), ("tile_mode", 1), ("bin_cap", 512), ("ablate", 0), ("supersample", 1), ("sample_shading", 1), ("depth_resolve", 0),
                ("present_fused", 0), ("overlays", 0), ("tbn", 0), ("stream_layout", 2), ("no_tail_items", 0), ("heavy_tiles", -1),
                ("broad_cap", 4096), ("clip_cap", 4096), ("broad_threshold", 16)]
EVENTS = [ev_camera_step, ev_instance_matrix, ev_material_upload, ev_resize_and_back, ev_read_surface, ev_surface_keep_itself] + \
         [option_event(*o) for o in FULL_OPTIONS] + [ev_mip_levels]


@pytest.fixture(scope="module")
def lit_pair():
    w, h = SIZES[0]
    p = Pair(w, h, 2, 1)
    p.settle((w, h, ONE))
    yield p
    p.close()


@pytest.mark.parametrize("event", EVENTS, ids=lambda e: e.__name__[3:])
def test_not_lit_then_lit_again(lit_pair, event):
    p = lit_pair
    w, h = p.w, p.h
    fif = p.surf.fif
    if event.__name__ == "ev_frames_in_flight":
        p.vis.k = 0                              # (frames go to the slots in turn from the moment the option was set)
    key = event(p, (w, h, ONE))
    history = [p.frame(key, f"frame {k} behind the event")[1] for k in range(4 * fif)]
    # the next frame is not lit -- but for the option itself, which leaves the visibility: with n = 1 the next kept frame stores
    assert history[0] == ((1, 1) if event is ev_surface_keep_itself else (0, 0)), history
    assert history[-fif:] == [(0, 1)] * fif and history.count((1, 1)) == fif, history
    p.settle((w, h, ONE), "back to the first view")


def test_nothing_is_lit_across_a_capacity_growth():
    """VK's overflow: the read finds it, the capacities grow, every slot forgets and the frame is rendered again, in full"""
    w, h = SIZES[0]
    sc = VK.SK.heavy_scene(1)
    want = bbo.render(sc)[0]
    rs = [Renderer(w, h), Renderer(w, h)]
    got = []
    for n, r in zip((1, 0), rs):
        for name, value in (("frames_in_flight", 1), ("no_tail_items", 0), ("bin_cap", 16), ("surface_keep", n)):
            r.set_option(name, value)
        handles = {"mesh": {}, "mat": {}}
        history = []
        for k in range(5):
            s0 = r.surface_keep_counts()
            r.render_scene(sc, handles)
            assert np.array_equal(bits(r.read_framebuffer()), bits(want)), (n, k)
            s1 = r.surface_keep_counts()
            history.append((s1["stored"] - s0["stored"], s1["lit"] - s0["lit"]))
        got.append(history)
        assert r.capacity_growths() >= 1
        r.close()
    # frame 0 overflows and is rendered again (full); frames 1 .. 3 are the slot's second .. fourth of a kind: kept from frame 1
    assert got == [[(0, 0), (1, 1), (0, 1), (0, 1), (0, 1)], [(0, 0)] * 5], got


# ---- 5. every route into a fragment, 6. the stored planes ----
@functools.lru_cache(None)
def routes_scene():
    """96 x 64, 3 x 2 tiles, two draws: a triangle that covers the top row of tiles and part of the bottom right one (whole tiles:
    kFullTile items, uniform waves; a partly covered tile: a list whose last item is partly filled), under the packed material;
    and in front of it, under a mixed one (maps of different sizes), a small triangle and one that crosses the near plane (a clip
    slot in the fragment word)"""
    w, h = SIZES[0]
    m = LC.materials()

    def verts(tris, z_uv):
        v = np.zeros(len(tris), bbo.VERTEX_DTYPE)
        v["pos"] = np.asarray(tris, np.float32)
        v["uv"] = np.linspace(0.0, z_uv, 2 * len(v)).reshape(-1, 2)
        v["normal"], v["tangent"] = (0, 0, -1), (1, 0, 0)
        return v
    big = verts([world(w, h, -20.0, -20.0, 3.0), world(w, h, 200.0, -20.0, 3.0), world(w, h, -20.0, 150.0, 3.0)], 3.0)
    small = verts([world(w, h, 88.0, 56.0, 2.0), world(w, h, 72.0, 56.0, 2.0), world(w, h, 80.0, 40.0, 2.0),
                   (0.1, 0.4, 1.5), (0.5, 0.4, 1.5), (0.3, -1.0, -0.5)], 1.0)   # the second one's apex: behind the camera
    inst = np.zeros(1, bbo.INSTANCE_DTYPE)
    inst[0] = scenes.instance(np.eye(4, dtype=np.float32))
    fu = scenes.frame_uniforms([scenes.light(0, pos=L0[0], color=L0[1], intensity=L0[2])], 0, 1.0)
    vu = scenes.view_uniforms((0, 0, 0), 0, 0, w, h, 1)
    return bbo.Scene(fu, vu, [bbo.DrawData(big, None, inst, bbo.MaterialData(m["packed"])), bbo.DrawData(small, None, inst, bbo.MaterialData(m["mixed"]))],
                     w, h, "surface keep routes")


def relit(sc, lights):
    fu = scenes.frame_uniforms([scenes.light(0, pos=p, color=c, intensity=i) for p, c, i in lights], int(sc.frame["enable_tone_mapping"]), float(sc.frame["exposure"]))
    return bbo.Scene(fu, sc.view, sc.draws, sc.width, sc.height, sc.name + ", relit")


ROUTE_SCENES = {"routes": routes_scene, "late clip slot, packed": lambda: LC.scene("packed"), "late clip slot, mixed": lambda: LC.scene("mixed")}


def test_the_routes_scene_has_every_route():
    sc = routes_scene()
    _, prim, _, stats = bbo.render(sc)
    covered = prim != bbo.NO_PRIM
    assert covered[:32].all(), "no whole tile"
    assert covered[32:, 64:].any() and not covered[32:, 64:].all(), "no partly covered tile"
    assert stats["n_clipped_prims"] >= 1 and (prim == 1).any() and (prim == 2).any(), "the mixed draw's triangles: one clipped, both seen"


@pytest.mark.parametrize("which", list(ROUTE_SCENES))
def test_every_route_into_a_fragment_lit_and_the_stored_planes(which):
    sc = ROUTE_SCENES[which]()
    w, h = sc.width, sc.height
    frames = [sc, relit(sc, (L1, L2)), relit(sc, ())]
    rs = [Renderer(w, h), Renderer(w, h)]
    handles = [{"mesh": {}, "mat": {}}, {"mesh": {}, "mat": {}}]
    for n, r in zip((1, 0), rs):
        for name, value in (("frames_in_flight", 1), ("no_tail_items", 0), ("surface_keep", n)):
            r.set_option(name, value)
    for k, frame in enumerate([sc, sc, sc] + frames):
        want, want_prim = bbo.render(frame)[:2]
        got = []
        for r, hd in zip(rs, handles):
            r.render_scene(frame, hd)
            got.append(r.read_framebuffer())
        assert np.array_equal(bits(got[0]), bits(want)), f"{which}, frame {k}: pixels differ from the oracle"
        assert np.array_equal(bits(got[0]), bits(got[1])) and rs[0].stats() == rs[1].stats(), f"{which}, frame {k}"
    assert rs[0].surface_keep_counts() == {"stored": 1, "lit": 4} and rs[1].surface_keep_counts() == {"stored": 0, "lit": 0}
    assert rs[0].view_keep_counts() == rs[1].view_keep_counts() == {"kept": 4, "full": 2}

    # the stored planes (read first: read_surface renders again, and forgets)
    with pytest.raises(BibimError):
        rs[1].read_surface_keep(0)
    with pytest.raises(BibimError):
        rs[0].read_surface_keep(1)
    values, index = rs[0].read_surface_keep(0)
    record = rs[0].read_surface()
    with pytest.raises(BibimError):
        rs[0].read_surface_keep(0)
    for r in rs:
        r.close()
    valid = index != NO_PIXEL
    shaded = np.flatnonzero((want_prim != bbo.NO_PRIM).reshape(-1))
    assert np.array_equal(np.sort(index[valid]), shaded), "the valid lanes cover the oracle's shaded pixels exactly once"
    if which == "routes":
        assert not valid.all(), "no partly filled item"
    assert np.array_equal(bits(values[valid]), bits(record.reshape(-1, 32)[index[valid], 6:18])), "P, normal, albedo, metallic, roughness, ao"


# ---- 7. modes that are never lit ----
def _fused(r):
    r.set_option("present_fused", 1)


def _deferred(r):
    r.set_option("render_pass", 1)


def _supersample(r):
    r.set_option("supersample", 2)


def _partition(r):
    r.set_partition(0, 2, 32)


def _short(r):
    r.set_option("no_tail_items", 40000)


def _aniso(r):
    r.set_option("max_anisotropy", 2)


def _mip(r):
    r.set_option("mip_levels", 2)


def _shadow(r):
    r.set_option("shadow_map", 64)


@pytest.mark.parametrize("mode", [_fused, _deferred, _supersample, _partition, _short, _aniso, _mip, _shadow], ids=lambda f: f.__name__[1:])
def test_modes_that_are_never_lit(mode):
    w, h = SIZES[0]
    sc = VK.scene(w, h, TWO)
    out = []
    for n in (1, 0):
        r = Renderer(w, h)
        for name, value in (("frames_in_flight", 1), ("no_tail_items", 0), ("surface_keep", n)):
            r.set_option(name, value)
        mode(r)
        handles = {"mesh": {}, "mat": {}}
        frames = []
        for k in range(5):
            r.render_scene(sc, handles)
            if mode is _shadow and k == 0:
                r.render_shadow_map(0, VK._light_view(64), 0.01)
            frames.append(r.read_presented() if mode is _fused else r.read_shard() if mode is _partition else r.read_framebuffer())
        out.append((frames, r.stats(), r.view_keep_counts(), live_resources()["device_allocs"]))
        assert r.surface_keep_counts() == {"stored": 0, "lit": 0}, mode.__name__
        r.close()
    (fa, sa, va, la), (fb, sb, vb, lb) = out
    assert all(np.array_equal(a, b, equal_nan=True) for a, b in zip(fa, fb)), "frames are unchanged"
    assert sa == sb and va == vb
    assert la == lb, "no surface buffer appears in the live counts"
    if mode in (_short, _aniso, _mip):
        assert va["kept"] >= 2    # (kept frames, shaded by the other kernels)
