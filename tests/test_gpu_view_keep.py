"""GPU: option "view_keep" -- a frame whose view, draws and geometry parameters are those its frame slot rendered last launches
its shading only (include/bibim_hip.h).

The frames and scenes of tests/test_gpu_sky_keep.py: 96 x 64 and 100 x 70, one small triangle per named tile, a 16-texel
material.  Every sequence runs on two contexts, "view_keep" 1 and 0.  Every frame is read back and compared bit for bit with
the CPU oracle and with the other context's frame, bbr_get_stats with the other context's, and bbr_view_keep_counts with a
host-side model of what each frame slot holds:

    the draws   are on the light path with nothing to fill from the slot's third frame in a row with the same descriptors,
                instance blocks and resources on (plan_static_records: key new -> key repeated, fill -> filled)
    a frame     is kept iff its draws are, its view is the one of the slot's last frame that was rendered in full, that
                frame could be kept behind, nothing forgot in between, and the frame itself may be kept

Every run asserts that it kept something and rendered something in full.  The frames shaded by the other kernels
("max_anisotropy" 2, "mip_levels" 2, a one-face shadow map) use inputs for which those kernels' rules give the plain frame:
magnified textures (one tap at level 0) and a light with nothing between it and the triangles (every fragment lit)."""
import functools

import numpy as np
import pytest

import test_gpu_sky_keep as SK
from bibim_renderer_amd import Renderer, textures
from oracle import bbo, scenes

SIZES = SK.SIZES
ONE = ((1, 0),)
TWO = ((0, 0), (2, 1))
L0 = ((0.3, 0.5, 0.0), (1.0, 0.9, 0.8), 6.0)          # (position, colour, intensity) of a point light
L1 = ((-0.4, 0.2, 0.5), (0.2, 1.0, 0.4), 9.0)
L2 = ((0.0, -0.6, 1.0), (0.9, 0.1, 1.0), 4.0)
bits = SK.bits


@functools.lru_cache(None)
def other_material():
    return bbo.MaterialData(textures.make_material(16))


@functools.lru_cache(None)
def instances(shift):
    inst = np.zeros(1, bbo.INSTANCE_DTYPE)
    inst[0] = scenes.instance(bbo.mat_translate(float(shift), 0.0, 0.0))
    return inst


@functools.lru_cache(None)
def scene(w, h, tiles, lights=(L0,), yaw=0.0, normal_map=1, shift=0.0, other_mat=False, tone=0, exposure=1.0):
    fu = scenes.frame_uniforms([scenes.light(0, pos=p, color=c, intensity=i) for p, c, i in lights], tone, exposure)
    vu = scenes.view_uniforms((0, 0, 0), yaw, 0, w, h, normal_map)
    mat = other_material() if other_mat else SK.material()
    return bbo.Scene(fu, vu, [bbo.DrawData(SK.mesh(w, h, tiles), None, instances(shift), mat)], w, h, "view keep")


@functools.lru_cache(None)
def oracle(*key):
    frame = bbo.render(scene(*key))[0]
    frame.setflags(write=False)
    return frame


def draws_key(key):
    """what plan_static_records compares of scene(*key): mesh, instance block, material"""
    k = dict(zip(("w", "h", "tiles", "lights", "yaw", "normal_map", "shift", "other_mat"), key))
    return (k["w"], k["h"], k["tiles"], k.get("shift", 0.0), k.get("other_mat", False))


def view_key(key):
    k = dict(zip(("w", "h", "tiles", "lights", "yaw"), key))
    return (k["w"], k["h"], k.get("yaw", 0.0))


class Model:
    """what each frame slot remembers; frames go to slots in turn from the moment "frames_in_flight" was set"""

    def __init__(self, fif):
        self.fif, self.k, self.last = fif, 0, 0
        self.draws = [None] * fif   # the draws key of the slot's last frame
        self.run = [0] * fif        # ... and how many frames in a row have had it
        self.view = [None] * fif    # the view the slot's visibility is of; None: forgotten, or no frame to keep behind

    def forget(self):
        self.view = [None] * self.fif

    def forget_statics(self):
        self.draws = [None] * self.fif

    def frame(self, key, slot=None, may=True, behind=True, statics=True):
        """is the next frame kept?  slot: a re-render into that slot; may: the frame itself may be kept; behind: a frame may be
        kept behind it; statics: option "static_records" """
        if slot is None:
            slot = self.k % self.fif
            self.k += 1
        self.last = slot
        if not statics:
            self.draws[slot] = None
        elif self.draws[slot] == draws_key(key):
            self.run[slot] += 1
        else:
            self.draws[slot], self.run[slot] = draws_key(key), 1
        kept = statics and self.run[slot] >= 3 and may and behind and self.view[slot] == view_key(key)
        if not kept:
            self.view[slot] = view_key(key) if behind else None
        return kept


class Pair:
    """the same calls on a context with "view_keep" 1 and one with 0, and the model of the first"""

    def __init__(self, w, h, fif, **options):
        self.w, self.h = w, h
        self.r = [Renderer(w, h), Renderer(w, h)]
        self.handles = [{"mesh": {}, "mat": {}}, {"mesh": {}, "mat": {}}]
        self.model = Model(fif)
        self.kept = self.full = 0
        for keep, r in zip((1, 0), self.r):
            r.set_option("frames_in_flight", fif)
            r.set_option("view_keep", keep)
            for name, value in options.items():
                r.set_option(name, value)

    def both(self, call):
        for r in self.r:
            call(r)

    def submit(self, key, record=None):
        for r, handles in zip(self.r, self.handles):
            if record is None:
                r.render_scene(scene(*key), handles)
            else:
                record(r, handles)

    def frame(self, key, what="", want=None, record=None, **model):
        """one frame of scene(*key) on both: pixels against the oracle (want: another reference; False: none) and against each
        other, statistics against each other, the counters against the model.  Returns the frame and whether it was kept."""
        c0 = self.r[0].view_keep_counts()
        g0 = self.r[0].capacity_growths()
        self.submit(key, record)
        got = [r.read_framebuffer() for r in self.r]
        kept = self.model.frame(key, **model)
        if self.r[0].capacity_growths() != g0:   # the read found an overflow: grown, every slot forgot, rendered again in its slot
            self.model.forget()
            assert not kept, f"{what}: the model keeps a frame that overflowed"
            self.model.frame(key, slot=self.model.last, **model)
            self.full += 1
            c0["full"] += 1
        c1 = self.r[0].view_keep_counts()
        assert (c1["kept"] - c0["kept"], c1["full"] - c0["full"]) == ((1, 0) if kept else (0, 1)), f"{what}: counters {c0} -> {c1}, model kept={kept}"
        self.kept += kept
        self.full += not kept
        if want is not False:
            assert np.array_equal(bits(got[0]), bits(oracle(*key) if want is None else want)), f"{what}: pixels differ from the oracle"
        assert np.array_equal(bits(got[0]), bits(got[1])), f"{what}: view_keep 1 and 0 differ"
        assert self.r[0].stats() == self.r[1].stats(), f"{what}: statistics differ"
        assert self.r[1].view_keep_counts()["kept"] == 0
        return got[0], kept

    def close(self):
        assert self.kept > 0 and self.full > 0, (self.kept, self.full)
        for r in self.r:
            r.close()


ROUTES = {"short": {}, "long": {"no_tail_items": 0}}   # 96 x 64: 96 item slots, below and above "no_tail_items"
# ... and the long route with the stages of a frame on streams of their own: the copy, the light table and the tail launch on
# one, the main launch on another ("stream_layout" 0 and 1)
LAYOUTS = {**ROUTES, "long, stage streams": {"no_tail_items": 0, "stream_layout": 0},
           "long, raster stream": {"no_tail_items": 0, "stream_layout": 1}}


# ---- 1. identical frames ----
@pytest.mark.gpu
@pytest.mark.parametrize("route", list(ROUTES))
@pytest.mark.parametrize("fif", [1, 2, 3, 4])
def test_identical_frames_are_kept_from_the_third_of_a_slot(fif, route):
    w, h = SIZES[fif % 2]
    p = Pair(w, h, fif, **ROUTES[route])
    key = (w, h, TWO)
    for k in range(4 * fif):
        _, kept = p.frame(key, f"frame {k}")
        assert kept == (k >= 2 * fif)
    if p.model.fif == 1:   # a kept frame reports every background tile as kept
        t = p.r[0].read_sky_tiles()
        assert (t == SK.KEPT).sum() == t.size - len(TWO) and (t == SK.FILLED).sum() == 0
    p.close()


# ---- 2. same view, new shading inputs ----
@pytest.mark.gpu
@pytest.mark.parametrize("route", list(LAYOUTS))
def test_lights_and_shading_parameters_change_under_a_kept_view(route):
    w, h = SIZES[1]
    fif = 2
    p = Pair(w, h, fif, **LAYOUTS[route])
    moved = ((0.1, 0.4, 0.3),) + L0[1:]
    recoloured = (moved[0], (0.1, 0.2, 1.0), 11.0)
    light_sets = [(L0,), (moved,), (recoloured,), (recoloured, L1, L2), (), (L2,), (L2,), (L2, L0), (L1, L0)]
    k = 0
    for lights in [(L0,)] * (2 * fif) + light_sets:
        for normal_map in (1, 0) if k >= 2 * fif else (1,):
            _, kept = p.frame((w, h, TWO, lights, 0.0, normal_map), f"frame {k}, {len(lights)} lights, normal map {normal_map}")
            assert kept == (k >= 2 * fif)
            k += 1
    # tone mapping and exposure are the frame block's: shading parameters of the deferred path and the presentation only
    _, kept = p.frame((w, h, TWO, (L1,), 0.0, 1, 0.0, False, 1, 1.7), "tone mapping")
    assert kept
    p.close()


# ---- 3. a kept frame shaded by the other kernels ----
def _light_view(side):
    lv = scenes.view_uniforms(L0[0], 0.0, 0.0, side, side, 0, fov=120.0)
    lv["view"] = bbo.mat_look_at(L0[0], (L0[0][0], L0[0][1], 2.0))
    return lv


def _aniso(p):
    p.both(lambda r: r.set_option("max_anisotropy", 2))


def _mip(p):
    p.both(lambda r: r.set_option("mip_levels", 2))
    p.model.forget_statics()      # (the chains: every material is another resource)


def _shadow(p):
    p.both(lambda r: r.set_option("shadow_map", 64))
    p.both(lambda r: r.render_shadow_map(0, _light_view(64), 0.01))
    for r in p.r:                 # nothing stands between the light and the triangles
        assert (r.read_shadow_mask()[bbo.render(scene(p.w, p.h, TWO))[1] != bbo.NO_PRIM] == 1).all()
    p.model.forget()              # (the mask's re-render: a diagnostic frame, and it forgets)
    p.model.frame((p.w, p.h, TWO), slot=p.model.last)
    p.full += 1


@pytest.mark.gpu
@pytest.mark.parametrize("switch", [_aniso, _mip, _shadow], ids=lambda f: f.__name__[1:])
def test_a_kept_frame_is_shaded_by_the_other_kernels(switch):
    w, h = SIZES[0]
    p = Pair(w, h, 1)
    key = (w, h, TWO)
    for k in range(3):
        p.frame(key, f"frame {k}")
    switch(p)
    kept_since = 0
    for k in range(4):
        _, kept = p.frame((w, h, TWO, (L0,) if k < 2 else (L0, L1)), f"frame {k} behind the switch")
        kept_since += kept
    assert kept and kept_since >= 2
    if switch is _aniso:
        assert kept_since == 4    # nothing but the kernel changed
    p.close()


# ---- 4. not kept, then kept again ----
def ev_camera_step(p, key):
    return key[:3] + ((L0,), 0.25), None


def ev_instance_matrix(p, key):
    return key[:3] + ((L0,), 0.0, 1, 0.01), None


def ev_material_rebound(p, key):
    p.model.forget_statics()      # (the new material's upload)
    return key[:3] + ((L0,), 0.0, 1, 0.0, True), None


def ev_material_upload(p, key):
    p.both(lambda r: r.upload_material(other_material().maps))
    p.model.forget_statics()
    return key, None


def ev_read_visibility(p, key):
    want = bbo.render(scene(*key))[1]
    for r in p.r:
        assert np.array_equal(r.read_visibility()[0], want)
    p.model.forget()
    p.model.frame(key, slot=p.model.last, may=False, behind=False)
    p.full += 1
    return key, None


def ev_resize_and_back(p, key):
    p.both(lambda r: r.resize(SIZES[1][0], SIZES[1][1]))
    p.both(lambda r: r.resize(p.w, p.h))
    p.model.forget()
    return key, None


def ev_tile_mode_and_back(p, key):
    p.both(lambda r: r.set_option("tile_mode", 0))
    p.both(lambda r: r.set_option("tile_mode", 1))
    p.model.forget()
    return key, None


def ev_static_records_off(p, key):
    p.both(lambda r: r.set_option("static_records", 0))
    for k in range(p.model.fif):
        _, kept = p.frame(key, f"static_records 0, frame {k}", statics=False)
        assert not kept
    p.both(lambda r: r.set_option("static_records", 1))
    return key, None


def ev_timing_1(p, key):
    p.both(lambda r: r.set_option("timing", 1))
    for k in range(p.model.fif + 1):
        _, kept = p.frame(key, f"timing 1, frame {k}", may=False)
        assert not kept
    for r in p.r:
        n, frame_ms, geometry_ms, raster_ms, shade_ms = r.timing_summary()
        assert n == p.model.fif + 1 and min(frame_ms, geometry_ms, raster_ms, shade_ms) > 0.0
    p.both(lambda r: r.set_option("timing", 0))
    return key, [True] * 6          # every stage ran, and a frame may be kept behind such a frame


def ev_queued_caster(p, key):
    p.both(lambda r: r.set_option("shadow_map", 64))

    def record(r, handles):
        sc = scene(*key)
        r.set_frame_uniforms(sc.frame)
        r.set_view_uniforms(sc.view)
        r.begin_frame()
        d = sc.draws[0]
        r.draw(handles["mesh"][id(d.vertices)], handles["mat"][id(d.material)], d.instances)
        r.queue_shadow_caster(0, 0, _light_view(64), 0.01)
        r.end_frame()
    _, kept = p.frame(key, "the frame with the queued caster", record=record, may=False, behind=False)
    assert not kept
    # the other slot still holds this view (a valid map is shading's business); the caster's slot has no frame to keep behind
    return key, [True, False, True, True, True, True]


EVENTS = [ev_camera_step, ev_instance_matrix, ev_material_rebound, ev_material_upload, ev_read_visibility, ev_resize_and_back,
          ev_tile_mode_and_back, ev_static_records_off, ev_timing_1, ev_queued_caster]


@pytest.mark.gpu
@pytest.mark.parametrize("event", EVENTS, ids=lambda e: e.__name__[3:])
def test_not_kept_then_kept_again(event):
    w, h = SIZES[0]
    fif = 2
    p = Pair(w, h, fif)
    key = (w, h, ONE)
    for k in range(3 * fif):
        _, kept = p.frame(key, f"frame {k}")
    assert kept
    key, expected = event(p, key)
    history = []
    for k in range(3 * fif):
        history.append(p.frame(key, f"frame {k} behind the event")[1])
    if expected:
        assert history == expected, history
    else:
        assert not any(history[:fif]) and all(history[2 * fif:]), history   # a full frame per slot at least, then kept again
    p.close()


# ---- 5. each of the two options without the other ----
@pytest.mark.gpu
@pytest.mark.parametrize("view_keep,sky_keep", [(1, 0), (0, 1)])
def test_view_keep_and_sky_keep_do_not_need_each_other(view_keep, sky_keep):
    w, h = SIZES[1]
    r = Renderer(w, h)
    r.set_option("frames_in_flight", 2)
    r.set_option("view_keep", view_keep)
    r.set_option("sky_keep", sky_keep)
    handles = {"mesh": {}, "mat": {}}
    sky_kept = 0
    for k, lights in enumerate([(L0,)] * 5 + [(L1,), (L1, L2)]):
        r.render_scene(scene(w, h, TWO, lights), handles)
        assert np.array_equal(bits(r.read_framebuffer()), bits(oracle(w, h, TWO, lights))), f"frame {k}"
        t = r.read_sky_tiles()
        sky_kept += int((t == SK.KEPT).sum())
        assert sky_keep or not t.any()
    c = r.view_keep_counts()
    r.close()
    assert (c["kept"], c["full"]) == ((3, 4) if view_keep else (0, 7)), c
    assert (sky_kept > 0) == bool(sky_keep)


# ---- 6. a capacity overflow ----
@pytest.mark.gpu
def test_nothing_is_kept_across_a_capacity_growth():
    """144 triangles on one tile against bins of 16: the read finds the overflow, the capacities grow, every slot forgets and the
    frame is rendered again, in full; the same frame twice more is then the slot's third and fourth of a kind"""
    w, h = SIZES[0]
    sc = SK.heavy_scene(1)
    want = bbo.render(sc)[0]
    key = (w, h, "heavy")
    p = Pair(w, h, 1, bin_cap=16)
    history = []
    for k in range(4):
        history.append(p.frame(key, f"frame {k}", want=want, record=lambda r, handles: r.render_scene(sc, handles))[1])
    assert p.r[0].capacity_growths() >= 1 and history == [False, True, True, True], history
    p.close()
