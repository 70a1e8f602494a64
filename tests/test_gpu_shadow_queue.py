"""GPU: shadow casters queued with the frame (bbr_queue_shadow_caster, k_shadow_pass_retire; DESIGN.md section 3, "Queued pass").

The rule under test: a sequence of calls with bbr_queue_shadow_caster(args) inside a frame gives, bit for bit in every output,
what the same sequence gives with bbr_render_shadow_caster(args) directly in front of that frame's bbr_end_frame, once per queued
slot in slot order.  So the oracle everywhere is a SECOND CONTEXT driven through the synchronous call at that place: every
script below is written once and run twice (Rig.how = "queue" / "sync"), and what the two runs hand out is compared with no
tolerance but for NaN payload ("equal": surface_chart.equal_but_for_nan_payload).  The scenes, casters and sizes are those of
tests/shadow_casters_scenes.py.  Every test calls a new symbol.

  1  equivalence   one caster of one face at R = 0, one of six faces at R = 1, two casters in slots 0 and 5 at R = 2; forward and
                   deferred, plain and present_fused: frame, presented image, every map, mask, face index, taps, the slots.  A
                   queue call before, between and after the draws gives the same bits
  2  in flight     four frames in flight, eight frames, the caster's view changes every frame, every third frame queues nothing,
                   every frame into a buffer of its own, the frames of a group held back on the GPU until all are recorded: each
                   is the synchronous context's frame of that step; 0 drains
  3  persistence   the caster stays for frames that queue nothing; a synchronous call replaces it; a drop drops it
  4  overflow      a first queued pass that exceeds its first capacities: after bbr_get_stats frame and maps are right; also with
                   a plain frame behind it, and for a host that never synchronises (the slot's reuse finds it)
  5  state         every refusal leaves slots, counters and the next frame alone, and is the synchronous call's refusal (code and
                   text); outside a frame; one slot twice; one light twice
  6  around        a partition of three, supersample 2 in both sample modes, both tile modes, static_records with repeated
                   draws, replay, resize, live_resources()"""
import ctypes as C

import numpy as np
import pytest
import torch

import shadow_casters_scenes as CS
import shadow_faces_scenes as FS
import shadow_scenes as SS
import surface_chart as SC
from bibim_renderer_amd import BibimError, Renderer
from bibim_renderer_amd import partition as P
from bibim_renderer_amd.renderer import live_resources
from oracle import bbo

pytestmark = pytest.mark.gpu

INVALID, NOT_IN_FRAME = -1, -6
KIND = "mixed"
equal = SC.equal_but_for_nan_payload
pass_id = lambda d: "deferred" if d else "forward"

SPOT = np.array([SS.light_view("spot")])
# the three cases of 1: (casters, R)
ONE_FACE = ((dict(slot=0, light=0, views=SPOT, bias=CS.BIAS),), 0)
SIX_FACES = ((dict(slot=0, light=2, views=FS.faces("cube"), bias=CS.BIAS),), 1)
TWO_SLOTS = ((dict(slot=0, light=2, views=FS.faces("cube"), bias=CS.BIAS), dict(slot=5, light=3, views=FS.faces("cascade"), bias=CS.BIAS)), 2)
CASES = {"one-face-R0": ONE_FACE, "six-faces-R1": SIX_FACES, "slots-0-and-5-R2": TWO_SLOTS}


def moving(step, slot=0, light=0):
    """the caster of 2 at `step`: shadow_casters_scenes' spot view turned about the receiver's normal, a new place every step"""
    return dict(slot=slot, light=light, views=CS._eight_views()[step % 8:step % 8 + 1], bias=CS.BIAS)


def expect(code, call, *args):
    with pytest.raises(BibimError) as e:
        call(*args)
    assert e.value.code == code, e.value


def state(r):
    light, faces = r.shadow_casters()
    return light.tolist(), faces.tolist()


class Rig:
    """A context with the scene's meshes and materials uploaded once, and frames recorded one way or the other:
    how = "queue": the casters of a frame go through queue_shadow_caster at `where` (0: before the draws .. n: after them);
    how = "sync":  through render_shadow_caster, in slot order, directly in front of end_frame."""

    def __init__(self, how, size=CS.FRAME_SMALL, side=64, radius=0, **options):
        self.how, self.size = how, tuple(size)
        self.r = r = Renderer(*size)
        for k, v in options.items():
            r.set_option(k, v)
        r.set_option("shadow_map", side)
        r.set_option("shadow_filter", radius)
        self.sc = CS.scene(KIND, size)
        mesh, mat, self.draws = {}, {}, []
        for d in self.sc.draws:
            if id(d.vertices) not in mesh:
                mesh[id(d.vertices)] = r.upload_mesh(d.vertices, d.indices)
            if id(d.material) not in mat:
                mat[id(d.material)] = r.upload_material(d.material.maps)
            self.draws.append((mesh[id(d.vertices)], mat[id(d.material)], d.instances))

    def resize(self, size):
        self.size = tuple(size)
        self.r.resize(*size)
        self.sc = CS.scene(KIND, size)

    def frame(self, casters=(), where=None):
        r = self.r
        where = len(self.draws) if where is None else where
        queue = lambda: [r.queue_shadow_caster(c["slot"], c["light"], c["views"], c["bias"]) for c in casters] if self.how == "queue" else None
        r.set_frame_uniforms(self.sc.frame)
        r.set_view_uniforms(self.sc.view)
        r.begin_frame()
        for i, (mesh, mat, inst) in enumerate(self.draws):
            if i == where:
                queue()
            r.draw(mesh, mat, inst)
        if where >= len(self.draws):
            queue()
        if self.how == "sync":
            for c in sorted(casters, key=lambda c: c["slot"]):
                r.render_shadow_caster(c["slot"], c["light"], c["views"], c["bias"])
        r.end_frame()

    def close(self):
        self.r.close()


def image(r, fused=False):
    """the last frame, and its presented image"""
    if fused:
        return {"presented": r.read_presented()}
    out = {"frame": r.read_framebuffer()}
    r.present()
    out["presented"] = r.read_presented()
    return out


def maps(r, casters):
    return {f"map {c['slot']}.{f}": r.read_shadow_caster_face(c["slot"], f) for c in casters for f in range(len(c["views"]))}


def verdicts(r, casters):
    out = {}
    for c in casters:
        s = c["slot"]
        out[f"mask {s}"], out[f"face {s}"], out[f"taps {s}"] = r.read_shadow_caster_mask(s), r.read_shadow_caster_face_index(s), r.read_shadow_caster_taps(s)
    return out


def everything(r, casters, fused=False):
    return {**image(r, fused), "slots": state(r), **maps(r, casters), **verdicts(r, casters)}


def assert_same(got, want, what=""):
    assert got.keys() == want.keys(), (what, sorted(got), sorted(want))
    for k in want:
        g, w = got[k], want[k]
        if isinstance(w, np.ndarray) and w.dtype == np.float32:
            assert equal(g, w), f"{what} {k}: {int((SC.bits(g) != SC.bits(w)).sum())} values differ from the synchronous context's"
        elif isinstance(w, np.ndarray):
            assert np.array_equal(g, w), f"{what} {k}: {int((g != w).sum())} values differ from the synchronous context's"
        else:
            assert g == w, f"{what} {k}: {g} != {w}"


def both(script, what="", **context):
    """`script(rig)` -> dict of outputs, under both ways of casting; the queued context's must be the synchronous one's"""
    out = {}
    for how in ("sync", "queue"):
        rig = Rig(how, **context)
        try:
            out[how] = script(rig)
        finally:
            rig.close()
    assert_same(out["queue"], out["sync"], what)
    return out["queue"]


# ---------------------------------------------------------------------------------------------------------------------
# 1. equivalence
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fused", [0, 1], ids=["plain", "present_fused"])
@pytest.mark.parametrize("deferred", [0, 1], ids=pass_id)
@pytest.mark.parametrize("case", list(CASES))
def test_queued_frame_is_the_synchronous_frame(case, deferred, fused):
    casters, radius = CASES[case]

    def script(rig):
        rig.frame(casters)
        return everything(rig.r, casters, fused)

    got = both(script, f"{case} {pass_id(deferred)}", size=CS.FRAME_DUMP, radius=radius, render_pass=deferred, present_fused=fused)
    assert got["slots"] == tuple(map(list, zip(*[(next((c["light"] for c in casters if c["slot"] == s), -1),
                                                   next((len(c["views"]) for c in casters if c["slot"] == s), 0)) for s in range(8)])))
    assert any((got[f"mask {c['slot']}"] == 2).sum() >= 32 for c in casters), "nothing is shadowed: the case shows nothing"


def test_queue_call_before_between_and_after_the_draws():
    casters, radius = TWO_SLOTS
    sync = Rig("sync", side=33, radius=radius)
    sync.frame(casters)
    want = {**image(sync.r), **maps(sync.r, casters)}
    sync.close()
    for where in (0, 1, 3):
        rig = Rig("queue", side=33, radius=radius)
        rig.frame(casters, where)
        got = {**image(rig.r), **maps(rig.r, casters)}
        rig.close()
        assert_same(got, want, f"queued in front of draw {where}:")


# ---------------------------------------------------------------------------------------------------------------------
# 2. a moving caster with frames in flight
# ---------------------------------------------------------------------------------------------------------------------
STEPS = 8
queues = lambda step: step % 3 != 2


@pytest.mark.parametrize("slot", [0, 5], ids=["slot0", "slot5-table"])
def test_moving_caster_with_four_frames_in_flight(slot):
    w, h = CS.FRAME_SMALL
    sync = Rig("sync", radius=1, frames_in_flight=4)
    want = []
    for step in range(STEPS):
        sync.frame([moving(step, slot)] if queues(step) else [])
        want.append(sync.r.read_framebuffer())
    sync.close()
    assert not equal(want[0], want[1]) and not equal(want[3], want[4]), "the caster does not move: the test shows nothing"

    rig = Rig("queue", radius=1, frames_in_flight=4)
    out = [torch.zeros((h, w, 4), dtype=torch.float32, device="cuda") for _ in range(STEPS)]
    torch.cuda.synchronize()  # (torch fills on its own stream; the library does not wait for that one)
    before = rig.r.shadow_queue_counts()
    # The frames must really be on the GPU together, or any library passes: every fourth frame's stream first waits for work on
    # a side stream that outlasts the recording of the frames behind it (a few matrix products), and the passes follow one another,
    # so a group's frames pile up behind it and run at once.  A pass that then wrote the map a frame in front of it still reads
    # -- one generation -- would be the next frame's map under that frame's shading.
    side, a = torch.cuda.Stream(), torch.zeros((4096, 4096), device="cuda")
    b = a @ a
    torch.cuda.synchronize()
    gates = []
    for step in range(STEPS):
        if step % 4 == 0:
            gates.append(torch.cuda.Event())
            with torch.cuda.stream(side):
                for _ in range(8):
                    torch.mm(a, a, out=b)
                gates[-1].record(side)
            rig.r.wait_event(gates[-1].cuda_event)
        rig.r.set_output_device_ptr(out[step].data_ptr(), out[step].numel() * 4)
        rig.frame([moving(step, slot)] if queues(step) else [])
    passes, drains = rig.r.shadow_queue_counts()
    rig.r.synchronize()
    got = [t.cpu().numpy() for t in out]
    after = rig.r.shadow_queue_counts()
    rig.close()
    assert before == (0, 0) and passes == sum(queues(s) for s in range(STEPS)) and drains == 0 and after == (passes, 0), (before, passes, drains, after)
    for step in range(STEPS):
        assert equal(got[step], want[step]), f"frame {step}: {int((SC.bits(got[step]) != SC.bits(want[step])).any(-1).sum())} pixels differ from the synchronous context's"


# ---------------------------------------------------------------------------------------------------------------------
# 3. persistence and replacement
# ---------------------------------------------------------------------------------------------------------------------
def test_caster_persists_is_replaced_and_dropped():
    first, second = moving(1), moving(5, light=2)

    def script(rig):
        r, out = rig.r, {}
        rig.frame([first])
        out["queued"], out["queued slots"] = r.read_framebuffer(), state(r)
        for k in range(3):
            rig.frame()
            out[f"kept {k}"], out[f"kept {k} slots"] = r.read_framebuffer(), state(r)
        r.render_shadow_caster(second["slot"], second["light"], second["views"], second["bias"])
        r.replay_frame()
        out["replaced"], out["replaced slots"] = r.read_framebuffer(), state(r)
        out.update(maps(r, [second]))
        r.drop_shadow_caster(0)
        r.replay_frame()
        out["dropped"], out["dropped slots"] = r.read_framebuffer(), state(r)
        return out

    got = both(script, radius=1)
    assert got["queued slots"][0][0] == 0 and got["kept 2 slots"] == got["queued slots"]
    assert equal(got["kept 2"], got["queued"]) and not equal(got["replaced"], got["queued"]) and not equal(got["dropped"], got["replaced"])
    assert got["replaced slots"][0][0] == 2 and got["dropped slots"] == ([-1] * 8, [0] * 8)


# ---------------------------------------------------------------------------------------------------------------------
# 4. overflow
# ---------------------------------------------------------------------------------------------------------------------
def test_first_queued_pass_overflows_its_first_capacities():
    one = CS.casters(KIND)[1]

    def script(rig):
        r = rig.r
        rig.frame([one])
        r.stats()
        return {"frame": r.read_framebuffer(), **maps(r, [one]), "slots": state(r), "grown": r.capacity_growths() > 0}

    got = both(script, side=200, bin_cap=4, broad_cap=1, clip_cap=1)
    assert got["grown"]
    want = CS.oracle_maps(KIND, one["slot"], 200)
    assert np.array_equal(SC.bits(got[f"map {one['slot']}.0"]), SC.bits(want[0])), "the map after the growth is not the oracle's depth"


def test_overflowed_pass_behind_a_plain_frame_is_rendered_again():
    """the frame that queued is no longer the recorded one when the host synchronises: the maps are complete all the same"""
    one = CS.casters(KIND)[1]

    def script(rig):
        r = rig.r
        rig.frame([one])
        rig.frame()
        r.stats()
        return {"frame": r.read_framebuffer(), **maps(r, [one]), "slots": state(r), "grown": r.capacity_growths() > 0}

    got = both(script, side=200, bin_cap=4, broad_cap=1, clip_cap=1)
    assert got["grown"]
    assert np.array_equal(SC.bits(got[f"map {one['slot']}.0"]), SC.bits(CS.oracle_maps(KIND, one["slot"], 200)[0]))


def test_overflowed_pass_is_rendered_again_for_a_host_that_only_streams():
    """no synchronising call: the overflow is found when the frame's slot is reused, and the pass is rendered again there"""
    one = CS.casters(KIND)[1]

    def script(rig):
        r = rig.r
        rig.frame([one])
        for _ in range(5):                                # (two frames in flight: the third frame reuses the first one's slot)
            rig.frame()
        drains = r.shadow_queue_counts()[1]
        out = {"frame": r.read_framebuffer(), **maps(r, [one]), "slots": state(r)}
        assert rig.how == "sync" or drains >= 1, drains
        return out

    got = both(script, side=200, bin_cap=4, broad_cap=1, clip_cap=1)
    assert np.array_equal(SC.bits(got[f"map {one['slot']}.0"]), SC.bits(CS.oracle_maps(KIND, one["slot"], 200)[0]))


# ---------------------------------------------------------------------------------------------------------------------
# 5. state and refusals
# ---------------------------------------------------------------------------------------------------------------------
def test_refusals_leave_everything_as_it_was():
    off = Renderer(*CS.FRAME_SMALL)
    off.begin_frame()
    expect(INVALID, off.queue_shadow_caster, 0, 0, SPOT, CS.BIAS)       # option shadow_map is 0
    off.end_frame()
    off.close()

    held = dict(slot=0, light=0, views=SPOT, bias=CS.BIAS)
    rig = Rig("queue", radius=1)
    r = rig.r
    rig.frame([held])
    want_frame, want_state, want_counts = r.read_framebuffer(), state(r), r.shadow_queue_counts()
    assert want_state[0][0] == 0 and want_counts == (1, 0)
    expect(NOT_IN_FRAME, r.queue_shadow_caster, 0, 0, SPOT, CS.BIAS)    # outside a frame
    views = lambda n: np.zeros(n, bbo.VIEW_DTYPE)
    refused = [(-1, 0, SPOT, CS.BIAS), (8, 0, SPOT, CS.BIAS), (0, 0, views(7), CS.BIAS), (0, -1, SPOT, CS.BIAS), (0, 100, SPOT, CS.BIAS),
               (0, 0, SPOT, float("nan")), (1, 0, SPOT, CS.BIAS)]      # (the last: slot 0, in use, holds light 0)

    def refusals():
        for args in refused:
            expect(INVALID, r.queue_shadow_caster, *args)
        assert r._L.bbr_queue_shadow_caster(r._ctx, 0, 0, 0, SPOT.ctypes.data_as(C.c_void_p), CS.BIAS) == INVALID   # no face
        assert r._L.bbr_queue_shadow_caster(r._ctx, 0, 0, 1, None, CS.BIAS) == INVALID                               # NULL blocks
        assert state(r) == want_state and r.shadow_queue_counts() == want_counts

    r.set_frame_uniforms(rig.sc.frame)
    r.set_view_uniforms(rig.sc.view)
    r.begin_frame()
    refusals()
    for mesh, mat, inst in rig.draws:
        r.draw(mesh, mat, inst)
    refusals()
    r.end_frame()
    assert state(r) == want_state and r.shadow_queue_counts() == want_counts
    assert equal(r.read_framebuffer(), want_frame), "a frame of refused calls is not the frame without them"
    rig.close()

    # The queued and the synchronous form judge a request alike: the same code, and the same text behind the call's name -- but
    # for the one-slot-per-light refusal, where the queued form also looks at what the frame has queued and says so.
    rig = Rig("queue", size=(32, 32), side=16)
    r = rig.r
    rig.frame([held])
    want_state, want_counts = state(r), r.shadow_queue_counts()

    def refusal(name, caster, light, n_faces, blocks, bias):
        rc = getattr(r._L, "bbr_" + name)(r._ctx, caster, light, n_faces, blocks.ctypes.data_as(C.c_void_p), bias)
        text = r._L.bbr_last_error(r._ctx).decode()
        assert text.startswith(name + ": "), text
        return rc, text[len(name) + 2:]

    one_slot_per_light = ("another caster slot, in use or queued in this frame, holds this light_index (one slot per light)",
                          "another caster slot in use holds this light_index (one slot per light)")
    faults = {"caster 8": (8, 0, 1, SPOT, CS.BIAS), "no face": (0, 0, 0, SPOT, CS.BIAS), "seven faces": (0, 0, 7, views(7), CS.BIAS),
              "light 100": (0, 100, 1, SPOT, CS.BIAS), "NaN bias": (0, 0, 1, SPOT, float("nan")), "light held by slot 0": (1, 0, 1, SPOT, CS.BIAS)}
    r.begin_frame()
    for mesh, mat, inst in rig.draws:
        r.draw(mesh, mat, inst)
    for what, args in faults.items():
        (q_rc, q_text), (s_rc, s_text) = refusal("queue_shadow_caster", *args), refusal("render_shadow_caster", *args)
        assert q_rc == s_rc == INVALID, (what, q_rc, s_rc)
        assert (q_text, s_text) == one_slot_per_light if what == "light held by slot 0" else q_text == s_text, (what, q_text, s_text)
    r.end_frame()
    assert state(r) == want_state and r.shadow_queue_counts() == want_counts
    rig.close()


def test_one_slot_twice_and_one_light_twice_in_a_frame():
    a, b = moving(2), moving(6)

    def script(rig):
        r = rig.r
        if rig.how == "queue":
            r.set_frame_uniforms(rig.sc.frame)
            r.set_view_uniforms(rig.sc.view)
            r.begin_frame()
            r.queue_shadow_caster(a["slot"], a["light"], a["views"], a["bias"])
            for mesh, mat, inst in rig.draws:
                r.draw(mesh, mat, inst)
            r.queue_shadow_caster(b["slot"], b["light"], b["views"], b["bias"])       # the last call for the slot stands
            r.queue_shadow_caster(3, 1, SPOT, CS.BIAS)
            expect(INVALID, r.queue_shadow_caster, 4, 1, SPOT, CS.BIAS)             # light 1 is queued in slot 3
            expect(INVALID, r.queue_shadow_caster, 4, b["light"], SPOT, CS.BIAS)    # ... and light 0 in slot 0
            r.end_frame()
        else:
            rig.frame([b, dict(slot=3, light=1, views=SPOT, bias=CS.BIAS)])
        return {"frame": r.read_framebuffer(), "slots": state(r), **maps(r, [b])}

    got = both(script, radius=0)
    assert got["slots"][0] == [0, -1, -1, 1, -1, -1, -1, -1]


# ---------------------------------------------------------------------------------------------------------------------
# 6. under the other modes
# ---------------------------------------------------------------------------------------------------------------------
def test_partition_of_three():
    casters, radius = TWO_SLOTS
    h = CS.FRAME_SMALL[1]
    shards = {"sync": [], "queue": []}
    for rank in range(3):
        def script(rig):
            band_rows = rig.r.tile_height()
            rig.r.set_partition(rank, 3, band_rows)
            rig.frame(casters)
            shards[rig.how].append((rig.r.read_shard(), band_rows))
            return maps(rig.r, casters)                      # (every rank renders the whole maps)
        both(script, f"rank {rank}", radius=radius)
    # (a shard's padding rows are never written: the rows of the frame are compared)
    whole = {how: P.unpack_gathered(np.stack([s for s, _ in shards[how]]), h, shards[how][0][1]) for how in shards}
    assert equal(whole["queue"], whole["sync"]), "the gathered frame is not the synchronous contexts'"


@pytest.mark.parametrize("sample_shading", [1, 0])
def test_supersample_two(sample_shading):
    casters, radius = SIX_FACES

    def script(rig):
        rig.frame(casters)
        return {"frame": rig.r.read_framebuffer(), "samples": rig.r.read_samples(), **maps(rig.r, casters)}   # (the pass stays S x S)

    both(script, size=(48, 30), radius=radius, sample_shading=sample_shading, supersample=2)


@pytest.mark.parametrize("tile_mode", [0, 1])
def test_tile_modes(tile_mode):
    casters, radius = TWO_SLOTS

    def script(rig):
        rig.frame(casters)
        return {**image(rig.r), **maps(rig.r, casters)}

    both(script, side=33, radius=radius, tile_mode=tile_mode)


@pytest.mark.parametrize("static_records", [1, 0])
def test_static_records(static_records):
    """one frame in flight, the same draws every frame: from the second frame on the descriptors the pass reads ask for
    k_geometry's light path (kDrawStaticPresent), into the pass slot's records, which hold no static part"""
    light_draws = {}

    def script(rig):
        r, out = rig.r, {}
        for step in range(4):
            rig.frame([moving(step), dict(slot=5, light=2, views=FS.faces("cube"), bias=CS.BIAS)])
            out[f"frame {step}"] = r.read_framebuffer()
        light_draws[rig.how] = r.static_record_counts()["light_draws"]
        out.update(maps(r, [moving(3), dict(slot=5, light=2, views=FS.faces("cube"), bias=CS.BIAS)]))
        return out

    both(script, radius=1, frames_in_flight=1, static_records=static_records)
    assert (light_draws["queue"] > 0) == bool(static_records), light_draws


def test_replay_frame():
    def script(rig):
        r, out = rig.r, {}
        rig.frame([moving(0)])
        rig.frame([moving(3)])
        for k in range(3):
            r.replay_frame()
        out["replayed"], out["slots"] = r.read_framebuffer(), state(r)
        out.update(maps(r, [moving(3)]))
        return out

    both(script, radius=1, frames_in_flight=3)


def test_resize_between_frames():
    def script(rig):
        r, out = rig.r, {}
        rig.frame([moving(0)])
        out["before"] = r.read_framebuffer()
        rig.resize(CS.FRAME_DUMP)
        rig.frame()                                   # (a resize keeps the casters)
        out["kept"], out["kept slots"] = r.read_framebuffer(), state(r)
        rig.frame([moving(4)])
        out["after"], out["after slots"] = r.read_framebuffer(), state(r)
        out.update(maps(r, [moving(4)]))
        return out

    both(script, radius=1, frames_in_flight=2)


def test_live_resources_return_to_their_start():
    before = live_resources()
    rig = Rig("queue", radius=1, frames_in_flight=4)
    for step in range(6):
        rig.frame([moving(step), moving(step, slot=5, light=2)])
    rig.r.synchronize()
    during = live_resources()
    rig.close()
    assert during["device_allocs"] > before["device_allocs"] and live_resources() == before
