"""GPU: option "auto_exposure" -- k_luminance, k_exposure and the present kernels that read the exposure from device memory,
against tests/exposure_reference.py: every field of the record and every byte, no tolerance anywhere (include/bibim_hip.h
"auto exposure").

The chart goes through bbr_present_buffer_auto (history 1), so its frames hold what no renderer produces; rendered frames go
through bbr_present (history 0), whose source is read back with bbr_read_framebuffer and given to the model."""
import functools

import numpy as np
import pytest

import bloom_reference as B
import exposure_reference as X
import test_gpu_sky_keep as SK
from bibim_renderer_amd import BibimError, Renderer, configs
from bibim_renderer_amd.renderer import live_resources
from oracle import bbo, scenes

pytestmark = pytest.mark.gpu

INVALID, NOT_IN_FRAME = -1, -6
GUARD = 64                       # bytes either side of the RGBA8 output
T, I = float(B.CHART_THRESHOLD), float(B.CHART_INTENSITY)
EXPOSURE = 0.7                   # the frame's own Exposure: what is applied when nothing is counted and there is no history
F32 = np.float32


def refused(code, call, *args):
    with pytest.raises(BibimError) as e:
        call(*args)
    assert e.value.code == code, e.value


def same_image(got, want):
    bad = (got != want).any(axis=2)
    assert not bad.any(), (int(bad.sum()), [(int(y), int(x), got[y, x].tolist(), want[y, x].tolist()) for y, x in np.argwhere(bad)[:5]])


def same_record(got, want):
    diff = X.same_record(got, want)
    assert diff is None, diff


def wanted_image(frame, levels, enable, exposure, hdr16):
    h, w = frame.shape[:2]
    v = B.bloomed(frame, levels, T, I) if levels else frame
    return bbo.present(v.reshape(-1, 4), enable, exposure, hdr16).reshape(h, w, 4)


@functools.lru_cache(None)
def chart(w, h, variant):
    f = X.chart_frame(w, h, variant)
    f.setflags(write=False)
    return f


@pytest.fixture(scope="module")
def chart_renderer():
    r = Renderer(64, 64)
    r.set_bloom(T, I)
    r.set_option("auto_exposure", 1)
    yield r
    r.close()


class BufferSource:
    """bbr_present_buffer_auto beside the model of history 1"""

    def __init__(self, r, p=X.DEFAULTS, levels=0):
        self.r, self.p, self.levels, self.history = r, p, levels, None
        r.set_option("bloom", levels)
        r.set_auto_exposure(*p)
        r.reset_exposure()

    def present(self, frame, enable, hdr16, fallback=EXPOSURE):
        """one call into a guarded buffer: the record and every byte against the model; returns the record"""
        import torch
        h, w = frame.shape[:2]
        src = torch.from_numpy(np.array(frame, np.float32)).cuda()
        out = torch.full((2 * GUARD + w * h * 4,), 0xA5, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        self.r.present_buffer_auto(src.data_ptr(), out.data_ptr() + GUARD, w, h, enable, fallback, hdr16)
        rec = self.r.read_exposure(1)
        torch.cuda.synchronize()
        got = out.cpu().numpy()
        assert (got[:GUARD] == 0xA5).all() and (got[-GUARD:] == 0xA5).all(), "the guard bytes around the image changed"
        want, self.history = X.expose(frame, self.p, self.history, fallback)
        same_record(rec, want)
        assert int(rec["counted"]) + int(rec["ignored"]) == w * h
        same_image(got[GUARD:-GUARD].reshape(h, w, 4), wanted_image(frame, self.levels, enable, want["applied"], hdr16))
        return rec


# ---- 1. the chart through bbr_present_buffer_auto ----
@pytest.mark.parametrize("levels", [0, 2])
@pytest.mark.parametrize("w,h", X.CHART_FRAMES)
def test_chart(chart_renderer, w, h, levels):
    src = BufferSource(chart_renderer, X.params(rate=0.5), levels)
    frame = chart(w, h, 0)
    for hdr16 in (False, True):
        for enable in (0, 1):
            src.present(frame, enable, hdr16)        # (the first without a history, the others adapt half way)


@pytest.mark.parametrize("lo,hi", [(0, 1000), (500, 950), (999, 1000)])
def test_chart_trims(chart_renderer, lo, hi):
    src = BufferSource(chart_renderer, X.params(lo=lo, hi=hi, key=0.5))
    for (w, h, variant) in [(64, 64, 1), (257, 33, 3), (257, 33, "flat")]:
        rec = src.present(chart(w, h, variant), 1, True)
        assert rec["kept"] == rec["counted"] - rec["counted"] * lo // 1000 - rec["counted"] * (1000 - hi) // 1000 > 0


def test_chart_variants_on_the_smallest_frames(chart_renderer):
    """a 1 x 1 frame holds one hazard: the other rotations of the list, ignored pixels alone among them"""
    src = BufferSource(chart_renderer, X.params(rate=0.25))
    flags = set()
    for (w, h) in [(1, 1), (2, 2), (3, 5)]:
        for variant in range(1, 6):
            flags.add(int(src.present(chart(w, h, variant), 1, True)["flags"]))
    assert 1 in flags and (2 in flags or 3 in flags), flags           # (a 1 x 1 frame of one ignored pixel is among them)


def test_one_bin_for_every_lane(chart_renderer):
    src = BufferSource(chart_renderer, X.params(lo=0, hi=1000))
    rec = src.present(chart(512, 256, "constant"), 1, True)
    assert rec["hist"].max() == 512 * 256 and rec["ignored"] == 0
    rec = src.present(chart(512, 256, "flat"), 1, False)
    assert rec["hist"].max() >= 512 * 256 - 64 and rec["ignored"] >= 7


def test_nothing_to_count(chart_renderer):
    src = BufferSource(chart_renderer, X.params(rate=0.5))
    dark = chart(257, 33, "ignored")
    rec = src.present(dark, 1, True, fallback=0.35)                   # no history: the caller's exposure
    assert rec["flags"] == 2 and rec["applied"] == F32(0.35) and rec["counted"] == 0
    lit = src.present(chart(64, 64, 0), 1, True)
    assert lit["flags"] == 0
    rec = src.present(dark, 1, True, fallback=0.35)                   # a history: it is applied and left as it is
    assert rec["flags"] == 3 and X.bits(rec["applied"]) == X.bits(lit["applied"]) == X.bits(rec["previous"])
    rec = src.present(chart(64, 64, 0), 1, True)
    assert rec["flags"] == 1 and X.bits(rec["previous"]) == X.bits(lit["applied"])
    chart_renderer.reset_exposure()
    src.history = None
    assert src.present(chart(64, 64, 0), 0, True)["flags"] == 0      # tone mapping off: E is computed and unused


# ---- 2. a sequence through bbr_present: the adapt steps of different slots are ordered on the device ----
def triangle_scene(w, h, intensity):
    inst = np.zeros(1, bbo.INSTANCE_DTYPE)
    inst[0] = scenes.instance(np.eye(4, dtype=np.float32))
    fu = scenes.frame_uniforms([scenes.light(0, pos=(0.3, 0.5, 0.0), color=(1.0, 0.9, 0.8), intensity=intensity)], 1, EXPOSURE)
    vu = scenes.view_uniforms((0, 0, 0), 0, 0, w, h, 1)
    return bbo.Scene(fu, vu, [bbo.DrawData(SK.mesh(w, h, ((0, 0), (1, 1))), None, inst, SK.material())], w, h, f"exposure step {intensity}")


@pytest.mark.parametrize("layout", [0, 1, 2])
@pytest.mark.parametrize("fif", [2, 4])
def test_sequence_across_slots(fif, layout):
    w = h = 64
    p = X.params(rate=0.25)
    r = Renderer(w, h)
    r.set_option("frames_in_flight", fif)
    r.set_option("stream_layout", layout)
    dim, bright = triangle_scene(w, h, 6.0), triangle_scene(w, h, 6.0 * 64.0)
    handles = r.render_scene(dim)
    r.read_framebuffer()                                              # (the capacities settle before frames overlap)
    r.set_option("auto_exposure", 1)
    r.set_auto_exposure(*p)
    refused(NOT_IN_FRAME, r.read_exposure, 0)
    for k in range(12):                                               # no synchronisation in between
        r.render_scene(dim if k < 6 else bright, handles)
        r.present()
    rec = r.read_exposure(0)
    image = r.read_presented()
    r.render_scene(dim, handles)
    f_dim = r.read_framebuffer()
    r.render_scene(bright, handles)
    f_bright = r.read_framebuffer()
    history, want = None, None
    for k in range(12):
        want, history = X.expose(f_dim if k < 6 else f_bright, p, history, EXPOSURE)
    same_record(rec, want)
    assert want["flags"] == 1 and X.bits(want["previous"]) != X.bits(want["applied"]) != X.bits(want["clamped"])
    same_image(image, wanted_image(f_bright, 0, 1, want["applied"], True))
    r.close()


@pytest.mark.parametrize("fif", [1, 4])
def test_parameters_set_between_presentations_in_flight(fif):
    """bbr_set_auto_exposure does not wait: a host calls it every frame with the rate of its clock.  Each presentation has the
    values stored when it was queued, in call order, through bbr_present and through the buffer call alike."""
    import torch
    w = h = 64
    steps = [X.params(0.18, 2.0 ** -10, 2.0 ** 10, 1.0, 500, 950), X.params(0.5, 0.01, 100.0, 0.25, 0, 1000), X.params(0.05, 0.01, 100.0, 0.75, 100, 300),
             X.params(0.3, 2.0, 3.0, 0.5, 999, 1000), X.params(0.18, 0.001, 1000.0, 0.125, 400, 600), X.params(1.0, 0.001, 1000.0, 0.9, 0, 1),
             X.params(0.18, 0.001, 1000.0, 0.0, 500, 950), X.params(0.25, 0.001, 1000.0, 0.3, 250, 750)]
    r = Renderer(w, h)
    r.set_option("frames_in_flight", fif)
    dim, bright = triangle_scene(w, h, 6.0), triangle_scene(w, h, 6.0 * 64.0)
    handles = r.render_scene(dim)
    f_dim = r.read_framebuffer()                                      # (the capacities settle before frames overlap)
    r.render_scene(bright, handles)
    f_bright = r.read_framebuffer()
    r.set_option("auto_exposure", 1)
    chart_frame = chart(64, 64, 4)
    src = torch.from_numpy(np.array(chart_frame, np.float32)).cuda()
    out = torch.zeros(w * h, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    for k, p in enumerate(steps):                                     # no synchronisation in between
        r.set_auto_exposure(*p)
        r.render_scene(bright if k % 2 else dim, handles)
        r.present()
        r.present_buffer_auto(src.data_ptr(), out.data_ptr(), w, h, 1, EXPOSURE)
    r.set_auto_exposure(*X.DEFAULTS)                                  # after the last presentation: it takes no part
    h0 = h1 = want0 = want1 = None
    for k, p in enumerate(steps):
        want0, h0 = X.expose(f_bright if k % 2 else f_dim, p, h0, EXPOSURE)
        want1, h1 = X.expose(chart_frame, p, h1, EXPOSURE)
    same_record(r.read_exposure(0), want0)
    same_record(r.read_exposure(1), want1)
    same_image(r.read_presented(), wanted_image(f_bright, 0, 1, want0["applied"], True))
    torch.cuda.synchronize()
    same_image(out.cpu().numpy().view(np.uint8).reshape(h, w, 4), wanted_image(chart_frame, 0, 1, want1["applied"], True))
    r.close()


# ---- 3. what the library repeats keeps E and the history ----
def ball_scene(w, h, maps64, intensity=None, tone=1):
    sc = scenes.shaderball_scene(configs.C2.scaled(w, h, 64), bbo.MaterialData(maps64))
    sc.frame["enable_tone_mapping"] = tone
    sc.frame["exposure"] = EXPOSURE
    if intensity is not None:
        sc.frame["lights"]["intensity"][:int(sc.frame["num_lights"])] = intensity
    return sc


def test_a_repeated_presentation_keeps_its_exposure(maps64):
    w, h = 96, 64
    p = X.params(rate=0.5)
    r = Renderer(w, h)
    r.set_option("auto_exposure", 1)
    r.set_auto_exposure(*p)
    handles = r.render_scene(ball_scene(w, h, maps64, 5.0))
    dim = r.read_framebuffer()                                        # (the capacities settle first: a frame that overflows is metered incomplete)
    r.present()
    first, history = X.expose(dim, p, None, EXPOSURE)
    same_record(r.read_exposure(0), first)
    r.render_scene(ball_scene(w, h, maps64, 80.0), handles)
    r.present()
    frame = r.read_framebuffer()
    second, history = X.expose(frame, p, history, EXPOSURE)
    before = r.read_exposure(0)
    same_record(before, second)
    image = r.read_presented()
    same_image(image, wanted_image(frame, 0, 1, second["applied"], True))
    r.read_visibility()                                               # renders the frame again, and presents it again
    assert np.array_equal(r.read_presented(), image)
    same_record(r.read_exposure(0), second)                           # not metered again: the record and the history stay
    r.replay_frame()
    r.present()                                                       # the host's call: one more presentation
    third, history = X.expose(frame, p, history, EXPOSURE)
    rec = r.read_exposure(0)
    same_record(rec, third)
    assert X.bits(rec["previous"]) == X.bits(before["applied"]) and rec["flags"] == 1
    same_image(r.read_presented(), wanted_image(frame, 0, 1, third["applied"], True))
    r.close()


# ---- 4. state ----
def test_refused_pairs():
    r = Renderer(64, 64)
    for bad in (-1, 2, 100):
        refused(INVALID, r.set_option, "auto_exposure", bad)
    r.set_option("auto_exposure", 1)
    refused(INVALID, r.set_option, "present_fused", 1)
    refused(INVALID, r.set_partition, 0, 2)
    r.set_partition(0, 1)
    r.set_option("present_fused", 0)
    assert r.shard_rows() == 64
    r.set_option("auto_exposure", 0)
    r.set_option("present_fused", 1)
    refused(INVALID, r.set_option, "auto_exposure", 1)
    r.set_option("present_fused", 0)
    r.set_partition(1, 2)
    refused(INVALID, r.set_option, "auto_exposure", 1)
    assert r.shard_rows() == 32
    refused(INVALID, r.read_exposure, 0)                              # the option stayed 0
    r.set_partition(0, 1)
    r.set_option("auto_exposure", 1)
    r.close()


def test_parameters_and_read_back_codes(maps64):
    import torch
    w, h = 37, 23
    r = Renderer(w, h)
    defaults = (F32(0.18), F32(2.0 ** -10), F32(2.0 ** 10), 1.0, 500, 950)
    assert r.get_auto_exposure() == defaults
    nan, inf = float("nan"), float("inf")
    for bad in [(0.0, 0.1, 1.0, 1.0, 500, 950), (-1.0, 0.1, 1.0, 1.0, 500, 950), (nan, 0.1, 1.0, 1.0, 500, 950), (inf, 0.1, 1.0, 1.0, 500, 950),
                (0.18, 0.0, 1.0, 1.0, 500, 950), (0.18, 2.0, 1.0, 1.0, 500, 950), (0.18, 0.1, inf, 1.0, 500, 950), (0.18, nan, 1.0, 1.0, 500, 950),
                (0.18, 0.1, 1.0, -0.1, 500, 950), (0.18, 0.1, 1.0, 1.5, 500, 950), (0.18, 0.1, 1.0, nan, 500, 950),
                (0.18, 0.1, 1.0, 1.0, -1, 950), (0.18, 0.1, 1.0, 1.0, 500, 500), (0.18, 0.1, 1.0, 1.0, 600, 500), (0.18, 0.1, 1.0, 1.0, 0, 1001)]:
        refused(INVALID, r.set_auto_exposure, *bad)
        assert r.get_auto_exposure() == defaults
    r.set_auto_exposure(0.5, 0.25, 0.25, 0.0, 0, 1)                   # stored at either value of the option
    assert r.get_auto_exposure() == (0.5, 0.25, 0.25, 0.0, 0, 1)
    src = torch.zeros(64 * 4 + 8, dtype=torch.float32, device="cuda")
    out = torch.zeros(64 + 8, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    s, o = src.data_ptr(), out.data_ptr()
    refused(INVALID, r.present_buffer_auto, s, o, 8, 8, 0, 1.0)       # the option is 0
    refused(INVALID, r.read_exposure, 0)
    r.set_option("auto_exposure", 1)
    refused(NOT_IN_FRAME, r.read_exposure, 0)
    refused(NOT_IN_FRAME, r.read_exposure, 1)
    refused(INVALID, r.read_exposure, 2)
    refused(INVALID, r.read_exposure, -1)
    refused(INVALID, r.present_buffer_auto, 0, o, 8, 8, 0, 1.0)
    refused(INVALID, r.present_buffer_auto, s, 0, 8, 8, 0, 1.0)
    refused(INVALID, r.present_buffer_auto, s + 4, o, 8, 8, 0, 1.0)
    refused(INVALID, r.present_buffer_auto, s, o + 2, 8, 8, 0, 1.0)
    for bw, bh in [(0, 8), (8, 0), (-1, 8), (32769, 1), (1, 32769)]:
        refused(INVALID, r.present_buffer_auto, s, o, bw, bh, 0, 1.0)
    refused(NOT_IN_FRAME, r.read_exposure, 1)
    r.present_buffer_auto(s + 16, o + 4, 8, 8, 0, 1.0)
    rec = r.read_exposure(1)
    assert rec["ignored"] == 64 and rec["flags"] == 2 and rec["applied"] == 1.0
    r.render_scene(ball_scene(w, h, maps64))
    refused(NOT_IN_FRAME, r.read_exposure, 0)                         # rendered, not presented
    r.present()
    assert r.read_exposure(0)["applied"] == F32(0.25)                 # e_min = e_max
    r.resize(48, 40)
    refused(NOT_IN_FRAME, r.read_exposure, 0)
    r.read_exposure(1)
    r.close()


def test_reset_forgets_both_histories(maps64):
    w, h = 37, 23
    p = X.params(rate=0.25)
    r = Renderer(w, h)
    r.set_option("auto_exposure", 1)
    r.set_auto_exposure(*p)
    src = BufferSource(r, p)
    handles = r.render_scene(ball_scene(w, h, maps64))
    for k in range(2):
        r.present()
        assert r.read_exposure(0)["flags"] == k
        assert src.present(chart(64, 64, k), 1, True)["flags"] == k
    r.reset_exposure()
    src.history = None
    r.render_scene(ball_scene(w, h, maps64), handles)
    r.present()
    rec = r.read_exposure(0)
    assert rec["flags"] == 0 and X.bits(rec["applied"]) == X.bits(rec["clamped"])
    assert src.present(chart(64, 64, 2), 1, True)["flags"] == 0
    r.close()


def test_option_0_is_the_plain_rule_and_images_stay(maps64):
    w, h = 96, 64
    sc = ball_scene(w, h, maps64)
    r = Renderer(w, h)
    handles = r.render_scene(sc)
    r.present()
    frame = r.read_framebuffer()
    plain = r.read_presented()
    same_image(plain, wanted_image(frame, 0, 1, EXPOSURE, True))
    r.set_option("auto_exposure", 1)
    assert np.array_equal(r.read_presented(), plain)                  # an image already presented is not redone
    r.read_visibility()                                               # ... nor metered when the library repeats it
    assert np.array_equal(r.read_presented(), plain)
    refused(NOT_IN_FRAME, r.read_exposure, 0)
    r.render_scene(sc, handles)
    r.present()
    rec = r.read_exposure(0)
    same_record(rec, X.expose(frame, X.DEFAULTS, None, EXPOSURE)[0])
    metered = r.read_presented()
    same_image(metered, wanted_image(frame, 0, 1, rec["applied"], True))
    assert (metered != plain).any()
    r.set_option("auto_exposure", 0)
    assert np.array_equal(r.read_presented(), metered)
    r.read_visibility()                                               # a repeat behind the option's return makes the same image
    assert np.array_equal(r.read_presented(), metered)
    r.render_scene(sc, handles)
    r.present()
    assert np.array_equal(r.read_presented(), plain)
    r.close()


def test_live_resources_return(maps64):
    import torch
    w, h = 96, 64
    start = live_resources()
    r = Renderer(w, h)
    r.set_option("frames_in_flight", 2)
    sc = ball_scene(w, h, maps64)
    handles = r.render_scene(sc)
    r.present()
    for _ in range(7):                                                # both slots reach their steady state (kept frames)
        r.render_scene(sc, handles)
        r.present()
    r.read_presented()
    src = torch.zeros(33 * 17 * 4, dtype=torch.float32, device="cuda")
    out = torch.zeros(33 * 17, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    r.present_buffer(src.data_ptr(), out.data_ptr(), 33 * 17, 0, 1.0)
    r.synchronize()
    before = live_resources()
    r.set_option("auto_exposure", 1)
    for _ in range(2):
        r.render_scene(sc, handles)
        r.present()
    r.present_buffer_auto(src.data_ptr(), out.data_ptr(), 33, 17, 0, 1.0)
    r.read_presented()
    torch.cuda.synchronize()
    during = live_resources()
    assert during["device_allocs"] == before["device_allocs"] + 3     # histograms, records, histories
    assert during["device_bytes"] == before["device_bytes"] + 5 * 257 * 4 + 5 * Renderer.EXPOSURE_RECORD.itemsize + 2 * 8
    assert during["events"] == before["events"] + 2                   # the two orderings
    r.set_option("auto_exposure", 0)
    assert live_resources() == before
    r.set_option("auto_exposure", 1)
    r.render_scene(sc, handles)
    r.present()
    r.read_presented()
    r.close()
    assert live_resources() == start


def test_steady_context_still_keeps(maps64):
    """the option and its calls leave the slots' visibility alone: a steady 64 x 64 context goes on keeping frames"""
    w, h = 64, 64
    sc = ball_scene(w, h, maps64)
    r = Renderer(w, h)
    r.set_option("frames_in_flight", 1)
    handles = r.render_scene(sc)
    for _ in range(4):
        r.render_scene(sc, handles)
        r.present()
    kept = r.view_keep_counts()["kept"]
    assert kept >= 1
    r.set_option("auto_exposure", 1)
    r.set_auto_exposure(0.3, 0.01, 100.0, 0.5, 100, 900)
    r.reset_exposure()
    for _ in range(3):
        r.render_scene(sc, handles)
        r.present()
    assert r.view_keep_counts()["kept"] == kept + 3                   # not one full frame in between
    frame = r.read_framebuffer()
    p, history, want = X.params(0.3, 0.01, 100.0, 0.5, 100, 900), None, None
    for _ in range(3):
        want, history = X.expose(frame, p, history, EXPOSURE)
    same_record(r.read_exposure(0), want)                             # a kept frame is metered like any other
    same_image(r.read_presented(), wanted_image(frame, 0, 1, want["applied"], True))
    r.close()


# ---- 5. the other frame modes ----
@pytest.mark.parametrize("mode", ["supersample", "supersample_merged", "deferred", "bloom_hdr32", "caller_buffers"])
def test_rendered_frame_modes(maps64, mode):
    import torch
    w, h = 64, 64
    r = Renderer(w, h)
    levels, hdr16 = (3, False) if mode == "bloom_hdr32" else (0, True)
    if mode.startswith("supersample"):
        r.set_option("supersample", 2)
        r.set_option("sample_shading", 0 if mode.endswith("merged") else 1)
    if mode == "deferred":
        r.set_option("render_pass", 1)
    r.set_option("bloom", levels)
    r.set_bloom(T, I)
    r.set_option("auto_exposure", 1)
    out = frame_buffer = None
    if mode == "caller_buffers":
        out = torch.zeros(h * w, dtype=torch.int32, device="cuda")
        frame_buffer = torch.zeros(h * w * 4, dtype=torch.float32, device="cuda")
        torch.cuda.synchronize()
        r.set_output_device_ptr(frame_buffer.data_ptr(), frame_buffer.numel() * 4)
    handles = r.render_scene(ball_scene(w, h, maps64, 40.0))
    r.read_framebuffer()                                              # (the capacities settle first: a frame that overflows is metered incomplete)
    r.render_scene(ball_scene(w, h, maps64, 40.0), handles)
    r.present(out.data_ptr() if out is not None else None, hdr16=hdr16)
    frame = r.read_framebuffer()
    rec = r.read_exposure(0)
    want, _ = X.expose(frame, X.DEFAULTS, None, EXPOSURE)
    same_record(rec, want)
    assert rec["counted"] > 0 and rec["flags"] == 0
    if out is not None:
        torch.cuda.synchronize()
        assert B.same_bits(frame_buffer.cpu().numpy().reshape(h, w, 4), frame)
        image = out.cpu().numpy().view(np.uint8).reshape(h, w, 4)
    else:
        image = r.read_presented()
    same_image(image, wanted_image(frame, levels, 1, want["applied"], hdr16))
    r.close()
