"""GPU: option "sky_keep" -- a tile that was background when its frame slot rendered last, and is background again, keeps
the clear colour it holds (k_raster's light-tile path skips the stores; include/bibim_hip.h).

Frames of 96 x 64 (3 x 2 tiles of 32 x 32) and 100 x 70 (4 x 3 tiles, the right column 4 pixels wide, the bottom row 6 pixels
high).  A scene is a set of small triangles, each round the centre of one whole tile and 8 pixels to each side, so its pixel box
lies strictly inside that tile: "no triangle stands on the tile" is exactly "the tile takes k_raster's nothing-touches-it exit",
and a model of what a slot remembers needs nothing but the set of tiles a frame's triangles stand on:

    a tile of a frame is   NONE    a triangle stands on it (or the frame could not keep at all)
                           KEPT    background, and background in the slot's previous frame with nothing forgotten in between
                           FILLED  background otherwise

Every frame read back is compared bit for bit with the CPU oracle's frame and with the same sequence under "sky_keep" 0 (the
behaviour before the option), and bbr_read_sky_tiles with the model.  Every run asserts that it kept and refilled something."""
import functools

import numpy as np
import pytest
import torch

import ui_reference as U
from bibim_renderer_amd import Renderer, textures
from bibim_renderer_amd.renderer import UiDrawData
from oracle import bbo, scenes

NONE, FILLED, KEPT = 0, 1, 2
TILE = 32
SIZES = [(96, 64), (100, 70)]
TAN = np.tan(np.radians(30.0))            # scenes.view_uniforms: fov 60 degrees


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def grid(w, h):
    return (w + TILE - 1) // TILE, (h + TILE - 1) // TILE


def tile_index(w, h, tx, ty):
    return ty * grid(w, h)[0] + tx


@functools.lru_cache(None)
def material():
    return bbo.MaterialData(textures.make_material(16))


@functools.lru_cache(None)
def mesh(w, h, tiles):
    """one triangle per (tx, ty) of `tiles`, round the tile's centre; the camera looks down +z from the origin"""
    def world(px, py, z=2.0):
        return ((px / (w / 2) - 1.0) * TAN * (w / h) * z, (1.0 - py / (h / 2)) * TAN * z, z)   # (the projection turns y over)
    tris = []
    for tx, ty in tiles or ((-4, -4),):   # (no tile: one triangle a hundred pixels outside the frame)
        cx, cy, s = tx * TILE + 16.0, ty * TILE + 16.0, 8.0
        tris += [world(cx + s, cy + s), world(cx - s, cy + s), world(cx, cy - s)]
    v = np.zeros(len(tris), bbo.VERTEX_DTYPE)
    v["pos"] = np.asarray(tris, np.float32)
    v["uv"] = np.linspace(0.0, 1.0, 2 * len(v)).reshape(-1, 2)
    v["normal"], v["tangent"] = (0, 0, -1), (1, 0, 0)
    return v


@functools.lru_cache(None)
def scene(w, h, tiles):
    """tiles: a tuple of (tx, ty); () is a frame of background alone"""
    inst = np.zeros(1, bbo.INSTANCE_DTYPE)
    inst[0] = scenes.instance(np.eye(4, dtype=np.float32))
    fu = scenes.frame_uniforms([scenes.light(0, pos=(0.3, 0.5, 0.0), color=(1.0, 0.9, 0.8), intensity=6.0)], 0, 1.0)
    vu = scenes.view_uniforms((0, 0, 0), 0, 0, w, h, 1)
    return bbo.Scene(fu, vu, [bbo.DrawData(mesh(w, h, tiles), None, inst, material())], w, h, f"sky keep {w}x{h} {tiles}")


@functools.lru_cache(None)
def oracle(w, h, tiles):
    frame, prim, _, _ = bbo.render(scene(w, h, tiles))
    frame.setflags(write=False)
    # the construction holds: every covered pixel lies well inside a tile the scene names, and each of those has some
    covered = prim != bbo.NO_PRIM
    for ty in range(grid(w, h)[1]):
        for tx in range(grid(w, h)[0]):
            box = covered[ty * TILE:(ty + 1) * TILE, tx * TILE:(tx + 1) * TILE]
            assert box.any() == ((tx, ty) in tiles), (tx, ty, tiles)
            if box.any():
                assert not box[:6].any() and not box[-6:].any() and not box[:, :6].any() and not box[:, -6:].any()
    assert (frame[~covered] == 0).all()
    return frame


class Model:
    """what each frame slot remembers; frames go to slots in turn from the moment "frames_in_flight" was set"""

    def __init__(self, w, h, fif):
        self.w, self.h, self.fif, self.k = w, h, fif, 0
        self.sky = [set() for _ in range(fif)]

    def forget(self):
        for s in self.sky:
            s.clear()

    def frame(self, tiles, may_keep=True):
        """the expected bbr_read_sky_tiles of the next frame"""
        gx, gy = grid(self.w, self.h)
        sky = self.sky[self.k % self.fif]
        self.k += 1
        want = np.zeros(gx * gy, np.uint8)
        if not may_keep:
            sky.clear()
            return want
        stood = {tile_index(self.w, self.h, tx, ty) for tx, ty in tiles}
        for t in range(gx * gy):
            if t not in stood:
                want[t] = KEPT if t in sky else FILLED
        sky -= stood
        sky |= set(range(gx * gy)) - stood
        return want


def new_renderer(w, h, fif, keep):
    r = Renderer(w, h)
    r.set_option("frames_in_flight", fif)
    r.set_option("sky_keep", keep)
    return r


def render(r, handles, w, h, tiles):
    """one frame -> (its pixels, its tile report)"""
    r.render_scene(scene(w, h, tiles), handles)
    return r.read_framebuffer(), r.read_sky_tiles()


def check_frame(got, tiles_got, w, h, tiles, want_tiles, what):
    assert np.array_equal(bits(got), bits(oracle(w, h, tiles))), f"{what}: pixels differ from the oracle"
    assert np.array_equal(tiles_got, want_tiles), f"{what}: tiles {tiles_got.tolist()}, model {want_tiles.tolist()}"


# ---- 1. a triangle that moves and then leaves ----
@pytest.mark.gpu
@pytest.mark.parametrize("size", SIZES)
@pytest.mark.parametrize("fif", [1, 2, 3])
def test_moving_triangle_leaves_no_stale_pixels(size, fif):
    w, h = size
    a, b = ((0, 0),), ((1, 1),)
    # F frames on tile A, F on tile B, F + 1 without it: every slot sees A covered -> sky -> sky and B sky -> covered -> sky
    sequence = [a] * fif + [b] * fif + [()] * (fif + 1)
    assert len(sequence) >= 2 * fif + 2
    r1, r0 = new_renderer(w, h, fif, 1), new_renderer(w, h, fif, 0)
    h1, h0 = {"mesh": {}, "mat": {}}, {"mesh": {}, "mat": {}}
    model = Model(w, h, fif)
    kept = filled_late = 0
    for k, tiles in enumerate(sequence):
        got1, t1 = render(r1, h1, w, h, tiles)
        got0, t0 = render(r0, h0, w, h, tiles)
        want = model.frame(tiles)
        check_frame(got1, t1, w, h, tiles, want, f"frame {k}")
        assert np.array_equal(bits(got1), bits(got0)), f"frame {k}: sky_keep 1 and 0 differ"
        assert not (t0 == KEPT).any() and not t0.any(), f"frame {k}: sky_keep 0 reports {t0.tolist()}"
        kept += int((t1 == KEPT).sum())
        filled_late += int((t1 == FILLED).sum()) if k >= fif else 0
    r1.close()
    r0.close()
    ta, tb = tile_index(w, h, 0, 0), tile_index(w, h, 1, 1)
    assert kept > 0 and filled_late >= 2 * fif, (kept, filled_late)   # A and B are refilled once per slot
    assert t1[ta] == KEPT and t1[tb] == KEPT                          # ... and kept in the last frame


# ---- 2. whatever may have written a frame, or moved it, makes every slot start over ----
# (an event that renders a frame of its own tells the model: the slots go on in turn)
def ev_tone_map(r, handles, model, w, h):
    r.tone_map(1, 1.2)
    return w, h


def ev_overlays(r, handles, model, w, h):
    r.set_option("overlays", 1)
    r.render_scene(scene(w, h, ((0, 0),)), handles)
    assert not np.any(model.frame(((0, 0),), may_keep=False)) and not r.read_sky_tiles().any()
    r.present()
    r.draw_overlays(0)
    r.set_option("overlays", 0)
    return w, h


def ev_draw_ui(r, handles, model, w, h):
    r.upload_ui_texture(np.full((2, 2, 4), 255, np.uint8))
    r.present()
    d = U.assemble([((0, 0, w, h), 1, [U.quad(3, 3, 20, 20, U.rgba(255, 0, 0, 128))])], (w, h))
    r.draw_ui(UiDrawData(d.vertices, d.indices, d.cmds, d.display_pos, d.display_size, d.framebuffer_scale))
    return w, h


def ev_external_output(r, handles, model, w, h):
    ext = torch.zeros((h, w, 4), dtype=torch.float32, device="cuda")
    r.set_output_device_ptr(ext.data_ptr(), ext.numel() * 4)
    r.render_scene(scene(w, h, ((0, 0),)), handles)
    assert not np.any(model.frame(((0, 0),), may_keep=False)) and not r.read_sky_tiles().any()
    assert np.array_equal(bits(ext.cpu().numpy()), bits(oracle(w, h, ((0, 0),))))
    r.set_output_device_ptr(None, 0)
    return w, h


def ev_resize_same(r, handles, model, w, h):
    r.resize(w, h)
    return w, h


def ev_resize_other(r, handles, model, w, h):
    w2, h2 = SIZES[1] if (w, h) == SIZES[0] else SIZES[0]
    r.resize(w2, h2)
    return w2, h2


def ev_tile_mode(r, handles, model, w, h):
    r.set_option("tile_mode", 0)
    r.set_option("tile_mode", 1)
    return w, h


def ev_partition(r, handles, model, w, h):
    r.set_partition(0, 2, 32)
    r.set_partition(0, 1, 0)
    return w, h


EVENTS = [ev_tone_map, ev_overlays, ev_draw_ui, ev_external_output, ev_resize_same, ev_resize_other, ev_tile_mode, ev_partition]


@pytest.mark.gpu
@pytest.mark.parametrize("event", EVENTS, ids=lambda e: e.__name__[3:])
def test_every_slot_starts_over_after(event):
    w, h = SIZES[0]
    fif, tiles = 2, ((0, 0),)
    r = new_renderer(w, h, fif, 1)
    handles = {"mesh": {}, "mat": {}}
    model = Model(w, h, fif)
    for k in range(2 * fif):                      # every slot fills, then keeps
        got, t = render(r, handles, w, h, tiles)
        check_frame(got, t, w, h, tiles, model.frame(tiles), f"frame {k}")
    assert (t == KEPT).sum() == t.size - 1
    w, h = event(r, handles, model, w, h)
    if (w, h) != SIZES[0]:                        # (another tile grid; the slots go on in turn)
        model_k, model = model.k, Model(w, h, fif)
        model.k = model_k
    model.forget()
    for k in range(fif):                          # the next frame of every slot keeps nothing ...
        got, t = render(r, handles, w, h, tiles)
        check_frame(got, t, w, h, tiles, model.frame(tiles), f"frame {k} after the event")
        assert not (t == KEPT).any() and (t == FILLED).sum() == t.size - 1
    for k in range(fif):                          # ... and the one after keeps again
        got, t = render(r, handles, w, h, tiles)
        check_frame(got, t, w, h, tiles, model.frame(tiles), f"frame {fif + k} after the event")
        assert (t == KEPT).sum() == t.size - 1
    r.close()


# ---- 3. modes that never keep ----
def _mode_frames(option, keep, w, h, read):
    r = new_renderer(w, h, 2, keep)
    if option:
        r.set_option(*option)
    handles = {"mesh": {}, "mat": {}}
    out = []
    for tiles in [((0, 0),)] * 4 + [()] * 3:
        r.render_scene(scene(w, h, tiles), handles)
        out.append((read(r), r.read_sky_tiles()))
    r.close()
    return out


def _read_frame(r):
    return bits(r.read_framebuffer())


def _read_presented(r):
    r.present()
    return r.read_presented()


def _read_with_visibility(r):
    prim, depth = r.read_visibility()
    return np.concatenate([bits(r.read_framebuffer()).ravel(), prim.ravel(), bits(depth).ravel()])


MODES = {"deferred": (("render_pass", 1), _read_frame), "present_fused": (("present_fused", 1), _read_presented),
         "supersample": (("supersample", 2), _read_frame), "visibility dump": (None, _read_with_visibility),
         "overlays": (("overlays", 1), _read_frame)}


@pytest.mark.gpu
@pytest.mark.parametrize("mode", list(MODES))
def test_modes_that_never_keep(mode):
    w, h = SIZES[1]
    option, read = MODES[mode]
    with_keep, without = _mode_frames(option, 1, w, h, read), _mode_frames(option, 0, w, h, read)
    for k, ((a, ta), (b, tb)) in enumerate(zip(with_keep, without)):
        assert np.array_equal(a, b), f"{mode}, frame {k}: sky_keep 1 and 0 differ"
        assert not (ta == KEPT).any() and not (tb == KEPT).any(), f"{mode}, frame {k}: kept {ta.tolist()}"
    if mode == "visibility dump":   # forward frames: the oracle's too, and the dump's re-render fills what the frame may have kept
        n = w * h * 4
        for k, tiles in enumerate([((0, 0),)] * 4 + [()] * 3):
            assert np.array_equal(with_keep[k][0][:n].reshape(h, w, 4), bits(oracle(w, h, tiles)))


@pytest.mark.gpu
def test_sky_keep_0_keeps_nothing_and_marks_nothing():
    w, h = SIZES[0]
    for got, t in _mode_frames(None, 0, w, h, _read_frame):
        assert not t.any()


# ---- 4. a tile rasterised from a heavy slot ----
HEAVY_GRID = 12   # 144 tiny triangles on one tile: above the threshold of 64 references


@functools.lru_cache(None)
def heavy_scene(tx):
    """SIZES[0]; 144 triangles of 0.9 pixels, one round each pixel centre of a 12 x 12 block in the middle of tile (tx, 0)"""
    w, h = SIZES[0]

    def world(px, py, z=2.0):
        return ((px / (w / 2) - 1.0) * TAN * (w / h) * z, (1.0 - py / (h / 2)) * TAN * z, z)   # (the projection turns y over)
    tris = []
    for j in range(HEAVY_GRID):
        for i in range(HEAVY_GRID):
            cx, cy, s = tx * TILE + 10.5 + i, 10.5 + j, 0.45
            tris += [world(cx + s, cy + s), world(cx - s, cy + s), world(cx, cy - s)]
    v = np.zeros(len(tris), bbo.VERTEX_DTYPE)
    v["pos"] = np.asarray(tris, np.float32)
    v["normal"], v["tangent"] = (0, 0, -1), (1, 0, 0)
    sc = scene(w, h, ())
    return bbo.Scene(sc.frame, sc.view, [bbo.DrawData(v, None, sc.draws[0].instances, material())], w, h, f"sky keep heavy {tx}")


@pytest.mark.gpu
def test_a_tile_rasterised_from_a_heavy_slot_refills():
    """One frame in flight, the long route, heavy tiles first.  Frame 0: tile 0 heavy (no heavy rows yet: its own workgroup does
    it), tile 1 background: filled.  Frame 1: tile 1 heavy -- the launch has heavy rows now, sized from frame 0's list, so a
    workgroup of those rows rasterises tile 1, whose word still says background, and tile 1's own workgroup leaves at once.
    Frame 2: background alone: tile 1 must be filled, not kept."""
    w, h = SIZES[0]
    r = new_renderer(w, h, 1, 1)
    r.set_option("no_tail_items", 0)
    r.set_option("heavy_tiles", 64)
    handles = {"mesh": {}, "mat": {}}
    reports = []
    for k, sc in enumerate([heavy_scene(0), heavy_scene(1), scene(w, h, ())]):
        r.render_scene(sc, handles)
        got = r.read_framebuffer()
        reports.append(r.read_sky_tiles())
        assert np.array_equal(bits(got), bits(bbo.render(sc)[0])), f"frame {k}: pixels differ from the oracle"
    r.close()
    assert reports[0].tolist() == [NONE, FILLED, FILLED, FILLED, FILLED, FILLED]
    assert reports[1].tolist() == [FILLED, NONE, KEPT, KEPT, KEPT, KEPT]
    assert reports[2].tolist() == [KEPT, FILLED, KEPT, KEPT, KEPT, KEPT]
