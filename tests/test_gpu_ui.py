"""GUI pass (bbr_draw_ui; src/main.cpp:172): the back end's draw lists blended into the presented image, GPU against
tests/ui_reference.py byte for byte.

The expected image is always ui_reference applied to the bytes read back from the GPU BEFORE the call, so that the pass is
separated from everything in front of it.  A read-back synchronises and lets the capacities settle (a frame that overflowed is
rendered and presented again), so the bytes read before the call are the ones the pass blends over."""
import os

import numpy as np
import pytest

import ui_reference as U
from conftest import GOLDEN
from bibim_renderer_amd import BibimError, Renderer, configs
from bibim_renderer_amd.renderer import UI_CMD_DTYPE, UI_VERTEX_DTYPE, UiDrawData
from oracle import bbo, scenes

pytestmark = pytest.mark.gpu

INVALID, NOT_IN_FRAME = -1, -6


def to_gpu(d):
    return UiDrawData(d.vertices, d.indices, d.cmds, d.display_pos, d.display_size, d.framebuffer_scale)


@pytest.fixture(scope="module")
def fixture_draw():
    z = np.load(os.path.join(GOLDEN, "ui_drawdata.npz"))
    draw = U.DrawData(z["vertices"].copy().view(U.VERTEX_DTYPE).reshape(-1), z["indices"], z["cmds"].copy().view(U.CMD_DTYPE).reshape(-1),
                      z["display_pos"], z["display_size"], z["framebuffer_scale"])
    atlas = np.full(z["atlas_alpha"].shape + (4,), 255, np.uint8)
    atlas[..., 3] = z["atlas_alpha"]
    return draw, atlas


@pytest.fixture(scope="module")
def hazard_textures(fixture_draw):
    rng = np.random.default_rng(7)
    return {1: fixture_draw[1], 2: np.array([[[255, 200, 90, 180]]], np.uint8), 3: rng.integers(0, 256, (3, 5, 4), dtype=np.uint8)}


def upload(r, textures):
    """handles 1, 2, 3, ... in this order: the numbers the draw data names"""
    for want in sorted(textures):
        assert r.upload_ui_texture(textures[want]) == want


def hazards(w, h, stack=3000):
    """the hazard list, inside the frame's top-left 128 x 128 pixels but for the last part; textures alternate per command"""
    rng = np.random.default_rng(11)
    col = lambda a: U.rgba(*rng.integers(0, 256, 3), a)
    parts = []
    # overlapping translucent quads on integer bounds (their diagonals run through pixel centres), both windings, uv beyond [0, 1]
    parts.append(((0, 0, w, h), 1, [U.quad(8 + 5 * k, 6 + 3 * k, 40 + 5 * k, 38 + 3 * k, col(60 + 40 * k), ((-0.5, -0.25), (2.5, 1.75)), flip=bool(k & 1))
                                    for k in range(5)]))
    # fractional scissor; zero-area and sub-pixel triangles among ordinary ones
    v = np.zeros(12, U.VERTEX_DTYPE)
    v["pos"] = [(20, 20), (20, 20), (50, 45),          # two vertices coincide
                (12, 12), (30, 30), (48, 48),          # collinear
                (33.4, 33.4), (33.6, 33.4), (33.5, 33.6),   # sub-pixel around the centre (33.5, 33.5): covers it
                (35.1, 35.1), (35.3, 35.1), (35.2, 35.3)]   # sub-pixel between centres: covers nothing
    v["uv"] = rng.random((12, 2)) * 3 - 1
    v["col"] = [col(200) for _ in range(12)]
    parts.append(((10.9, -3.0, 60.1, 49.9), 3, [(v, np.arange(12, dtype=np.uint16)), U.quad(5.5, 2.25, 70.75, 55.5, col(150), ((0, 0), (4, 4)))]))
    # vertices at +-30 000 pixels, a scissor with a negative origin
    big = np.zeros(3, U.VERTEX_DTYPE)
    big["pos"] = [(-30000.0, -29000.0), (30000.0, -28000.5), (100.25, 30000.0)]
    big["uv"] = [(0, 0), (900, 0), (450, 900)]
    big["col"] = [U.rgba(255, 0, 0, 90), U.rgba(0, 255, 0, 40), U.rgba(0, 0, 255, 140)]
    parts.append(((-20.5, -7.25, 90.5, 100.0), 2, [(big, np.array([0, 1, 2], np.uint16)), (big, np.array([2, 1, 0], np.uint16))]))
    parts.append(((0, 0, w, h), 3, []))                                                        # elem_count 0
    parts.append(((w + 0.5, 0, w + 50, h), 1, [U.quad(0, 0, w, h, col(255))]))                 # scissors that admit nothing:
    parts.append(((0, -9.0, w, -0.5), 2, [U.quad(0, 0, w, h, col(255))]))                      # beyond the frame, above it,
    parts.append(((30.0, 0, 12.0, h), 3, [U.quad(0, 0, w, h, col(255))]))                      # turned inside out
    # stacked quads inside the tile (1, 1): its ordered list crosses the 1024-entry chunk and the 256-box scan step
    quads = []
    for k in range(stack):
        x0, y0 = 33 + (k * 7) % 19, 34 + (k * 5) % 17
        quads.append(U.quad(x0, y0, x0 + 3 + k % 9, y0 + 2 + k % 11, col(3 + k % 60), flip=bool(k % 3 == 0)))
    parts.append(((32.0, 32.0, 64.0, 64.0), 2, quads))
    # a translucent quad over the frame's bottom-right corner and beyond it (tiles that the frame cuts)
    parts.append(((w - 37.5, h - 41.25, w + 100, h + 100), 3, [U.quad(w - 50, h - 50, w + 20, h + 30, col(120), ((0.1, 0.2), (0.9, 1.4)))]))
    return U.assemble(parts, (w, h))


def small_list(w, h, seed):
    rng = np.random.default_rng(seed)
    quads = [U.quad(*(rng.random(2) * (w / 2, h / 2)), *(rng.random(2) * (w / 2, h / 2) + (w / 2, h / 2)), U.rgba(*rng.integers(0, 256, 4)),
                    flip=bool(k & 1)) for k in range(3 + seed)]
    return U.assemble([((0, 0, w, h), 1 + seed % 3, quads), ((3.5, 2.5, w - 7.25, h - 1.5), 1 + (seed + 1) % 3, quads[:2])], (w, h))


def scene_of(w, h, maps64):
    return scenes.shaderball_scene(configs.C2.scaled(w, h, 64), bbo.MaterialData(maps64))


def presented_base(r, sc, handles=None):
    handles = r.render_scene(sc, handles)
    r.present()
    return r.read_presented(), handles


def check_equal(got, want, base, draw):
    bad = (got != want).any(axis=2)
    assert not bad.any(), (int(bad.sum()), [(int(y), int(x), got[y, x].tolist(), want[y, x].tolist()) for y, x in np.argwhere(bad)[:5]])
    boxes = [U.scissor(c["clip_rect"], draw, base.shape[1], base.shape[0]) for c in draw.cmds if c["elem_count"]]
    outside = np.ones(base.shape[:2], bool)
    for b in boxes:
        if b is not None:
            outside[b[1]:b[3], b[0]:b[2]] = False
    assert np.array_equal(got[outside], base[outside])                 # nothing outside the scissors was touched


@pytest.mark.parametrize("fused", [False, True])
def test_fixture_over_a_frame(maps64, fixture_draw, fused):
    draw, atlas = fixture_draw
    textures = {1: atlas, 2: maps64["albedo"]}
    sc = scene_of(1280, 720, maps64)
    r = Renderer(1280, 720)
    r.set_option("present_fused", int(fused))
    upload(r, textures)
    base, _ = presented_base(r, sc)
    assert (base[..., :3] != 0).any()
    r.draw_ui(to_gpu(draw))
    got = r.read_presented()
    want = U.render(base, draw, textures)
    assert (want != base).any(axis=2).sum() > 150000                   # the window is really there
    check_equal(got, want, base, draw)
    r.close()


@pytest.fixture(scope="module")
def hazard_case(hazard_textures):
    """(draw data, a function giving the expected image over a base) per frame size: the reference runs once per size"""
    cache = {}

    def get(w, h, base):
        if (w, h) not in cache:
            draw = hazards(w, h)
            cache[(w, h)] = (draw, base.copy(), U.render(base, draw, hazard_textures))
        draw, seen, want = cache[(w, h)]
        assert np.array_equal(seen, base), "the frame in front of the pass is not deterministic"
        return draw, want
    return get


@pytest.mark.parametrize("size,tile_mode", [((128, 128), 1), ((333, 207), 1), ((333, 207), 0)])
def test_hazard_list(maps64, hazard_textures, hazard_case, size, tile_mode):
    w, h = size
    r = Renderer(w, h)
    r.set_option("tile_mode", tile_mode)                               # the scene's tile size changes nothing
    upload(r, hazard_textures)
    base, _ = presented_base(r, scene_of(w, h, maps64))
    draw, want = hazard_case(w, h, base)
    assert len(draw.indices) // 3 > 6000 and (draw.cmds["vtx_offset"][1:] != 0).all() and (draw.cmds["elem_count"] == 0).any()
    r.draw_ui(to_gpu(draw))
    check_equal(r.read_presented(), want, base, draw)
    assert (want != base).any(axis=2).sum() > 3000
    r.close()


def test_caller_buffer_and_a_frame_presented_again(maps64, hazard_textures):
    import torch
    w, h = 128, 128
    sc = scene_of(w, h, maps64)
    draw = small_list(w, h, 2)
    r = Renderer(w, h)
    upload(r, hazard_textures)
    base, handles = presented_base(r, sc)
    want = U.render(base, draw, hazard_textures)
    for _ in range(2):                                                 # the same call on a frame presented again: the same bytes
        r.present()
        r.draw_ui(to_gpu(draw))
        assert np.array_equal(r.read_presented(), want)
    out = torch.zeros(h * w, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    r.present(out.data_ptr())
    r.draw_ui(to_gpu(draw))
    r.synchronize()
    got = out.cpu().numpy().view(np.uint8).reshape(h, w, 4)
    assert np.array_equal(got, want)
    r.close()


def test_fused_frame_in_a_caller_buffer(maps64, hazard_textures):
    """option present_fused AND a caller's buffer: bbr_present copied the slot's image to the buffer before the GUI was in it,
    so the pass has to bring the buffer up to date; the list's scissors leave rows and columns of the frame untouched"""
    import torch
    w, h = 333, 207
    r = Renderer(w, h)
    r.set_option("present_fused", 1)
    upload(r, hazard_textures)
    base, handles = presented_base(r, scene_of(w, h, maps64))
    quads = [U.quad(20.5, 40.25, 300.0, 150.5, U.rgba(250, 40, 90, 130)), U.quad(100, 60, 333, 207, U.rgba(10, 200, 90, 70), flip=True)]
    draw = U.assemble([((31.5, 50.0, 290.0, 140.5), 1, quads), ((120.0, 70.0, 310.5, 180.0), 3, quads[1:])], (w, h))
    want = U.render(base, draw, hazard_textures)
    assert (want != base).any(axis=2).sum() > 20000
    out = torch.zeros(h * w, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    r.present(out.data_ptr())
    r.draw_ui(to_gpu(draw))
    r.synchronize()
    got = out.cpu().numpy().view(np.uint8).reshape(h, w, 4)
    check_equal(got, want, base, draw)
    assert np.array_equal(r.read_presented(), want)                    # the slot's image and the caller's copy agree
    r.close()


def test_a_freed_texture_handle_is_handed_out_again(maps64, hazard_textures):
    w, h = 128, 128
    r = Renderer(w, h)
    upload(r, hazard_textures)
    base, _ = presented_base(r, scene_of(w, h, maps64))
    rng = np.random.default_rng(5)
    textures = dict(hazard_textures)
    for _ in range(3):                                                 # an atlas rebuilt again and again: the same handle
        r.free_ui_texture(2)
        textures[2] = rng.integers(0, 256, (4, 7, 4), dtype=np.uint8)
        assert r.upload_ui_texture(textures[2]) == 2
    assert r.upload_ui_texture(np.zeros((1, 1, 4), np.uint8)) == 4      # nothing dead is left: the table grows
    draw = U.assemble([((0, 0, w, h), 2, [U.quad(10, 12, 100, 90, U.rgba(255, 255, 255, 200), ((-1, -1), (2, 2)))])], (w, h))
    r.draw_ui(to_gpu(draw))
    check_equal(r.read_presented(), U.render(base, draw, textures), base, draw)
    r.close()


@pytest.mark.parametrize("frames_in_flight", [1, 3])
def test_six_frames_with_different_draw_data(maps64, hazard_textures, frames_in_flight):
    """nothing synchronises between the frames: a slot's staging, records and image are reused while its neighbours are in
    flight; the fifth list is larger than any before (staging and records grow), the last one is compared"""
    w, h = 333, 207
    sc = scene_of(w, h, maps64)
    r = Renderer(w, h)
    r.set_option("frames_in_flight", frames_in_flight)
    upload(r, hazard_textures)
    base, handles = presented_base(r, sc)
    lists = [small_list(w, h, k) for k in range(4)] + [hazards(w, h, stack=400), small_list(w, h, 9)]
    for d in lists:
        r.render_scene(sc, handles)
        r.present()
        r.draw_ui(to_gpu(d))
    got = r.read_presented()
    check_equal(got, U.render(base, lists[-1], hazard_textures), base, lists[-1])
    r.close()


def test_growth_and_resize(maps64, hazard_textures):
    w, h = 128, 128
    r = Renderer(w, h)
    upload(r, hazard_textures)
    base, handles = presented_base(r, scene_of(w, h, maps64))
    small, large = small_list(w, h, 1), hazards(w, h, stack=700)
    r.draw_ui(to_gpu(small))
    assert np.array_equal(r.read_presented(), U.render(base, small, hazard_textures))
    r.present()
    r.draw_ui(to_gpu(large))                                           # larger than any before: the slot's buffers grow
    assert np.array_equal(r.read_presented(), U.render(base, large, hazard_textures))
    r.resize(333, 207)
    with pytest.raises(BibimError) as e:
        r.draw_ui(to_gpu(small_list(333, 207, 1)))
    assert e.value.code == NOT_IN_FRAME
    base, _ = presented_base(r, scene_of(333, 207, maps64))
    d = small_list(333, 207, 4)
    r.draw_ui(to_gpu(d))
    check_equal(r.read_presented(), U.render(base, d, hazard_textures), base, d)
    r.close()


def test_status_codes_and_nothing_drawn(maps64, hazard_textures):
    w, h = 128, 128
    sc = scene_of(w, h, maps64)
    good = small_list(w, h, 3)
    r = Renderer(w, h)
    upload(r, hazard_textures)

    def code(d):
        with pytest.raises(BibimError) as e:
            r.draw_ui(to_gpu(d))
        return e.value.code

    assert code(good) == NOT_IN_FRAME                                  # before a frame
    handles = r.render_scene(sc)
    assert code(good) == NOT_IN_FRAME                                  # before a present
    r.present()
    base = r.read_presented()

    def variant(**kw):
        d = U.DrawData(good.vertices.copy(), good.indices.copy(), good.cmds.copy(), good.display_pos, good.display_size, good.framebuffer_scale)
        for k, v in kw.items():
            setattr(d, k, v)
        return d

    assert code(variant(display_size=(w + 1.0, float(h)))) == INVALID  # (int)(display_size * framebuffer_scale) is not the extent
    assert code(variant(framebuffer_scale=(1.0, 2.0))) == INVALID
    assert code(variant(display_size=(0.0, float(h)))) == INVALID
    bad = variant()
    bad.cmds["elem_count"][0] -= 1
    assert code(bad) == INVALID                                        # elem_count % 3
    bad = variant()
    bad.cmds["idx_offset"][1] = len(good.indices) - 3
    assert code(bad) == INVALID                                        # idx_offset + elem_count > n_indices
    bad = variant()
    bad.cmds["vtx_offset"][0] = len(good.vertices) - 2
    assert code(bad) == INVALID                                        # vtx_offset + index >= n_vertices
    bad = variant()
    bad.vertices["uv"][1, 0] = np.nan
    assert code(bad) == INVALID
    bad = variant()
    bad.vertices["pos"][0, 1] = 40000.0
    assert code(bad) == INVALID                                        # snapped coordinate beyond 2^23
    for handle in (0, 4, -1):
        bad = variant()
        bad.cmds["texture"][1] = handle
        assert code(bad) == INVALID                                    # a texture that never existed
    extra = r.upload_ui_texture(np.zeros((2, 2, 4), np.uint8))
    bad = variant()
    bad.cmds["texture"][0] = extra
    r.free_ui_texture(extra)
    assert code(bad) == INVALID                                        # ... or is not alive any more
    with pytest.raises(BibimError):
        r.free_ui_texture(extra)
    dead = variant()
    dead.cmds["texture"][1], dead.cmds["elem_count"][1] = 77, 0        # a command that draws nothing names no texture
    assert np.array_equal(r.read_presented(), base)                    # none of the rejected calls touched the image
    r.draw_ui(to_gpu(dead))
    assert np.array_equal(r.read_presented(), U.render(base, dead, hazard_textures))
    r.close()

    r = Renderer(w, 256)                                               # two bands of two ranks: a partitioned context
    upload(r, hazard_textures)
    r.set_partition(0, 2, 64)
    r.render_scene(scene_of(w, 256, maps64))
    r.present()
    with pytest.raises(BibimError) as e:
        r.draw_ui(to_gpu(small_list(w, 256, 3)))
    assert e.value.code == INVALID
    r.close()
