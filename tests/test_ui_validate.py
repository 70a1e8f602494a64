"""bbr_ui_validate: the host-only check (no context, no device) that keeps a malformed GUI draw list from reaching a kernel.
Every rejection include/bibim_hip.h lists, the returned box, and the header behind it (csrc/bb_ui.h) in a stand-alone program
under AddressSanitizer + UBSan on heap arrays of the exact size."""
import json
import os
import shutil
import subprocess

import numpy as np
import pytest

import ui_reference as U
from bibim_renderer_amd.renderer import UI_CMD_DTYPE, UI_VERTEX_DTYPE, UiDrawData, ui_validate
from conftest import GOLDEN, ROOT

OK, INVALID = 0, -1
W, H = 64, 48


def draw(cmds=None, vertices=None, indices=None, **kw):
    v, i = U.quad(4, 4, 20, 12, U.rgba(255, 255, 255, 128))
    c = np.zeros(1, UI_CMD_DTYPE)
    c[0] = ((0, 0, W, H), 1, 0, 0, 6)
    d = UiDrawData(v if vertices is None else vertices, i if indices is None else indices, c if cmds is None else cmds,
                   kw.get("display_pos", (0, 0)), kw.get("display_size", (W, H)), kw.get("framebuffer_scale", (1, 1)))
    return d


def commands(*rows):
    c = np.zeros(len(rows), UI_CMD_DTYPE)
    for k, r in enumerate(rows):
        c[k] = r
    return c


def test_dtypes_are_the_headers_layouts():
    assert UI_CMD_DTYPE.itemsize == 32 and UI_VERTEX_DTYPE.itemsize == 20
    assert UI_CMD_DTYPE == U.CMD_DTYPE and UI_VERTEX_DTYPE == U.VERTEX_DTYPE


def test_valid_draw_data_and_its_box():
    assert ui_validate(draw(), W, H) == (OK, (0, 0, W, H))
    c = commands(((2.5, -3.0, 30.2, 20.9), 1, 0, 0, 6), ((40.0, 10.0, 90.0, 47.5), 1, 0, 0, 6), ((70.0, 0.0, 90.0, 9.0), 1, 0, 0, 6),
                 ((0.0, 0.0, W, H), 1, 0, 0, 0))
    # [2, 29) x [0, 20) and [40, 64) x [10, 47); the command beyond the frame and the one without elements add nothing
    assert ui_validate(draw(c), W, H) == (OK, (2, 0, 64, 47))
    assert ui_validate(draw(commands(((70.0, 0.0, 90.0, 9.0), 1, 0, 0, 6))), W, H) == (OK, (0, 0, 0, 0))
    empty = UiDrawData(np.zeros(0, UI_VERTEX_DTYPE), np.zeros(0, np.uint16), np.zeros(0, UI_CMD_DTYPE), (0, 0), (W, H))
    assert ui_validate(empty, W, H) == (OK, (0, 0, 0, 0))


def test_box_follows_display_pos_and_framebuffer_scale():
    c = commands(((110.0, 205.0, 120.0, 215.5), 1, 0, 0, 6))
    d = draw(c, display_pos=(100, 200), display_size=(32, 24), framebuffer_scale=(2, 2))
    assert ui_validate(d, W, H) == (OK, (20, 10, 40, 31))           # (10, 5, 20, 15.5) * 2
    assert U.scissor(c[0]["clip_rect"], U.DrawData(d.vertices, d.indices, c, (100, 200), (32, 24), (2, 2)), W, H) == (20, 10, 40, 31)


@pytest.mark.parametrize("cmd", [((0, 0, W, H), 1, 0, 0, 5), ((0, 0, W, H), 1, 0, 0, 4),            # elem_count % 3
                                 ((0, 0, W, H), 1, 0, 3, 6), ((0, 0, W, H), 1, 0, 0xFFFFFFFD, 6),  # idx_offset + elem_count
                                 ((0, 0, W, H), 1, 1, 0, 6), ((0, 0, W, H), 1, 0xFFFFFFFF, 0, 6),  # vtx_offset + index
                                 ((90, 0, 99, H), 1, 1, 0, 6)])                                    # ... in a command that is skipped
def test_bad_command_is_rejected(cmd):
    assert ui_validate(draw(commands(cmd)), W, H)[0] == INVALID


def test_index_past_the_vertices_is_rejected():
    assert ui_validate(draw(indices=np.array([0, 1, 4, 0, 2, 3], np.uint16)), W, H)[0] == INVALID
    assert ui_validate(draw(indices=np.array([0, 1, 3, 0, 2, 3], np.uint16)), W, H)[0] == OK


@pytest.mark.parametrize("field,k", [("pos", 0), ("pos", 1), ("uv", 0), ("uv", 1)])
@pytest.mark.parametrize("bad", [np.inf, -np.inf, np.nan])
def test_non_finite_vertex_is_rejected(field, k, bad):
    v, _ = U.quad(4, 4, 20, 12, 0)
    v[field][3, k] = bad
    assert ui_validate(draw(vertices=v), W, H)[0] == INVALID


def test_snapped_coordinate_must_stay_within_two_to_the_23():
    v, _ = U.quad(4, 4, 20, 12, 0)
    v["pos"][1, 0] = 32768.0          # 2 / 64 is exact: ndc 1023, 32 * 1023 + 32 = 32768 pixels = 2^23 / 256
    v["pos"][2, 1] = -30000.0
    assert ui_validate(draw(vertices=v), W, H)[0] == OK
    v["pos"][1, 0] = 32768.01
    assert ui_validate(draw(vertices=v), W, H)[0] == INVALID
    v["pos"][1, 0] = -32768.0         # the other side (display size = frame: a position is its pixel coordinate)
    assert ui_validate(draw(vertices=v), W, H)[0] == OK
    v["pos"][1, 0] = -32768.01
    assert ui_validate(draw(vertices=v), W, H)[0] == INVALID
    v["pos"][1, 0] = 3.0e38
    assert ui_validate(draw(vertices=v), W, H)[0] == INVALID


@pytest.mark.parametrize("size", [(0.0, H), (W, 0.0), (-W, H), (W, np.nan), (np.inf, H)])
def test_display_size_must_be_positive(size):
    assert ui_validate(draw(display_size=size), W, H)[0] == INVALID


def test_frame_and_null_arguments():
    L = __import__("bibim_renderer_amd")._capi.lib()
    assert L.bbr_ui_validate(None, W, H, None) == INVALID
    assert ui_validate(draw(), 0, H)[0] == INVALID and ui_validate(draw(), W, 40000)[0] == INVALID
    d = draw().struct()
    d.vertices = None
    assert L.bbr_ui_validate(d, W, H, None) == INVALID
    d = draw()
    s = d.struct()
    assert L.bbr_ui_validate(s, W, H, None) == OK                    # the box is optional


def test_committed_draw_data_is_valid_and_boxed_like_the_reference():
    z = np.load(os.path.join(GOLDEN, "ui_drawdata.npz"))
    d = UiDrawData(z["vertices"].copy().view(UI_VERTEX_DTYPE).reshape(-1), z["indices"], z["cmds"].copy().view(UI_CMD_DTYPE).reshape(-1),
                   z["display_pos"], z["display_size"], z["framebuffer_scale"])
    rc, box = ui_validate(d, 1280, 720)
    ref = U.DrawData(d.vertices, d.indices, d.cmds, d.display_pos, d.display_size, d.framebuffer_scale)
    boxes = [U.scissor(c["clip_rect"], ref, 1280, 720) for c in ref.cmds if c["elem_count"]]
    boxes = np.array([b for b in boxes if b is not None])
    assert rc == OK and box == (boxes[:, 0].min(), boxes[:, 1].min(), boxes[:, 2].max(), boxes[:, 3].max())
    assert ui_validate(d, 1280, 721)[0] == OK                       # (the extent is bbr_draw_ui's to check, not the validator's)


def test_validate_header_under_address_and_ub_sanitizers(tmp_path):
    """tests/ui_validate_check.cpp with the host compiler: csrc/bb_ui.h alone, the runtimes linked into the program"""
    cxx = shutil.which("g++") or shutil.which("c++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path / "ui_validate_check")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-static-libasan", "-static-libubsan",
                           "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "bibim_renderer_amd", "csrc"),
                           os.path.join(ROOT, "tests", "ui_validate_check.cpp"), "-o", exe])
    p = subprocess.run([exe], capture_output=True, text=True)
    assert p.returncode == 0, p.stdout + p.stderr
    assert p.stdout.count(" ok\n") == 35 and "WRONG" not in p.stdout
    # the library's decode table (std::pow on the host) is the reference's, bit for bit
    dec = [l for l in p.stdout.splitlines() if l.startswith("dec ")][0].split()[1:]
    assert [int(x, 16) for x in dec] == json.load(open(os.path.join(GOLDEN, "ui_tables.json")))["dec_bits"]
