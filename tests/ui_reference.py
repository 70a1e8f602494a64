"""CPU statement of the GUI pass (bbr_draw_ui; DESIGN.md section 3, include/bibim_hip.h "GUI pass"), in numpy.

Written from the rule and the back end (external/imgui/imgui_impl_vulkan.cpp:122-126, 181-183, 301-306, 406-425, 610-618, 716,
724-732), not from the kernels.  Everything is binary32 in the rule's operand order, with the exact fmaf of aniso_reference:

  vertex     scale = 2 / display_size, translate = -1 - display_pos scale, ndc = pos scale + translate (multiply, then add),
             xs = fmaf(ndc, half, half) with half = 0.5 (float)fb extent, X = rint(256 xs)
  coverage   pixel (px, py) has its centre at (256 px + 128, 256 py + 128); a triangle of negative area has vertices 1 and 2
             exchanged with their attributes, zero area draws nothing; with the area positive, edge i from vertex i to i + 1,
             E_i = dx_i (Yc - Y_i) - dy_i (Xc - X_i); the centre is covered iff every E_i > 0, or = 0 on a left edge (dy < 0) or
             a top edge (dy = 0, dx > 0)
  scissor    r = (clip_rect - display_pos) framebuffer_scale; skipped unless r.x < fb_w, r.y < fb_h, r.z >= 0, r.w >= 0;
             negative r.x / r.y become 0; offset = trunc(r.x), extent = trunc(r.z - r.x) (a negative difference: 0)
  attribute  planes in binary64 from the area S: l1dx = dy2 / S, l1dy = -dx2 / S, l2dx = -dy1 / S, l2dy = dx1 / S, each
             (1 / S) times the integer, rounded to binary32 once; l = fmaf(ldx, dx, ldy dy) with (dx, dy) the centre minus
             vertex 0; a = fmaf(l2, a2 - a0, fmaf(l1, a1 - a0, a0)); a colour channel is (float)byte (1 / 255)
  fragment   src = colour texel, texel one bilinear tap (REPEAT, LOD 0: aniso_reference.bilinear, the oracle's sampler)
  blend      d = DEC[byte], ia = 1 - sa, o = fmaf(s, sa, d ia), byte = #{k: THR[k] <= o}; alpha oa = sa ia,
             byte = rint(255 clamp01(oa)); the bytes are the destination of the next fragment
  order      command order, then index order
"""
from __future__ import annotations

import numpy as np

from aniso_reference import F, bilinear, fmaf

VERTEX_DTYPE = np.dtype([("pos", "<f4", (2,)), ("uv", "<f4", (2,)), ("col", "<u4")])
CMD_DTYPE = np.dtype([("clip_rect", "<f4", (4,)), ("texture", "<i4"), ("vtx_offset", "<u4"), ("idx_offset", "<u4"),
                      ("elem_count", "<u4")])


def _eotf(x):
    x = np.asarray(x, np.float64)
    return np.where(x <= 0.04045, x / 12.92, ((x + 0.055) / 1.055) ** 2.4)


DEC = _eotf(np.arange(256) / 255.0).astype(F)                       # the linear value a byte stands for
THR = _eotf((np.arange(1, 256) - 0.5) / 255.0).astype(F)            # t_k: the linear value at which the byte becomes k


def srgb8(o):
    """the sRGB UNORM8 encode of the presentation: the number of thresholds <= o (NaN: 0)"""
    o = np.asarray(o, F)
    n = np.searchsorted(THR, o, side="right")
    return np.where(np.isnan(o), 0, n).astype(np.uint8)


def blend(dst, src):
    """one fragment each: dst uint8 [n, 4], src binary32 [n, 4] -> uint8 [n, 4]"""
    dst = np.asarray(dst, np.uint8)
    src = np.asarray(src, F)
    sa = src[:, 3]
    ia = (F(1.0) - sa).astype(F)
    out = np.empty(dst.shape, np.uint8)
    for k in range(3):
        di = (DEC[dst[:, k]] * ia).astype(F)
        out[:, k] = srgb8(fmaf(src[:, k], sa, di))
    oa = (sa * ia).astype(F)
    oa = np.where(oa < 0, F(0), np.where(oa > 1, F(1), oa)).astype(F)
    out[:, 3] = np.rint((F(255.0) * oa).astype(F)).astype(np.uint8)
    return out


class DrawData:
    def __init__(self, vertices, indices, cmds, display_pos, display_size, framebuffer_scale=(1.0, 1.0)):
        self.vertices = np.ascontiguousarray(vertices, VERTEX_DTYPE).reshape(-1)
        self.indices = np.ascontiguousarray(indices, np.uint16).reshape(-1)
        self.cmds = np.ascontiguousarray(cmds, CMD_DTYPE).reshape(-1)
        self.display_pos = tuple(float(x) for x in display_pos)
        self.display_size = tuple(float(x) for x in display_size)
        self.framebuffer_scale = tuple(float(x) for x in framebuffer_scale)

    def extent(self):
        return tuple(int(F(self.display_size[k]) * F(self.framebuffer_scale[k])) for k in range(2))


def scissor(clip, draw, fb_w, fb_h):
    """(x0, y0, x1, y1) with exclusive ends, cut to the frame, or None when the command is skipped or nothing can pass"""
    r = [(F(clip[k]) - F(draw.display_pos[k & 1])) * F(draw.framebuffer_scale[k & 1]) for k in range(4)]
    if not (r[0] < fb_w and r[1] < fb_h and r[2] >= 0 and r[3] >= 0):
        return None
    r[0], r[1] = max(r[0], F(0)), max(r[1], F(0))
    box = [0, 0, 0, 0]
    for k, lim in ((0, fb_w), (1, fb_h)):
        off = int(r[k])
        diff = F(r[k + 2] - r[k])
        ext = int(min(diff, F(4294967040.0))) if diff >= 1 else 0
        box[k], box[k + 2] = off, min(off + ext, lim)
    return tuple(box) if box[2] > box[0] and box[3] > box[1] else None


def snap(draw, pos):
    """pos binary32 [n, 2] -> int64 [n, 2] in 1/256 pixel"""
    fb = draw.extent()
    out = np.empty(pos.shape, np.int64)
    for k in range(2):
        scale = F(2.0) / F(draw.display_size[k])
        translate = F(-1.0) - F(F(draw.display_pos[k]) * scale)
        half = F(0.5) * F(fb[k])
        ndc = ((pos[:, k] * scale).astype(F) + translate).astype(F)
        out[:, k] = np.rint((fmaf(ndc, half, half) * F(256.0)).astype(F)).astype(np.int64)
    return out


class Fragments:
    """what one triangle did: handed to render()'s observer before the bytes are written back"""
    __slots__ = ("cmd", "tri", "X", "Y", "attr", "texture", "px", "py", "dst", "out")


def render(image, draw, textures, observer=None):
    """image uint8 [h, w, 4] (not modified) -> the image after the pass.  textures: handle -> uint8 [h, w, 4]."""
    img = np.array(image, np.uint8)
    fb_h, fb_w = img.shape[:2]
    assert draw.extent() == (fb_w, fb_h), (draw.extent(), (fb_w, fb_h))
    P = snap(draw, draw.vertices["pos"])
    uv = draw.vertices["uv"].astype(F)
    col = draw.vertices["col"]
    rgba = np.stack([((col >> (8 * k)) & 0xFF).astype(F) * (F(1.0) / F(255.0)) for k in range(4)], axis=1).astype(F)
    A = np.concatenate([uv, rgba], axis=1).astype(F)                 # u v r g b a per vertex
    tri_no = -1
    for ci, cmd in enumerate(draw.cmds):
        n = int(cmd["elem_count"])
        sc = scissor(cmd["clip_rect"], draw, fb_w, fb_h) if n else None
        if sc is None:
            continue
        tex = np.ascontiguousarray(textures[int(cmd["texture"])], np.uint8)
        idx = draw.indices[int(cmd["idx_offset"]):int(cmd["idx_offset"]) + n].astype(np.int64) + int(cmd["vtx_offset"])
        for t in range(n // 3):
            tri_no += 1
            v = [int(i) for i in idx[3 * t:3 * t + 3]]
            X = [int(P[i, 0]) for i in v]
            Y = [int(P[i, 1]) for i in v]
            S = (X[1] - X[0]) * (Y[2] - Y[0]) - (X[2] - X[0]) * (Y[1] - Y[0])
            if S == 0:
                continue
            if S < 0:
                v[1], v[2] = v[2], v[1]
                X[1], X[2] = X[2], X[1]
                Y[1], Y[2] = Y[2], Y[1]
                S = -S
            x0 = max(sc[0], -((128 - min(X)) // 256))                # first pixel whose centre is >= min
            x1 = min(sc[2], (max(X) - 128) // 256 + 1)
            y0 = max(sc[1], -((128 - min(Y)) // 256))
            y1 = min(sc[3], (max(Y) - 128) // 256 + 1)
            if x0 >= x1 or y0 >= y1:
                continue
            Xc = (np.arange(x0, x1, dtype=np.int64) * 256 + 128)[None, :]
            Yc = (np.arange(y0, y1, dtype=np.int64) * 256 + 128)[:, None]
            inside = np.ones((y1 - y0, x1 - x0), bool)
            for i in range(3):
                j = (i + 1) % 3
                dx, dy = X[j] - X[i], Y[j] - Y[i]
                E = dx * (Yc - Y[i]) - dy * (Xc - X[i])
                inside &= (E >= 0) if (dy < 0 or (dy == 0 and dx > 0)) else (E > 0)
            py, px = np.nonzero(inside)
            if not len(py):
                continue
            py, px = py + y0, px + x0
            rS = 1.0 / float(S)
            dx1, dy1, dx2, dy2 = X[1] - X[0], Y[1] - Y[0], X[2] - X[0], Y[2] - Y[0]
            l1dx, l1dy = F(float(dy2) * rS), F(-float(dx2) * rS)
            l2dx, l2dy = F(-float(dy1) * rS), F(float(dx1) * rS)
            dxp = (px * 256 + 128 - X[0]).astype(F)
            dyp = (py * 256 + 128 - Y[0]).astype(F)
            l1 = fmaf(l1dx, dxp, (l1dy * dyp).astype(F))
            l2 = fmaf(l2dx, dxp, (l2dy * dyp).astype(F))
            a0, d1, d2 = A[v[0]], (A[v[1]] - A[v[0]]).astype(F), (A[v[2]] - A[v[0]]).astype(F)
            attr = fmaf(l2[:, None], d2[None, :], fmaf(l1[:, None], d1[None, :], a0[None, :]))
            texel = bilinear(tex, attr[:, 0], attr[:, 1])
            src = (attr[:, 2:6] * texel).astype(F)
            dst = img[py, px]
            out = blend(dst, src)
            if observer is not None:
                f = Fragments()
                f.cmd, f.tri, f.X, f.Y, f.attr, f.texture, f.px, f.py, f.dst, f.out = ci, tri_no, X, Y, A[v], tex, px, py, dst, out
                observer(f)
            img[py, px] = out
    return img


def quad(x0, y0, x1, y1, col, uv=((0.0, 0.0), (1.0, 1.0)), flip=False):
    """(vertices [4], indices [6]) of an axis-aligned quad as the GUI's PrimRect emits it (a b c, a c d); flip reverses the
    winding of both triangles"""
    v = np.zeros(4, VERTEX_DTYPE)
    v["pos"] = [(x0, y0), (x1, y0), (x1, y1), (x0, y1)]
    (u0, v0), (u1, v1) = uv
    v["uv"] = [(u0, v0), (u1, v0), (u1, v1), (u0, v1)]
    v["col"] = col
    idx = [0, 2, 1, 0, 3, 2] if flip else [0, 1, 2, 0, 2, 3]
    return v, np.array(idx, np.uint16)


def rgba(r, g, b, a):
    return (int(a) << 24) | (int(b) << 16) | (int(g) << 8) | int(r)


def assemble(parts, display_size, display_pos=(0.0, 0.0), framebuffer_scale=(1.0, 1.0)):
    """parts: [(clip_rect, texture, [(vertices, indices), ...])] -> DrawData, one command per part, vtx_offset = the part's
    first vertex (so that it is not 0 from the second part on)"""
    vs, is_, cmds = [], [], np.zeros(len(parts), CMD_DTYPE)
    nv = ni = 0
    for k, (clip, texture, prims) in enumerate(parts):
        cmds[k]["clip_rect"], cmds[k]["texture"], cmds[k]["vtx_offset"], cmds[k]["idx_offset"] = clip, texture, nv, ni
        local = 0
        for v, i in prims:
            vs.append(v)
            is_.append((i.astype(np.int64) + local).astype(np.uint16))
            local += len(v)
            ni += len(i)
            cmds[k]["elem_count"] += len(i)
        nv += local
    vertices = np.concatenate(vs) if vs else np.zeros(0, VERTEX_DTYPE)
    indices = np.concatenate(is_) if is_ else np.zeros(0, np.uint16)
    return DrawData(vertices, indices, cmds, display_pos, display_size, framebuffer_scale)
