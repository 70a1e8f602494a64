"""Scenes for shadow mapping (option "shadow_map"): a receiver, occluders, four lights and the light's
view block.  TEST INFRASTRUCTURE ONLY; no test lives here.

The camera is the surface chart's (tests/surface_chart.py): `view` = identity, an exact orthographic `proj`, world x, y in
[-4, 4] fill the frame and z in [-2, 2] maps into depth (0.25, 0.75).  A pixel's world position is therefore closed-form on the
CPU: x, y from the pixel centre, z from the plane of the triangle that wins the pixel (`positions64`).

  receiver   the chart's tilted quad z = 0.3125 x + 0.1875 y, normal map on.  Both casters look along its normal, so all of
             it has ONE depth in the light's frame: where the map holds the receiver's own depth, the last bit of two
             different evaluations decides at bias 0
  occluders  two quads parallel to the receiver, 0.75 in front of it as the lights see it (the camera keeps the larger z, so
             it looks through them at the receiver): a block, and a sliver 0.09 wide -- three texels of the largest map
  lights     four; the caster is index 2 (CASTER), never 0
  kinds      "ortho"    a directional caster, an orthographic light projection of half extent 3: the receiver runs beyond the
                        light's frustum on all four sides
             "spot"     a spot caster 1.5 in front of the receiver, a perspective light projection of 110 degrees: the
                        receiver runs beyond its frustum on all sides.  The receiver ends at x = -2.75; the strip left of it
                        shows a wall parallel to it and 1.75 further from the camera -- behind the light: w <= 0
             "clipped"  "spot" plus a triangle that crosses the light's near plane: the map itself goes through the clipper
"""
from __future__ import annotations

import functools

import numpy as np

import surface_chart as SC
from oracle import bbo, scenes

KINDS = ("ortho", "spot", "clipped")
CASTER = 2
FRAME_SMALL = (97, 61)          # off both tile grids
FRAME_DUMP = (128, 128)         # the dumps
SIDES = (1, 33, 64, 200)        # a single texel, off the tile grid, one 64-tile, several tiles
BIASES = (0.0, 2.0 ** -8, -1.0, 2.0)   # an ulp decides; the working value; everything inside shadowed; nothing shadowed
BIAS = 2.0 ** -8
OFFSET = 0.75                   # occluders: this far in front of the receiver
# x0, x1, y0, y1 of the two occluders, where each light sees them
BLOCK = {"ortho": (-1.5, 1.0, -1.0, 1.5), "spot": (0.25, 1.5, -1.25, 0.0)}
SLIVER = {"ortho": (2.0, 2.09375, -3.0, 3.0), "spot": (-0.5, -0.46875, -1.5, 1.5)}

f32 = SC.f32


def receiver_z(x, y):
    return SC.TILT[0] * x + SC.TILT[1] * y


def _quad(x0, x1, y0, y1, dz):
    v = np.zeros(4, bbo.VERTEX_DTYPE)
    for k, (x, y) in enumerate([(x0, y0), (x0, y1), (x1, y1), (x1, y0)]):     # the chart's order: front-facing
        v["pos"][k] = (x, y, receiver_z(x, y) - dz)
        v["uv"][k] = ((x + 4.0) / 8.0, (4.0 - y) / 8.0)
    v["normal"] = (SC.TILT[0], SC.TILT[1], -1.0)
    v["tangent"] = (1.0, 0.0, SC.TILT[0])
    return v


# where the spot caster sits and looks; its near plane is NEAR in front of it
NORMAL = np.array([SC.TILT[0], SC.TILT[1], -1.0])                      # of the receiver, towards the lights
SPOT_TARGET = (0.5, 0.0, SC.TILT[0] * 0.5)                             # on the receiver
SPOT_EYE = tuple(float(v) for v in f32(np.asarray(SPOT_TARGET) + 1.5 * NORMAL / np.sqrt((NORMAL * NORMAL).sum())))
SPOT_FOV, NEAR, FAR = 110.0, 0.25, 16.0
DIR_ORTHO = tuple(-NORMAL)
ORTHO_HALF, ORTHO_DISTANCE = 3.0, 8.0
WALL_X, WALL_OFFSET = -2.75, -1.75                                      # spot kinds: the wall behind the light


def _near_crossing_triangle():
    """a triangle through the spot's near plane: one vertex behind the light, two in front of it, all in front of the
    receiver (smaller z), wound like the quads"""
    v = np.zeros(3, bbo.VERTEX_DTYPE)
    pts = [(0.625, 0.4375, -1.5625), (1.25, 0.4375, -0.5625), (0.8125, -0.4375, -0.4375)]
    for k, p in enumerate(pts):
        v["pos"][k] = p
        v["uv"][k] = ((p[0] + 4.0) / 8.0, (4.0 - p[1]) / 8.0)
    v["normal"] = (SC.TILT[0], SC.TILT[1], -1.0)
    v["tangent"] = (1.0, 0.0, SC.TILT[0])
    return v


@functools.lru_cache(None)
def _draws(kind):
    one = np.zeros(1, bbo.INSTANCE_DTYPE)
    one[0]["model"] = one[0]["inv_model"] = np.eye(4, dtype=np.float32)
    mat = bbo.MaterialData(SC.material("packed", 6))
    where = "ortho" if kind == "ortho" else "spot"
    recv, ridx = _quad(-4.0, 4.0, -4.0, 4.0, 0.0), SC.QUAD_INDEX.copy()
    if where == "spot":
        recv = np.concatenate([_quad(WALL_X, 4.0, -4.0, 4.0, 0.0), _quad(-4.0, WALL_X, -4.0, 4.0, -WALL_OFFSET)])
        ridx = np.concatenate([SC.QUAD_INDEX, SC.QUAD_INDEX + 4]).astype(np.uint32)
    occ = np.concatenate([_quad(*BLOCK[where], OFFSET), _quad(*SLIVER[where], OFFSET)])
    idx = np.concatenate([SC.QUAD_INDEX, SC.QUAD_INDEX + 4]).astype(np.uint32)
    if kind == "clipped":
        occ = np.concatenate([occ, _near_crossing_triangle()])
        idx = np.concatenate([idx, np.array([8, 9, 10], np.uint32)])
    return (bbo.DrawData(recv, ridx, one, mat), bbo.DrawData(occ, idx, one, mat))


def lights(kind):
    """four lights, the caster at index CASTER; the others as the chart's regular set"""
    a, view_pos = SC.set_a()
    if kind == "ortho":
        a[CASTER] = SC.L(2, dir=DIR_ORTHO, color=(0.9, 0.8, 0.7), intensity=2.5)
    else:
        d = f32(SPOT_TARGET) - f32(SPOT_EYE)
        a[1], a[CASTER] = a[2], SC.L(1, pos=SPOT_EYE, dir=d, color=(1.0, 0.9, 0.6), intensity=40.0, inner=0.9, outer=0.2)
    return a, view_pos


def light_view(kind):
    """the caster's 144-byte view block: `view` and `proj` (the rest is ignored by the pass)"""
    vu = np.zeros((), bbo.VIEW_DTYPE)
    if kind == "ortho":
        d = np.asarray(DIR_ORTHO, np.float64)
        d /= np.sqrt((d * d).sum())
        vu["view"] = bbo.mat_look_at(f32(-ORTHO_DISTANCE * d), f32((0.0, 0.0, 0.0)))
        p = np.zeros((4, 4), np.float32)       # m[col][row]; depth = (FAR - z) / (FAR - NEAR): the nearer, the larger
        p[0][0], p[1][1] = 1.0 / ORTHO_HALF, -1.0 / ORTHO_HALF
        p[2][2], p[3][2], p[3][3] = -1.0 / (FAR - NEAR), FAR / (FAR - NEAR), 1.0
        vu["proj"] = p
    else:
        vu["view"] = bbo.mat_look_at(f32(SPOT_EYE), f32(SPOT_TARGET))
        vu["proj"] = bbo.mat_perspective(SPOT_FOV, 1.0, NEAR, FAR)
    vu["view_pos"] = (123.0, 456.0, 789.0)     # ignored
    vu["enable_normal_map"] = 7                # ignored
    return vu


def scene(kind, size=FRAME_SMALL, caster_type=None, num_lights=None):
    """the camera's frame of `kind`; caster_type replaces the caster's type (the model's SHADOWED pixels: an unknown one)"""
    ls, view_pos = lights(kind)
    if caster_type is not None:
        ls[CASTER] = dict(ls[CASTER], type=int(caster_type))
    if num_lights is not None:
        ls = ls[:num_lights]
    fu, vu = SC.uniforms(ls, view_pos, 1.0, 1)
    return bbo.Scene(fu, vu, list(_draws(kind)), size[0], size[1], f"shadow {kind}")


def map_scene(kind, side):
    """the S x S frame of the same draws from the light: its oracle depth is the map"""
    sc = scene(kind)
    return bbo.Scene(sc.frame, light_view(kind), sc.draws, side, side, f"shadow map {kind} {side}")


@functools.lru_cache(None)
def oracle_map(kind, side):
    """[S, S] float32: bbo.render's depth of the light's frame (uncovered texels: what the oracle returns for them)"""
    depth = bbo.render(map_scene(kind, side), want_prim=False)[2]
    depth.setflags(write=False)
    return depth


def pixel_xy64(size):
    """world x, y of the pixel centres in binary64, [h, w] each"""
    w, h = size
    x = ((np.arange(w) + 0.5) / w * 2.0 - 1.0) * 4.0
    y = -((np.arange(h) + 0.5) / h * 2.0 - 1.0) * 4.0
    return np.broadcast_to(x[None, :], (h, w)), np.broadcast_to(y[:, None], (h, w))


@functools.lru_cache(None)
def positions64(kind, size=FRAME_SMALL):
    """([h, w, 3] binary64 world positions of the camera's pixels, [h, w] bool covered, [h, w] bool receiver): the plane of the
    triangle the oracle picks for the pixel, at the pixel centre's x, y"""
    sc = scene(kind, size)
    prim = bbo.render(sc, want_depth=False)[1]
    tris = []
    for d in sc.draws:
        tris.append(d.vertices["pos"][d.indices.reshape(-1, 3)].astype(np.float64))
    tris = np.concatenate(tris)                                  # [n_prims, 3, 3], in primitive order
    covered = prim != bbo.NO_PRIM
    p = tris[np.where(covered, prim, 0)]                         # [h, w, 3, 3]
    x, y = pixel_xy64(size)
    nrm = np.cross(p[..., 1, :] - p[..., 0, :], p[..., 2, :] - p[..., 0, :])
    z = p[..., 0, 2] - (nrm[..., 0] * (x - p[..., 0, 0]) + nrm[..., 1] * (y - p[..., 0, 1])) / nrm[..., 2]
    P = np.stack([x, y, z], -1)
    P.setflags(write=False)
    return P, covered, covered & (prim < 2)


# ---------------------------------------------------------------------------------------------------------------------
# census
# ---------------------------------------------------------------------------------------------------------------------
MIN_SHARE, MIN_BEHIND, MIN_SELF = 0.05, 64, 64


def clip64(kind, P):
    """M (P, 1) in binary64 for P[..., 3], M the exact product of the light's two matrices: [..., 4]"""
    L = light_view(kind)
    M = L["proj"].astype(np.float64).T @ L["view"].astype(np.float64).T      # (the blocks store m[col][row])
    return np.concatenate([P, np.ones(P.shape[:-1] + (1,))], -1) @ M.T


def census(kind, side, bias, P, covered, depth_map, mask=None, P_surface=None):
    """Binary64 counts on positions P[h, w, 3], each a factor 2 clear of the threshold that decides it; with `mask` (the classes
    somebody computed) a clear pixel must also carry its class.  Returns shares of the covered pixels and counts:
      outside   w <= 0, or the texel coordinate xs or ys at least one texel outside [0, S)
      inside    w > 0 and xs, ys at least one texel inside [0, S); both at least 2^-8 texel away from a texel edge, so that the
                texel is the one binary32 picks
      shadowed  inside, and the map texel lies more than 2 |bias| above the fragment's depth (the threshold is the bias)
      lit       inside, and the map texel lies less than |bias| / 2 above the fragment's depth
      behind    pixels with w <= 0, counted
      self      at bias 0: inside pixels whose map texel is within 2^-20 of their own depth (the receiver's own depth is in
                the map: rounding decides), counted.  Where the test sees a rounded position (the deferred pass), P_surface is
                the surface's own: the map holds ITS depth"""
    c = clip64(kind, np.asarray(P, np.float64))
    S = float(side)
    with np.errstate(all="ignore"):
        w = c[..., 3]
        xs, ys = (c[..., 0] / w * 0.5 + 0.5) * S, (c[..., 1] / w * 0.5 + 0.5) * S
        z = c[..., 2] / w
        out = (w <= 0) | (xs <= -1) | (xs >= S + 1) | (ys <= -1) | (ys >= S + 1)
        edge = lambda a: np.abs(a - np.rint(a)) >= 2.0 ** -8
        inside = (w > 0) & (xs >= 1) & (xs <= S - 1) & (ys >= 1) & (ys <= S - 1) & edge(xs) & edge(ys)
        i = np.clip(np.where(inside, xs, 0).astype(np.int64), 0, side - 1)
        j = np.clip(np.where(inside, ys, 0).astype(np.int64), 0, side - 1)
        gap = depth_map[j, i].astype(np.float64) - z
        own = gap
        if P_surface is not None:
            cs = clip64(kind, np.asarray(P_surface, np.float64))
            own = depth_map[j, i].astype(np.float64) - cs[..., 2] / cs[..., 3]
    shadowed, lit = inside & (gap > 2 * abs(bias)), inside & (gap < abs(bias) / 2)
    if bias == 0:
        shadowed, lit = inside & (gap > 2.0 ** -20), inside & (gap < -2.0 ** -20)
    if mask is not None:
        out, shadowed, lit = out & (mask == 3), shadowed & (mask == 2), lit & (mask == 1)
    n = max(int(covered.sum()), 1)
    share = lambda a: float((a & covered).sum()) / n
    return {"outside": share(out), "shadowed": share(shadowed), "lit": share(lit), "behind": int(((w <= 0) & covered).sum()),
            "self": int((inside & covered & (np.abs(own) <= 2.0 ** -20)).sum())}


def check_census(kind, side, c_bias, c_zero):
    """the minima on a census at bias BIAS and one at bias 0"""
    for k in ("lit", "shadowed", "outside"):
        assert c_bias[k] >= MIN_SHARE, (kind, side, k, c_bias)
    if kind != "ortho":
        assert c_bias["behind"] >= MIN_BEHIND, (kind, side, c_bias)
    assert c_zero["self"] >= MIN_SELF, (kind, side, c_zero)
