"""Scenes for shadow maps of up to six faces (bbr_render_shadow_faces; DESIGN.md section 3, "Faces"), on top of
tests/shadow_scenes.py: its camera (the surface chart's), its tilted receiver, its quads and its light lists.
TEST INFRASTRUCTURE ONLY; no test lives here.

  "cube"     a point light (index CASTER) at E, between the receiver's level and a wall behind it, with the six faces of
             cube_views(E, 96 degrees, 0.125, 16): +X, -X, +Y, -Y, +Z, -Z.
             receiver   the tilted quad on x in [-0.5, 4]; left of it a wall 1.75 nearer to the camera
             occluders  six quads, each 0.4375 or 1.3125 nearer to the camera than the receiver's plane.  Two of them are wound
                        the other way round, ON PURPOSE: the -X and -Z faces look at the scene from the side the camera culls,
                        so the wall and the occluders that face the camera are not in those two maps; occluders wound towards
                        the light are in them -- and are invisible to the camera.  Every face thereby has both lit and shadowed
                        pixels in the camera's frame
  "cascade"  shadow_scenes' "ortho" scene with two nested orthographic faces of half extent 1.5 and 3 that look the same way:
             the inner face decides inside its extent, the outer one only beyond it
"""
from __future__ import annotations

import functools

import numpy as np

import shadow_reference as SR
import shadow_scenes as SS
import surface_chart as SC
from oracle import bbo

KINDS = ("cube", "cascade")
CASTER = SS.CASTER
FRAME_SMALL, FRAME_DUMP = SS.FRAME_SMALL, SS.FRAME_DUMP
SIDES = (33, 64, 200)
BIASES, BIAS = SS.BIASES, SS.BIAS
E = (-0.75, 0.25, SS.receiver_z(-0.75, 0.25) - 0.875)
FOV, NEAR, FAR = 96.0, 0.125, 16.0
CASCADE_HALVES = (1.5, 3.0)
# x0, x1, y0, y1, dz, reversed winding
OCCLUDERS = ((-0.45, -0.2, -0.25, 0.5, 0.4375, False),
             (0.5, 0.59375, -3.0, 3.0, 0.4375, False),
             (-1.25, -0.95, 0.0, 0.5, 1.3125, True),
             (-1.75, -1.55, -0.75, 1.25, 1.3125, True),
             (-1.5, 1.0, 1.0, 1.2, 0.4375, False),
             (-1.5, 1.0, -0.7, -0.5, 0.4375, False))
# the census (the conditions of the tests: caps and minima, not measurements)
MIN_PER_FACE = {FRAME_SMALL: 32, FRAME_DUMP: 100}
MIN_OVERLAP = 500

f32 = SC.f32
CUBE_DIRS = ((1, 0, 0), (-1, 0, 0), (0, 1, 0), (0, -1, 0), (0, 0, 1), (0, 0, -1))
CUBE_UPS = ((0, 1, 0), (0, 1, 0), (0, 0, -1), (0, 0, 1), (0, 1, 0), (0, 1, 0))


def cube_views(pos, fov, near, far):
    """six view blocks at `pos` from the oracle's lookAt and perspective: what bb::cubeShadowViews must give bit for bit"""
    out = np.zeros(6, bbo.VIEW_DTYPE)
    pos = f32(pos)
    for f in range(6):
        out[f]["view"] = bbo.mat_look_at(pos, pos + f32(CUBE_DIRS[f]), f32(CUBE_UPS[f]))
        out[f]["proj"] = bbo.mat_perspective(fov, 1.0, near, far)
        out[f]["view_pos"] = pos
    return out


def faces(kind, fov=FOV):
    """the caster's view blocks, [F] of VIEW_DTYPE"""
    if kind == "cube":
        return cube_views(E, fov, NEAR, FAR)
    out = np.zeros(len(CASCADE_HALVES), bbo.VIEW_DTYPE)
    for f, half in enumerate(CASCADE_HALVES):
        out[f] = SS.light_view("ortho")
        p = out[f]["proj"].copy()
        p[0][0], p[1][1] = 1.0 / half, -1.0 / half
        out[f]["proj"] = p
    return out


@functools.lru_cache(None)
def _draws(kind):
    if kind == "cascade":
        return SS._draws("ortho")
    one = np.zeros(1, bbo.INSTANCE_DTYPE)
    one[0]["model"] = one[0]["inv_model"] = np.eye(4, dtype=np.float32)
    mat = bbo.MaterialData(SC.material("packed", 6))
    recv = np.concatenate([SS._quad(-0.5, 4.0, -4.0, 4.0, 0.0), SS._quad(-4.0, -0.5, -4.0, 4.0, 1.75)])
    ridx = np.concatenate([SC.QUAD_INDEX, SC.QUAD_INDEX + 4]).astype(np.uint32)
    occ, idx = [], []
    for k, (x0, x1, y0, y1, dz, rev) in enumerate(OCCLUDERS):
        occ.append(SS._quad(x0, x1, y0, y1, dz))
        q = SC.QUAD_INDEX.reshape(2, 3)
        idx.append((q[:, ::-1] if rev else q).reshape(-1) + 4 * k)
    return (bbo.DrawData(recv, ridx, one, mat), bbo.DrawData(np.concatenate(occ), np.concatenate(idx).astype(np.uint32), one, mat))


def lights(kind):
    if kind == "cascade":
        return SS.lights("ortho")
    a, view_pos = SS.lights("spot")
    a[CASTER] = SC.L(0, pos=E, color=(1.0, 0.9, 0.6), intensity=12.0)
    return a, view_pos


def scene(kind, size=FRAME_SMALL):
    ls, view_pos = lights(kind)
    fu, vu = SC.uniforms(ls, view_pos, 1.0, 1)
    return bbo.Scene(fu, vu, list(_draws(kind)), size[0], size[1], f"shadow faces {kind}")


@functools.lru_cache(None)
def oracle_maps(kind, side, fov=FOV):
    """[F, S, S] float32: bbo.render's depth of each face's frame"""
    sc = scene(kind)
    maps = np.stack([bbo.render(bbo.Scene(sc.frame, np.array(L), sc.draws, side, side, f"face {f}"), want_prim=False)[2]
                     for f, L in enumerate(faces(kind, fov))])
    maps.setflags(write=False)
    return maps


@functools.lru_cache(None)
def matrices(kind, fov=FOV):
    return tuple(SR.proj_view(L) for L in faces(kind, fov))


@functools.lru_cache(None)
def positions64(kind, size=FRAME_SMALL):
    """([h, w, 3] binary64 world positions of the camera's pixels, [h, w] bool covered): the plane of the triangle the oracle
    picks for the pixel, at the pixel centre's x, y (shadow_scenes.positions64, for these scenes)"""
    sc = scene(kind, size)
    prim = bbo.render(sc, want_depth=False)[1]
    tris = np.concatenate([d.vertices["pos"][d.indices.reshape(-1, 3)].astype(np.float64) for d in sc.draws])
    covered = prim != bbo.NO_PRIM
    p = tris[np.where(covered, prim, 0)]
    x, y = SS.pixel_xy64(size)
    nrm = np.cross(p[..., 1, :] - p[..., 0, :], p[..., 2, :] - p[..., 0, :])
    z = p[..., 0, 2] - (nrm[..., 0] * (x - p[..., 0, 0]) + nrm[..., 1] * (y - p[..., 0, 1])) / nrm[..., 2]
    P = np.stack([x, y, z], -1)
    P.setflags(write=False)
    return P, covered


def census(mask, face, covered, n_faces):
    """what a mask and a face index hold: LIT and SHADOWED covered pixels per deciding face, covered pixels OUTSIDE everywhere"""
    mask, face = np.asarray(mask), np.asarray(face)
    return {"lit": [int(((mask == SR.LIT) & (face == f) & covered).sum()) for f in range(n_faces)],
            "shadowed": [int(((mask == SR.SHADOWED) & (face == f) & covered).sum()) for f in range(n_faces)],
            "outside": int(((mask == SR.OUTSIDE) & covered).sum())}


def check_census(c, size, what=""):
    """the cube scene's minima at 96 degrees"""
    least = MIN_PER_FACE[tuple(size)]
    assert min(c["lit"]) >= least and min(c["shadowed"]) >= least, (what, size, c)
    assert c["outside"] == 0, (what, size, c)
