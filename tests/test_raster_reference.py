"""The oracle's fixed-function triangle stage (clip, snap, cull, coverage, depth, perspective-correct varyings) against
tests/raster_reference.py, an exact rasteriser written from the Vulkan model and not from bb_oracle.c.

Margin layer: on every pixel the reference can decide (no primitive within the position uncertainty delta of an edge, the
winner ahead of every rival by more than both depth tolerances) the oracle's primitive id is the reference's, its depth
and its vUV lie within the derived tolerances (raster_reference's docstring: C_POS = 3, K_DEPTH = 4, K_VARY = 24), and at
most 1 % of a frame is undecided.
Exact layer: scenes whose snapping, planes and varyings are exact in binary32 (w = 1 or w in {1, 2, 4}, power-of-two
extents, vertices on the 1/256 grid): coverage with every tie, n_fragments, depth bits, equal-depth winners, vUV bits,
against integers evaluated here with the top-left rule as the Vulkan specification words it.

Measured (recorded in tests/golden/raster_reference.json by `python tests/test_raster_reference.py --write`): worst
depth error / tolerance, vUV error / tolerance and undecided share per scene."""
import json
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
if __name__ == "__main__":   # run as a script (--write): what tests/conftest.py does for pytest
    sys.path.insert(0, os.path.dirname(HERE))

from oracle import bbo, scenes
import raster_reference as RR

RECORD = os.path.join(HERE, "golden", "raster_reference.json")


# ---------------------------------------------------------------------------------------------------------------------
# scenes
# ---------------------------------------------------------------------------------------------------------------------

def _identity_instance():
    inst = np.zeros(1, bbo.INSTANCE_DTYPE)
    inst[0]["model"] = inst[0]["inv_model"] = np.eye(4, dtype=np.float32)
    return inst


def _scene_of(pos, uv, vu, W, H, name):
    v = np.zeros(len(pos), bbo.VERTEX_DTYPE)
    v["pos"], v["uv"] = pos, uv
    v["normal"], v["tangent"] = (0, 0, -1), (1, 0, 0)
    return bbo.Scene(scenes.frame_uniforms([]), vu, [bbo.DrawData(v, None, _identity_instance(), bbo.MaterialData())], W, H, name)


def soup_scene(W, H, seed, n=240, near=0.02):
    """seeded triangle soup: ordinary triangles, slivers, sub-pixel triangles, triangles 6x the view, vertices behind the
    camera, triangles across the far plane; identity view (so the forward and the deferred vertex stage compute the same clip coordinates), near plane 0.02"""
    rng = np.random.default_rng(seed)
    vu = scenes.view_uniforms((0, 0, 0), 0.0, 0.0, W, H, 0, near=near, far=100.0)
    assert np.array_equal(np.abs(vu["view"]), np.eye(4, dtype=np.float32))
    px, py = float(vu["proj"][0, 0]), float(vu["proj"][1, 1])

    def at(nx, ny, z):  # view-space point that lands on NDC (nx, ny) at view depth z
        return (nx * z / px, ny * z / py, z)

    pos = []
    for t in range(n):
        kind = t % 6
        c = rng.uniform(-1, 1, 2)
        zs = rng.uniform(0.5, 6.0) * rng.uniform(0.8, 1.25, 3)
        if kind == 0:    # ordinary
            r = rng.uniform(0.03, 0.6)
            ang = np.sort(rng.uniform(0, 2 * np.pi, 3))[::rng.choice([-1, 1])]
            tri = [at(c[0] + r * np.cos(a), c[1] + r * np.sin(a), z) for a, z in zip(ang, zs)]
        elif kind == 1:  # sliver: third vertex almost on the long edge (0 .. 2 pixels off)
            d = rng.uniform(-1.5, 1.5, 2)
            s = rng.uniform(-0.2, 1.2)
            off = rng.uniform(-2, 2) * np.array([-d[1], d[0]]) / np.hypot(*d) * (2.0 / min(W, H))
            pts = [c, c + d, c + s * d + off]
            tri = [at(p[0], p[1], z) for p, z in zip(pts, zs)]
        elif kind == 2:  # sub-pixel
            pts = [c + rng.uniform(-1.5, 1.5, 2) * np.array([2.0 / W, 2.0 / H]) for _ in range(3)]
            tri = [at(p[0], p[1], z) for p, z in zip(pts, zs)]
        elif kind == 3:  # 6x the view
            ang = np.sort(rng.uniform(0, 2 * np.pi, 3))[::rng.choice([-1, 1])]
            tri = [at(c[0] + 6 * np.cos(a), c[1] + 6 * np.sin(a), z) for a, z in zip(ang, zs * 5)]   # (behind most of the rest)
        elif kind == 4:  # vertices behind the camera / inside the near plane
            tri = [(rng.uniform(-0.5, 0.5), rng.uniform(-0.5, 0.5), rng.uniform(-0.5, 2.5)) for _ in range(3)]
        else:            # across the far plane (view depth 100)
            r = rng.uniform(0.2, 1.0)
            ang = np.sort(rng.uniform(0, 2 * np.pi, 3))[::rng.choice([-1, 1])]
            tri = [at(c[0] + r * np.cos(a), c[1] + r * np.sin(a), z) for a, z in zip(ang, rng.uniform(40.0, 300.0, 3))]
        pos += tri
    uv = rng.uniform(-2, 2, (3 * n, 2))
    return _scene_of(np.array(pos, np.float32), uv.astype(np.float32), vu, W, H, f"soup{seed}@{W}x{H}")


def single_primitive_scene(scene, p):
    d = scene.draws[0]
    v = d.vertices[3 * p: 3 * p + 3].copy()
    return bbo.Scene(scene.frame, scene.view, [bbo.DrawData(v, None, d.instances, d.material)], scene.width, scene.height,
                     f"{scene.name}#{p}")


def hostile_finite_input(seed):
    from test_gpu_parity import hostile_scene
    return hostile_scene(seed=seed)


def ball_scene(which, W, H, thin=1):
    """C2 / C3 ShaderBall scene (and C3 with the camera inside the lattice); `thin` keeps every thin-th triangle of the ball"""
    from bibim_renderer_amd import configs
    cfg = {"c2": configs.C2, "c3": configs.C3, "inside": configs.C3}[which].scaled(W, H, 64)
    ball = scenes.load_shaderball_vertices()
    if thin > 1:
        ball = np.ascontiguousarray(ball.reshape(-1, 3)[::thin].reshape(-1))
    sc = scenes.shaderball_scene(cfg, bbo.MaterialData(), ball)
    if which == "inside":
        sc.view = scenes.view_uniforms((-1.0, -0.55, 1.6), 35.0, -5.0, W, H, 1, near=0.05)
    return sc


# seeds 1..4 were tried at every size: on the reference alone each of the twenty frames stays under the 1 % cap (0.013 % ..
# 0.46 % undecided); kept are seeds that leave many different primitives visible (17 .. 75 distinct winners)
SOUPS = [(333, 207, 1), (416, 240, 2), (1001, 77, 3), (16384, 33, 3), (31, 4096, 4)]
MARGIN_SCENES = {f"soup {w}x{h}": (lambda w=w, h=h, s=s: soup_scene(w, h, s)) for w, h, s in SOUPS}
MARGIN_SCENES.update({f"hostile seed {s}": (lambda s=s: hostile_finite_input(s)) for s in (0, 1)})
MARGIN_SCENES.update({"C2 ball 320x180": lambda: ball_scene("c2", 320, 180),
                      "C3 balls 480x270": lambda: ball_scene("c3", 480, 270, thin=4),
                      "camera inside 256x144": lambda: ball_scene("inside", 256, 144, thin=4)})

_measured = {}


def margin_check(name, scene, prim, depth, stats, uv_image=None):
    """the shared assertions of the margin layer (the GPU file calls this with the kernels' outputs)"""
    res = reference_of(name, scene)
    rep = _measured.setdefault(name, {})
    RR.check_visibility(res, prim, depth, rep)
    if uv_image is not None:
        RR.check_uv(res, uv_image, rep)
    RR.check_stats(res, stats)
    return res


_cache = {}


def reference_of(name, scene):
    if name not in _cache:
        _cache[name] = RR.rasterise(scene)
    return _cache[name]


@pytest.mark.parametrize("name", list(MARGIN_SCENES))
def test_margin_layer_oracle(name):
    sc = MARGIN_SCENES[name]()
    _, prim, depth, st = bbo.render(sc)
    uv, _, _, _ = bbo.render(sc, flags=bbo.FLAG_OUTPUT_UV)
    res = margin_check(name, sc, prim, depth, st, uv)
    assert (res.winner != RR.NONE).sum() > 0.02 * prim.size, "the scene must put geometry on the screen"


def test_clipped_primitives_alone_cover_every_pixel_once():
    """each clipped primitive of one soup on its own: the interior edges of the clip fan hit no pixel twice
    (n_fragments == covered pixels) and miss none the reference surely covers"""
    sc = soup_scene(416, 240, 2)
    clip, _ = RR.scene_primitives(sc)
    clipped = np.nonzero(~RR.all_in(clip))[0].tolist()
    seen = 0
    for p in clipped:
        one = single_primitive_scene(sc, p)
        _, prim, depth, st = bbo.render(one)
        covered = prim != bbo.NO_PRIM
        assert st["n_fragments"] == covered.sum(), (p, st)
        res = RR.rasterise(one, want_uv=False)
        sure = res.winner == 0
        assert covered[sure].all(), f"primitive {p}: {int((sure & ~covered).sum())} surely covered pixels missed"
        RR.check_visibility(res, prim, depth)
        seen += bool(sure.any())
    assert seen >= 8, seen


# ---------------------------------------------------------------------------------------------------------------------
# exact layer
# ---------------------------------------------------------------------------------------------------------------------

EW = EH = 64   # power-of-two extents: the viewport transform is exact


def exact_view(perspective):
    """identity view + a hand-written projection (the ABI takes the matrix bytes as they are), M[column][row].
    w = 1:        clip = (2 x / W - 1, 2 y / H - 1, z, 1) for a vertex position (x, y, z) = (framebuffer x, y, depth)
    perspective:  position (x w, y w, w):  clip = ((2 x / W - 1) w, (2 y / H - 1) w, 1/2, w), depth = 1 / (2 w)"""
    vu = np.zeros((), bbo.VIEW_DTYPE)
    vu["view"] = np.eye(4, dtype=np.float32)
    P = np.zeros((4, 4), np.float32)
    P[0, 0], P[1, 1] = 2.0 / EW, 2.0 / EH
    if perspective:
        P[2, 0], P[2, 1], P[2, 3], P[3, 2] = -1.0, -1.0, 1.0, 0.5
    else:
        P[3, 0], P[3, 1], P[2, 2], P[3, 3] = -1.0, -1.0, 1.0, 1.0
    vu["proj"] = P
    return vu


def exact_triangles():
    """[n, 3, 2] integer vertex coordinates in 1/256 pixel"""
    rng = np.random.default_rng(11)
    c = lambda x, y: (int(x * 256), int(y * 256))
    T = []
    # edges through rows, columns and diagonals of pixel centres; horizontal top / bottom, vertical left / right edges
    T += [[c(4.5, 4.5), c(24.5, 4.5), c(24.5, 24.5)], [c(4.5, 4.5), c(24.5, 24.5), c(4.5, 24.5)],   # a quad split on its diagonal
          [c(30.5, 2.5), c(50.5, 2.5), c(40.5, 12.5)], [c(30.5, 20.5), c(40.5, 10.5), c(50.5, 20.5)],  # flat top / flat bottom
          [c(2.5, 30.5), c(12.5, 40.5), c(2.5, 50.5)], [c(20.5, 30.5), c(20.5, 50.5), c(10.5, 40.5)],  # vertical left / right edge
          [c(40.5, 30.5), c(60.5, 30.5), c(60.5, 50.5)], [c(40.5, 30.5), c(60.5, 50.5), c(40.5, 50.5)],
          [c(40.5, 30.5), c(60.5, 30.5), c(60.5, 50.5)]]                                                # the same again: a depth tie
    # a fan around a vertex on a pixel centre, rim vertices on and off centres, clockwise in y-down space
    rim = [c(32.5 + 20 * np.cos(a), 32.5 + 20 * np.sin(a)) for a in np.linspace(0, 2 * np.pi, 13)[:-1]]
    rim[3], rim[6], rim[9] = c(32.5, 52.5), c(12.5, 32.5), c(32.5, 12.5)
    T += [[c(32.5, 32.5), rim[i], rim[(i + 1) % 12]] for i in range(12)]
    # zero area and back-facing
    T += [[c(5.5, 5.5), c(10.5, 10.5), c(15.5, 15.5)], [c(5.5, 5.5), c(5.5, 5.5), c(9.5, 30.5)],
          [c(4.5, 4.5), c(24.5, 24.5), c(24.5, 4.5)]]
    # random: vertices on centres, on the 1/256 grid, both windings, some outside the frame
    for _ in range(60):
        on_centre = rng.random(3) < 0.5
        p = rng.integers(-8 * 256, (EW + 8) * 256, (3, 2))
        p = np.where(on_centre[:, None], (p // 256) * 256 + 128, p)
        T.append([tuple(int(v) for v in q) for q in p])
    return np.array(T, np.int64)


def is_top_or_left(a, b, c):
    """Vulkan / D3D wording of the fill rule, y down: a TOP edge is exactly horizontal with the third vertex below it; a LEFT
    edge is not horizontal and has the triangle's interior to its right"""
    if a[1] == b[1]:
        return c[1] > a[1]
    # x of the edge's line at the third vertex's height, compared with the third vertex (exact, cross-multiplied)
    side = (c[0] - a[0]) * (b[1] - a[1]) - (b[0] - a[0]) * (c[1] - a[1])
    return side * (1 if b[1] > a[1] else -1) > 0


def exact_coverage(tri):
    """bool [EH, EW]: pixel centres covered by the front-facing (clockwise, y down) triangle, ties by the top-left rule"""
    a = tri
    area2 = sum(int(a[i][0]) * int(a[(i + 1) % 3][1]) - int(a[(i + 1) % 3][0]) * int(a[i][1]) for i in range(3))
    if area2 <= 0:   # Vulkan: area = -1/2 sum(...); CLOCKWISE front face = negative area; zero area covers nothing
        return np.zeros((EH, EW), bool)
    X, Y = np.meshgrid(np.arange(EW, dtype=np.int64) * 256 + 128, np.arange(EH, dtype=np.int64) * 256 + 128)
    inside = np.ones((EH, EW), bool)
    for i in range(3):
        p, q, r = (tuple(int(v) for v in a[(i + k) % 3]) for k in range(3))
        s = (q[0] - p[0]) * (Y - p[1]) - (q[1] - p[1]) * (X - p[0])
        s_r = (q[0] - p[0]) * (r[1] - p[1]) - (q[1] - p[1]) * (r[0] - p[0])
        same_side = s * (1 if s_r > 0 else -1) > 0
        inside &= same_side | ((s == 0) & is_top_or_left(p, q, r))
    return inside


def exact_scene(perspective):
    """scene + per-triangle (vertices, depth plane, uv plane) in exact dyadic numbers"""
    T = exact_triangles()
    n = len(T)
    rng = np.random.default_rng(12)
    x, y = T[..., 0] / 256.0, T[..., 1] / 256.0
    if perspective:
        # w in {1, 2, 4} at columns 0, 32, 48: depth = 1 / (2 w) = 1/2 - x / 128 is linear on the screen; vertices sit on those columns
        # (every x is replaced by one of the three columns, so the hand-built shapes of the w = 1 scene -- fan, diagonals, flat
        # tops -- mostly collapse here; what this scene adds is coverage and depth bits of triangles whose vertices differ in w,
        # with rows of centres on their edges.  vUV bits are asserted on the w = 1 layout only: with w != 1 the contract's
        # rcp of the interpolated 1/w is not exact.)
        cols = np.array([0.0, 32.0, 48.0]); ws = np.array([1.0, 2.0, 4.0])
        k = rng.integers(0, 3, (n, 3))
        x = cols[k]
        T = T.copy(); T[..., 0] = (x * 256).astype(np.int64)
        w = ws[k]
        pos = np.stack([x * w, y * w, w], -1)
        plane = np.tile([0.5, -1.0 / 128, 0.0], (n, 1))
    else:
        # depth = o + s (x / 256 + y / 512): dyadic, exact in binary32 at every pixel centre; o = 0 and o = 1 flat: the clamp's ends
        o = rng.integers(0, 5, n) / 8.0
        s = rng.integers(0, 2, n).astype(np.float64)
        o[9:21] = 0.25; s[9:21] = 1.0          # the fan shares one plane
        o[7], s[7], o[8], s[8] = o[6], s[6], o[6], s[6]   # equal depth: API order decides
        o[0], s[0], o[2], s[2] = 1.0, 0.0, 0.0, 0.0       # flat on the near plane / flat on the cleared value
        plane = np.stack([o, s / 256, s / 512], -1)
        pos = np.stack([x, y, plane[:, :1] + plane[:, 1:2] * x + plane[:, 2:3] * y], -1)
    uv = np.stack([x / 64, y / 64 + x / 128], -1)
    sc = _scene_of(pos.reshape(-1, 3).astype(np.float32), uv.reshape(-1, 2).astype(np.float32), exact_view(perspective), EW, EH,
                   "exact perspective" if perspective else "exact w=1")
    assert np.array_equal(sc.draws[0].vertices["pos"].astype(np.float64), pos.reshape(-1, 3))
    return sc, T, plane


def exact_expectation(T, plane):
    prim = np.full((EH, EW), bbo.NO_PRIM, np.int64)
    depth = np.zeros((EH, EW))
    X, Y = np.meshgrid(np.arange(EW) + 0.5, np.arange(EH) + 0.5)
    n_fragments = 0
    for t in range(len(T)):
        cov = exact_coverage(T[t])
        n_fragments += int(cov.sum())
        z = np.clip(plane[t, 0] + plane[t, 1] * X + plane[t, 2] * Y, 0.0, 1.0)
        win = cov & (z >= depth)   # GREATER_OR_EQUAL on a buffer cleared to 0, API order
        prim[win], depth[win] = t, z[win]
    return prim, depth, n_fragments


def exact_check(perspective, prim, depth, stats):
    """bit for bit: coverage with every tie, the winners, the depth bits, n_fragments (the GPU file calls this too)"""
    _, T, plane = exact_scene(perspective)
    want_prim, want_depth, n_fragments = exact_expectation(T, plane)
    assert np.array_equal(want_depth.astype(np.float32).astype(np.float64), want_depth), "the expectation itself must be binary32"
    bad = prim.astype(np.int64) != want_prim
    assert not bad.any(), f"{int(bad.sum())} pixels differ, first (y, x) = {tuple(np.argwhere(bad)[0])}"
    assert np.array_equal(depth.view(np.uint32), want_depth.astype(np.float32).view(np.uint32))
    assert stats["n_shaded"] == int((want_prim != bbo.NO_PRIM).sum())
    if "n_fragments" in stats:   # (the oracle counts them; the C ABI's statistics do not)
        assert stats["n_fragments"] == n_fragments
    return want_prim


@pytest.mark.parametrize("perspective", [False, True], ids=["w=1", "w in 1,2,4"])
def test_exact_layer_oracle(perspective):
    sc, T, plane = exact_scene(perspective)
    _, prim, depth, st = bbo.render(sc)
    want = exact_check(perspective, prim, depth, st)
    covered = want != bbo.NO_PRIM
    assert covered.sum() > 1000 and len(np.unique(want[covered])) > (10 if perspective else 30)  # (one shared plane: all ties)
    if not perspective:
        assert (depth == 1.0).any() and ((depth == 0.0) & covered).any()       # both ends of the clamp are on the screen
        assert (want == 8).any() and not (want == 6).any()   # triangle 8 repeats triangle 6 at the same depth: the later one wins


def fan_scene():
    """triangles 9 .. 20 of the exact scene on their own + how often each pixel centre is covered by the integer rule"""
    sc, T, _ = exact_scene(False)
    d = sc.draws[0]
    fan = bbo.Scene(sc.frame, sc.view, [bbo.DrawData(d.vertices[27:63].copy(), None, d.instances, d.material)], EW, EH)
    return fan, sum(exact_coverage(T[t]).astype(int) for t in range(9, 21))


def test_exact_layer_fan_covers_every_pixel_once():
    """the real fan: twelve triangles around a vertex on a pixel centre, rim vertices on centres too -- the pixels inside
    are hit exactly once, spokes through rows, columns and diagonals of centres included"""
    fan, once = fan_scene()
    _, prim, _, st = bbo.render(fan)
    assert once.max() == 1 and once[32, 32] == 1 and once.sum() > 900
    assert np.array_equal(prim != bbo.NO_PRIM, once == 1) and st["n_fragments"] == once.sum()


def exact_uv_scene():
    """axis-aligned right triangles with power-of-two legs, vertices 3/256 off the centres: the doubled area is a power of two,
    so the binary32 barycentric planes and their sum are exact, and with vertex vUV of a few bits so are the products of the
    interpolation.  Per rectangle (x0, y0, lx, ly): vUV = (1/4 + (x - x0) / lx, 1/2 + 3/2 (y - y0) / ly).
    Returns the scene, the triangles (1/256 pixel) and per triangle the rectangle it belongs to."""
    T, R = [], []
    for (x0, y0, lx, ly) in ((2, 3, 16, 8), (20, 1, 32, 32), (5, 30, 8, 16), (30, 40, 16, 16), (1, 50, 4, 8)):
        a, b, c = (x0 * 256 + 131, y0 * 256 + 125), ((x0 + lx) * 256 + 131, y0 * 256 + 125), ((x0 + lx) * 256 + 131, (y0 + ly) * 256 + 125)
        d = (x0 * 256 + 131, (y0 + ly) * 256 + 125)
        T += [[a, b, c], [a, c, d]]
        R += [(a[0] / 256.0, a[1] / 256.0, lx, ly)] * 2
    T = np.array(T, np.int64)
    x, y = T[..., 0] / 256.0, T[..., 1] / 256.0
    r = np.array(R)[:, None, :]
    pos = np.stack([x, y, np.full(x.shape, 0.5)], -1)
    uv = np.stack([0.25 + (x - r[..., 0]) / r[..., 2], 0.5 + 1.5 * (y - r[..., 1]) / r[..., 3]], -1)
    return _scene_of(pos.reshape(-1, 3).astype(np.float32), uv.reshape(-1, 2).astype(np.float32), exact_view(False), EW, EH, "exact uv"), T, R


def test_exact_layer_vuv_bits():
    sc, T, R = exact_uv_scene()
    uv, prim, _, _ = bbo.render(sc, flags=bbo.FLAG_OUTPUT_UV)
    X, Y = np.meshgrid(np.arange(EW) + 0.5, np.arange(EH) + 0.5)
    seen = np.zeros((EH, EW), bool)
    for t, (xa, ya, lx, ly) in zip(T, R):
        cov = exact_coverage(t)
        assert not (seen & cov).any() and cov.sum() > 10
        seen |= cov
        want = np.stack([0.25 + (X - xa) / lx, 0.5 + 1.5 * (Y - ya) / ly], -1)
        assert np.array_equal(want.astype(np.float32).astype(np.float64), want)
        assert np.array_equal(uv[cov][:, :2].view(np.uint32), want.astype(np.float32)[cov].view(np.uint32))
    assert np.array_equal(prim != bbo.NO_PRIM, seen) and seen.sum() > 1000


def clamp_scene():
    """64 triangles whose horizontal top edge runs through pixel centres at depth exactly 1 (even ones) or 0 (odd ones); vertex 0,
    which anchors the binary32 plane, is the third one, at a depth that makes the slope non-dyadic"""
    pos = []
    for i in range(64):
        x0, y0 = 0.5 + (i % 8) * 8, 0.5 + (i // 8) * 8
        end = 1.0 if i % 2 == 0 else 0.0
        other = 0.05 + (i * 37 % 97) / 97.0 * 0.9
        pos += [(x0, y0 + 7, other), (x0, y0, end), (x0 + 7, y0, end)]
    return _scene_of(np.array(pos, np.float32), np.zeros((len(pos), 2), np.float32), exact_view(False), EW, EH, "clamp")


def clamp_check(prim, depth, stats):
    assert stats["n_raster_tris"] == 64 and (depth <= 1.0).all() and (depth >= 0.0).all()
    for i in range(64):
        y, x = (i // 8) * 8, (i % 8) * 8
        edge = depth[y, x:x + 7].astype(np.float64)
        assert (prim[y, x:x + 7] == i).all() and (np.abs(edge - (1.0 if i % 2 == 0 else 0.0)) <= 2.0 ** -21).all(), (i, edge)


def test_depth_stays_inside_the_clamp_on_planes_that_round():
    """triangles that touch depth 1 and depth 0 along a row of pixel centres, evaluated from a vertex 7 rows away with slopes
    that are not dyadic: whatever the binary32 plane rounds to there, the stored depth is inside [0, 1] (and within the
    rounding of three operations on values <= 1 of the end it touches)"""
    sc = clamp_scene()
    _, prim, depth, st = bbo.render(sc)
    clamp_check(prim, depth, st)


def contract_depth(X, Y, z, Xc, Yc):
    """DESIGN section 2's arithmetic contract for the depth of a (sub-)triangle at a pixel centre, WITHOUT the clamp: 24.8
    integer coordinates X, Y, binary32 vertex depths z; slopes set up once in binary64 and rounded once; the plane is
    evaluated relative to vertex 0 as fmaf(dzdx, dx, fmaf(dzdy, dy, z0)).  binary32 throughout (tbn_reference.fmaf)."""
    from tbn_reference import fmaf
    f = np.float32
    dx1, dy1, dx2, dy2 = int(X[1] - X[0]), int(Y[1] - Y[0]), int(X[2] - X[0]), int(Y[2] - Y[0])
    S = dx1 * dy2 - dx2 * dy1
    rS = 1.0 / float(S)
    dz1, dz2 = float(f(z[1])) - float(f(z[0])), float(f(z[2])) - float(f(z[0]))
    dzdx = f((dz1 * float(dy2) - dz2 * float(dy1)) * rS)
    dzdy = f((dz2 * float(dx1) - dz1 * float(dx2)) * rS)
    return float(fmaf(dzdx, f(Xc - X[0]), fmaf(dzdy, f(Yc - Y[0]), f(z[0]))))


def clamp_overshoot_scene():
    """64 triangles (vertex 0 below, vertex 1 the top-left corner ON a pixel centre, vertex 2 to its right on the same row)
    whose vertex 1 lies at depth exactly 1 (even cells) or 0 (odd cells), picked by a seeded search so that the contract's
    UNCLAMPED binary32 plane, anchored at vertex 0, comes out above 1 (below 0) at vertex 1's pixel: only the clamp puts
    1.0 (0.0) there.  Returns the scene and the unclamped model value per triangle."""
    rng = np.random.default_rng(21)
    pos, model = [], []
    while len(model) < 64:
        i = len(model)
        end = 1.0 if i % 2 == 0 else 0.0
        x1, y1 = 0.5 + (i % 8) * 8, 0.5 + (i // 8) * 8
        a, b, c = rng.integers(2, 8), rng.integers(2, 8), rng.integers(1, 7) + rng.integers(0, 256) / 256.0
        c = min(c, a - 1 / 256.0)
        z0, z2 = np.float32(rng.uniform(0.02, 0.98)), np.float32(rng.uniform(0.02, 0.98))
        v = [(x1 + c, y1 + b, z0), (x1, y1, np.float32(end)), (x1 + a, y1, z2)]
        X = [int(round(q[0] * 256)) for q in v]; Y = [int(round(q[1] * 256)) for q in v]
        m = contract_depth(X, Y, [q[2] for q in v], X[1], Y[1])
        if (m > 1.0) if end == 1.0 else (m < 0.0):
            pos += v; model.append(m)
    return _scene_of(np.array(pos, np.float32), np.zeros((len(pos), 2), np.float32), exact_view(False), EW, EH, "clamp overshoot"), model


def clamp_overshoot_check(prim, depth, model):
    """not vacuous: the unclamped contract value is outside [0, 1] at every one of the 64 pixels; stored: the end itself, bit for bit"""
    assert all((m > 1.0) if i % 2 == 0 else (m < 0.0) for i, m in enumerate(model))
    for i in range(64):
        y, x = (i // 8) * 8, (i % 8) * 8
        want = np.float32(1.0 if i % 2 == 0 else 0.0)
        assert prim[y, x] == i, (i, prim[y, x])
        assert depth[y, x].view(np.uint32) == want.view(np.uint32), (i, float(depth[y, x]), model[i])


def test_depth_clamp_holds_where_the_binary32_plane_overshoots():
    """both halves of the clamp, each on 32 pixels where the contract's plane evaluation provably leaves [0, 1]"""
    sc, model = clamp_overshoot_scene()
    _, prim, depth, st = bbo.render(sc)
    assert st["n_raster_tris"] == 64
    clamp_overshoot_check(prim, depth, model)


# ---------------------------------------------------------------------------------------------------------------------
# recorded results (informative; the tests assert the derived bounds, not these numbers)
# ---------------------------------------------------------------------------------------------------------------------

def _write_record():
    for name in MARGIN_SCENES:
        test_margin_layer_oracle(name)
        print(name, _measured[name], flush=True)
    out = {"constants": {"C_POS": RR.C_POS, "K_DEPTH": RR.K_DEPTH, "K_VARY": RR.K_VARY, "max_undecided_share": RR.MAX_UNDECIDED},
           "oracle": {k: {m: float(f"{v:.4g}") for m, v in r.items()} for k, r in _measured.items()}}
    with open(RECORD, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")


if __name__ == "__main__":
    if "--write" in sys.argv:
        _write_record()
