"""Surface charts: 128 x 128 frames whose pixels are a CHOSEN population of surface points for the light loop
(`light_surface` in csrc/bb_kernels.hip.h; oracle `light_surface_contract`).  TEST INFRASTRUCTURE ONLY.

The camera is `view` = identity with an orthographic `proj` (w = 1): world x, y in [-4, 4] s fill the frame (y flipped
like mat_perspective), z in [-2, 2] s maps into depth (0.25, 0.75); s is a power of two, so every matrix entry is exact.
`view_pos` is free (the shader takes it from the uniform block, not from the matrix), the model matrix is the identity
and s sits in the vertex positions.  Hence the fragment stage is handed P = any point of the box, a normal and an
8-bit material that the chart chooses, and lights / view position can be put anywhere -- on the surface itself included.

  charts      fine     32 x 32 quads of 4 x 4 pixels, own random z per corner, one random unnormalised normal per quad,
                       one texel per pixel of 128^2 maps, EnableNormalMap = 0: a wave's fragments come from 8 triangles
              coarse   ONE tilted quad over the whole frame, EnableNormalMap = 1 with random normal texels: full tiles,
                       waves of one triangle
              clipped  the coarse quad extended past the guard band and the far plane: through the clipper
              mixed    fine with maps of three sizes (one not a power of two) and no metallic map
              peak     fine with every quad's normal pointing at a far viewer and roughness texels 1..3 (set i only)
  light sets  functions below returning (list of light dicts, view_pos); dicts as tests/test_oracle_contract.py's
              glsl_f64_light_loop takes them, `uniforms()` turns them into the blocks
  census      binary64 counts on the surface values a frame was shaded from, a factor 2 clear of each threshold
"""
from __future__ import annotations

import numpy as np

from oracle import bbo, scenes

W = H = 128
N_PIX = W * H
CHARTS = ("fine", "coarse", "clipped", "mixed")
SEEDS = {"fine": 5, "coarse": 6, "clipped": 6, "mixed": 7, "material": 31}
UNKNOWN = 5          # a light type the GLSL has no branch for
f32 = lambda a: np.asarray(a, np.float32)


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def equal_but_for_nan_payload(got, want):
    """NaN in the same places, every other value bit-equal (+-inf and the sign of zero included).  x86 and the GPU produce
    different default NaNs, so a NaN's sign and payload are not part of the contract."""
    got, want = np.ascontiguousarray(got, np.float32), np.ascontiguousarray(want, np.float32)
    if got.shape != want.shape:
        return False
    ng, nw = np.isnan(got), np.isnan(want)
    return bool(np.array_equal(ng, nw) and np.array_equal(bits(got)[~nw], bits(want)[~nw]))


# ---------------------------------------------------------------------------------------------------------------------
# camera
# ---------------------------------------------------------------------------------------------------------------------
def ortho_view(s, view_pos, enable_normal_map):
    vu = np.zeros((), bbo.VIEW_DTYPE)
    vu["view"] = np.eye(4, dtype=np.float32)
    p = np.zeros((4, 4), np.float32)           # m[col][row]
    p[0][0], p[1][1], p[2][2], p[3][2], p[3][3] = 0.25 / s, -0.25 / s, 0.125 / s, 0.5, 1.0
    vu["proj"] = p
    vu["view_pos"] = view_pos
    vu["enable_normal_map"] = enable_normal_map
    return vu


def pixel_xy(s=1.0):
    """world x, y of the pixel centres, [H, W] each (exact in binary32 for s a power of two)"""
    c = (np.arange(W) + 0.5) / W * 8.0 - 4.0
    x = np.broadcast_to(c[None, :] * s, (H, W))
    y = np.broadcast_to(-c[:, None] * s, (H, W))    # proj[1][1] < 0: row 0 is y = +4 s ... see test_chart_orientation
    return x, y


# ---------------------------------------------------------------------------------------------------------------------
# materials
# ---------------------------------------------------------------------------------------------------------------------
def _texels(rng, shape, channels=(0,)):
    """random 8-bit texels; 0 and 255 forced on a scattered sixteenth, an independent pattern per call"""
    t = rng.integers(0, 256, shape + (4,), dtype=np.uint8)
    forced = rng.random(shape) < 1.0 / 16.0
    value = np.where(rng.random(shape) < 0.5, 0, 255).astype(np.uint8)
    for c in channels:
        t[..., c] = np.where(forced, value, t[..., c])
    return t


def material(kind="packed", min_roughness=0):
    """kind 'packed': five 128^2 maps; 'mixed': three sizes, one not a power of two, no metallic map (default: 0)"""
    rng = np.random.Generator(np.random.PCG64(SEEDS["material"]))
    maps = {"albedo": _texels(rng, (128, 128), (0, 1, 2)), "metallic": _texels(rng, (128, 128)),
            "roughness": _texels(rng, (128, 128)), "ao": _texels(rng, (128, 128)),
            "normal": rng.integers(0, 256, (128, 128, 4), dtype=np.uint8)}
    if kind == "mixed":
        del maps["metallic"]
        maps["ao"] = _texels(rng, (48, 80))
        maps["normal"] = rng.integers(0, 256, (64, 64, 4), dtype=np.uint8)
        maps["height"] = rng.integers(0, 256, (64, 64, 4), dtype=np.uint8)
    if min_roughness:
        maps["roughness"] = np.maximum(maps["roughness"], np.uint8(min_roughness))
    return maps


# ---------------------------------------------------------------------------------------------------------------------
# geometry
# ---------------------------------------------------------------------------------------------------------------------
QUAD_INDEX = np.array([0, 1, 2, 2, 3, 0], np.uint32)     # _wall_scene's order: front-facing under this camera
TILT = (0.3125, 0.1875)                                   # coarse: z = 0.3125 x + 0.1875 y, |z| <= 2 s on the frame


def _fine_mesh(seed, s):
    rng = np.random.Generator(np.random.PCG64(seed))
    n = 32
    v = np.zeros((n, n, 4), bbo.VERTEX_DTYPE)
    e = np.arange(n + 1) * 0.25 - 4.0                      # quad edges in units of s
    x0, x1, y0, y1 = e[None, :-1], e[None, 1:], e[:-1, None], e[1:, None]
    corners = [(x0, y0), (x0, y1), (x1, y1), (x1, y0)]
    z = rng.uniform(-1.875, 1.875, (n, n, 4))
    normal = rng.normal(size=(n, n, 3)) * np.exp2(rng.integers(-3, 4, (n, n, 1)))
    for k, (cx, cy) in enumerate(corners):
        cx, cy = np.broadcast_to(cx, (n, n)), np.broadcast_to(cy, (n, n))
        v["pos"][:, :, k, 0], v["pos"][:, :, k, 1], v["pos"][:, :, k, 2] = cx * s, cy * s, z[:, :, k] * s
        v["uv"][:, :, k, 0], v["uv"][:, :, k, 1] = (cx + 4.0) / 8.0, (4.0 - cy) / 8.0   # texel (column, row) = pixel
        v["normal"][:, :, k] = normal
    v["tangent"] = (1.0, 0.0, 0.0)
    idx = (np.arange(n * n, dtype=np.uint32)[:, None] * 4 + QUAD_INDEX[None, :]).ravel()
    return v.ravel(), idx


def _coarse_mesh(s, x_far=4.0):
    v = np.zeros(4, bbo.VERTEX_DTYPE)
    xy = [(-4.0, -4.0), (-4.0, 4.0), (x_far, 4.0), (x_far, -4.0)]
    for k, (x, y) in enumerate(xy):
        v["pos"][k] = (x * s, y * s, (TILT[0] * x + TILT[1] * y) * s)
        v["uv"][k] = ((x + 4.0) / 8.0, (4.0 - y) / 8.0)
    v["normal"] = (TILT[0], TILT[1], -1.0)                 # towards the viewer
    v["tangent"] = (1.0, 0.0, TILT[0])                     # in the plane
    return v, QUAD_INDEX.copy()


def chart(name, s=1.0, min_roughness=0):
    """(draws, enable_normal_map) of a chart at scale s"""
    one = np.zeros(1, bbo.INSTANCE_DTYPE)
    one[0]["model"] = one[0]["inv_model"] = np.eye(4, dtype=np.float32)
    if name in ("fine", "mixed"):
        v, idx = _fine_mesh(SEEDS[name], s)
        maps, nm = material("mixed" if name == "mixed" else "packed", min_roughness), 0
    elif name == "peak":
        v, idx = _fine_mesh(SEEDS["fine"], s)
        centre = v["pos"].reshape(-1, 4, 3).mean(1, dtype=np.float64)
        v["normal"] = np.repeat(f32(np.asarray(VIEW_PEAK, np.float64) * s - centre), 4, axis=0)
        maps, nm = material("packed"), 0
        maps["roughness"] = (1 + maps["roughness"] % 3).astype(np.uint8)
    else:
        v, idx = _coarse_mesh(s, 320.0 if name == "clipped" else 4.0)   # NDC x = 80: past the +-32 w guard band
        maps, nm = material("packed", min_roughness), 1
    return [bbo.DrawData(v, idx, one, bbo.MaterialData(maps))], nm


def planned_prims(name):
    return 2048 if name in ("fine", "mixed", "peak") else 2


VIEW_PEAK = (0.5, -1.0, -1024.0)


def set_i():
    """specular peak: the one light AT the viewer (L == V bit for bit, H = normalize(2 V)), for the chart "peak" whose
    normals point at the viewer to within 2e-4 rad: N.H is 1 - ulp, 1 or 1 + ulp by rounding, and where it is exactly 1
    on a texel of roughness 1/255 .. 3/255 (a^4 < 2^-25, so a^4 - 1 rounds to -1) the GGX denominator q = fma(N.H^2,
    a2 - 1, 1) is exactly 0 while a2 N.V N.L is not: S = x * (1 / 0) = +inf, the only way to a zero `den` with a
    non-zero numerator (roughness 0 gives 0 * inf = NaN)"""
    return [L(0, pos=VIEW_PEAK, color=(1.0, 0.9, 0.8), intensity=4e6)], f32(VIEW_PEAK)


# ---------------------------------------------------------------------------------------------------------------------
# lights
# ---------------------------------------------------------------------------------------------------------------------
def L(type, pos=(0, 0, 0), dir=(0, 0, 0), color=(1, 1, 1), intensity=1.0, inner=0.0, outer=0.0):
    return dict(type=int(type), pos=f32(pos), dir=f32(dir), color=f32(color), intensity=np.float32(intensity),
                inner=np.float32(inner), outer=np.float32(outer))


def uniforms(lights, view_pos, s, enable_normal_map):
    fu = scenes.frame_uniforms([scenes.light(l["type"], pos=l["pos"], dir=l["dir"], color=l["color"], intensity=l["intensity"],
                                             inner=l["inner"], outer=l["outer"]) for l in lights])
    return fu, ortho_view(s, f32(view_pos), enable_normal_map)


def scene(name, lights, view_pos, s=1.0, min_roughness=0, draws=None):
    if draws is None:
        draws, nm = chart(name, s, min_roughness)
    else:
        draws, nm = draws
    fu, vu = uniforms(lights, view_pos, s, nm)
    return bbo.Scene(fu, vu, draws, W, H, f"chart {name}")


def lights64(lights):
    """the dicts widened for glsl_f64_light_loop / conditioning"""
    out = []
    for l in lights:
        out.append({k: (np.asarray(v, np.float64) if isinstance(v, np.ndarray) else (v if k == "type" else float(v)))
                    for k, v in l.items()})
    return out


VIEW_A = (0.5, -1.0, -7.0)


def set_a(s=1.0, gain=1.0):
    """regular: types 0, 1, 2, 0, every light and the viewer at z <= -5 s (the viewer's side of the chart's box: |L + V| stays
    away from 0, which conditioning() does not know), and every light at least 40 degrees away from the viewer as the chart
    sees them: a black metal (albedo 0, metallic 1: one texel in a thousand) shows the Fresnel term (1 - H.V)^5 alone, which
    carries 5 eps32 / (1 - H.V) -- another cancellation conditioning() does not know"""
    k = np.float32(s)
    lights = [L(0, pos=f32((9.0, 6.0, -5.0)) * k, color=(1.0, 0.9, 0.8), intensity=160.0 * gain),
              L(1, pos=f32((-8.0, 7.0, -6.0)) * k, dir=(1.0, -0.875, 0.75), color=(0.7, 1.0, 0.9), intensity=400.0 * gain,
                inner=0.96, outer=0.80),
              L(2, dir=(1.0, 1.5, 1.0), color=(0.3, 0.4, 0.9), intensity=1.5),
              L(0, pos=f32((-9.0, -8.0, -5.0)) * k, color=(0.9, 0.3, 0.2), intensity=250.0 * gain)]
    return lights, f32(VIEW_A) * k


S_TINY, S_HUGE = 2.0 ** -66, 2.0 ** 62
# Where the first light of sets d / e sits, in units of s.  The census wants the squared distance a factor 2 clear of the
# threshold on >= 10 % of the pixels on EACH side, on every chart: d (s fixed) needs |light - P| < 5.66 s and > 11.3 s in a
# box 8 s wide -- a search over positions found (6, 5, 2.5), behind the surface, with 10.4 % as the smaller side on the worst
# chart; e (s = 2^62) needs < 2.83 s and > 5.66 s: (-1.5, -2, -2), just in front of the box, 17 %.
POS_D, POS_E = (6.0, 5.0, 2.5), (-1.5, -2.0, -2.0)


def set_d():
    """tiny world, s = 2^-66: the squared light distance is denormal (< 2^-126) for part of the frame and normal for the
    rest; point and spot intensities x 2^-118"""
    k = np.float32(S_TINY)
    lights, view = set_a(S_TINY, 2.0 ** -118)
    lights[0]["pos"] = f32(POS_D) * k
    return lights, view


def set_e():
    """huge world, s = 2^62: the squared light distance overflows (>= 2^128) for part of the frame; intensities x 2^116 (att
    is about 2^-128); the viewer close enough for |view - P|^2 to overflow on part of the frame only"""
    k = np.float32(S_HUGE)
    lights, _ = set_a(S_HUGE, 2.0 ** 116)
    lights[0]["pos"] = f32(POS_E) * k
    return lights, f32((0.5, -1.0, -4.0)) * k


SPOT_POS, SPOT_DIR = (1.0, -0.5, -3.0), (-0.125, 0.25, 1.0)
SPOT_CASES = {                      # inner, outer, dir; what the cone factor can be on the chart: 0, (0, 1), 1, NaN
    "inner == outer": (0.9375, 0.9375, SPOT_DIR, {"0", "1"}),
    "inner < outer": (0.875, 0.96875, SPOT_DIR, {"0", "mid", "1"}),
    "dir = 0": (0.96, 0.80, (0.0, 0.0, 0.0), {"nan"}),
    "outer > 1": (1.5, 1.25, SPOT_DIR, {"0"}),
    "outer < -1": (0.5, -1.5, SPOT_DIR, {"mid", "1"}),
    "edge across": (0.96875, 0.875, SPOT_DIR, {"0", "mid", "1"}),
}


def set_f(case):
    inner, outer, d, _ = SPOT_CASES[case]
    return [L(1, pos=SPOT_POS, dir=d, color=(1.0, 0.8, 0.6), intensity=150.0, inner=inner, outer=outer)], f32(VIEW_A)


def _many_lights(n, seed=99):
    rng = np.random.Generator(np.random.PCG64(seed))
    out = []
    for i in range(n):
        t = (0, 1, 2, UNKNOWN)[i % 4]
        pos = f32(rng.uniform(-6, 6, 3)); pos[2] = np.float32(rng.uniform(-9, -5))
        out.append(L(t, pos=pos, dir=f32(rng.uniform(-0.5, 0.5, 3)) + f32((0, 0, 1)), color=f32(rng.uniform(0.1, 1, 3)),
                     intensity=float(rng.uniform(0.5, 4.0)), inner=0.9, outer=0.6))
    return out


def set_g(case):
    """list shapes: where an unknown type sits next to the one-ahead prefetch, and the two ends of the count"""
    a, view = set_a()
    unknown = lambda i: L(UNKNOWN + i, pos=(0.0, 0.0, -6.0), dir=(0.0, 0.0, 1.0), color=(9.0, 9.0, 9.0), intensity=1000.0,
                          inner=0.9, outer=0.5)
    lights = {"no lights": [], "unknown first": [unknown(0)] + a, "unknown last": a + [unknown(0)],
              "two unknown in a row": a[:2] + [unknown(0), unknown(-9)] + a[2:], "only unknown": [unknown(0), unknown(1), unknown(2)],
              "99 lights": _many_lights(99)}[case]
    return lights, view


G_CASES = ("no lights", "unknown first", "unknown last", "two unknown in a row", "only unknown", "99 lights")


def set_h(case):
    """radiance ends"""
    a, view = set_a()
    extra = {"denormal radiance": [L(0, pos=(-1.0, 1.0, -5.5), color=(2e-20, 1.5e-20, 1e-20), intensity=1e-20)],     # ~1e-40
             "overflowing radiance": [L(1, pos=SPOT_POS, dir=SPOT_DIR, color=(3e20, 2e20, 1e20), intensity=2e19, inner=0.97, outer=0.9)],
             "negative intensity": [L(0, pos=(-1.0, 1.0, -5.5), color=(1.0, 0.5, 0.25), intensity=-40.0)],
             "inf - inf": [L(2, dir=(0.5, 0.25, 1.0), color=(1e30, 1e30, 1e30), intensity=1e30),
                           L(2, dir=(-0.5, 0.5, 1.0), color=(1e30, 1e30, 1e30), intensity=-1e30)]}[case]
    return a[:1] + extra, view


H_CASES = ("denormal radiance", "overflowing radiance", "negative intensity", "inf - inf")

D_ANTI = f32((0.25, -0.5, -1.0))     # set c: light at P + d, viewer at P - d


def antipodal_pixels(P, d=D_ANTI):
    """[n] bool: f32(Q - P) == -f32(view - P) bit for bit, with Q = f32(P + d), view = f32(P - d), and both non-zero"""
    P = f32(P).reshape(-1, 3)
    Q, V = P + d, P - d
    a, b = Q - P, V - P
    return (bits(a) == bits(-b)).all(-1) & (a != 0).any(-1)


def set_b(P_point, P_spot):
    """coincident: a point light and a spot light at exactly the P of two pixels (their pixels are NaN: 0 * inf)"""
    a, view = set_a()
    return [a[0], L(0, pos=P_point, color=(0.8, 0.9, 1.0), intensity=3.0),
            L(1, pos=P_spot, dir=(0.0, 0.25, 1.0), color=(1.0, 0.7, 0.7), intensity=2.0, inner=0.9, outer=0.5)], view


def set_c(P_pixel):
    a, _ = set_a()
    return [L(0, pos=f32(P_pixel) + D_ANTI, color=(1.0, 1.0, 0.8), intensity=4.0), a[2]], f32(P_pixel) - D_ANTI


def hazard_set(P_point, P_spot, P_anti):
    """the lights of sets b, c, f and h that leave the frame informative, together (8 lights): a light whose value is NaN
    or infinite on every pixel (dir = 0, overflowing radiance, the +-inf pair) would hide all the others and has frames
    of its own"""
    a, _ = set_a()
    f = lambda c: set_f(c)[0][0]
    lights = [L(0, pos=P_point, color=(0.8, 0.9, 1.0), intensity=3.0),
              L(1, pos=P_spot, dir=(0.0, 0.25, 1.0), color=(1.0, 0.7, 0.7), intensity=2.0, inner=0.9, outer=0.5),
              L(0, pos=f32(P_anti) + D_ANTI, color=(1.0, 1.0, 0.8), intensity=4.0),
              f("inner == outer"), f("inner < outer"), f("outer < -1"),
              set_h("denormal radiance")[0][1], set_h("negative intensity")[0][1]]
    return lights, f32(P_anti) - D_ANTI


# ---------------------------------------------------------------------------------------------------------------------
# surfaces and census
# ---------------------------------------------------------------------------------------------------------------------
def _unit(a):
    return a / np.sqrt((a * a).sum(-1))[..., None]


def model_surface(sc, prim, s=1.0):
    """Where no surface read-back is to be had (the CPU tests): the light loop's inputs modelled in binary64 from the
    scene, [n, 12].  P is affine on the winning triangle `prim` [H, W] (its plane through the pixel centre's x, y), the
    normal is the vertex normal (EnableNormalMap = 0) or TBN * (texel * 2 - 1), the material the pixel's own texel
    (nearest texel for a map that is not 128^2).  Close to what the oracle shades, not bit for bit."""
    d = sc.draws[0]
    v = d.vertices
    tri = d.indices.reshape(-1, 3)[prim.ravel()]                       # [n, 3] vertex numbers
    p = v["pos"][tri].astype(np.float64)                               # [n, 3, 3]
    x, y = pixel_xy(s)
    x, y = x.ravel(), y.ravel()
    e1, e2 = p[:, 1] - p[:, 0], p[:, 2] - p[:, 0]
    nrm = np.cross(e1, e2)
    z = p[:, 0, 2] - (nrm[:, 0] * (x - p[:, 0, 0]) + nrm[:, 1] * (y - p[:, 0, 1])) / nrm[:, 2]
    P = np.stack([x, y, z], -1)
    N = _unit(v["normal"][tri[:, 0]].astype(np.float64))
    rows, cols = np.divmod(np.arange(N_PIX), W)
    maps = d.material.maps

    def texel(name, default):
        m = maps.get(name)
        if m is None:
            return np.full((N_PIX, 3), default, np.float64)
        return m[rows * m.shape[0] // H, cols * m.shape[1] // W, :3].astype(np.float64) / 255.0
    if int(sc.view["enable_normal_map"]):
        T = _unit(v["tangent"][tri[:, 0]].astype(np.float64))
        B = np.cross(N, T)
        t = texel("normal", 0.5) * 2.0 - 1.0
        N = T * t[:, 0:1] + B * t[:, 1:2] + N * t[:, 2:3]
    return np.concatenate([P, N, texel("albedo", 1.0), texel("metallic", 0.0)[:, :1], texel("roughness", 0.0)[:, :1],
                           texel("ao", 1.0)[:, :1]], -1)


def census(surf, lights, view_pos):
    """binary64 counts on surface values surf[n, 12] (P, normal, albedo, metallic, roughness, ao), a factor 2 clear of
    every threshold.  Returns a dict of fractions of the n samples (and per-light lists)."""
    surf = np.asarray(surf, np.float64).reshape(-1, 12)
    P, normal, rough = surf[:, 0:3], surf[:, 3:6], surf[:, 10]
    n = len(surf)
    out = {"n": n, "roughness_0": float((rough == 0).mean())}
    with np.errstate(all="ignore"):
        N = _unit(normal)
        ndv = (N * _unit(np.asarray(view_pos, np.float64) - P)).sum(-1)
        out["ndv_negative"] = float((ndv < 0).mean())
        ndl_neg = np.zeros(n, bool)
        d2_lo, d2_hi, d2_sub, d2_norm = [], [], [], []
        for l in lights64(lights):
            if l["type"] in (0, 1):
                Lv = l["pos"] - P
                d2 = (Lv * Lv).sum(-1)
                ndl_neg |= (N * _unit(Lv)).sum(-1) < 0
                d2_sub.append(float((d2 < 2.0 ** -127).mean())); d2_norm.append(float((d2 > 2.0 ** -125).mean()))
                d2_lo.append(float((d2 < 2.0 ** 127).mean())); d2_hi.append(float((d2 > 2.0 ** 129).mean()))
            elif l["type"] == 2:
                ndl_neg |= (N * -_unit(l["dir"])).sum(-1) < 0
        out["ndl_negative_some_light"] = float(ndl_neg.mean())
        out["d2_denormal"], out["d2_normal"], out["d2_finite"], out["d2_overflows"] = d2_sub, d2_norm, d2_lo, d2_hi
    return out


def cone_factor_kinds(surf, light):
    """which values the spot factor clamp((theta - outer) / (inner - outer), 0, 1) takes on the samples, in binary64 and
    1/8 clear of both clamps (x <= -1/8, 1/8 <= x <= 7/8, x >= 9/8): a set out of {"0", "mid", "1", "nan"}"""
    P = np.asarray(surf, np.float64).reshape(-1, 12)[:, 0:3]
    l = lights64([light])[0]
    with np.errstate(all="ignore"):
        theta = (_unit(l["pos"] - P) * _unit(-l["dir"])).sum(-1)
        x = (theta - l["outer"]) / (l["inner"] - l["outer"])
    kinds = set()
    if np.isnan(x).any():
        kinds.add("nan")
    if (x <= -0.125).any():
        kinds.add("0")
    if (x >= 1.125).any():
        kinds.add("1")
    if ((x >= 0.125) & (x <= 0.875)).any():
        kinds.add("mid")
    return kinds


def check_census(case, name, surf, lights, view_pos):
    """the census conditions that depend on the inputs alone, asserted (case names: tests/test_gpu_surface_chart.py CASES);
    surf[n, 12] in binary32 values, before any binary16 store.  Returns the census."""
    c = census(surf, lights, view_pos)
    assert c["ndv_negative"] >= 0.25, c["ndv_negative"]
    if any(l["type"] in (0, 1, 2) for l in lights):
        assert c["ndl_negative_some_light"] >= 0.25, c["ndl_negative_some_light"]
    if name in ("fine", "mixed") and case != "a":
        assert 0.03 <= c["roughness_0"] <= 0.10, c["roughness_0"]
    if case == "a":
        assert c["roughness_0"] == 0 and (np.asarray(surf).reshape(-1, 12)[:, 10] >= 5.999 / 255).all()
    if case in ("d", "e"):
        lo, hi = (c["d2_denormal"], c["d2_normal"]) if case == "d" else (c["d2_finite"], c["d2_overflows"])
        assert min(lo[0], hi[0]) >= 0.10, (lo, hi)          # the first light, on every chart
    if case.startswith("f "):
        kinds = cone_factor_kinds(surf, lights[0])
        assert kinds == SPOT_CASES[case[2:]][3], (case, kinds)
    return c


def surface_values(dump):
    """[h, w, 32] surface read-back -> [n, 12] light-loop inputs"""
    return np.ascontiguousarray(dump[..., 6:18], np.float32).reshape(-1, 12)


def gbuffer_values(gbuf):
    """[h, w, 4, 4] G-buffer -> [n, 12] light-loop inputs of the deferred pass (brdf.frag reads xyz of each attachment)"""
    g = np.ascontiguousarray(gbuf, np.float32).reshape(-1, 4, 4)
    return np.ascontiguousarray(np.concatenate([g[:, 0, :3], g[:, 1, :3], g[:, 2, :3], g[:, 3, :3]], -1))


def glsl_args(lights, view_pos, surf):
    """arguments of glsl_f64_light_loop / conditioning from light dicts and surf[n, 12], widened"""
    s = np.asarray(surf, np.float64).reshape(-1, 12)
    return lights64(lights), np.asarray(view_pos, np.float64), s[:, 0:3], s[:, 3:6], s[:, 6:9], s[:, 9], s[:, 10], s[:, 11]
