"""CPU statement of the anisotropic filter rule (option "max_anisotropy"), vectorised in numpy.

Written from the rule, not from the kernel.  Everything is binary32 in the rule's operand order:

  footprint   per map of w x h texels: ax = dudx (float)w, ay = dvdx (float)h, px2 = fmaf(ax, ax, ay ay); py2 likewise from
              the y differences; mx / mn their larger / smaller; the long axis is x iff px2 > py2
  tap count   N = 1 + #{n in 1..15: (float)(n n) mn < mx}, then min(N, max_anisotropy); N = 1 if !(mx > 1) or any of the
              four differences is not finite
  taps        N = 1: the one tap at (u, v).  N >= 2, i = 1..N: o = fmaf((float)i, R[N + 1], -0.5), R[k] the correctly
              rounded 1 / k; (u_i, v_i) = (fmaf(o, du, u), fmaf(o, dv, v)) with (du, dv) the long axis' differences; each
              tap is the sampler of the oracle (bbo.sample: REPEAT, its non-finite guard, / 255 inside)
  average     acc = t_1; acc = acc + t_i in tap order; value = acc R[N]; the normal sample is fmaf(value, 2, -1)
  materials   a material whose present shaded maps (albedo, metallic, roughness, ao, normal) share one size is sampled as
              ONE texture of that size (absent maps are uniform): one N for the five; otherwise every map has the N of its
              own size (an absent map is 1 x 1).  The height map (deferred pass only) always has its own.

bilinear() is the vectorised form of bbo.sample; tests/test_aniso_reference.py shows the two equal bit for bit."""
from __future__ import annotations

import numpy as np

F = np.float32
MAP_NAMES = ("albedo", "metallic", "roughness", "ao", "normal", "height")  # PBRMapType order
SHADED = MAP_NAMES[:5]
# `default` material texels (oracle/bb_oracle.c, k_default_texel)
DEFAULT_TEXEL = {"albedo": (255, 255, 255, 255), "metallic": (0, 0, 0, 255), "roughness": (0, 0, 0, 255),
                 "ao": (255, 255, 255, 255), "normal": (127, 127, 255, 255), "height": (0, 0, 0, 255)}
MAX_ANISO = 16
R = np.concatenate([[F(0)], F(1.0) / np.arange(1, MAX_ANISO + 2, dtype=F)]).astype(F)  # R[k] = 1 / k, k = 1 .. 17


def fmaf(a, b, c):
    """binary32 fma.  The product of two binary32 numbers is exact in binary64 (48 bits); the sum with c is not, so it is
    made error-free (s + e exactly, Knuth's TwoSum) and s is rounded to odd: the last bit of an inexact s is forced to 1.
    Rounding a round-to-odd binary64 value (53 >= 2 * 24 + 2 bits) to binary32 is the correct single rounding."""
    a, b, c = (np.asarray(x, F).astype(np.float64) for x in (a, b, c))
    with np.errstate(all="ignore"):
        p = a * b
        s = p + c
        t = s - p
        e = (p - (s - t)) + (c - t)
        ok = np.isfinite(s) & np.isfinite(e)
        bits = np.ascontiguousarray(s).view(np.int64)
        inexact_even = ok & (e != 0) & ((bits & 1) == 0)
        away = np.signbit(e) == np.signbit(s)          # the exact value lies further from zero than s
        bits = np.where(inexact_even, bits + np.where(away, 1, -1), bits)
        return bits.view(np.float64).astype(F)


def tap_count(dudx, dvdx, dudy, dvdy, w, h, max_aniso):
    """N (int32) and the long axis (0 = x, 1 = y) per element"""
    dudx, dvdx, dudy, dvdy = (np.asarray(x, F) for x in (dudx, dvdx, dudy, dvdy))
    fw, fh = F(w), F(h)
    with np.errstate(all="ignore"):
        ax, ay = dudx * fw, dvdx * fh
        px2 = fmaf(ax, ax, ay * ay)
        bx, by = dudy * fw, dvdy * fh
        py2 = fmaf(bx, bx, by * by)
        x_axis = px2 > py2
        mx, mn = np.where(x_axis, px2, py2), np.where(x_axis, py2, px2)
        n = np.ones(np.shape(mx), np.int32)
        for k in range(1, MAX_ANISO):
            n += (F(k * k) * mn < mx)
        n = np.minimum(n, np.int32(max_aniso))
        finite = np.isfinite(dudx) & np.isfinite(dvdx) & np.isfinite(dudy) & np.isfinite(dvdy)
        n = np.where(~(mx > F(1.0)) | ~finite, np.int32(1), n)
    return n.astype(np.int32), np.where(x_axis, 0, 1).astype(np.int32)


def texture_of(img, name):
    """the RGBA8 array a map is sampled from: its own, or the 1 x 1 default"""
    if img is None:
        return np.array(DEFAULT_TEXEL[name], np.uint8).reshape(1, 1, 4)
    return np.ascontiguousarray(img, np.uint8)


def bilinear(tex, u, v):
    """bbo.sample on arrays: tex uint8 [h, w, 4], u / v binary32 [n] -> [n, 4] binary32"""
    h, w = tex.shape[:2]
    u, v = np.asarray(u, F), np.asarray(v, F)
    with np.errstate(all="ignore"):
        x, y = fmaf(u, F(w), F(-0.5)), fmaf(v, F(h), F(-0.5))
        x = np.where(np.abs(x) < F(1073741824.0), x, F(0.0))
        y = np.where(np.abs(y) < F(1073741824.0), y, F(0.0))
    xf, yf = np.floor(x), np.floor(y)
    fx, fy = (x - xf).astype(F), (y - yf).astype(F)
    ix, iy = xf.astype(np.int64), yf.astype(np.int64)
    x0, x1, y0, y1 = ix % w, (ix + 1) % w, iy % h, (iy + 1) % h          # (numpy's % is REPEAT for negative indices too)
    t = tex.astype(F)
    a, b, c, d = t[y0, x0], t[y0, x1], t[y1, x0], t[y1, x1]
    top = fmaf(fx[:, None], b - a, a)
    bot = fmaf(fx[:, None], d - c, c)
    return (fmaf(fy[:, None], bot - top, top) * (F(1.0) / F(255.0))).astype(F)


def tap_positions(u, v, du, dv, n, i):
    """tap i (1-based) of n, elementwise; n = 1 is (u, v) itself"""
    n = np.asarray(n, np.int64)
    o = fmaf(F(i), R[np.minimum(n + 1, MAX_ANISO + 1)], F(-0.5))
    with np.errstate(all="ignore"):
        ui, vi = fmaf(o, du, u), fmaf(o, dv, v)
    return np.where(n == 1, np.asarray(u, F), ui).astype(F), np.where(n == 1, np.asarray(v, F), vi).astype(F)


def filter_texture(tex, footprint, n, axis):
    """[m, 4] binary32: the average of n taps along the long axis; footprint [m, 6] = u v dudx dvdx dudy dvdy"""
    fp = np.asarray(footprint, F).reshape(-1, 6)
    u, v = fp[:, 0], fp[:, 1]
    du = np.where(axis == 0, fp[:, 2], fp[:, 4]).astype(F)
    dv = np.where(axis == 0, fp[:, 3], fp[:, 5]).astype(F)
    acc = np.zeros((len(fp), 4), F)
    for i in range(1, int(n.max(initial=1)) + 1):
        live = np.nonzero(i <= n)[0]
        ui, vi = tap_positions(u[live], v[live], du[live], dv[live], n[live], i)
        t = bilinear(tex, ui, vi)
        acc[live] = t if i == 1 else (acc[live] + t).astype(F)
    return np.where((n == 1)[:, None], acc, (acc * R[n][:, None]).astype(F)).astype(F)


def shared_size(maps):
    """(w, h) when the material's present shaded maps share one size (1 x 1 when none is present), else None"""
    sizes = {(maps[k].shape[1], maps[k].shape[0]) for k in SHADED if maps.get(k) is not None}
    if len(sizes) > 1:
        return None
    return sizes.pop() if sizes else (1, 1)


def filter_maps(material, footprint, enable_normal_map, deferred, max_aniso):
    """slots 12..27 of the surface record for every footprint row [m, 6]:
    albedo(3) metallic roughness ao height normal-sample(3) taps(6).  material: dict name -> uint8 [h, w, 4] or None"""
    maps = dict(material)
    fp = np.asarray(footprint, F).reshape(-1, 6)
    out = np.zeros((len(fp), 16), F)
    size = shared_size(maps)

    def one(name):
        tex = texture_of(maps.get(name), name)
        w, h = size if (size is not None and name != "height") else (tex.shape[1], tex.shape[0])
        if (tex.shape[1], tex.shape[0]) != (w, h):       # an absent map inside a packed material: uniform at the shared size
            tex = np.broadcast_to(tex, (h, w, 4))
        n, axis = tap_count(fp[:, 2], fp[:, 3], fp[:, 4], fp[:, 5], w, h, max_aniso)
        return filter_texture(tex, fp, n, axis), n

    s, n = one("albedo")
    out[:, 0:3], out[:, 10] = s[:, :3], n
    for col, name in ((3, "metallic"), (4, "roughness"), (5, "ao")):
        s, n = one(name)
        out[:, col], out[:, 10 + MAP_NAMES.index(name)] = s[:, 0], n
    if deferred:
        s, n = one("height")
        out[:, 6], out[:, 15] = s[:, 0], n
    if enable_normal_map:
        s, n = one("normal")
        out[:, 7:10], out[:, 14] = fmaf(s[:, :3], F(2.0), F(-1.0)), n
    return out
