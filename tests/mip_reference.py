"""CPU statement of the mip chain and the trilinear rule (option "mip_levels"), vectorised in numpy.

Written from the rule, not from the kernels.  TEST INFRASTRUCTURE ONLY, next to tests/aniso_reference.py, whose exact fmaf,
footprint, taps and average it reuses.

  chain       a map of w x h texels has L = min(mip_levels, 1 + floor(log2 max(w, h))) levels, level k of max(1, w >> k) x
              max(1, h >> k) texels; per channel byte, texel (x, y) of level k + 1 = (s + 2) >> 2, s the integer sum of the
              level-k bytes at columns min(2x, w_k - 1), min(2x + 1, w_k - 1) and the same two rows.  An absent map is
              1 x 1 and has one level.  A packed material's level k is texture_chart.pack_bytes of the five level-k maps.
  N           aniso_reference.tap_count on the LEVEL-0 size; mx the larger of px2, py2
  level       P = mx R2[N], R2[k] the correctly rounded 1 / k^2.  A difference not finite, or !(P > 1): d = 0, delta = 0.
              Otherwise, b the bits of P: e = (b >> 23) - 127, d = e >> 1, delta = 0.5 ((float)(e & 1) + (float)(b & 0x7FFFFF)
              2^-23); d >= L - 1: d = L - 1, delta = 0
  value       hi = aniso_reference.filter_texture on level d; delta == 0: hi itself; otherwise lo = the same on level d + 1
              and fmaf(delta, lo - hi, hi); the normal sample is fmaf(value, 2, -1)
  materials   as in aniso_reference: present shaded maps of one size are ONE texture with one (N, d, delta), otherwise one
              per map; the height map (deferred pass only) always has its own

The scenes of the GPU tests (tests/test_gpu_mip.py) and their census live here too, so that tests/test_mip_reference.py
can show on the oracle's uv frame, without a GPU, that they hold every class."""
from __future__ import annotations

import functools

import numpy as np

import aniso_reference as A
import surface_chart as SC
import texture_chart as TC
from oracle import bbo

F = np.float32
MAX_LEVELS = 15
R2 = np.concatenate([[F(0)], F(1.0) / (np.arange(1, A.MAX_ANISO + 1, dtype=F) ** 2).astype(F)]).astype(F)   # R2[k] = 1 / k^2
# lambda = 1/2 log2 P with log2(1 + t) taken as t: low by at most 1/2 max(log2(1 + t) - t), at t = 1 / ln 2 - 1
_T = 1.0 / np.log(2.0) - 1.0
LEVEL_BOUND = 0.5 * (np.log2(1.0 + _T) - _T)                      # 0.0430...


# ---------------------------------------------------------------------------------------------------------------------
# chain
# ---------------------------------------------------------------------------------------------------------------------
def level_count(w, h, mip_levels):
    return min(int(mip_levels), 1 + int(max(w, h)).bit_length() - 1)


def level_size(w, h, k):
    return max(1, w >> k), max(1, h >> k)


def reduce_level(tex):
    """the next level of uint8 [h, w, 4]"""
    h, w = tex.shape[:2]
    w1, h1 = level_size(w, h, 1)
    x, y = np.arange(w1), np.arange(h1)
    xa, xb = np.minimum(2 * x, w - 1), np.minimum(2 * x + 1, w - 1)
    ya, yb = np.minimum(2 * y, h - 1), np.minimum(2 * y + 1, h - 1)
    t = tex.astype(np.uint32)
    s = t[ya][:, xa] + t[ya][:, xb] + t[yb][:, xa] + t[yb][:, xb]
    return ((s + 2) >> 2).astype(np.uint8)


def chain(tex, mip_levels):
    """[level 0, level 1, ...] of uint8 [h, w, 4]"""
    tex = np.ascontiguousarray(tex, np.uint8)
    out = [tex]
    while len(out) < level_count(tex.shape[1], tex.shape[0], mip_levels):
        out.append(reduce_level(out[-1]))
    return out


def material_chains(maps, mip_levels):
    """name -> chain of every map of a material (an absent one: its 1 x 1 default, one level)"""
    return {k: chain(A.texture_of(maps.get(k), k), mip_levels if maps.get(k) is not None else 1) for k in A.MAP_NAMES}


def packed_levels(maps, mip_levels):
    """the packed form of every level of a material's packed set (uint8 arrays), or None for an unpacked material"""
    size = A.shared_size(maps)
    if size is None:
        return None
    chains = material_chains(maps, mip_levels)
    out = []
    for k in range(level_count(size[0], size[1], mip_levels)):
        level = {name: chains[name][k] for name in A.SHADED if maps.get(name) is not None}
        if not level:                                   # no shaded map supplied: 1 x 1, one level, the defaults
            level = {}
        out.append(TC.pack_bytes(level))
    return out


def level_table(w, h, mip_levels):
    """[(w_k, h_k, first byte, bytes)] of the packed levels of a w x h set, laid out one behind the other"""
    out, at = [], 0
    for k in range(level_count(w, h, mip_levels)):
        wk, hk = level_size(w, h, k)
        n = TC.packed_bytes_needed(wk, hk)
        out.append((wk, hk, at, n))
        at += n
    return out


# ---------------------------------------------------------------------------------------------------------------------
# level rule
# ---------------------------------------------------------------------------------------------------------------------
def long_axis(dudx, dvdx, dudy, dvdy, w, h):
    """mx of the anisotropic rule's footprint on a map of w x h (binary32), and whether the four differences are finite"""
    dudx, dvdx, dudy, dvdy = (np.asarray(x, F) for x in (dudx, dvdx, dudy, dvdy))
    fw, fh = F(w), F(h)
    with np.errstate(all="ignore"):
        ax, ay = dudx * fw, dvdx * fh
        px2 = A.fmaf(ax, ax, ay * ay)
        bx, by = dudy * fw, dvdy * fh
        py2 = A.fmaf(bx, bx, by * by)
        mx = np.where(px2 > py2, px2, py2).astype(F)
    return mx, np.isfinite(dudx) & np.isfinite(dvdx) & np.isfinite(dudy) & np.isfinite(dvdy)


def level_of(P, finite, levels):
    """(d int64, delta binary32) from P binary32"""
    P = np.ascontiguousarray(P, F)
    with np.errstate(all="ignore"):
        live = np.asarray(finite, bool) & (P > F(1.0))
    b = P.view(np.uint32).astype(np.int64)
    e = (b >> 23) - 127
    d = e >> 1
    delta = (F(0.5) * ((e & 1).astype(F) + (b & 0x7FFFFF).astype(F) * F(2.0 ** -23))).astype(F)
    last = d >= levels - 1
    d, delta = np.where(last, levels - 1, d), np.where(last, F(0.0), delta)
    return np.where(live, d, 0).astype(np.int64), np.where(live, delta, F(0.0)).astype(F)


def level_rule(footprint, w, h, n, levels):
    fp = np.asarray(footprint, F).reshape(-1, 6)
    mx, finite = long_axis(fp[:, 2], fp[:, 3], fp[:, 4], fp[:, 5], w, h)
    with np.errstate(all="ignore"):
        P = (mx * R2[n]).astype(F)
    return level_of(P, finite, levels) + (P,)


# ---------------------------------------------------------------------------------------------------------------------
# filter
# ---------------------------------------------------------------------------------------------------------------------
def filter_chain(levels, footprint, n, axis, d, delta):
    """[m, 4] binary32: the trilinear value from a chain (list of uint8 [h_k, w_k, 4])"""
    fp = np.asarray(footprint, F).reshape(-1, 6)
    out = np.zeros((len(fp), 4), F)
    for k in np.unique(d):
        at = np.flatnonzero(d == k)
        hi = A.filter_texture(levels[k], fp[at], n[at], axis[at])
        blend = delta[at] != 0
        if blend.any():
            b = at[blend]
            lo = A.filter_texture(levels[k + 1], fp[b], n[b], axis[b])
            with np.errstate(all="ignore"):
                hi[blend] = A.fmaf(delta[b][:, None], (lo - hi[blend]).astype(F), hi[blend])
        out[at] = hi
    return out


def filter_maps(material, footprint, enable_normal_map, deferred, max_aniso, mip_levels):
    """slots 12..31 of the surface record for every footprint row [m, 6]: aniso_reference.filter_maps' sixteen, then d and
    delta of the packed set / the albedo map, and d and delta of the height map (deferred, else 0)"""
    maps = dict(material)
    fp = np.asarray(footprint, F).reshape(-1, 6)
    out = np.zeros((len(fp), 20), F)
    size = A.shared_size(maps)
    chains = material_chains(maps, mip_levels)

    def one(name):
        own = chains[name]
        if size is not None and name != "height":
            w, h = size
            count = level_count(w, h, mip_levels)
            if maps.get(name) is None:                  # absent inside a packed material: uniform on every level
                own = [np.broadcast_to(own[0], level_size(w, h, k)[::-1] + (4,)) for k in range(count)]
        else:
            w, h = own[0].shape[1], own[0].shape[0]
            count = len(own)
        assert len(own) == count
        n, axis = A.tap_count(fp[:, 2], fp[:, 3], fp[:, 4], fp[:, 5], w, h, max_aniso)
        d, delta, _ = level_rule(fp, w, h, n, count)
        return filter_chain(own, fp, n, axis, d, delta), n, d, delta

    s, n, d, delta = one("albedo")
    out[:, 0:3], out[:, 10], out[:, 16], out[:, 17] = s[:, :3], n, d, delta
    for col, name in ((3, "metallic"), (4, "roughness"), (5, "ao")):
        s, n, _, _ = one(name)
        out[:, col], out[:, 10 + A.MAP_NAMES.index(name)] = s[:, 0], n
    if deferred:
        s, n, d, delta = one("height")
        out[:, 6], out[:, 15], out[:, 18], out[:, 19] = s[:, 0], n, d, delta
    if enable_normal_map:
        s, n, _, _ = one("normal")
        out[:, 7:10], out[:, 14] = A.fmaf(s[:, :3], F(2.0), F(-1.0)), n
    return out


# ---------------------------------------------------------------------------------------------------------------------
# scenes of the GPU tests: 128 x 128, the charts' orthographic camera (w = 1)
#   steps    sixteen axis-aligned strips of eight rows, strip j with uv = 2^(j - 5) x the pixel grid / 128: every difference
#            is a power of two, so on a power-of-two map P = 4^k exactly -- every level with delta = 0, the magnified strips
#            and the strips clamped to the last level
#   tilted   the surface charts' tilted coarse quad with uv running over some twenty repeats, not aligned with the grid:
#            delta != 0 nearly everywhere, several tap counts
#   nan      the texture chart's `nanvertex` gradient chart: differences that are not finite
# ---------------------------------------------------------------------------------------------------------------------
W, H, N_PIX = SC.W, SC.H, SC.N_PIX
SCENES = ("steps", "tilted", "nan")
STRIPS = 16
# what each scene claims: the census classes it must hold (>= MIN_CLASS pixels each)
CLAIMS = {"steps": ("every level", "whole level", "clamped", "magnified"), "tilted": ("blended",), "nan": ("not finite",)}
MIN_CLASS = 64


def _strip_mesh():
    v = np.zeros((STRIPS, 4), bbo.VERTEX_DTYPE)
    rows = H // STRIPS
    for j in range(STRIPS):
        y_top, y_bot = 4.0 - 8.0 * (j * rows) / H, 4.0 - 8.0 * ((j + 1) * rows) / H
        scale = 2.0 ** (j - 5)
        for k, (x, y) in enumerate(((-4.0, y_bot), (-4.0, y_top), (4.0, y_top), (4.0, y_bot))):
            v["pos"][j, k] = (x, y, 0.5)
            v["uv"][j, k] = (scale * (x + 4.0) / 8.0, scale * (4.0 - y) / 8.0)
    v["normal"] = (SC.TILT[0], SC.TILT[1], -1.0)
    v["tangent"] = (1.0, 0.0, SC.TILT[0])
    idx = (np.arange(STRIPS, dtype=np.uint32)[:, None] * 4 + SC.QUAD_INDEX[None, :]).ravel()
    return v.ravel(), idx


def _tilted_mesh():
    v, idx = SC._coarse_mesh(1.0)
    x, y = v["pos"][:, 0].astype(np.float64), v["pos"][:, 1].astype(np.float64)
    v["uv"][:, 0] = (37.0 * (x + 4.0) + 5.0 * (4.0 - y)) / 16.0     # ~ 20 repeats across the frame, skewed
    v["uv"][:, 1] = (-3.0 * (x + 4.0) + 11.0 * (4.0 - y)) / 16.0
    return v, idx


def scene(name, materials):
    """the frame of a scene with its materials (a tuple of map dicts; two: one triangle / every other strip each)"""
    one = np.zeros(1, bbo.INSTANCE_DTYPE)
    one[0]["model"] = one[0]["inv_model"] = np.eye(4, dtype=np.float32)
    mats = [bbo.MaterialData(m) for m in materials]
    if name == "steps":
        v, idx = _strip_mesh()
    elif name == "tilted":
        v, idx = _tilted_mesh()
    else:
        assert name == "nan"
        v, idx = TC._gradient_mesh("nanvertex")
    if len(mats) == 1:
        draws = [bbo.DrawData(v, idx, one, mats[0])]
    else:                                                  # triangles alternate between the two materials, a draw each
        tris = idx.reshape(-1, 3)
        draws = [bbo.DrawData(v.copy(), tris[i::2].ravel().copy(), one, m) for i, m in enumerate(mats)]
    lights, view = SC.set_a()
    fu, vu = SC.uniforms(lights, view, 1.0, 1)
    return bbo.Scene(fu, vu, draws, W, H, f"mip {name}")


def pixel_material(sc, prim):
    """[N_PIX] material number of every pixel's winner (0 where nothing is covered)"""
    prim = np.asarray(prim).ravel()
    if len(sc.draws) == 1:
        return np.zeros(len(prim), np.int64)
    return ((prim != bbo.NO_PRIM) & (prim >= sc.draws[0].n_prims)).astype(np.int64)


def filter_rows(sc, materials, prim, rec, deferred, max_aniso, mip_levels):
    """slots 12..31 for every row of rec (the covered pixels' records), each with the material of its winner"""
    rec = np.asarray(rec, F)
    which = pixel_material(sc, prim)
    out = np.zeros((len(rec), 20), F)
    for i, m in enumerate(materials):
        at = np.flatnonzero(which == i)
        out[at] = filter_maps(m, rec[at, :6], 1, bool(deferred), max_aniso, mip_levels)
    return out


def model_differences(uv, prim):
    """[h, w, 4] dudx dvdx dudy dvdy from a uv frame where the right and the lower neighbour have the same winner, and the
    mask of those pixels: there the kernel's own-plane differences are the frame's (tests/test_gpu_aniso.py)"""
    uv, prim = np.asarray(uv, F)[..., :2], np.asarray(prim)
    ok = np.zeros(prim.shape, bool)
    ok[:-1, :-1] = (prim[:-1, :-1] != bbo.NO_PRIM) & (prim[:-1, :-1] == prim[:-1, 1:]) & (prim[:-1, :-1] == prim[1:, :-1])
    d = np.zeros(prim.shape + (4,), F)
    with np.errstate(all="ignore"):
        d[:-1, :-1, 0:2] = uv[:-1, 1:] - uv[:-1, :-1]
        d[:-1, :-1, 2:4] = uv[1:, :-1] - uv[:-1, :-1]
    return d, ok


def census(name, d, delta, P, finite, levels):
    """counts of the level classes on per-pixel arrays of ONE texture with `levels` levels; asserts what `name` claims"""
    d, delta, P = np.asarray(d).ravel(), np.asarray(delta).ravel(), np.asarray(P, F).ravel()
    finite = np.asarray(finite, bool).ravel()
    with np.errstate(all="ignore"):
        live = finite & (P > F(1.0))
        out = {"level": [int((finite & (d == k)).sum()) for k in range(levels)],
               "whole level": int((live & (d >= 1) & (delta == 0) & (d < levels - 1)).sum()),
               "clamped": int((live & (d == levels - 1) & (P >= F(4.0) ** (levels - 1))).sum()),
               "magnified": int((finite & ~(P > F(1.0))).sum()),
               "not finite": int((~finite).sum()),
               "blended": int((delta != 0).sum()), "pixels": int(len(d))}
    claims = CLAIMS[name]
    if "every level" in claims:
        assert min(out["level"]) >= MIN_CLASS, (name, out)
    for c in ("whole level", "clamped", "magnified", "not finite"):
        if c in claims:
            assert out[c] >= MIN_CLASS, (name, c, out)
    if "blended" in claims:
        assert 4 * out["blended"] >= out["pixels"], (name, out)
    return out


@functools.lru_cache(None)
def maps64():
    """five 64^2 maps and a 16^2 height map: seven levels, and five"""
    rng = np.random.Generator(np.random.PCG64(77))
    m = {k: TC._map(rng, k, 64, 64) for k in A.SHADED}
    m["height"] = TC._map(rng, "height", 16, 16)
    return m
