"""Texture charts: 128 x 128 frames whose pixels are a CHOSEN population of texture coordinates for the sampler
(`bilinear_taps`, `wrap_repeat`, the block-linear addressing of the packed material and `filter_channel` in
csrc/bb_kernels.hip.h; oracle `bbo.sample`).  TEST INFRASTRUCTURE ONLY, next to tests/surface_chart.py, whose camera
(`ortho_view`, s = 1, view = identity, w = 1), `pixel_xy`, `_texels` and equality rule it reuses.

  point chart     one primitive per pixel (16 384 primitives, one non-indexed draw): vertex 0 exactly on the pixel centre,
                  vertex 1 0.75 pixel to the right, vertex 2 0.75 pixel below, a random z per primitive.  The barycentrics
                  at the centre are (1, 0, 0): vUV is uv[0], so ANY binary32 pair can be planted at a pixel.  Every lane of
                  a wave has another primitive: the per-lane gather path.
                    flat   uv[1] = uv[2] = uv[0]: the differences are 0; +-inf arrives as NaN (0 * inf)
                    steep  uv[1] = (0.25, 0.25), uv[2] = (-0.75, -0.75): +-inf arrives as +-inf, -0 as +0, and the
                           differences handed to the anisotropic rule are huge or not finite
  gradient chart  the `coarse` quad of the surface charts (normal map on, full tiles, the scalar path) and its `clipped`
                  form with uv running linearly over [-40, 40] x [-33, 47]; `nanvertex`: coarse with one vertex' uv
                  (NaN, 3e38)
  hazard list     per axis, a function of the map's extent n along it (hazard_list); the classes a..i of `classes`
  planting        rows 0..63 (the sweep): u and v drawn from the layout's lists by two independent seeded permutations,
                  cycled over the pixels -- every value of every list occurs.  Rows 64..127 (the cross): the sweep alone
                  cannot meet the census (the product of two rare classes, e.g. 4 cutoff values of 1600 on both axes, is
                  expected on 0.1 pixel), so the cross is stratified: slot j takes the class pair (j mod 9, j div 9 mod 9)
                  of the layout's map number (j div 81 mod #sizes), the value a member of that class in that size's list,
                  and the slots are scattered over the rows by a third seeded permutation.
  census          of the point charts (the gradient charts reach no rare class), on the uv a frame was ACTUALLY sampled at
                  (the oracle's FLAG_OUTPUT_UV frame, the kernel's dump): every
                  class holds >= 64 pixels per axis and every pair {f, g, h, i} x {a..i} >= 4 pixels, for every distinct
                  map size of the layout.  Exempt, because no binary32 value can be in them: g on an axis of extent 1
                  (u * 1 - 0.5 is finite for every finite u), h on the flat chart (0 * inf).
  models          packed_index: the block-linear record index typed from the comment in bilinear_taps; pack_bytes: the
                  packed form in numpy; aniso_reference.bilinear / filter_maps are the bit-exact sampler model
"""
from __future__ import annotations

import functools

import numpy as np

import aniso_reference as A
import surface_chart as SC
from oracle import bbo

W, H, N_PIX = SC.W, SC.H, SC.N_PIX
F = np.float32
SEEDS = {"texels": 41, "z": 42, "u": 43, "v": 44, "cross": 45, "members": 46}
CLASSES = "abcdefghi"
DEAD = "fghi"                   # the sampler replaces the coordinate by 0: cutoff, overflow, infinite, NaN
MIN_CLASS, MIN_PAIR = 64, 4
SWEEP = N_PIX // 2              # pixels of the sweep; the rest is the cross
CUTOFF = 2.0 ** 30
PACKED_TEXEL_BYTES, PACKED_PAD, TAP_LOAD_BYTES = 9, 16, 12
POINT_CHARTS, GRADIENT_CHARTS = ("flat", "steep"), ("coarse", "clipped", "nanvertex")
CHARTS = POINT_CHARTS + GRADIENT_CHARTS


# ---------------------------------------------------------------------------------------------------------------------
# material layouts
# ---------------------------------------------------------------------------------------------------------------------
PACKED_SIZES = [(2, 2), (4, 4), (5, 3), (3, 5), (6, 10), (7, 1), (1, 7), (17, 5), (48, 80), (64, 2), (8, 3), (130, 2),
                (16384, 3), (3, 16384)]                                   # w x h
FIVE_SIZES = {"albedo": (5, 3), "metallic": (64, 64), "roughness": (1, 7), "ao": (48, 80), "normal": (130, 2), "height": (17, 5)}
LAYOUTS = ([f"packed {w}x{h}" for w, h in PACKED_SIZES] + ["absent", "all 1x1", "normal only 6x10"]
           + ["albedo 1x1 rest 6x10", "albedo 6x10 roughness 1x1", "five sizes", "both"])
INVARIANCE_LAYOUTS = ("packed 6x10", "both")


def _map(rng, name, w, h):
    if name in ("normal", "height"):
        return rng.integers(0, 256, (h, w, 4), dtype=np.uint8)
    return SC._texels(rng, (h, w), (0, 1, 2) if name == "albedo" else (0,))


@functools.lru_cache(None)
def materials(layout):
    """the layout's materials, a tuple of dicts name -> uint8 [h, w, 4] (one; two for "both": even / odd columns)"""
    rng = np.random.Generator(np.random.PCG64([SEEDS["texels"], LAYOUTS.index(layout)]))
    if layout.startswith("packed "):
        w, h = map(int, layout[7:].split("x"))
        return ({k: _map(rng, k, w, h) for k in A.MAP_NAMES},)        # the height map at the same size (its own fetch)
    if layout == "absent":
        return ({},)
    if layout == "all 1x1":
        return ({k: _map(rng, k, 1, 1) for k in A.SHADED},)
    if layout == "normal only 6x10":
        return ({"normal": _map(rng, "normal", 6, 10)},)
    if layout == "albedo 1x1 rest 6x10":
        return ({k: _map(rng, k, *((1, 1) if k == "albedo" else (6, 10))) for k in A.SHADED},)
    if layout == "albedo 6x10 roughness 1x1":
        return ({"albedo": _map(rng, "albedo", 6, 10), "roughness": _map(rng, "roughness", 1, 1)},)
    if layout == "five sizes":
        return ({k: _map(rng, k, *wh) for k, wh in FIVE_SIZES.items()},)
    assert layout == "both"
    return (materials("packed 6x10")[0], materials("five sizes")[0])


def expect_packed(layout):
    return tuple(layout.startswith("packed ") or layout in ("absent", "all 1x1", "normal only 6x10") or (layout == "both" and i == 0)
                 for i in range(len(materials(layout))))


def sampled_sizes(maps):
    """the distinct (w, h) the six fetches of a material run at, in map order"""
    shared = A.shared_size(maps)
    out = []
    for k in A.MAP_NAMES:
        m = maps.get(k)
        wh = shared if (shared is not None and k != "height") else ((m.shape[1], m.shape[0]) if m is not None else (1, 1))
        if wh not in out:
            out.append(wh)
    return out


def layout_sizes(layout):
    """[(material number, (w, h))] of the layout"""
    return [(i, wh) for i, m in enumerate(materials(layout)) for wh in sampled_sizes(m)]


# ---------------------------------------------------------------------------------------------------------------------
# hazard list and classes
# ---------------------------------------------------------------------------------------------------------------------
def _ulp_neighbours(a):
    a = np.asarray(a, F)
    with np.errstate(all="ignore"):
        return np.concatenate([a, np.nextafter(a, F(np.inf)), np.nextafter(a, F(-np.inf))]).astype(F)


@functools.lru_cache(None)
def hazard_list(n):
    """binary32 texture coordinates for an axis of extent n (bit-distinct values, NaN once)"""
    k = np.arange(-2 * n, 3 * n + 1, dtype=np.float64)
    if 2 * len(k) > 512:          # evenly, but the texels at every wrap (j n - 2 .. j n + 1) stay
        edge = (np.arange(-2, 4)[:, None] * n + np.arange(-2, 2)[None, :]).ravel()
        edge = edge[(edge >= -2 * n) & (edge <= 3 * n)].astype(np.float64)
        k = np.union1d(k[np.round(np.linspace(0, len(k) - 1, 256 - len(edge))).astype(np.int64)], edge)
    grid = np.concatenate([k / n, (k + 0.5) / n])
    special = [0.0, -0.0, -0.5 / n, -1e-30, 1e-45, -1e-45, CUTOFF / n, -CUTOFF / n, (CUTOFF - 64) / n, -(CUTOFF - 64) / n,
               (2.0 ** 24 + 0.5) / n, 1e6, -1e6, 3e38, -3e38, np.inf, -np.inf, np.nan]
    with np.errstate(all="ignore"):
        vals = _ulp_neighbours(np.concatenate([grid, special]).astype(F))
    nan = np.isnan(vals)
    b = np.unique(SC.bits(vals[~nan]))
    out = np.concatenate([b.view(F), [F(np.nan)]]).astype(F)
    out.setflags(write=False)
    return out


def texel_coordinate(u, n):
    """x = fmaf(u, n, -0.5) in binary32"""
    return A.fmaf(np.asarray(u, F), F(n), F(-0.5))


def classes(u, n):
    """[9, len(u)] bool, rows a..i (not exclusive: a texel centre at the wrap is both a and c).  a is kept below 2^20,
    where a binary32 x is not an integer by its format alone."""
    u = np.asarray(u, F)
    x = texel_coordinate(u, n).astype(np.float64)
    with np.errstate(all="ignore"):
        fin = np.isfinite(x)
        ax = np.abs(x)
        live = fin & (ax < CUTOFF)
        fl = np.floor(np.where(live, x, 0.0))
        return np.stack([live & (x == fl) & (ax < 2.0 ** 20),
                         live & (x >= -1) & (x < 0),
                         live & (x >= 0) & (np.mod(fl, n) == n - 1),
                         live & (x < -1),
                         live & (ax >= 2.0 ** 20),
                         fin & (ax >= CUTOFF),
                         np.isfinite(u) & np.isinf(x),
                         np.isinf(u),
                         np.isnan(u)])


def dead(u, n):
    """the sampler takes x = 0: classes f, g, h, i"""
    return classes(u, n)[5:].any(0)


def exempt_classes(n, chart):
    e = set()
    if n == 1:
        e.add("g")
    if chart == "flat":
        e.add("h")
    return e


def census(uv, w, h, chart, pixels=None):
    """counts per axis and per pair on uv[n, 2] for a map of w x h; asserts the minimums.  Returns the counts."""
    uv = np.asarray(uv, F).reshape(-1, 2)
    if pixels is not None:
        uv = uv[pixels]
    cu, cv = classes(uv[:, 0], w), classes(uv[:, 1], h)
    eu, ev = exempt_classes(w, chart), exempt_classes(h, chart)
    out = {"u": {}, "v": {}, "min_pair": None}
    for axis, c, e in (("u", cu, eu), ("v", cv, ev)):
        for i, name in enumerate(CLASSES):
            out[axis][name] = int(c[i].sum())
            assert name in e or out[axis][name] >= MIN_CLASS, f"{w}x{h} {chart}: class {name} on {axis} holds {out[axis][name]} pixels"
    pairs = (cu[:, None, :] & cv[None, :, :]).sum(-1)                 # [class of u, class of v]
    worst = None
    for i, a in enumerate(CLASSES):
        for j, b in enumerate(CLASSES):
            if (a in DEAD or b in DEAD) and a not in eu and b not in ev:
                assert pairs[i, j] >= MIN_PAIR, f"{w}x{h} {chart}: pair ({a}, {b}) holds {int(pairs[i, j])} pixels"
                worst = int(pairs[i, j]) if worst is None else min(worst, int(pairs[i, j]))
    out["min_pair"] = worst
    return out


def check_census(layout, chart, uv):
    """the census of every map size of the layout on uv[h, w, 2] / [n, 2]; for "both" on the material's own columns"""
    out = {}
    cols = np.arange(N_PIX) % W
    for i, (w, h) in layout_sizes(layout):
        pixels = None if layout != "both" else (cols % 2 == i)
        out[f"{i}:{w}x{h}"] = census(uv, w, h, chart, pixels)
    return out


# ---------------------------------------------------------------------------------------------------------------------
# planting
# ---------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(None)
def planted_uv(layout):
    """uv[0] of every pixel's primitive, [N_PIX, 2] binary32"""
    by_material = [[wh for j, wh in layout_sizes(layout) if j == i] for i in range(len(materials(layout)))]
    uv = np.zeros((N_PIX, 2), F)
    members_rng = np.random.Generator(np.random.PCG64(SEEDS["members"]))
    cross = SWEEP + np.random.Generator(np.random.PCG64(SEEDS["cross"])).permutation(N_PIX - SWEEP)
    for axis, key in ((0, "u"), (1, "v")):
        with np.errstate(all="ignore"):
            both = np.concatenate([hazard_list(n) for n in dict.fromkeys(s[axis] for sizes in by_material for s in sizes)])
        nan = np.isnan(both)
        full = np.concatenate([np.unique(SC.bits(both[~nan])).view(F), [F(np.nan)]]).astype(F)
        perm = np.random.Generator(np.random.PCG64(SEEDS[key])).permutation(len(full))
        uv[:SWEEP, axis] = full[perm[np.arange(SWEEP) % len(full)]]
        for i, sizes in enumerate(by_material):            # the cross, on the material's own pixels ("both": its columns)
            where = cross if len(by_material) == 1 else cross[(cross % W) % 2 == i]
            slot = np.arange(len(where))
            cls_of_slot = (slot % 9) if axis == 0 else ((slot // 9) % 9)
            size_of_slot = (slot // 81) % len(sizes)
            for e, s in enumerate(sizes):
                lst = hazard_list(s[axis])
                member = classes(lst, s[axis])
                for c in range(9):
                    at = np.flatnonzero((size_of_slot == e) & (cls_of_slot == c))
                    pool = lst[member[c]] if member[c].any() else lst       # (g at extent 1 has no member: any value)
                    pool = pool[members_rng.permutation(len(pool))]
                    uv[where[at], axis] = pool[np.arange(len(at)) % len(pool)]
    uv.setflags(write=False)
    return uv


def arriving_uv(planted, chart):
    """what the interpolation at barycentrics (1, 0, 0) makes of uv[0]: flat 1 uv + 0 uv + 0 uv (inf -> NaN), steep
    uv + 0 * 0.25 + 0 * -0.75 (-0 -> +0)"""
    p = np.asarray(planted, F)
    with np.errstate(all="ignore"):
        return np.where(np.isinf(p), F(np.nan), p).astype(F) if chart == "flat" else (p + F(0.0)).astype(F)


# ---------------------------------------------------------------------------------------------------------------------
# geometry and scenes
# ---------------------------------------------------------------------------------------------------------------------
def _point_mesh(uv0, chart, pixels):
    """three vertices per pixel of `pixels` (flat indices)"""
    z = np.random.Generator(np.random.PCG64(SEEDS["z"])).uniform(-1.875, 1.875, N_PIX)[pixels]
    x, y = SC.pixel_xy()
    x, y = x.ravel()[pixels], y.ravel()[pixels]
    d = 0.75 / 16.0
    v = np.zeros((len(pixels), 3), bbo.VERTEX_DTYPE)
    for k, (dx, dy) in enumerate(((0.0, 0.0), (d, 0.0), (0.0, -d))):
        v["pos"][:, k, 0], v["pos"][:, k, 1], v["pos"][:, k, 2] = x + dx, y + dy, z
    v["uv"][:, 0] = uv0[pixels]
    if chart == "flat":
        v["uv"][:, 1] = v["uv"][:, 2] = uv0[pixels]
    else:
        v["uv"][:, 1], v["uv"][:, 2] = (0.25, 0.25), (-0.75, -0.75)
    v["normal"] = (SC.TILT[0], SC.TILT[1], -1.0)
    v["tangent"] = (1.0, 0.0, SC.TILT[0])
    return v.ravel()


def _gradient_mesh(chart):
    v, idx = SC._coarse_mesh(1.0, 320.0 if chart == "clipped" else 4.0)
    x, y = v["pos"][:, 0].astype(np.float64), v["pos"][:, 1].astype(np.float64)
    v["uv"][:, 0], v["uv"][:, 1] = -40.0 + 10.0 * (x + 4.0), -33.0 + 10.0 * (4.0 - y)
    if chart == "nanvertex":
        v["uv"][1] = (np.nan, 3e38)                    # a vertex of the first triangle only
    return v, idx


@functools.lru_cache(None)
def scene(layout, chart):
    """the frame of a layout on a chart: set a's lights, EnableNormalMap = 1"""
    one = np.zeros(1, bbo.INSTANCE_DTYPE)
    one[0]["model"] = one[0]["inv_model"] = np.eye(4, dtype=np.float32)
    mats = [bbo.MaterialData(m) for m in materials(layout)]
    if chart in POINT_CHARTS:
        uv0 = planted_uv(layout)
        cols = np.arange(N_PIX) % W
        parts = [np.arange(N_PIX)] if len(mats) == 1 else [np.flatnonzero(cols % 2 == i) for i in range(2)]
        draws = [bbo.DrawData(_point_mesh(uv0, chart, p), None, one, m) for p, m in zip(parts, mats)]
    else:
        v, idx = _gradient_mesh(chart)
        if len(mats) == 1:
            draws = [bbo.DrawData(v, idx, one, mats[0])]
        else:                                              # one triangle of the quad per material
            draws = [bbo.DrawData(v.copy(), idx[3 * i:3 * i + 3].copy(), one, m) for i, m in enumerate(mats)]   # (own mesh each)
    lights, view = SC.set_a()
    fu, vu = SC.uniforms(lights, view, 1.0, 1)
    return bbo.Scene(fu, vu, draws, W, H, f"texture chart {layout} {chart}")


def pixel_material(layout, chart, prim):
    """[N_PIX] material number of every pixel's winner"""
    if len(materials(layout)) == 1:
        return np.zeros(N_PIX, np.int64)
    first = scene(layout, chart).draws[0].n_prims
    return (np.asarray(prim).ravel() >= first).astype(np.int64)


def expected_prim(layout):
    """the point chart's winner of every pixel, [H, W]: its own primitive"""
    if len(materials(layout)) == 1:
        return np.arange(N_PIX, dtype=np.uint32).reshape(H, W)
    cols = np.arange(N_PIX) % W
    prim = np.zeros(N_PIX, np.uint32)
    n0 = 0
    for i in range(2):
        at = np.flatnonzero(cols % 2 == i)
        prim[at] = n0 + np.arange(len(at))
        n0 += len(at)
    return prim.reshape(H, W)


# ---------------------------------------------------------------------------------------------------------------------
# models
# ---------------------------------------------------------------------------------------------------------------------
def filter_rows(layout, chart, prim, rec, deferred, max_aniso):
    """slots 12..27 for every pixel: aniso_reference.filter_maps with the material of the pixel's winner"""
    rec = np.asarray(rec, F).reshape(N_PIX, -1)
    which = pixel_material(layout, chart, prim)
    out = np.zeros((N_PIX, 16), F)
    for i, m in enumerate(materials(layout)):
        at = np.flatnonzero(which == i)
        out[at] = A.filter_maps(m, rec[at, :6], 1, bool(deferred), max_aniso)
    return out


def wrapped_taps(u, v, w, h):
    """(x0, x1, y0, y1) of the sampler's four taps, int64"""
    with np.errstate(all="ignore"):
        x, y = texel_coordinate(u, w), texel_coordinate(v, h)
        x = np.where(np.abs(x) < F(CUTOFF), x, F(0.0))
        y = np.where(np.abs(y) < F(CUTOFF), y, F(0.0))
    ix, iy = np.floor(x).astype(np.int64), np.floor(y).astype(np.int64)
    return ix % w, (ix + 1) % w, iy % h, (iy + 1) % h


def packed_index(x, y, w):
    """record number of texel (x, y) in a packed material of width w: 4 x 4 blocks, blocks in row-major order"""
    x, y = np.asarray(x, np.int64), np.asarray(y, np.int64)
    return ((y >> 2) * (-(-w // 4)) + (x >> 2)) * 16 + (y & 3) * 4 + (x & 3)


def packed_bytes_needed(w, h):
    return (-(-w // 4)) * (-(-h // 4)) * 16 * PACKED_TEXEL_BYTES + PACKED_PAD


def pack_bytes(maps):
    """the packed form of a material in numpy (None when its supplied shaded maps differ in size)"""
    size = A.shared_size(maps)
    if size is None:
        return None
    w, h = size
    out = np.zeros(packed_bytes_needed(w, h), np.uint8)
    rec = out[:len(out) - PACKED_PAD].reshape(-1, PACKED_TEXEL_BYTES)
    y, x = np.divmod(np.arange(w * h), w)
    at = packed_index(x, y, w)
    t = {k: np.broadcast_to(A.texture_of(maps.get(k), k), (h, w, 4)).reshape(-1, 4) for k in A.SHADED}
    rec[at, 0:3], rec[at, 3] = t["albedo"][:, :3], t["metallic"][:, 0]
    rec[at, 4:7], rec[at, 7], rec[at, 8] = t["normal"][:, :3], t["roughness"][:, 0], t["ao"][:, 0]
    return out


def host_pack(maps):
    """bbr_pack_material: (packable, w, h, bytes, the packed form or None)"""
    import ctypes as C

    from bibim_renderer_amd import _capi
    arr, keep = (_capi.BbrImage * 6)(), []
    for i, name in enumerate(A.MAP_NAMES):
        a = maps.get(name)
        if a is None:
            arr[i] = _capi.BbrImage(None, 0, 0)
        else:
            a = np.ascontiguousarray(a, np.uint8)
            keep.append(a)
            arr[i] = _capi.BbrImage(a.ctypes.data, a.shape[1], a.shape[0])
    ok, w, h, n = C.c_int32(), C.c_int32(), C.c_int32(), C.c_uint64()
    L = _capi.lib()
    assert L.bbr_pack_material(arr, C.byref(ok), C.byref(w), C.byref(h), C.byref(n), None, 0) == 0
    out = None
    if ok.value:
        out = np.full(n.value + 64, 0xA5, np.uint8)                      # a canary behind the reported size
        assert L.bbr_pack_material(arr, C.byref(ok), C.byref(w), C.byref(h), C.byref(n), out.ctypes.data, n.value) == 0
        assert (out[n.value:] == 0xA5).all(), "the pack function wrote past the size it reports"
        out = out[:n.value]
    return bool(ok.value), w.value, h.value, int(n.value), out


# ---------------------------------------------------------------------------------------------------------------------
# the binary64 layer and the closed forms, on footprints sampled with ONE tap
# ---------------------------------------------------------------------------------------------------------------------
EPS32 = float(np.finfo(np.float32).eps)
COLUMNS = (("albedo", 0, (0, 1, 2)), ("metallic", 3, (0,)), ("roughness", 4, (0,)), ("ao", 5, (0,)), ("height", 6, (0,)),
           ("normal", 7, (0, 1, 2)))
# the normal sample is stored as fmaf(value, 2, -1), a binary32 number in [-1, 1]: its rounding moves the value it stands for,
# (sample + 1) / 2, by at most half of half an ulp of 1
NORMAL_ROUNDING = 2.0 ** -26


def check_values(maps, uv, got, deferred, np_bilinear, label=""):
    """got[n, 10]: albedo(3) metallic roughness ao height normal-sample(3) (slots 12..21 of a surface record; the normal
    sample is fmaf(value, 2, -1), EnableNormalMap = 1) sampled with one tap at uv[n, 2].  Asserts
      * both axes dead: the value is byte(0, 0) * (1 / 255) in binary32, bit for bit (the normal: fmaf of it)
      * one axis dead: np_bilinear with that axis' texel coordinate 0 (u = 0.5 / n), within the tolerance of the other
      * none dead and |u| w, |v| h < 2^20: np_bilinear within 4 eps32 (1 + max(|u| w, |v| h)) + 1e-7
        (the normal: (sample + 1) / 2 against it, the tolerance wider by the rounding of the stored sample, 2^-26)
    and returns the worst error / tolerance."""
    uv = np.asarray(uv, F).reshape(-1, 2)
    got = np.asarray(got, F)
    shared = A.shared_size(maps)
    worst = 0.0
    for name, col, chans in COLUMNS:
        if name == "height" and not deferred:
            continue
        tex = A.texture_of(maps.get(name), name)
        w, h = shared if (shared is not None and name != "height") else (tex.shape[1], tex.shape[0])
        tex = np.broadcast_to(tex, (h, w, 4)) if tex.shape[:2] != (h, w) else tex
        du, dv = dead(uv[:, 0], w), dead(uv[:, 1], h)
        g = got[:, [col + c for c in range(len(chans))]]
        both = du & dv
        origin = (tex[0, 0, list(chans)].astype(F) * (F(1.0) / F(255.0))).astype(F)
        if name == "normal":
            origin = A.fmaf(origin, F(2.0), F(-1.0))
        assert np.array_equal(SC.bits(g[both]), SC.bits(np.broadcast_to(origin, g[both].shape))), f"{label} {name}: a dead pixel is not texel (0, 0)"
        with np.errstate(all="ignore"):
            u64 = np.where(du, 0.5 / w, uv[:, 0].astype(np.float64))
            v64 = np.where(dv, 0.5 / h, uv[:, 1].astype(np.float64))
            mag = np.maximum(np.where(du, 0.0, np.abs(u64) * w), np.where(dv, 0.0, np.abs(v64) * h))
        ok = ~both & (mag < 2.0 ** 20)
        want = np_bilinear(tex, u64[ok], v64[ok])[:, list(chans)]
        tol = 4 * EPS32 * (1.0 + mag[ok]) + 1e-7 + (NORMAL_ROUNDING if name == "normal" else 0.0)
        value = (g[ok].astype(np.float64) + 1.0) / 2.0 if name == "normal" else g[ok].astype(np.float64)
        err = np.abs(value - want).max(1)
        if len(err):
            worst = max(worst, float((err / tol).max()))
        assert (err <= tol).all(), f"{label} {name}: error / tolerance {float((err / tol).max()):.3g} against binary64"
    return worst
