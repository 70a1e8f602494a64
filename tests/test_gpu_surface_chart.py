"""GPU: the light loop (`light_surface`, csrc/bb_kernels.hip.h) on hazard surfaces -- guards, clamps, light lists.

tests/surface_chart.py builds 128 x 128 frames whose pixels are a chosen surface population; every frame rendered here is
held against three references, and its inputs are counted (the numbers 1-4 return in the checks' names and messages):
  1  the whole pipeline: frame, winning primitive, depth bits, n_shaded (deferred: G-buffer texels too) equal the oracle's
  2  the loop alone: the frame equals the oracle's light loop on the values the kernel itself dumped (bbr_read_surface;
     deferred: bbr_read_gbuffer) -- together with 1 this separates a slip in the loop from one in front of it
  3  set a only: the GPU's colour against the GLSL typed in binary64 (tests/test_oracle_contract.py), on the dumped inputs,
     within that file's own bounds -- the one comparison that does not pass through the oracle
  4  a census in binary64 on the dumped inputs, so that no hazard test passes vacuously
"equal": NaN in the same pixels and channels, every other value bit-equal, +-inf and the sign of zero included (x86 and
the GPU produce different default NaNs: sign and payload are not part of the contract).

Every case is one or two frames of 16 384 pixels; the whole file's wall time is recorded in tests/golden/surface_chart.json."""
import functools
import json
import os
from types import SimpleNamespace

import numpy as np
import pytest

import surface_chart as SC
from conftest import GOLDEN
from test_oracle_contract import BOUND_EPS, WELL, conditioning, glsl_f64_light_loop, rel_err
from bibim_renderer_amd import Renderer
from oracle import bbo, scenes

pytestmark = pytest.mark.gpu

W, H = SC.W, SC.H
equal = SC.equal_but_for_nan_payload
bits = SC.bits
PIX_POINT, PIX_SPOT, PIX_VIEW = 40 * W + 50, 90 * W + 30, 64 * W + 100     # pixels whose P a light / the viewer is put at
pass_id = lambda d: "deferred" if d else "forward"


# ---------------------------------------------------------------------------------------------------------------------
# frames
# ---------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(None)
def draws(name, s=1.0, min_roughness=0):
    return SC.chart(name, s, min_roughness)


FRAMES_IN_FLIGHT = 2


def gpu(sc, deferred=0, before=None, **opts):
    """one frame and its read-backs; `before`: a scene every frame slot renders first"""
    r = Renderer(W, H)
    r.set_option("render_pass", deferred)
    r.set_option("frames_in_flight", FRAMES_IN_FLIGHT)
    for k, v in opts.items():
        r.set_option(k, v)
    if before is not None:
        h = None
        for _ in range(FRAMES_IN_FLIGHT + 1):       # every slot has seen it, whichever slot the next frame takes
            h = r.render_scene(before, h)
    r.render_scene(sc)
    g = SimpleNamespace(deferred=deferred, fused=bool(opts.get("present_fused")))
    if g.fused:
        r.present()
        g.presented = r.read_presented()
        g.frame = None
    else:
        g.frame = r.read_framebuffer()
    g.prim, g.depth = r.read_visibility()
    g.stats = r.stats()
    g.surf = r.read_surface()
    g.gbuf = r.read_gbuffer() if deferred else None
    again = r.read_presented() if g.fused else r.read_framebuffer()      # the dumps re-render the frame: the same bits
    r.close()
    assert np.array_equal(again, g.presented) if g.fused else equal(again, g.frame)
    g.inputs = SC.gbuffer_values(g.gbuf) if deferred else SC.surface_values(g.surf)   # what the light loop was handed
    return g


def oracle_of(sc, deferred):
    if deferred:
        ref, gbuf, prim, depth, st = bbo.render_deferred(sc)
    else:
        ref, prim, depth, st = bbo.render(sc)
        gbuf = None
    return SimpleNamespace(frame=ref, gbuf=gbuf, prim=prim, depth=depth, stats=st)


def check_1_and_2(sc, g, where=None):
    """assertion 1 (whole pipeline against the oracle) and 2 (the loop alone on the kernel's own dump); `where`: the pixels
    assertion 1 holds the colour on (all by default)"""
    o = oracle_of(sc, g.deferred)
    assert (o.prim != bbo.NO_PRIM).all(), "the chart does not cover the frame"
    assert np.array_equal(g.prim, o.prim), f"{int((g.prim != o.prim).sum())} pixels pick another primitive"
    assert np.array_equal(bits(g.depth), bits(o.depth))
    assert g.stats["n_shaded"] == o.stats["n_shaded"] == W * H
    assert g.stats["n_clipped_prims"] == o.stats["n_clipped_prims"]
    lit = bbo.light_surface(sc.frame, sc.view, g.inputs, literal=False).reshape(H, W, 4)
    if g.fused:
        tone, exposure = int(sc.frame["enable_tone_mapping"]), float(sc.frame["exposure"])
        assert np.array_equal(g.presented, bbo.present(o.frame, tone, exposure)), "1: presented bytes"
        assert np.array_equal(g.presented, bbo.present(lit, tone, exposure)), "2: presented bytes of the loop on the dump"
        return o
    if g.deferred and where is None:
        assert equal(g.gbuf, o.gbuf), "1: G-buffer texels differ"
    sel = slice(None) if where is None else where
    assert equal(g.frame[sel], o.frame[sel]), f"1: the frame is not the oracle's ({mismatch(g.frame[sel], o.frame[sel])})"
    assert equal(g.frame, lit), f"2: the frame is not the oracle's loop on the dumped surface ({mismatch(g.frame, lit)})"
    return o


def mismatch(got, want):
    ng, nw = np.isnan(got), np.isnan(want)
    diff = (ng != nw) | (~nw & ~ng & (bits(got) != bits(want)))
    return f"{int(diff.any(-1).sum())} pixels differ, {int((ng != nw).sum())} values NaN on one side only"


@functools.lru_cache(None)
def first_pass(name, deferred):
    """the P the light loop is handed at every pixel, [n, 3]: from a first frame under set a"""
    lights, view = SC.set_a()
    g = gpu(SC.scene(name, lights, view, draws=draws(name)), deferred)
    return np.ascontiguousarray(g.inputs[:, 0:3])


def antipodal_pixel(P):
    found = np.flatnonzero(SC.antipodal_pixels(P))
    assert len(found) >= 1, "no pixel with f32(Q - P) == -f32(view - P)"
    return int(found[len(found) // 2])


# ---------------------------------------------------------------------------------------------------------------------
# the sets
# ---------------------------------------------------------------------------------------------------------------------
CASES = (["a", "b lights", "b view", "c", "d", "e"] + [f"f {c}" for c in SC.SPOT_CASES] + [f"g {c}" for c in SC.G_CASES]
         + [f"h {c}" for c in SC.H_CASES])
ALL_NAN = ("f dir = 0", "h inf - inf")          # a NaN cone factor / inf * 0 or inf - inf on every pixel: the frame is NaN, and must be


def build(case, name, deferred):
    """(scene, lights, view_pos, s) of a case"""
    s, min_roughness = 1.0, 0
    if case == "a":
        (lights, view), min_roughness = SC.set_a(), 6
    elif case.startswith("b"):
        P = first_pass(name, deferred)
        lights, view = SC.set_b(P[PIX_POINT], P[PIX_SPOT])
        if case == "b view":
            view = P[PIX_VIEW].copy()
    elif case == "c":
        P = first_pass(name, deferred)
        lights, view = SC.set_c(P[antipodal_pixel(P)])
    elif case == "d":
        (lights, view), s = SC.set_d(), SC.S_TINY
    elif case == "e":
        (lights, view), s = SC.set_e(), SC.S_HUGE
    elif case.startswith("f "):
        lights, view = SC.set_f(case[2:])
    elif case.startswith("g "):
        lights, view = SC.set_g(case[2:])
    else:
        lights, view = SC.set_h(case[2:])
    return SC.scene(name, lights, view, s, draws=draws(name, s, min_roughness)), lights, view, s


@pytest.mark.parametrize("case", CASES)
@pytest.mark.parametrize("deferred", [0, 1], ids=pass_id)
@pytest.mark.parametrize("name", SC.CHARTS)
def test_light_set(name, deferred, case):
    sc, lights, view, s = build(case, name, deferred)
    g = gpu(sc, deferred)
    o = check_1_and_2(sc, g)
    ref = o.frame.reshape(-1, 4)
    surf = SC.surface_values(g.surf)           # the census is taken on the binary32 values (deferred: before the binary16 store)
    c = SC.check_census(case, name, surf, lights, view)
    finite = np.isfinite(ref[:, :3]).all(-1)
    print(f"{name} {pass_id(deferred)} {case}: {finite.mean():.1%} finite pixels, {np.isnan(ref).any(-1).mean():.1%} with a NaN; "
          f"roughness 0 {c['roughness_0']:.1%}, N.V < 0 {c['ndv_negative']:.1%}, N.L < 0 {c['ndl_negative_some_light']:.1%}")
    # -- 4. census --
    if case in ALL_NAN:
        assert np.isnan(ref[:, :3]).all()
    elif case == "h overflowing radiance":
        assert not finite.any() and (ref[:, :3] == np.inf).all(-1).mean() >= 0.01 and np.isnan(ref[:, :3]).all(-1).mean() >= 0.25
    elif not (deferred and case in ("d", "e")):      # (the G-buffer's binary16 P is 0 / inf in the tiny / huge world)
        assert finite.mean() >= 0.5, "the frame says little: most pixels are not finite"
    P = g.inputs[:, 0:3]
    if case.startswith("b"):
        assert np.array_equal(bits(P), bits(first_pass(name, deferred))), "P changed between the passes"
        assert np.array_equal(bits(lights[1]["pos"]), bits(P[PIX_POINT])) and np.array_equal(bits(lights[2]["pos"]), bits(P[PIX_SPOT]))
        assert np.isnan(ref[PIX_POINT, :3]).all() and np.isnan(ref[PIX_SPOT, :3]).all()      # 0 * inf
        if case == "b view":
            assert np.array_equal(bits(sc.view["view_pos"]), bits(P[PIX_VIEW]))
            assert np.isfinite(ref[PIX_VIEW]).all()
    if case == "c":
        assert np.array_equal(bits(P), bits(first_pass(name, deferred)))
        at = antipodal_pixel(P)
        q, v = SC.f32(lights[0]["pos"]), SC.f32(sc.view["view_pos"])
        assert np.array_equal(bits(q - P[at]), bits(-(v - P[at]))) and (q != P[at]).any(), "L = -V does not hold bit for bit"
        assert np.isfinite(ref[at]).all()
    if case == "g no lights":
        assert int(sc.frame["num_lights"]) == 0
        amb = (np.float32(0.03) * g.inputs[:, 6:9]) * g.inputs[:, 11:12]     # fp32: fma(0.03 albedo, ao, +0) is this rounded product
        assert amb.dtype == np.float32 and np.array_equal(bits(g.frame.reshape(-1, 4)[:, :3]), bits(amb)), "only the ambient term"
    if case in ("g unknown first", "g unknown last", "g two unknown in a row"):
        known = [l for l in lights if l["type"] in (0, 1, 2)]
        plain = SC.scene(name, known, view, draws=draws(name))
        assert len(known) == 4 and equal(g.frame, oracle_of(plain, deferred).frame), "an unknown type contributes"
    if case == "g only unknown":
        plain = SC.scene(name, [], view, draws=draws(name))
        assert equal(g.frame, oracle_of(plain, deferred).frame)
    # -- 3. against the GLSL in binary64 --
    if case == "a":
        args = SC.glsl_args(lights, view, g.inputs)
        want = glsl_f64_light_loop(*args)
        h = conditioning(args[0], args[1], args[2], args[3], args[6])
        err = rel_err(g.frame.reshape(-1, 4)[:, :3].astype(np.float64), want)
        well = h >= WELL
        bound = 1e-5 + BOUND_EPS / h
        worst = float((err / bound).max())
        print(f"  3: {name} {pass_id(deferred)}: {well.mean():.1%} well conditioned, worst well-conditioned error {err[well].max():.3g}, "
              f"worst error / bound {worst:.4g}")
        assert np.isfinite(want).all() and well.mean() >= 0.5
        assert err[well].max() <= 1e-5
        assert (err <= bound).all()
        recorded = json.load(open(os.path.join(GOLDEN, "surface_chart.json")))["gpu"]["worst_error_over_bound"][f"{name} {pass_id(deferred)}"]
        assert abs(worst - recorded) <= 0.05 * recorded, f"the record says {recorded} (tools/surface_chart_record.py rewrites it)"


@pytest.mark.parametrize("deferred", [0, 1], ids=pass_id)
def test_specular_peak_with_a_zero_denominator(deferred):
    """set i on the chart "peak": the GGX denominator is exactly 0 under a non-zero numerator on hundreds of pixels, the one
    way into bb_rcp's guard at `S` with a result that is not NaN anyway (S = +inf)"""
    lights, view = SC.set_i()
    sc = SC.scene("peak", lights, view, draws=draws("peak"))
    g = gpu(sc, deferred)
    o = check_1_and_2(sc, g)
    rgb = o.frame.reshape(-1, 4)[:, :3]
    n_inf, n_nan = int((rgb == np.inf).all(-1).sum()), int(np.isnan(rgb).any(-1).sum())
    print(f"peak {pass_id(deferred)}: {n_inf} pixels +inf, {n_nan} with a NaN")
    rough = SC.surface_values(g.surf)[:, 10]
    assert (rough > 0).all() and (rough <= 3.001 / 255).all()
    assert n_inf >= 100 and n_nan <= 100 and np.isfinite(rgb).all(-1).mean() >= 0.5


# ---------------------------------------------------------------------------------------------------------------------
# every call site of the loop, on one combined hazard scene
# ---------------------------------------------------------------------------------------------------------------------
SITES = {"forward 32x32": (0, {"tile_mode": 1}), "forward 64x64": (0, {"tile_mode": 0}), "deferred": (1, {}),
         "present_fused": (0, {"present_fused": 1}), "tail launch": (0, {"no_tail_items": 0}),
         "max_anisotropy 16": (0, {"max_anisotropy": 16})}


@pytest.mark.parametrize("site", list(SITES))
@pytest.mark.parametrize("name", SC.CHARTS)
def test_call_sites_on_the_combined_hazard_scene(name, site):
    deferred, opts = SITES[site]
    P = first_pass(name, deferred)
    at = antipodal_pixel(P)
    lights, view = SC.hazard_set(P[PIX_POINT], P[PIX_SPOT], P[at])
    sc = SC.scene(name, lights, view, draws=draws(name))
    sc.frame["enable_tone_mapping"], sc.frame["exposure"] = 1, 1.25
    # tail launch: the long route sizes its main launch from the frame the slot rendered before -- a near-empty one here, so
    # that nearly all of the chart's items are left to the tail
    before = scenes.triangle_scene(W, H) if site == "tail launch" else None
    g = gpu(sc, deferred, before, **opts)
    where = None
    if site == "max_anisotropy 16":
        where = (g.surf[..., 22:28] <= 1).all(-1)
        print(f"{name}: {int(where.sum())} one-tap pixels")
        # (clipped: a quarter; u reaches 40 on the extended quad and its rounding puts the footprint above one texel elsewhere)
        assert where.sum() >= (W * H // 8 if name == "clipped" else W * H)
    o = check_1_and_2(sc, g, where)
    ref = o.frame.reshape(-1, 4)
    if name == "clipped":
        assert g.stats["n_clipped_prims"] >= 1
    assert len(lights) == 8
    assert np.array_equal(bits(P), bits(g.inputs[:, 0:3]))
    assert np.isnan(ref[PIX_POINT, :3]).all() and np.isnan(ref[PIX_SPOT, :3]).all() and np.isfinite(ref[at]).all()
    assert np.isfinite(ref[:, :3]).all(-1).mean() >= 0.9
