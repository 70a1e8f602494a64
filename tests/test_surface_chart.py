"""CPU side of the surface charts (tests/surface_chart.py; the GPU side is tests/test_gpu_surface_chart.py).

  * the charts are what they claim: every pixel covered, the planned primitive counts, the clipped chart clips, and the
    binary64 model of a chart's surface agrees with what the oracle shades
  * the census conditions hold on the ORACLE's frames, on the modelled surface (no surface read-back on this side): the
    seeds in surface_chart.SEEDS were chosen here
  * the oracle's semantics at each hazard, on hand-built surfaces through bbo.light_surface
  * assertion 3 (the colour against the GLSL in binary64) on the oracle alone, on the charts' population"""
import json
import os

import numpy as np
import pytest

import surface_chart as SC
from conftest import GOLDEN
from test_oracle_contract import BOUND_EPS, WELL, conditioning, glsl_f64_light_loop, rel_err
from oracle import bbo

W, H = SC.W, SC.H
STATIC_CASES = (["a", "d", "e"] + [f"f {c}" for c in SC.SPOT_CASES] + [f"g {c}" for c in SC.G_CASES] + [f"h {c}" for c in SC.H_CASES])


def static_case(case, name):
    s, min_roughness = 1.0, 0
    if case == "a":
        (lights, view), min_roughness = SC.set_a(), 6
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
    return SC.scene(name, lights, view, s, min_roughness), lights, view, s


# ---------------------------------------------------------------------------------------------------------------------
# construction
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("s", [1.0, SC.S_TINY, SC.S_HUGE], ids=["s=1", "tiny", "huge"])
@pytest.mark.parametrize("name", SC.CHARTS)
def test_chart_construction(name, s):
    lights, view = SC.set_a(s)
    sc = SC.scene(name, lights, view, s)
    ref, prim, depth, st = bbo.render(sc)
    assert (prim != bbo.NO_PRIM).all(), "a pixel is not covered"
    assert st["n_shaded"] == W * H and st["n_prims"] == sc.n_prims == SC.planned_prims(name)
    assert (st["n_clipped_prims"] >= 1) == (name == "clipped")
    assert 0.25 <= depth.min() and depth.max() <= 0.75
    for m in (sc.view["proj"], sc.draws[0].vertices["pos"]):
        assert np.isfinite(m).all() and (np.abs(m[m != 0]) >= 2.0 ** -126).all()       # s is exact in every entry
    if name in ("fine", "mixed"):                       # a wave's 64 fragments come from eight triangles: 4 x 4 pixel quads
        quads = prim.reshape(32, 4, 32, 4) // 2
        assert (quads == quads[:, :1, :, :1]).all() and len(np.unique(prim)) == 2048
    prim2 = bbo.render_deferred(sc, want_gbuffer=False)[2]
    assert np.array_equal(prim, prim2)


@pytest.mark.parametrize("name", SC.CHARTS)
def test_the_modelled_surface_is_what_the_oracle_shades(name):
    """orientation of the pixel grid, texel addressing and the TBN product of surface_chart.model_surface: the oracle's
    loop on the model against the oracle's frame (not bit for bit: the model is binary64 and affine)"""
    lights, view = SC.set_a()
    sc = SC.scene(name, lights, view, min_roughness=6)
    ref, prim, _, _ = bbo.render(sc)
    lit = bbo.light_surface(sc.frame, sc.view, SC.model_surface(sc, prim), literal=False).reshape(H, W, 4)
    err = np.abs(lit - ref).max(-1) / np.maximum(np.abs(ref).max(-1), 1e-6)
    # mixed: the 48 x 80 ao map is filtered where the model takes one texel; ao enters the ambient term 0.03 albedo ao only
    share = (err <= (0.1 if name == "mixed" else 1e-3)).mean()
    assert share >= 0.97, share


# ---------------------------------------------------------------------------------------------------------------------
# census on the oracle's frames
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", STATIC_CASES)
@pytest.mark.parametrize("name", SC.CHARTS)
def test_census_on_the_oracle(name, case):
    sc, lights, view, s = static_case(case, name)
    ref, prim, _, _ = bbo.render(sc)
    surf = SC.model_surface(sc, prim, s)
    c = SC.check_census(case, name, surf, lights, view)
    ref = ref.reshape(-1, 4)
    finite = np.isfinite(ref[:, :3]).all(-1).mean()
    if case == "f dir = 0":
        assert np.isnan(ref[:, :3]).all()
    elif case == "h overflowing radiance":      # inf inside the cone where N.L > 0, inf * 0 = NaN everywhere else: no finite pixel
        assert finite == 0 and (ref[:, :3] == np.inf).all(-1).mean() >= 0.01 and np.isnan(ref[:, :3]).all(-1).mean() >= 0.25
    elif case == "h inf - inf":                 # inf * 0 where one light's N.L is 0, inf - inf where both are positive
        assert np.isnan(ref[:, :3]).all()
    else:
        assert finite >= 0.5, finite
    if case == "h negative intensity":
        assert (ref[:, :3] < 0).any()
    if case == "h denormal radiance":
        fu = sc.frame["lights"][1]
        ci = fu["color"] * fu["intensity"]
        assert (ci > 0).all() and (ci < 2.0 ** -126).all()
    recorded = json.load(open(os.path.join(GOLDEN, "surface_chart.json")))["census"].get(f"{name} {case}")
    if recorded is not None:
        for k, v in recorded.items():
            assert np.allclose(c[k], v, atol=0.02), (k, c[k], v)


def test_the_peak_chart_has_pixels_with_a_zero_denominator():
    """census of set i: S = x / 0 = +inf (not NaN) on hundreds of pixels, both passes"""
    lights, view = SC.set_i()
    sc = SC.scene("peak", lights, view)
    ref, prim, _, st = bbo.render(sc)
    assert (prim != bbo.NO_PRIM).all() and st["n_prims"] == SC.planned_prims("peak")
    for frame in (ref, bbo.render_deferred(sc, want_gbuffer=False)[0]):
        rgb = frame.reshape(-1, 4)[:, :3]
        assert (rgb == np.inf).all(-1).sum() >= 100 and np.isnan(rgb).any(-1).sum() <= 100
        assert np.isfinite(rgb).all(-1).mean() >= 0.5
    rough = SC.model_surface(sc, prim)[:, 10]
    assert (rough > 0).all() and (rough <= 3 / 255).all()


def test_antipodal_and_coincident_pixels_exist_on_the_charts():
    for name in ("fine", "coarse"):
        lights, view = SC.set_a()
        sc = SC.scene(name, lights, view)
        prim = bbo.render(sc)[1]
        P = SC.f32(SC.model_surface(sc, prim)[:, :3])
        found = np.flatnonzero(SC.antipodal_pixels(P))
        assert len(found) >= 1
        at = found[len(found) // 2]
        lights, view = SC.set_c(P[at])
        surf = SC.f32(SC.model_surface(sc, prim))
        fu, vu = SC.uniforms(lights, view, 1.0, 0)
        out = bbo.light_surface(fu, vu, surf[at:at + 1], literal=False)
        assert np.isfinite(out).all()


# ---------------------------------------------------------------------------------------------------------------------
# the oracle's semantics at each hazard, on hand-built surfaces
# ---------------------------------------------------------------------------------------------------------------------
def surface(P=(0.5, -0.25, 0.75), normal=(0.2, 0.3, -1.0), albedo=(0.8, 0.5, 0.3), metallic=0.25, roughness=0.5, ao=0.75):
    return SC.f32([list(P) + list(normal) + list(albedo) + [metallic, roughness, ao]])


def lit(lights, view, surf, literal=False):
    fu, vu = SC.uniforms(lights, view, 1.0, 0)
    return bbo.light_surface(fu, vu, surf, literal=literal)[0]


VIEW = SC.f32((0.5, -1.0, -7.0))
PLAIN = SC.L(0, pos=(1.0, 2.0, -6.0), color=(1.0, 0.9, 0.8), intensity=50.0)


@pytest.mark.parametrize("literal", [False, True], ids=["contract", "literal"])
def test_oracle_semantics_at_the_hazards(literal):
    s = surface()
    P = s[0, :3]
    base = lit([PLAIN], VIEW, s, literal)
    assert np.isfinite(base).all() and (base[:3] > 0).all()
    # a light at P: att = inf, L = 0 * inf -> NaN
    assert np.isnan(lit([PLAIN, SC.L(0, pos=P, intensity=3.0)], VIEW, s, literal)[:3]).all()
    assert np.isnan(lit([SC.L(1, pos=P, dir=(0, 0, 1), intensity=3.0, inner=0.9, outer=0.5)], VIEW, s, literal)[:3]).all()
    # the viewer at P: V = NaN, every clamped cosine of it 0 -> finite
    assert np.isfinite(lit([PLAIN], P, s, literal)).all()
    # L = -V exactly: H = normalize(0) = NaN, max(N.H, 0) = 0 and saturate(H.V) = 0 -> finite
    assert SC.antipodal_pixels(P)[0]
    anti = lit([SC.L(0, pos=P + SC.D_ANTI, intensity=4.0)], P - SC.D_ANTI, s, literal)
    assert np.isfinite(anti).all()
    # spot edges
    spot = lambda **k: SC.L(1, pos=(1.0, -0.5, -3.0), color=(1.0, 0.8, 0.6), intensity=150.0, **k)
    eq = lit([spot(dir=SC.SPOT_DIR, inner=0.9375, outer=0.9375)], VIEW, s, literal)
    assert np.isfinite(eq).all()
    assert np.isnan(lit([spot(dir=(0, 0, 0), inner=0.96, outer=0.8)], VIEW, s, literal)[:3]).all()
    # radiance ends
    pair = [SC.L(2, dir=(0.5, 0.25, 1.0), color=(1e30,) * 3, intensity=1e30), SC.L(2, dir=(0.5, 0.25, 1.0), color=(1e30,) * 3, intensity=-1e30)]
    assert np.isnan(lit(pair, VIEW, s, literal)[:3]).all()
    assert (lit(pair[:1], VIEW, s, literal)[:3] == np.inf).all()
    # unknown types first and last: the same as without them, bit for bit
    u = SC.L(SC.UNKNOWN, pos=(0, 0, -6), dir=(0, 0, 1), color=(9, 9, 9), intensity=1000.0, inner=0.9, outer=0.5)
    for lights in ([u, PLAIN], [PLAIN, u], [u, u, PLAIN, u], ):
        assert np.array_equal(SC.bits(lit(lights, VIEW, s, literal)), SC.bits(base))
    amb = lit([u, u], VIEW, s, literal)
    assert np.array_equal(SC.bits(amb), SC.bits(lit([], VIEW, s, literal)))
    assert np.array_equal(SC.bits(amb[:3]), SC.bits((np.float32(0.03) * s[0, 6:9]) * s[0, 11]))


def test_equality_rule_ignores_only_the_nan_payload():
    a = SC.f32([0.0, 1.0, np.inf, np.nan])
    b = a.copy(); b.view(np.uint32)[3] ^= 0x80000001           # another NaN
    assert SC.equal_but_for_nan_payload(a, b)
    for i, v in ((0, -0.0), (1, np.nextafter(np.float32(1), np.float32(2))), (2, -np.inf), (3, 0.0), (0, np.nan)):
        c = a.copy(); c[i] = v
        assert not SC.equal_but_for_nan_payload(a, c), i


# ---------------------------------------------------------------------------------------------------------------------
# assertion 3 on the oracle alone
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", SC.CHARTS)
def test_oracle_against_the_glsl_in_binary64_on_the_charts_population(name):
    sc, lights, view, _ = static_case("a", name)
    prim = bbo.render(sc)[1]
    surf = SC.f32(SC.model_surface(sc, prim))
    args = SC.glsl_args(lights, view, surf)
    want = glsl_f64_light_loop(*args)
    h = conditioning(args[0], args[1], args[2], args[3], args[6])
    bound = 1e-5 + BOUND_EPS / h
    well = h >= WELL
    assert np.isfinite(want).all() and well.mean() >= 0.5, well.mean()
    worst = 0.0
    for literal in (True, False):
        got = bbo.light_surface(sc.frame, sc.view, surf, literal=literal)[:, :3].astype(np.float64)
        err = rel_err(got, want)
        print(f"{name} literal={literal}: {well.mean():.1%} well conditioned, worst well-conditioned error {err[well].max():.3g}, "
              f"worst error / bound {(err / bound).max():.3g}")
        assert err[well].max() <= 1e-5
        assert (err <= bound).all()
        worst = max(worst, float((err / bound).max()))
    rec = json.load(open(os.path.join(GOLDEN, "surface_chart.json")))
    assert rec["seeds"] == SC.SEEDS and rec["frame"] == [W, H]
    assert set(rec["oracle"]["worst_error_over_bound"]) == set(SC.CHARTS)
    assert set(rec["gpu"]["worst_error_over_bound"]) == {f"{c} {p}" for c in SC.CHARTS for p in ("forward", "deferred")}
    assert abs(rec["oracle"]["worst_error_over_bound"][name] - worst) <= 0.05 * worst + 1e-3
