"""GPU: k_geometry / k_raster against tests/raster_reference.py DIRECTLY (not via the oracle), through the C ABI: the scenes and
the assertion functions of tests/test_raster_reference.py -- primitive id and depth on every pixel the reference decides, the
exact layer bit for bit -- on the routes where the kernels choose differently: both tile shapes, the three item routes, the
every-tile list at both extremes, the bin-overflow replay, the deferred pass, and a 3-rank partition reassembled (a partitioned
context has no visibility read-back, so there the frame's alpha channel = coverage is what is compared, not id or depth).
The deferred pass is compared on the scenes whose view matrix is the identity -- the soups, the hostile inputs, the exact layer:
its vertex stage computes P (V p) where the forward one, which is what bbo.vertex_stage gives the reference, computes (P V) p,
and only there are the two the same binary32 numbers; C2, C3 and the camera-inside view go through the forward pass only.
The soups also go through the bit-exact comparison with the oracle: random slivers and sub-pixel triangles are shapes the
parity suite lacks."""
import numpy as np
import pytest

from bibim_renderer_amd import Renderer
from bibim_renderer_amd import partition as P
from oracle import bbo
import raster_reference as RR
import test_raster_reference as T

pytestmark = pytest.mark.gpu

OPTIONS = [{"tile_mode": 0}, {"tile_mode": 1}, {"broad_threshold": 1}, {"broad_threshold": 100000}, {"bin_cap": 8},
           {"render_pass": 1}]


def gpu_visibility(scene, **opts):
    r = Renderer(scene.width, scene.height)
    for k, v in opts.items():
        r.set_option(k, v)
    r.render_scene(scene)
    prim, depth = r.read_visibility()
    st = r.stats()
    r.close()
    return prim, depth, st


def same_clip_coordinates_in_both_passes(scene):
    """the deferred vertex stage computes P (V p), the forward one (P V) p: the same binary32 numbers when V is the identity"""
    return np.array_equal(np.abs(scene.view["view"]), np.eye(4, dtype=np.float32))


@pytest.mark.parametrize("name", list(T.MARGIN_SCENES))
def test_margin_layer_gpu_item_routes(name, item_route_heavy):
    sc = T.MARGIN_SCENES[name]()
    prim, depth, st = gpu_visibility(sc)
    T.margin_check(name, sc, prim, depth, st)


@pytest.mark.parametrize("name", list(T.MARGIN_SCENES))
def test_margin_layer_gpu_options(name):
    sc = T.MARGIN_SCENES[name]()
    for opts in OPTIONS:
        if "render_pass" in opts and not same_clip_coordinates_in_both_passes(sc):
            continue   # (module docstring: the reference has the forward vertex stage's clip coordinates)
        prim, depth, st = gpu_visibility(sc, **opts)
        try:
            T.margin_check(name, sc, prim, depth, st)
        except AssertionError as e:
            raise AssertionError(f"with {opts}: {e}") from e


@pytest.mark.parametrize("name,tile_mode", [("soup 333x207", 0), ("soup 1001x77", 1), ("C3 balls 480x270", 0)])
def test_margin_layer_gpu_partition_of_three_reassembled(name, tile_mode):
    """bands one tile high (a band is a whole number of tile rows), interleaved over three ranks"""
    sc = T.MARGIN_SCENES[name]()
    res = T.reference_of(name, sc)
    shards, n_shaded = [], 0
    for rank in range(3):
        r = Renderer(sc.width, sc.height)
        r.set_option("tile_mode", tile_mode)
        band_rows = r.tile_height()
        r.set_partition(rank, 3, band_rows)
        assert r.shard_rows() == P.shard_rows(sc.height, 3, band_rows)
        r.render_scene(sc)
        shards.append(r.read_shard())
        n_shaded += r.stats()["n_shaded"]
        r.close()
    frame = P.unpack_gathered(np.stack(shards), sc.height, band_rows)
    covered = frame[..., 3] == 1.0
    assert ((frame[..., 3] == 0.0) | covered).all()
    assert 1.0 - res.decided.mean() <= RR.MAX_UNDECIDED
    wrong = res.decided & (covered != (res.winner != RR.NONE))
    assert not wrong.any(), f"{int(wrong.sum())} decided pixels covered / empty against the reference"
    assert n_shaded == covered.sum()


@pytest.mark.parametrize("size", [s for s in T.SOUPS], ids=lambda s: f"{s[0]}x{s[1]}")
def test_soups_bit_exact_against_the_oracle(size, item_route):
    from test_gpu_parity import check
    sc = T.soup_scene(*size)
    check(sc)
    check(sc, tile_mode=1)


def test_clipped_primitives_alone_gpu():
    sc = T.soup_scene(416, 240, 2)
    clip, _ = RR.scene_primitives(sc)
    seen = 0
    for p in np.nonzero(~RR.all_in(clip))[0].tolist():
        one = T.single_primitive_scene(sc, p)
        prim, depth, st = gpu_visibility(one)
        covered = prim != bbo.NO_PRIM
        assert st["n_shaded"] == covered.sum()
        res = RR.rasterise(one, want_uv=False)
        sure = res.winner == 0
        assert covered[sure].all(), f"primitive {p}: {int((sure & ~covered).sum())} surely covered pixels missed"
        RR.check_visibility(res, prim, depth)
        seen += bool(sure.any())
    assert seen >= 8, seen


@pytest.mark.parametrize("perspective", [False, True], ids=["w=1", "w in 1,2,4"])
@pytest.mark.parametrize("opts", [{"tile_mode": 0}, {"tile_mode": 1}, {"render_pass": 1}, {"bin_cap": 8}, {"broad_threshold": 1}],
                         ids=lambda o: " ".join(f"{k}={v}" for k, v in o.items()))
def test_exact_layer_gpu(perspective, opts, item_route_heavy):
    sc, _, _ = T.exact_scene(perspective)
    prim, depth, st = gpu_visibility(sc, **opts)
    T.exact_check(perspective, prim, depth, st)


@pytest.mark.parametrize("tile_mode", [0, 1])
def test_exact_layer_fan_and_clamp_gpu(tile_mode):
    fan, once = T.fan_scene()
    prim, _, st = gpu_visibility(fan, tile_mode=tile_mode)
    assert np.array_equal(prim != bbo.NO_PRIM, once == 1) and st["n_shaded"] == once.sum()
    prim, depth, st = gpu_visibility(T.clamp_scene(), tile_mode=tile_mode)
    T.clamp_check(prim, depth, st)
    sc, model = T.clamp_overshoot_scene()
    prim, depth, st = gpu_visibility(sc, tile_mode=tile_mode)
    assert st["n_raster_tris"] == 64
    T.clamp_overshoot_check(prim, depth, model)
