"""GPU: bbr_set_option as a whole -- every name it knows, what it accepts and refuses, and what a call makes the frame slots
forget (options "sky_keep" and "view_keep"; include/bibim_hip.h).

The frame is the smallest with both kinds of tile: 64 x 64 at the default 32 x 32 tiles, tests/test_gpu_sky_keep.py's triangle
on tile (0, 0) and three tiles of background, two frames in flight, the forward path.  The expectations are the literal tables
below, taken from the library as it stood before bbr_set_option became a table of its own: a row of that table which states a
range, a flag or a refusal differently shows here.  One row is not that library's: "ablate" 1 on a normal build.  It was meant to
be refused ("diagnostic builds only") and was accepted, because the `#ifdef` in front of the refusal saw the function-like
macro of the same name that the kernel header defines in every build; the chart holds what was meant.

VALUES   per name: the accepted range (None: unbounded on that side; a set for "depth_resolve") and the default.  On a fresh
         context both edges are accepted, each followed by the default again; the nearest value outside each edge is refused
         with BBR_ERR_INVALID_ARGUMENT and a message that names the option.
FORGETS  per name: what the call does to a context in the steady state (each slot's frame kept, its background tiles kept) when
         it sets the value the option already has, and when it asks for a refused value: KEEPS -- the next frame of each slot
         is a kept one and reports its background tiles kept -- or FULL -- it is rendered in full and fills them.  Every frame
         is compared bit for bit with the CPU oracle's.

Cross-option refusals pinned elsewhere and not repeated: the pair "supersample" 3 / "sample_shading" 0 in both orders
(test_gpu_sample_shading.test_option_values_and_the_refused_pair), the pair "mip_levels" >= 2 / "shadow_map" > 0 in both orders
(test_gpu_shadow_map's option test), the render extent limit of "supersample" (test_gpu_supersample).  Pinned here, because
nowhere else: the three "between begin_frame and end_frame" refusals and "tile_mode" against a partition's band_rows."""
import numpy as np
import pytest

import test_gpu_sky_keep as SK
from bibim_renderer_amd import Renderer
from bibim_renderer_amd._capi import BibimError

INVALID = -1
W = H = 64
TILES = ((0, 0),)
FIF = 2
I64_MIN, I64_MAX = -2 ** 63, 2 ** 63 - 1

# name: (lowest accepted, highest accepted, default)
VALUES = {
    "gbuffer_view": (-1, 3, -1),
    "render_pass": (0, 1, 0),
    "timing": (0, 2, 0),
    "timing_stride": (1, 1024, 1),
    "frames_in_flight": (1, 4, 2),
    "tile_mode": (0, 1, 1),
    "bin_cap": (1, 1 << 20, 512),
    "ablate": (0, 0, 0),                      # (a normal build: 1 is for the diagnostic one)
    "max_anisotropy": (1, 16, 1),
    "mip_levels": (1, 15, 1),
    "supersample": (1, 4, 1),
    "sample_shading": (0, 1, 1),
    "depth_resolve": ({0, 1, 4, 8}, None, 0),
    "shadow_map": (0, 8192, 0),
    "shadow_filter": (0, 2, 0),
    "static_records": (0, 1, 1),
    "sky_keep": (0, 1, 1),
    "view_keep": (0, 1, 1),
    "present_fused": (None, None, 0),         # (any value: non-zero is on)
    "overlays": (None, None, 0),
    "tbn": (None, None, 0),
    "stream_layout": (0, 2, 2),
    "push_mode": (0, 1, 1),
    "no_tail_items": (0, None, 40000),
    "heavy_tiles": (-1, 1 << 24, -1),
    "broad_cap": (1, 1 << 24, 4096),
    "clip_cap": (1, 1 << 24, 4096),
    "broad_threshold": (1, None, 16),
}

KEEPS, FULL = "keeps", "full"
# name: (a refused value or None where there is none, after setting the value it has, after the refused value)
FORGETS = {
    "gbuffer_view": (4, KEEPS, KEEPS),        # the two calls that do not wait for the GPU: nothing is forgotten
    "render_pass": (2, KEEPS, KEEPS),
    "timing": (3, KEEPS, KEEPS),
    "timing_stride": (0, KEEPS, KEEPS),
    "frames_in_flight": (5, FULL, FULL),
    "tile_mode": (2, FULL, FULL),
    "bin_cap": (0, FULL, FULL),
    "ablate": (1, FULL, FULL),
    "max_anisotropy": (17, KEEPS, KEEPS),
    "mip_levels": (16, FULL, KEEPS),          # (an accepted value starts a new resource epoch: the draws are new ones)
    "supersample": (5, FULL, FULL),
    "sample_shading": (2, FULL, FULL),
    "depth_resolve": (2, FULL, FULL),
    "shadow_map": (8193, KEEPS, KEEPS),
    "shadow_filter": (3, KEEPS, KEEPS),
    "static_records": (2, KEEPS, KEEPS),
    "sky_keep": (2, KEEPS, KEEPS),
    "view_keep": (2, KEEPS, KEEPS),
    "present_fused": (None, FULL, None),
    "overlays": (None, FULL, None),
    "tbn": (None, FULL, None),
    "stream_layout": (3, FULL, FULL),
    "push_mode": (2, KEEPS, KEEPS),
    "no_tail_items": (-1, FULL, FULL),
    "heavy_tiles": (-2, FULL, FULL),
    "broad_cap": (0, FULL, FULL),
    "clip_cap": (0, FULL, FULL),
    "broad_threshold": (0, FULL, FULL),
}
NAMES = list(VALUES)


def test_the_tables_name_the_same_options():
    assert len(NAMES) == 28 and list(FORGETS) == NAMES


def refused(r, name, value, *words):
    with pytest.raises(BibimError) as e:
        r.set_option(name, value)
    assert e.value.code == INVALID, e.value
    for word in (name,) + words:
        assert word in str(e.value), e.value


def accepted_and_refused(name):
    lo, hi, default = VALUES[name]
    if isinstance(lo, set):
        return sorted(lo), sorted({v + d for v in lo for d in (-1, 1)} - lo), default
    ok = [I64_MIN if lo is None else lo, I64_MAX if hi is None else hi]
    bad = ([] if lo is None else [lo - 1]) + ([] if hi is None else [hi + 1])
    return ok, bad, default


# ---- 1. values ----
@pytest.fixture(scope="module")
def fresh():
    r = Renderer(W, H)
    yield r
    r.close()


@pytest.mark.gpu
@pytest.mark.parametrize("name", NAMES)
def test_accepted_and_refused_values(fresh, name):
    r = fresh
    ok, bad, default = accepted_and_refused(name)
    for v in bad:
        refused(r, name, v)
    for v in ok:
        r.set_option(name, v)
        r.set_option(name, default)
    for v in bad:                             # (behind the accepted ones as in front of them)
        refused(r, name, v)


@pytest.mark.gpu
def test_an_unknown_name_is_refused(fresh):
    refused(fresh, "no_such_option", 0, "unknown option")
    refused(fresh, "", 0, "unknown option")


@pytest.mark.gpu
def test_refusals_between_begin_frame_and_end_frame(fresh):
    r = fresh
    r.begin_frame()
    for name in ("supersample", "sample_shading", "depth_resolve"):
        refused(r, name, VALUES[name][2], "between begin_frame and end_frame")
    r.end_frame()
    for name in ("supersample", "sample_shading", "depth_resolve"):
        r.set_option(name, VALUES[name][2])


@pytest.mark.gpu
def test_tile_mode_against_band_rows(fresh):
    r = fresh
    r.set_partition(0, 2, 32)
    refused(r, "tile_mode", 0, "band_rows")   # 32 rows are no multiple of 64
    r.set_option("tile_mode", 1)
    r.set_partition(0, 2, 64)
    r.set_option("tile_mode", 0)
    r.set_option("tile_mode", 1)
    r.set_partition(0, 1, 0)
    r.set_option("tile_mode", 0)
    r.set_option("tile_mode", 1)


# ---- 2. what a call forgets ----
BACKGROUND = {KEEPS: SK.KEPT, FULL: SK.FILLED}


class Steady:
    """one context, its handles, and frames of the one scene"""

    def __init__(self):
        self.r = Renderer(W, H)
        self.r.set_option("frames_in_flight", FIF)
        self.handles = {"mesh": {}, "mat": {}}

    def frame(self, what):
        """one frame -> KEEPS or FULL, from the counters; the tile report must say the same, the pixels are the oracle's"""
        c0 = self.r.view_keep_counts()
        got, tiles = SK.render(self.r, self.handles, W, H, TILES)
        c1 = self.r.view_keep_counts()
        kept, full = c1["kept"] - c0["kept"], c1["full"] - c0["full"]
        assert (kept, full) in ((1, 0), (0, 1)), (what, kept, full)
        kind = KEEPS if kept else FULL
        assert np.array_equal(SK.bits(got), SK.bits(SK.oracle(W, H, TILES))), f"{what}: pixels differ from the oracle"
        return kind, tiles.tolist()

    def settle(self, what):
        """to the steady state: each slot's third frame of a kind is kept, and keeps its background"""
        for k in range(3 * FIF):
            kind, tiles = self.frame(f"{what}, settling frame {k}")
        for k in range(FIF):
            kind, tiles = self.frame(f"{what}, steady frame {k}")
            assert kind == KEEPS and tiles == [SK.NONE, SK.KEPT, SK.KEPT, SK.KEPT], (what, k, kind, tiles)

    def after(self, what):
        """the next frame of each slot: (kind, background class), the same for every slot"""
        seen = set()
        for k in range(FIF):
            kind, tiles = self.frame(f"{what}, frame {k}")
            assert tiles[0] == SK.NONE and len(set(tiles[1:])) == 1, (what, k, tiles)
            seen.add((kind, tiles[1]))
        assert len(seen) == 1, (what, seen)
        return seen.pop()


@pytest.fixture(scope="module")
def steady():
    s = Steady()
    s.settle("first")
    yield s
    s.r.close()


@pytest.mark.gpu
@pytest.mark.parametrize("name", NAMES)
def test_what_a_call_forgets(steady, name):
    s = steady
    bad, want_same, want_refused = FORGETS[name]
    s.r.set_option(name, VALUES[name][2])     # the value it has
    got = s.after(f"{name} = {VALUES[name][2]}")
    s.settle(f"behind {name}")
    assert got == (want_same, BACKGROUND[want_same]), (name, "the value it has", got)
    if bad is None:
        return
    refused(s.r, name, bad)
    got = s.after(f"{name} = {bad} (refused)")
    s.settle(f"behind {name} refused")
    assert got == (want_refused, BACKGROUND[want_refused]), (name, "a refused value", got)
