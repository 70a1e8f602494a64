"""The exchange chart (tests/exchange_chart.py) on the CPU: is the model right, is the population what it claims to be, would a
wrong kernel be noticed.

  1  the model against bibim_renderer_amd/partition.py, the host-side description the older exchange tests use: blocks, block
     sizes, shard rows, ownership and the whole frame, on every case and form.  binary16 NaNs apart: numpy's conversion and the
     model's keep different payload bits, and no comparison anywhere looks at a NaN's payload
  2  the model's binary16 rounding against the oracle's (bbo.half_round, the contract of DESIGN.md) and against numpy's on the
     whole population, and its widening on all 65536 halves
  3  every mutant differs from the model on every case whose geometry lets it
  4  the census: conditions on the population, per case what that case answers for
  5  the pinned record tests/golden/exchange_chart.json (tools/exchange_chart_record.py rewrites it)"""
import json
import os

import numpy as np
import pytest

from bibim_renderer_amd import partition as P
from oracle import bbo
import exchange_chart as X

RECORD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "exchange_chart.json")
PARTITIONED = [n for n, c in X.CASES.items() if c.world > 1]


def same_halves_but_for_nan_payload(a, b):
    a, b = (np.ascontiguousarray(x).reshape(-1).view("<u2") for x in (a, b))
    na, nb = (a & 0x7FFF) > 0x7C00, (b & 0x7FFF) > 0x7C00
    return a.size == b.size and np.array_equal(na, nb) and np.array_equal(a[~na], b[~na])


def same_bits_but_for_nan_payload(a, b):
    a, b = (np.ascontiguousarray(x).reshape(-1).view(np.uint32) for x in (a, b))
    na, nb = X.is_nan_bits(a), X.is_nan_bits(b)
    return a.size == b.size and np.array_equal(na, nb) and np.array_equal(a[~na], b[~na])


# ---- 1: the model against partition.py ------------------------------------------------------------------------------
@pytest.mark.parametrize("name", X.CASES)
def test_1_model_is_partition_py(name):
    c = X.CASES[name]
    assert X.shard_rows(c) == P.shard_rows(c.height, c.world, c.band_rows)
    for rank in range(c.world):
        own = X.source_rows(c, rank)
        assert np.array_equal(own[own >= 0], P.owned_rows(c.height, rank, c.world, c.band_rows))
        assert X.padding_rows(c, rank) == X.shard_rows(c) - len(P.owned_rows(c.height, rank, c.world, c.band_rows))
    for form in X.FORMS:
        assert X.block_bytes(c, form) == P.exchange_block_bytes(form, c.height, c.width, c.world, c.band_rows)
        for rank in range(c.world):
            src = X.source_shard(name, form, rank)
            theirs = P.encode_block(src if form == X.RGBA8 else src.view(np.float32), form)
            mine = X.block(name, form, rank)
            assert mine.size == X.block_bytes(c, form)
            assert same_halves_but_for_nan_payload(mine, theirs) if form == X.RGBA16F else np.array_equal(mine, theirs), (form, rank)
        theirs = P.decode_gathered(X.gathered(name, form), form, c.height, c.width, c.world, c.band_rows)
        mine = X.whole(name, form)
        assert mine.shape == theirs.shape
        assert np.array_equal(mine, theirs) if form == X.RGBA8 else same_bits_but_for_nan_payload(mine, theirs), form
    theirs = P.decode_gathered(X.gathered16_hazard(name), X.RGBA16F, c.height, c.width, c.world, c.band_rows)
    assert same_bits_but_for_nan_payload(X.whole_frame(c, X.RGBA16F, X.gathered16_hazard(name)), theirs)


@pytest.mark.parametrize("name", X.CASES)
def test_1_ownership_and_un_interleave_are_inverse(name):
    """the two directions are written separately (source_rows from the ownership rule, place_of_row as the kernel walks): every
    framebuffer row is held exactly once, and the whole frame is made of the rows the shards say they hold"""
    c = X.CASES[name]
    held = np.concatenate([X.source_rows(c, r) for r in range(c.world)])
    assert sorted(held[held >= 0]) == list(range(c.height))
    frame = X.whole(name, X.RGBA32F)
    for rank in range(c.world):
        src = X.source_rows(c, rank)
        assert np.array_equal(frame[src[src >= 0]], X.shard(name, rank)[src >= 0])
        for row, y in enumerate(src):
            if y >= 0:
                assert X.place_of_row(c, int(y)) == (rank, row)


def test_1_cases_reach_their_edges():
    assert set(X.EDGES) == set(X.CASES)
    n = {k: X.shard_pixels(c) for k, c in X.CASES.items()}
    pad = {k: [X.padding_rows(c, r) for r in range(c.world)] for k, c in X.CASES.items()}
    assert (n["1x1"], n["63x1"], n["64x1"], n["65x1"], n["256x8"], n["2049x1"]) == (1, 63, 64, 65, 2048, 2049)
    assert X.packed_layout(1) == (32, 16)                                  # 12 bytes, pad 4, one word, pad 8
    assert n["333x211"] % 64 == 55 and 12 * n["333x211"] % 8 == 4
    assert X.shard_rows(X.CASES["7x33/2"]) == 32 and pad["7x33/2"] == [0, 31]            # the last band has one row
    assert X.shard_rows(X.CASES["3x32/3"]) == 64 and pad["3x32/3"] == [32, 64, 64]       # band >= height, two ranks own nothing
    assert X.n_bands(X.CASES["5x100/17"]) == 4 and pad["5x100/17"] == [0, 0, 0, 28] + [32] * 13
    assert X.n_bands(X.CASES["1x544/17"]) == 17 and pad["1x544/17"] == [0] * 17
    assert pad["64x65/4"] == [0, 0, 31, 32] and pad["333x211/3"] == [13, 32, 32]
    for k in PARTITIONED:                                                  # with a partition every block is whole 16-byte pieces
        assert n[k] % 32 == 0 and all(X.block_bytes(X.CASES[k], f) % 16 == 0 for f in X.FORMS)
    # more peers than one launch of the push kernel takes (kMaxPushPeers = 15): rank 9 of 17 wraps inside the first launch and
    # needs a second one for rank 8
    assert [(9 + k) % 17 for k in range(1, 17)] == P.push_order(9, 17) and P.push_order(9, 17)[15:] == [8]
    for form, (block, gather, whole) in X.ALIGN.items():                  # every block size keeps the form's alignment
        assert all(X.block_bytes(c, form) % max(block, gather) == 0 for c in X.CASES.values())


# ---- 2: the model's binary16 ------------------------------------------------------------------------------------------
def population_values():
    return np.unique(np.concatenate([X._pool(n).reshape(-1) for n in X.CASES] + [X.midpoints(), X.specials()]))


def test_2_rounding_is_the_oracles_and_numpys():
    u = population_values()
    assert u.size > 300000
    mine = X.widen_bits(X.half_bits(u))
    assert same_bits_but_for_nan_payload(mine, bbo.half_round(u.view(np.float32)))
    with np.errstate(over="ignore"):
        assert same_halves_but_for_nan_payload(X.half_bits(u), u.view(np.float32).astype(np.float16))


def test_2_widening_is_exact_on_every_half():
    h = np.arange(65536, dtype=np.uint16)
    assert same_bits_but_for_nan_payload(X.widen_bits(h), h.view(np.float16).astype(np.float32))
    finite = (h & 0x7FFF) < 0x7C00
    assert np.array_equal(X.half_bits(X.widen_bits(h[finite])), h[finite])        # and rounding is the identity on halves


def test_2_the_ties_are_ties():
    m = X.midpoints().reshape(2, -1, 3)
    assert m.shape[1] == 0x7C00 and X.is_tie(m[:, :, 1]).all() and not X.is_tie(m[:, :, 0]).any() and not X.is_tie(m[:, :, 2]).any()
    even = X.half_bits(m[0, :, 1])                                          # a tie goes to the even neighbour: 0x0000 .. 0x7C00
    assert np.array_equal(even, (np.arange(0x7C00) + 1) // 2 * 2)
    assert np.array_equal(X.half_bits(m[0, :, 0]), np.arange(0x7C00)) and np.array_equal(X.half_bits(m[0, :, 2]), np.arange(0x7C00) + 1)
    assert int(m[0, -1, 1]) == 0x477FF000 and int(m[0, 0, 1]) == 0x33000000


# ---- 3: the mutants ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mutant", X.MUTANTS)
def test_3_every_mutant_differs_from_the_model(mutant):
    cases = X.mutant_cases(mutant)
    assert cases, "no case can tell this mutant from the model"
    assert all(X.mutant_differs(mutant, n) for n in cases), [n for n in cases if not X.mutant_differs(mutant, n)]
    if X.MUTANTS[mutant].get("swap"):
        assert set(cases) == set(PARTITIONED) - {"3x32/3"}
    if X.MUTANTS[mutant].get("drop_padding"):
        assert set(cases) == set(PARTITIONED) - {"1x544/17"}


def test_3_each_rounding_mutant_is_told_apart_by_its_own_values():
    """not by the bulk of the population alone: the values named for it"""
    def differs(u, **kw):
        return X.half_bits(np.asarray(u, np.uint32), **kw) != X.half_bits(np.asarray(u, np.uint32))
    assert differs([0x477FF000, 0x47800000, 0x7F7FFFFF], clamp=True).all()
    assert differs([0x33000001, 0x33800000, 0x387FC000, 0xB3800000], flush=True).all()      # 2^-25 + 1 ulp, 2^-24, the largest subnormal half
    assert differs([0x3F801000], rounding="away").all() and not differs([0x3F803000], rounding="away").any()   # ties to the even / odd side
    assert differs([0x3F801001, 0x3F803000], rounding="trunc").all()
    a = np.asarray(list(X.ALPHAS.values()), np.uint32)
    assert [k for k, g in zip(X.ALPHAS, X.alpha_bit(a, "ge1") != X.alpha_bit(a)) if g] == ["1.0 + 1 ulp", "2.0", "+inf"]
    assert [k for k, g in zip(X.ALPHAS, X.alpha_bit(a, "ne0") == X.alpha_bit(a)) if g] == ["1.0", "+0.0", "-0.0"]


# ---- 4: the census ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", X.WHOLE_POPULATION)
def test_4_census_of_the_cases_that_hold_the_whole_population(name):
    values = X._pool(name)[:, :3]
    assert np.isin(X.midpoints(), values).all(), "a tie is missing"
    for ch in range(3):
        assert np.isin(X.specials(), values[:, ch]).all(), "a special is missing from a channel"
    cs = X.census(name)
    for cls, per_channel in cs["colour"].items():
        print(f"    {cls:32s} {per_channel}")
        assert min(per_channel) >= 1, cls                                  # every class in each colour channel
    print("   ", cs["alpha"], cs["mask words"], cs["rounding"])
    assert min(cs["alpha"].values()) >= 64                                 # every alpha class on at least 64 pixels
    assert all(cs["mask words"][k] >= 1 for k in ("all ones", "all zeros", "mixed", "partial, both values"))
    assert cs["rounding"]["differs from truncation"] >= 1000 and cs["rounding"]["differs from round half away"] >= 1000
    for key, exposure in {**X.EXPOSURES, "1.2": 1.2}.items():
        taken = cs["bb_exp"][key]
        print(f"    exposure {key:6s} {taken}")
        for branch in X.EXP_BRANCHES:                                      # every path the exposure can reach is taken, no other
            assert (taken[branch] >= 3) == (branch in X.reachable_branches(exposure)), (key, branch)


@pytest.mark.parametrize("name", ["256x8", "64x65/4"])
def test_4_census_of_the_tone_map_cases(name):
    """the world-1 and the partitioned case of the tone-map test hold every colour class in every channel and steer bb_exp down
    every path an exposure can reach"""
    cs = X.census(name)
    assert all(min(v) >= 1 for v in cs["colour"].values())
    for key, exposure in {**X.EXPOSURES, "1.2": 1.2}.items():
        for branch in X.EXP_BRANCHES:
            assert (cs["bb_exp"][key][branch] >= 3) == (branch in X.reachable_branches(exposure)), (key, branch)


def test_4_census_of_the_push_case():
    """64x65/4, the case of the narrow push in all four forms, tells the rounding, alpha and mask-order mutants apart by itself"""
    cs = X.census("64x65/4")
    assert min(cs["alpha"].values()) >= 64
    assert all(cs["mask words"][k] >= 1 for k in ("all ones", "all zeros", "mixed"))
    assert cs["rounding"]["differs from truncation"] >= 1000 and cs["rounding"]["differs from round half away"] >= 1000
    assert all(X.mutant_differs(m, "64x65/4") for m, kw in X.MUTANTS.items()
               if kw.get("form") in (X.RGBA16F, X.PACKED) and kw.get("mask_pad", True))


def test_4_mask_words_of_the_small_cases():
    kinds = {n: {k for k, v in X.mask_census(n).items() if v} for n in X.CASES}
    assert kinds["1x1"] == {"partial, one value"} and kinds["63x1"] == {"partial, both values"} and kinds["64x1"] == {"mixed"}
    assert kinds["65x1"] == {"all ones", "partial, one value"}
    assert kinds["1x544/17"] == {"partial, both values"}                   # n = 32: half a word per rank
    for n in ("2049x1", "7x33/2", "5x100/17"):
        assert {"all ones", "all zeros", "mixed"} <= kinds[n]
    for name, c in X.CASES.items():                                        # every shard carries both bit values where it can
        for r in range(c.world):
            bit = X.alpha_bit(X.shard(name, r)[..., 3])
            assert X.shard_pixels(c) == 1 or (bit.any() and not bit.all()), (name, r)


def test_4_the_hazard_gather_buffer_walks_every_half():
    seen = np.zeros(65536, bool)
    for name in X.WHOLE_POPULATION:
        g = X.gathered16_hazard(name).view("<u2")
        seen[g] = True
        assert not np.array_equal(g, X.gathered(name, X.RGBA16F).view("<u2"))
    assert seen.all()
    small = X.gathered16_hazard("64x65/4").view("<u2")
    assert ((small & 0x7FFF) > 0x7C00).sum() > 50 and (((small & 0x7C00) == 0) & ((small & 0x3FF) != 0)).sum() > 50


# ---- 5: the pinned record ---------------------------------------------------------------------------------------------
def test_5_the_population_is_the_recorded_one():
    want = json.load(open(RECORD))
    got = json.loads(json.dumps(X.record()))
    assert got["seeds"] == want["seeds"] and got["colour_population"] == want["colour_population"]
    assert list(got["cases"]) == list(want["cases"])
    for name in got["cases"]:
        assert got["cases"][name] == want["cases"][name], name
