"""The exchange chart: the step behind the frame -- the wire forms of the exchange (k_pack_shard, k_pack_shard_half,
k_unpack_gathered<Form>, k_push_block<V>), k_tone_map and k_present -- on shards whose values the chart chooses by bit pattern.

TEST INFRASTRUCTURE ONLY.  Three things live here:

  the model       the partition and the four block forms as include/bibim_hip.h documents them (bbr_set_partition,
                  BBR_SHARD_*, "Alignment"), in plain numpy on BIT PATTERNS (uint32 / uint16 / uint8, never a float
                  conversion): band ownership and shard row order with the padding rows, block sizes, the RGBA32F / RGBA8
                  copies, the packed layout, binary16 in an integer formulation of round-to-nearest-even of its own, and the
                  un-interleave of `world` blocks into the row-major frame.  It does not import bibim_renderer_amd.partition;
                  tests/test_exchange_chart.py holds the two against each other.
  the population  per case one shard per rank, padding rows included (they travel and go through the tone map like any other
                  row).  Colour channels: every binary16 tie at -1, 0, +1 binary32 ulp in both signs, the specials, the
                  values that steer bb_exp for each exposure, random bit patterns.  Alpha: ten bit patterns laid out so that
                  the mask words come in all four kinds.  Deterministic: PCG64 on SEEDS.
  the mutants     wrong models (MUTANTS); each differs from the model on the chart's own inputs, which is what makes a
                  bit-exact comparison with the model worth something.

The record of the population (census counts, a sha256 of every shard and block) is tests/golden/exchange_chart.json, written
by tools/exchange_chart_record.py."""
import functools
import hashlib
from collections import namedtuple

import numpy as np

SEEDS = {"colour": 0xE8C0, "alpha": 0xE8C1, "wire16": 0xE8C2}

RGBA32F, PACKED, RGBA8, RGBA16F = 0, 1, 2, 3            # BBR_SHARD_*
FORMS = (RGBA32F, PACKED, RGBA8, RGBA16F)
FORM_NAMES = {RGBA32F: "rgba32f", PACKED: "packed", RGBA8: "rgba8", RGBA16F: "rgba16f"}
# include/bibim_hip.h, "Alignment": (block written, gather buffer read, whole frame written) per form
ALIGN = {RGBA32F: (4, 16, 16), PACKED: (8, 8, 16), RGBA8: (4, 4, 4), RGBA16F: (8, 8, 16)}

Case = namedtuple("Case", "width height world band_rows tile_mode")
# the smallest that still reach each edge (what each is there for: EDGES below, asserted by tests/test_exchange_chart.py)
CASES = {
    "1x1": Case(1, 1, 1, 32, 1),
    "63x1": Case(63, 1, 1, 32, 1),
    "64x1": Case(64, 1, 1, 32, 1),
    "65x1": Case(65, 1, 1, 32, 1),
    "256x8": Case(256, 8, 1, 32, 1),
    "2049x1": Case(2049, 1, 1, 32, 1),
    "333x211": Case(333, 211, 1, 32, 1),
    "7x33/2": Case(7, 33, 2, 32, 1),
    "3x32/3": Case(3, 32, 3, 64, 0),
    "5x100/17": Case(5, 100, 17, 32, 1),
    "1x544/17": Case(1, 544, 17, 32, 1),
    "64x65/4": Case(64, 65, 4, 32, 1),
    "333x211/3": Case(333, 211, 3, 32, 1),
}
EDGES = {
    "1x1": "one pixel: a one-bit mask word, 12 n mod 8 = 4, a 16-byte tail of padding",
    "63x1": "one partial mask word with both bit values",
    "64x1": "exactly one full mask word, no partial one",
    "65x1": "a full word of ones and a partial word of one pixel",
    "256x8": "n = 2048: exactly one workgroup of k_present, eight full 256-thread grids",
    "2049x1": "n = 2049: one pixel in k_present's second workgroup and in the ninth 256-thread block",
    "333x211": "n mod 64 = 55, 12 n mod 8 = 4; holds the whole colour population",
    "7x33/2": "the last band has one row",
    "3x32/3": "64-row tiles, a band taller than the frame, two ranks own nothing",
    "5x100/17": "four bands over 17 ranks: thirteen own nothing; more than kMaxPushPeers peers",
    "1x544/17": "width 1, seventeen ranks of one band each, no padding row anywhere",
    "64x65/4": "blocks that are multiples of 16 bytes (the push's wide form unless a pointer forbids it), one rank owns nothing",
    "333x211/3": "the whole colour population on a partition: uneven ownership, odd width",
}

# exposures of the tone-map tests; 1.2 is what the present tests put into the frame's uniforms
EXPOSURES = {"1.0": 1.0, "0.0": 0.0, "-0.0": -0.0, "-1.0": -1.0, "inf": float("inf"), "nan": float("nan"), "1e-30": 1e-30,
             "1e30": 1e30}
PRESENT_SETTINGS = ((0, 1.0), (1, 1.2))
_STEERING_EXPOSURES = (1.0, 1.2, -1.0, 1e-30, 1e30)      # the finite non-zero ones: the others leave nothing to steer


def index_of(name):
    return list(CASES).index(name)


def _rng(kind, name, extra=0):
    return np.random.Generator(np.random.PCG64([SEEDS[kind], index_of(name), extra]))


def _frozen(a):
    a.setflags(write=False)
    return a


# =====================================================================================================================
# the model: partition
# =====================================================================================================================
def n_bands(c):
    return -(-c.height // c.band_rows)


def shard_rows(c):
    """rows of every rank's shard (bbr_shard_rows): without a partition the shard is the frame; with one, the most bands a
    rank can own, times band_rows -- equal for all ranks, so that equal-sized blocks reassemble the frame"""
    return c.height if c.world == 1 else -(-n_bands(c) // c.world) * c.band_rows


def shard_pixels(c):
    return shard_rows(c) * c.width


def source_rows(c, rank):
    """for every row of `rank`'s shard the framebuffer row it holds, -1 for a padding row: band b (band_rows framebuffer rows)
    belongs to rank b % world, a shard is [local band][row in band]"""
    if c.world == 1:
        return np.arange(c.height, dtype=np.int64)
    src = np.full(shard_rows(c), -1, np.int64)
    for local in range(shard_rows(c) // c.band_rows):
        band = rank + local * c.world
        for r in range(c.band_rows):
            y = band * c.band_rows + r
            if y < c.height:
                src[local * c.band_rows + r] = y
    return src


def padding_rows(c, rank):
    return int((source_rows(c, rank) < 0).sum())


def place_of_row(c, y, swap=False):
    """framebuffer row y -> (rank, row of that rank's shard): the direction the un-interleave takes.  swap: the mutant that
    exchanges band % world with band / world (kept inside the buffers, as a model has to be)"""
    band, r = divmod(y, c.band_rows)
    rank, local = band % c.world, band // c.world
    if swap:
        rank, local = (band // c.world) % c.world, (band % c.world) % (shard_rows(c) // c.band_rows or 1)
    return rank, local * c.band_rows + r


# =====================================================================================================================
# the model: binary16, on bit patterns
# =====================================================================================================================
def _split(u):
    """binary32 bits -> (the sign where binary16 has it, biased exponent e, fraction bits, quotient q, remainder rem, half):
    with the 24-bit significand sig, |x| = sig * 2^(max(e, 1) - 150) = (q + rem / 2^shift) grid steps of the binary16 grid at x -- 2^13 binary32
    steps where the result is a normal half (e >= 113), 2^-24 = 2^(126 - max(e, 1)) of the significand's units below."""
    u = np.asarray(u).astype(np.uint64)
    a = u & np.uint64(0x7FFFFFFF)
    e = (a >> np.uint64(23)).astype(np.int64)
    frac = a & np.uint64(0x7FFFFF)
    sig = np.where(e > 0, frac | np.uint64(0x800000), frac)
    shift = np.where(e >= 113, 13, np.minimum(126 - np.maximum(e, 1), 40)).astype(np.uint64)
    q = sig >> shift
    rem = sig & ((np.uint64(1) << shift) - np.uint64(1))
    half = np.uint64(1) << (shift - np.uint64(1))
    return ((u >> np.uint64(16)) & np.uint64(0x8000)), e, frac, q, rem, half


def half_bits(u, rounding="even", flush=False, clamp=False):
    """binary32 bits -> the bits of the nearest binary16 value, ties to even; overflow (>= 65520) to infinity, subnormal
    halves kept, the sign of zero kept.  NaN -> a NaN (quiet, the top payload bits: not part of any comparison).
    Mutants: rounding "trunc" / "away" (ties away from zero), flush (subnormal halves to zero), clamp (overflow to 65504)."""
    sign, e, frac, q, rem, half = _split(u)
    if rounding == "even":
        up = (rem > half) | ((rem == half) & ((q & np.uint64(1)) == 1))
    elif rounding == "away":
        up = rem >= half
    else:
        assert rounding == "trunc"
        up = np.zeros(q.shape, bool)
    q = q + up.astype(np.uint64)
    # a normal half: exponent field e - 112, fraction q - 1024; a carry out of the fraction (q = 2048) moves the exponent up by
    # itself, as does a subnormal that rounds up to q = 1024, the smallest normal
    h = np.where(e >= 113, ((np.maximum(e, 113) - 113).astype(np.uint64) << np.uint64(10)) + q, q)
    h = np.where(h >= 0x7C00, np.uint64(0x7BFF if clamp else 0x7C00), h)
    if flush:
        h = np.where(h < 0x0400, np.uint64(0), h)
    h = np.where(e == 255, np.where(frac == 0, np.uint64(0x7C00), np.uint64(0x7E00) | (frac >> np.uint64(13))), h)
    return (sign | h).astype(np.uint16)


def widen_bits(h):
    """binary16 bits -> the binary32 bits of the same value (exact: every binary16 value is a binary32 value).  A NaN keeps
    its payload in the top bits and is made quiet, as a conversion does; no comparison looks at it."""
    h = np.asarray(h).astype(np.uint32)
    sign, e, m = (h & 0x8000) << 16, (h >> 10) & 31, h & 0x3FF
    p = np.zeros(h.shape, np.uint32)                         # floor(log2 m) of a subnormal's fraction
    for k in range(1, 10):
        p += m >= (1 << k)
    sub = np.where(m == 0, 0, ((p + 103) << 23) | ((m << (23 - p)) & 0x7FFFFF))   # m * 2^-24 = 1.f * 2^(p - 24)
    out = np.where(e == 0, sub, ((e + 112) << 23) | (m << 13))
    out = np.where(e == 31, 0x7F800000 | (m << 13) | np.where(m != 0, 0x00400000, 0), out)
    return (sign | out).astype(np.uint32)


def is_nan_bits(u):
    return (np.asarray(u) & 0x7FFFFFFF) > 0x7F800000


def is_tie(u):
    """binary32 bits of a finite value exactly half way between two neighbouring binary16 values (65520, half way between
    65504 and 2^16, included; nothing above it)"""
    _, e, _, _, rem, half = _split(u)
    return (rem == half) & ((np.asarray(u) & 0x7FFFFFFF) <= 0x477FF000)


# =====================================================================================================================
# the model: blocks
# =====================================================================================================================
def packed_layout(n, mask_pad=True):
    """(block bytes, offset of the masks): rgb[n][3], pad to 8, one 64-bit word per 64 pixels, pad to 16"""
    rgb = 12 * n
    mask_offset = -(-rgb // 8) * 8 if mask_pad else rgb
    return -(-(mask_offset + 8 * (-(-n // 64))) // 16) * 16, mask_offset


def block_bytes(c, form, n=None):
    n = shard_pixels(c) if n is None else n
    return {RGBA32F: 16 * n, PACKED: packed_layout(n)[0], RGBA8: 4 * n, RGBA16F: 8 * n}[form]


def alpha_bit(alpha_bits, alpha="one"):
    """the packed form's bit: set where alpha has exactly the bits of 1.0f.  Mutants: "ge1" (alpha >= 1.0), "ne0" (alpha != 0)"""
    a = np.asarray(alpha_bits, np.uint32)
    if alpha == "one":
        return a == 0x3F800000
    if alpha == "ge1":
        return (a >= 0x3F800000) & (a <= 0x7F800000)          # positive, at least 1.0, not NaN
    assert alpha == "ne0"
    return (a & 0x7FFFFFFF) != 0                              # NaN != 0 is true


def encode_block(shard, form, rounding="even", flush=False, clamp=False, alpha="one", mask_bits="little", mask_pad=True):
    """a shard -- uint32 bits [rows, W, 4], for RGBA8 the presented uint8 [rows, W, 4] -- as the bytes that travel"""
    if form == RGBA8:
        assert shard.dtype == np.uint8
        return np.ascontiguousarray(shard).reshape(-1).copy()
    assert shard.dtype == np.uint32
    px = shard.reshape(-1, 4)
    n = len(px)
    if form == RGBA32F:
        return px.astype("<u4").view(np.uint8).reshape(-1)
    if form == RGBA16F:
        return half_bits(px, rounding, flush, clamp).astype("<u2").view(np.uint8).reshape(-1)
    size, mask_offset = packed_layout(n, mask_pad)
    out = np.zeros(size, np.uint8)                            # the padding is zero
    out[:12 * n] = np.ascontiguousarray(px[:, :3]).astype("<u4").view(np.uint8).reshape(-1)
    words = -(-n // 64)
    bit = np.zeros(words * 64, np.uint64)
    bit[:n] = alpha_bit(px[:, 3], alpha)
    k = np.arange(64, dtype=np.uint64)
    place = k if mask_bits == "little" else np.uint64(63) - k
    masks = (bit.reshape(words, 64) << place).sum(axis=1, dtype=np.uint64)
    out[mask_offset:mask_offset + 8 * words] = masks.astype("<u8").view(np.uint8)
    return out


def decode_block(block, form, rows, width):
    """one block -> the shard it unpacks to: uint32 bits [rows, W, 4] (RGBA8: uint8)"""
    n = rows * width
    block = np.ascontiguousarray(block, np.uint8)
    assert block.size == {RGBA32F: 16 * n, PACKED: packed_layout(n)[0], RGBA8: 4 * n, RGBA16F: 8 * n}[form]
    if form == RGBA8:
        return block.reshape(rows, width, 4)
    if form == RGBA32F:
        return block.view("<u4").astype(np.uint32).reshape(rows, width, 4)
    if form == RGBA16F:
        return widen_bits(block.view("<u2")).reshape(rows, width, 4)
    mask_offset = packed_layout(n)[1]
    out = np.empty((n, 4), np.uint32)
    out[:, :3] = block[:12 * n].view("<u4").reshape(n, 3)
    masks = block[mask_offset:mask_offset + 8 * (-(-n // 64))].view("<u8").astype(np.uint64)
    j = np.arange(n, dtype=np.uint64)
    out[:, 3] = np.where((masks[(j >> np.uint64(6)).astype(np.int64)] >> (j & np.uint64(63))) & np.uint64(1), 0x3F800000, 0)
    return out.reshape(rows, width, 4)


def whole_frame(c, form, gathered, swap=False):
    """`world` blocks back to back -> the row-major whole frame [H, W, 4] (uint32 bits; RGBA8: uint8)"""
    rows, size = shard_rows(c), block_bytes(c, form)
    gathered = np.ascontiguousarray(gathered, np.uint8).reshape(-1)
    assert gathered.size == c.world * size
    shards = [decode_block(gathered[r * size:(r + 1) * size], form, rows, c.width) for r in range(c.world)]
    out = np.empty((c.height, c.width, 4), shards[0].dtype)
    for y in range(c.height):
        rank, row = place_of_row(c, y, swap)
        out[y] = shards[rank][row]
    return out


# =====================================================================================================================
# the population
# =====================================================================================================================
def f32_bits(x):
    return np.asarray(x, np.float32).reshape(-1).view(np.uint32).copy()


@functools.lru_cache(None)
def midpoints():
    """the midpoint of every pair of neighbouring non-negative binary16 values (0x0000 .. 0x7BFF with its upper neighbour;
    the last pair is 65504 / 2^16, midpoint 65520) at -1, 0, +1 binary32 ulp, in both signs: 31744 * 6 bit patterns.
    A midpoint of two binary16 values has one more significant bit than they: exact in binary64 and in binary32."""
    h = np.arange(0x7C00, dtype=np.uint32)
    lo = widen_bits(h)
    hi = np.where(h == 0x7BFF, np.uint32(0x47800000), widen_bits(np.minimum(h + 1, 0x7BFF)))
    mid64 = (lo.view(np.float32).astype(np.float64) + hi.view(np.float32).astype(np.float64)) / 2
    mid = mid64.astype(np.float32)
    assert np.array_equal(mid.astype(np.float64), mid64)
    m = mid.view(np.uint32)
    pos = np.stack([m - 1, m, m + 1], axis=1).reshape(-1)
    return _frozen(np.concatenate([pos, pos | 0x80000000]).astype(np.uint32))


QUIET_NANS = (0x7FC00000, 0xFFC00000, 0x7FC00001, 0x7FFFFFFF, 0x7FD55555, 0xFFEAAAAA)
SIGNALLING_NANS = (0x7F800001, 0xFF800001, 0x7FBFFFFF, 0x7FA00000, 0x7F801234, 0xFF955555)
SUBNORMALS = (0x00000001, 0x00000002, 0x00400000, 0x007FFFFF, 0x80000001, 0x80400000, 0x807FFFFF)


@functools.lru_cache(None)
def specials():
    """the values that are not ties; every colour channel of a case gets them all where it has the room"""
    s = [0x00000000, 0x80000000, 0x7F800000, 0xFF800000, *QUIET_NANS, *SIGNALLING_NANS, *SUBNORMALS,
         0x00800000, 0x80800000,                               # the smallest normal
         0x32FFFFFF, 0x33000000, 0x33000001, 0xB2FFFFFF, 0xB3000000, 0xB3000001,   # 2^-25: the tie between 0 and 2^-24
         0x477FEFFF, 0x477FF000, 0x477FF001, 0xC77FEFFF, 0xC77FF000, 0xC77FF001,   # 65520: the tie between 65504 and infinity
         0x477FE000, 0x47800000, 0xC77FE000, 0xC7800000,       # 65504 and 2^16 themselves
         0x7F7FFFFF, 0xFF7FFFFF]
    # -x * exposure below -104, around both guards, above 88.7228317, and inside the normal range, for each exposure that can
    # be steered at all
    for e in _STEERING_EXPOSURES:
        for t in (200.0, 1000.0, 104.5, 104.0, 103.5, 10.0, 1.0, 0.5, 1e-3, -0.5, -1.0, -10.0, -88.0, -88.7228317, -89.0, -100.0, -1000.0):
            s.extend(f32_bits(np.float32(t) / np.float32(e)))
    return _frozen(np.asarray(s, np.uint32))


ALPHAS = {"1.0": 0x3F800000, "+0.0": 0x00000000, "-0.0": 0x80000000, "1.0 + 1 ulp": 0x3F800001, "1.0 - 1 ulp": 0x3F7FFFFF,
          "-1.0": 0xBF800000, "0.5": 0x3F000000, "2.0": 0x40000000, "+inf": 0x7F800000, "nan": 0x7FC00001}
_ALPHA_BITS = np.asarray(list(ALPHAS.values()), np.uint32)


def _alpha_of_shard(n, rank, rng):
    """word w of the shard is of kind (w + rank) % 4: all ones, all zeros (cycling through the nine patterns that are not 1.0),
    mixed, mixed; a mixed word of two or more pixels is made to hold both bit values, and so is a partial last word"""
    a = np.empty(n, np.uint32)
    others = _ALPHA_BITS[1:]
    for w in range(-(-n // 64)):
        lo, hi = 64 * w, min(64 * w + 64, n)
        kind = (w + rank) % 4
        if n <= 64 or (hi - lo < 64 and hi - lo >= 2):
            kind = 2
        if kind == 0:
            a[lo:hi] = 0x3F800000
        elif kind == 1:
            a[lo:hi] = others[(np.arange(lo, hi) + w) % len(others)]
        else:
            a[lo:hi] = _ALPHA_BITS[rng.integers(0, len(_ALPHA_BITS), hi - lo)]
            if hi - lo >= 2:
                a[lo], a[lo + 1] = 0x3F800000, others[w % len(others)]
    return a


@functools.lru_cache(None)
def _pool(name):
    """all ranks' shards of a case as one pool of world * n pixels: uint32 bits [world * n, 4]"""
    c = CASES[name]
    n, total = shard_pixels(c), c.world * shard_pixels(c)
    dealt = np.random.Generator(np.random.PCG64(SEEDS["colour"])).permutation(midpoints())   # the same deal for every case
    rng = _rng("colour", name)
    pool = np.empty((total, 4), np.uint32)
    for ch in range(3):
        s, m = rng.permutation(specials()), rng.permutation(dealt[ch::3])
        if total < 2 * len(s):                               # a small case: half specials, half ties
            vals = np.concatenate([s[:(total + 1) // 2], m[:total // 2]])
        else:
            vals = np.concatenate([s, m])[:total]
        fill = rng.integers(0, 2 ** 32, total - len(vals), dtype=np.uint64).astype(np.uint32)   # random bit patterns fill the rest
        pool[:, ch] = rng.permutation(np.concatenate([vals, fill]))
    arng = _rng("alpha", name)
    for rank in range(c.world):
        pool[rank * n:(rank + 1) * n, 3] = _alpha_of_shard(n, rank, arng)
    return _frozen(pool)


def shard(name, rank):
    """the fp32 shard of `rank` as uint32 bits [shard_rows, W, 4] (read-only, shared)"""
    c = CASES[name]
    n = shard_pixels(c)
    return _pool(name)[rank * n:(rank + 1) * n].reshape(shard_rows(c), c.width, 4)


def shard_f32(name, rank):
    return shard(name, rank).view(np.float32)


@functools.lru_cache(None)
def presented(name, rank, enable=0, exposure=1.0, hdr16=True):
    """the presented shard (uint8 [rows, W, 4]): the oracle's, of the fp32 shard"""
    from oracle import bbo
    return _frozen(bbo.present(shard_f32(name, rank), enable, exposure, hdr16))


def source_shard(name, form, rank):
    return presented(name, rank) if form == RGBA8 else shard(name, rank)


@functools.lru_cache(None)
def block(name, form, rank):
    return _frozen(encode_block(source_shard(name, form, rank), form))


@functools.lru_cache(None)
def gathered(name, form):
    return _frozen(np.concatenate([block(name, form, r) for r in range(CASES[name].world)]))


@functools.lru_cache(None)
def whole(name, form):
    return _frozen(whole_frame(CASES[name], form, gathered(name, form)))


@functools.lru_cache(None)
def gathered16_hazard(name):
    """an RGBA16F gather buffer the pack kernel could not have made: the model's blocks, with the four halves of every third
    pixel replaced by a walk through ALL 65536 binary16 bit patterns (NaNs with every payload, subnormals, +-inf, +-0) as far
    as the case has room"""
    g = gathered(name, RGBA16F).view("<u2").astype(np.uint16).reshape(-1, 4)
    walk = _rng("wire16", name).permutation(65536).astype(np.uint16)
    sel = np.arange(len(g)) % 3 == 1
    k = int(sel.sum()) * 4
    g[sel] = np.resize(walk, k).reshape(-1, 4)
    return _frozen(g.astype("<u2").view(np.uint8).reshape(-1))


def test_ranks(name):
    """the ranks a GPU test builds a context for: the first and the last (the result must not depend on the rank)"""
    return sorted({0, CASES[name].world - 1})


# =====================================================================================================================
# the mutants
# =====================================================================================================================
MUTANTS = {
    "truncation": dict(form=RGBA16F, rounding="trunc"),
    "round half away": dict(form=RGBA16F, rounding="away"),
    "subnormal halves flushed": dict(form=RGBA16F, flush=True),
    "overflow clamped to 65504": dict(form=RGBA16F, clamp=True),
    "alpha bit as >= 1.0": dict(form=PACKED, alpha="ge1"),
    "alpha bit as != 0": dict(form=PACKED, alpha="ne0"),
    "big-endian mask bits": dict(form=PACKED, mask_bits="big"),
    "mask offset without the pad to 8": dict(form=PACKED, mask_pad=False),
    "band % world exchanged with band / world": dict(swap=True),
    "padding rows dropped": dict(drop_padding=True),
}


def mutant_cases(mutant):
    """the cases on which a mutant can differ at all, from the geometry alone"""
    kw = MUTANTS[mutant]
    if kw.get("swap"):          # needs a band whose index and whose quotient by world name different places
        return [n for n, c in CASES.items() if c.world > 1 and n_bands(c) > 1]
    if kw.get("drop_padding"):
        return [n for n, c in CASES.items() if any(padding_rows(c, r) for r in range(c.world))]
    if kw.get("mask_pad") is False:
        return [n for n, c in CASES.items() if shard_pixels(c) % 2]
    if kw.get("mask_bits"):     # needs a word that is not its own mirror image: a mixed one
        return [n for n in CASES if mask_census(n)["mixed"] + mask_census(n)["partial, both values"]]
    return ["333x211", "333x211/3"]     # rounding and alpha mutants: the cases that hold the whole population


def mutant_differs(mutant, name):
    c, kw = CASES[name], dict(MUTANTS[mutant])
    form = kw.pop("form", RGBA32F)
    if kw.pop("swap", False):
        return not np.array_equal(whole_frame(c, form, gathered(name, form), swap=True), whole(name, form))
    if kw.pop("drop_padding", False):
        return any(not np.array_equal(encode_block(shard(name, r)[source_rows(c, r) >= 0], form), block(name, form, r))
                   for r in range(c.world))
    return any(not np.array_equal(encode_block(shard(name, r), form, **kw), block(name, form, r)) for r in range(c.world))


# =====================================================================================================================
# the census
# =====================================================================================================================
def colour_classes(u):
    """class name -> mask over binary32 bit patterns, by predicate on the bits (not by how the population was made)"""
    u = np.asarray(u, np.uint32)
    a = u & 0x7FFFFFFF
    finite = a < 0x7F800000
    tie = is_tie(u)
    sub16 = a < 0x38800000                                   # below 2^-14: the result is a subnormal half or zero
    return {
        "tie, normal half": tie & ~sub16 & (a != 0x477FF000),
        "tie, subnormal half": tie & sub16 & (a != 0x33000000),
        "tie - 1 ulp": finite & is_tie(a + 1) & (a != 0),
        "tie + 1 ulp": finite & is_tie(a - np.uint32(1)) & (a != 0),
        "tie, negative": tie & (u >> 31 == 1),
        "65520, the tie with infinity": a == 0x477FF000,
        "above 65520": finite & (a > 0x477FF000),
        "2^-25, the tie with zero": a == 0x33000000,
        "2^-25 - 1 ulp": a == 0x32FFFFFF,
        "2^-25 + 1 ulp": a == 0x33000001,
        "+0": u == 0, "-0": u == 0x80000000, "+inf": u == 0x7F800000, "-inf": u == 0xFF800000,
        "quiet nan": is_nan_bits(u) & ((u & 0x00400000) != 0),
        "signalling nan": is_nan_bits(u) & ((u & 0x00400000) == 0),
        "binary32 subnormal": (a > 0) & (a < 0x00800000),
        "smallest normal": a == 0x00800000,
        "largest finite": a == 0x7F7FFFFF,
    }


def _all_shards(name):
    return _pool(name)


def colour_census(name):
    """class -> [count in r, in g, in b] over all ranks' shards of the case"""
    px = _all_shards(name)
    return {k: [int(m[:, ch].sum()) for ch in range(3)] for k, m in colour_classes(px[:, :3]).items()}


def alpha_census(name):
    a = _all_shards(name)[:, 3]
    return {k: int((a == v).sum()) for k, v in ALPHAS.items()}


def mask_census(name):
    """kinds of mask word over all ranks' packed blocks, read from the model's blocks"""
    c = CASES[name]
    n = shard_pixels(c)
    out = {"all ones": 0, "all zeros": 0, "mixed": 0, "partial, both values": 0, "partial, one value": 0}
    for r in range(c.world):
        b = block(name, PACKED, r)
        off = packed_layout(n)[1]
        masks = b[off:off + 8 * (-(-n // 64))].view("<u8")
        for w, m in enumerate(int(x) for x in masks):
            live = min(64, n - 64 * w)
            if live < 64:
                both = 0 < m < (1 << live) - 1
                out["partial, both values" if both else "partial, one value"] += 1
            else:
                out["all ones" if m == 2 ** 64 - 1 else "all zeros" if m == 0 else "mixed"] += 1
    return out


def rounding_census(name):
    """values whose round-to-nearest-even half differs from the truncated one / from the half-away one (all four channels)"""
    u = _all_shards(name)
    u = u[~is_nan_bits(u)]
    even = half_bits(u)
    return {"differs from truncation": int((even != half_bits(u, "trunc")).sum()),
            "differs from round half away": int((even != half_bits(u, "away")).sum())}


EXP_BRANCHES = ("underflow", "nan", "overflow", "main")


def exp_branches(x, exposure):
    """which path of bb_exp each colour value takes under an exposure, counted from the oracle's input -x * exposure (one
    binary32 multiplication): x < -104 -> 0; NaN -> NaN; x > 88.7228317 -> inf; the main path otherwise"""
    with np.errstate(all="ignore"):
        t = -np.asarray(x, np.float32) * np.float32(exposure)
    nan = np.isnan(t)
    under, over = ~nan & (t < np.float32(-104.0)), ~nan & (t > np.float32(88.7228317))
    return {"underflow": int(under.sum()), "nan": int(nan.sum()), "overflow": int(over.sum()),
            "main": int((~nan & ~under & ~over).sum())}


def reachable_branches(exposure):
    """the paths -x * exposure can take at all.  A finite non-zero exposure reaches all four.  Zero of either sign makes the
    product +-0 or (x infinite or NaN) NaN: the main path and NaN only.  An infinite exposure makes it +-inf or (x zero or NaN)
    NaN: both saturating guards and NaN, never the main path.  A NaN exposure makes every product NaN."""
    e = np.float32(exposure)
    if np.isnan(e):
        return ("nan",)
    if np.isinf(e):
        return ("underflow", "nan", "overflow")
    if e == 0:
        return ("nan", "main")
    return EXP_BRANCHES


def exp_census(name):
    x = _all_shards(name)[:, :3].view(np.float32)
    return {k: exp_branches(x, e) for k, e in {**EXPOSURES, "1.2": 1.2}.items()}


def census(name):
    return {"colour": colour_census(name), "alpha": alpha_census(name), "mask words": mask_census(name),
            "rounding": rounding_census(name), "bb_exp": exp_census(name)}


# what each case answers for (tests/test_exchange_chart.py asserts exactly these; the others are smaller slices of the same
# population and answer for their geometry, EDGES)
WHOLE_POPULATION = ("333x211", "333x211/3")


def sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def record():
    """what tests/golden/exchange_chart.json pins: the population cannot drift unnoticed"""
    cases = {}
    for name, c in CASES.items():
        cases[name] = {"case": list(c), "shard_rows": shard_rows(c),
                       "padding_rows": [padding_rows(c, r) for r in range(c.world)],
                       "shards_sha256": sha(_pool(name)),
                       "blocks_sha256": {FORM_NAMES[f]: sha(gathered(name, f)) for f in FORMS},
                       "hazard16_sha256": sha(gathered16_hazard(name)),
                       "census": census(name)}
    return {"seeds": SEEDS, "colour_population": {"ties": int(midpoints().size), "specials": int(specials().size)}, "cases": cases}
