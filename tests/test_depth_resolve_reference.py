"""The rule of option "depth_resolve" as tests/depth_resolve_reference.py states it (no GPU): hand blocks with ties, uncovered
samples, zero depths and a denormal; and a census of the scenes the GPU tests use, so that none of them can pass with the
three rules giving the same answer."""
import itertools

import numpy as np
import pytest

import depth_resolve_reference as DR
import depth_resolve_scenes as S

F, U = np.float32, np.uint32
NS = (2, 3, 4)
W, H = 37, 23                      # the output extent of the GPU tests
NO = DR.NO_PRIM


def block(n, depths, prims=None):
    """one output pixel: n*n depths (and winners) in index order k = j * n + i, as [n, n] fine arrays"""
    d = np.asarray(depths, F).reshape(n, n)
    p = None if prims is None else np.asarray(prims, U).reshape(n, n)
    return d, p


def picked(n, depths, mode):
    return int(DR.select(block(n, depths)[0], n, mode)[0, 0])


@pytest.mark.parametrize("n", NS)
def test_all_equal_selects_sample_zero(n):
    for value in (0.0, 0.25, 1.0):
        for mode in DR.MODES:
            assert picked(n, [value] * (n * n), mode) == 0


@pytest.mark.parametrize("n", NS)
def test_ties_go_to_the_first_index(n):
    last = n * n - 1
    d = [0.5] * (n * n)
    d[1], d[last] = 0.75, 0.75                       # the largest twice: k = 1 and the last
    assert picked(n, d, DR.MAX) == 1 and picked(n, d, DR.MIN) == 0 and picked(n, d, DR.SAMPLE_ZERO) == 0
    d = [0.5] * (n * n)
    d[2], d[last] = 0.125, 0.125                     # the smallest twice
    assert picked(n, d, DR.MIN) == 2 and picked(n, d, DR.MAX) == 0
    d = [0.5] * (n * n)
    d[n], d[n + 1] = 0.125, 0.125                    # ... in the second fine row: the row-major order decides
    assert picked(n, d, DR.MIN) == n


@pytest.mark.parametrize("n", NS)
def test_an_uncovered_sample_under_min(n):
    d = [0.5 + 0.01 * k for k in range(n * n)]
    p = list(range(100, 100 + n * n))
    d[n], p[n] = 0.0, NO                             # one uncovered sample: the cleared depth, no winner
    fd, fp = block(n, d, p)
    depth, prim = DR.resolve(fd, fp, n, DR.MIN)
    assert depth.view(U)[0, 0] == 0 and prim[0, 0] == NO
    depth, prim = DR.resolve(fd, fp, n, DR.MAX)
    assert depth[0, 0] == F(d[n * n - 1]) and prim[0, 0] == 100 + n * n - 1
    depth, prim = DR.resolve(fd, fp, n, DR.SAMPLE_ZERO)
    assert depth[0, 0] == F(0.5) and prim[0, 0] == 100


@pytest.mark.parametrize("n", NS)
def test_a_covered_zero_ties_an_uncovered_sample(n):
    d = [0.5] * (n * n)
    p = list(range(7, 7 + n * n))
    d[1], d[3] = 0.0, 0.0                            # k = 1 covered at the far plane (bits 0), k = 3 uncovered
    p[3] = NO
    fd, fp = block(n, d, p)
    depth, prim = DR.resolve(fd, fp, n, DR.MIN)
    assert depth.view(U)[0, 0] == 0 and prim[0, 0] == 8          # the first of the two: the covered one
    d[1], d[3], p[1], p[3] = d[3], d[1], NO, 10                   # the other way round: the uncovered one comes first
    fd, fp = block(n, d, p)
    assert DR.resolve(fd, fp, n, DR.MIN)[1][0, 0] == NO


@pytest.mark.parametrize("n", NS)
def test_one_against_a_denormal(n):
    tiny = np.array([1], U).view(F)[0]               # the smallest denormal: bits 1, above the cleared 0
    d = np.full(n * n, 1.0, F)
    d[n * n - 1] = tiny
    assert picked(n, d, DR.MIN) == n * n - 1 and picked(n, d, DR.MAX) == 0
    d[2] = 0.0
    assert picked(n, d, DR.MIN) == 2                 # ... and 0 is below the denormal
    depth, _ = DR.resolve(*block(n, d), n, DR.MIN)
    assert depth.view(U)[0, 0] == 0
    d[2] = tiny
    depth, _ = DR.resolve(*block(n, d), n, DR.MIN)
    assert depth.view(U)[0, 0] == 1 and picked(n, d, DR.MIN) == 2


def test_one_sample_is_the_identity():
    rng = np.random.default_rng(3)
    d = rng.random((5, 7), F)
    p = rng.integers(0, 1 << 32, (5, 7), dtype=np.uint64).astype(U)
    for mode in DR.MODES:
        depth, prim = DR.resolve(d, p, 1, mode)
        assert np.array_equal(depth.view(U), d.view(U)) and np.array_equal(prim, p)


def test_blocks_are_the_colour_resolves():
    """sample k of output pixel (x, y) is fine pixel (n x + k % n, n y + k // n)"""
    n, h, w = 3, 2, 4
    fine = np.arange(n * h * n * w, dtype=U).reshape(n * h, n * w)
    b = DR.blocks(fine, n)
    for y, x, k in itertools.product(range(h), range(w), range(n * n)):
        assert b[y, x, k] == fine[n * y + k // n, n * x + k % n]


def test_values_that_select_nothing():
    d = np.zeros((2, 2), F)
    for mode in (DR.NONE, DR.AVERAGE, 3, -1):
        with pytest.raises(ValueError):
            DR.select(d, 2, mode)


# ---------------------------------------------------------------------------------------------------------------------
# census: the scenes of the GPU tests tell the rules apart
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["ball", "balls"])
@pytest.mark.parametrize("n", NS)
def test_census_of_the_gpu_scenes(name, n):
    _, prim, depth = S.oracle(name, n * W, n * H, n)
    d = {m: DR.resolve(depth, prim, n, m)[0].view(U) for m in DR.MODES}
    zero_max = int((d[DR.SAMPLE_ZERO] != d[DR.MAX]).sum())
    zero_min = int((d[DR.SAMPLE_ZERO] != d[DR.MIN]).sum())
    all_three = int(((d[DR.SAMPLE_ZERO] != d[DR.MAX]) & (d[DR.SAMPLE_ZERO] != d[DR.MIN]) & (d[DR.MIN] != d[DR.MAX])).sum())
    print(f"{name} n={n}: SAMPLE_ZERO != MAX at {zero_max}, != MIN at {zero_min}, all three differ at {all_three} output pixels")
    assert zero_max >= 64 and zero_min >= 64 and all_three >= 32


@pytest.mark.parametrize("n", [2, 4])
def test_constant_depth_chart_selects_sample_zero(n):
    _, prim, depth = S.oracle("chart", n * W, n * H, n)
    assert len(np.unique(depth.view(U))) == 1 and (prim != NO).all()     # every entry of the chart at one depth
    for mode in DR.MODES:
        assert not DR.select(depth, n, mode).any()
    winners = {m: DR.resolve(depth, prim, n, m)[1] for m in DR.MODES}
    assert np.array_equal(winners[DR.MIN], prim[::n, ::n]) and np.array_equal(winners[DR.MAX], prim[::n, ::n])


@pytest.mark.parametrize("n", NS)
def test_census_of_the_comb(n):
    """markers: 178 pixels under SAMPLE_ZERO, 356 under MIN, none under MAX; every pair of rules at least 128 pixels apart in the
    overlaid image and at least 64 in the TBN image"""
    w, h = n * S.COMB_W, n * S.COMB_H
    markers, lines, drawn = {}, {}, {}
    for mode in DR.MODES:
        base, keys, _ = S.overlaid("comb", w, h, n, mode, tbn=True)
        _, _, markers[mode] = S.overlaid("comb", w, h, n, mode)
        lines[mode] = S.tr.composite(base, keys)
        drawn[mode] = int((markers[mode] != base).any(axis=2).sum())
    print(f"comb n={n}: marker pixels {drawn}")
    assert drawn == {DR.SAMPLE_ZERO: 178, DR.MIN: 356, DR.MAX: 0}
    for a, b in itertools.combinations(DR.MODES, 2):
        overlay_apart = int((markers[a] != markers[b]).any(axis=2).sum())
        tbn_apart = int((lines[a] != lines[b]).any(axis=2).sum())
        print(f"  {DR.NAMES[a]} / {DR.NAMES[b]}: overlay {overlay_apart}, TBN {tbn_apart} pixels apart")
        assert overlay_apart >= 128 and tbn_apart >= 64
