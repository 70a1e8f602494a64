"""The numpy model of option "sample_shading" 0 (tests/sample_merge_reference.py) against hand-built blocks, its own
properties, and a census of the oracle's primitive frames: the scenes of tests/test_gpu_sample_shading.py hold every kind
of output pixel the kernels distinguish.  No GPU is needed."""
import itertools

import numpy as np
import pytest

import resolve_reference as RR
import sample_merge_reference as M

F = np.float32
NO = M.NO_PRIM
W, H = 37, 23


def set_partitions(items):
    """every partition of `items` into non-empty sets, as lists of lists"""
    if not items:
        yield []
        return
    first, rest = items[0], items[1:]
    for part in set_partitions(rest):
        yield [[first]] + part
        for i in range(len(part)):
            yield part[:i] + [[first] + part[i]] + part[i + 1:]


def expected_rep(block):
    """the rule, sample by sample, on one block given as a list of winners"""
    out = []
    for k, p in enumerate(block):
        out.append(k if p == NO else min(e for e in range(k + 1) if block[e] == p))
    return out


# ---------------------------------------------------------------------------------------------------------------------
# hand-built blocks
# ---------------------------------------------------------------------------------------------------------------------
def test_the_fifteen_partitions_of_four_samples():
    parts = list(set_partitions([0, 1, 2, 3]))
    assert len(parts) == 15
    seen = set()
    for part in parts:
        prim = [0] * 4
        for number, members in enumerate(part):
            for k in members:
                prim[k] = 100 - 7 * number                     # (not in index order: only equality counts)
        rep = M.rep_map(np.array(prim, np.uint32).reshape(2, 2), 2).ravel().tolist()
        want = [min(m) for k in range(4) for m in part if k in m]
        assert rep == want == expected_rep(prim), (part, rep)
        seen.add(tuple(rep))
        # the same with uncovered samples mixed in: every subset of the samples uncovered
        for uncovered in itertools.chain.from_iterable(itertools.combinations(range(4), c) for c in range(1, 5)):
            holed = [NO if k in uncovered else p for k, p in enumerate(prim)]
            rep = M.rep_map(np.array(holed, np.uint32).reshape(2, 2), 2).ravel().tolist()
            assert rep == expected_rep(holed), (part, uncovered, rep)
            assert all(rep[k] == k for k in uncovered)          # an uncovered sample stands for itself
            assert all(holed[rep[k]] == holed[k] for k in range(4))
    assert len(seen) == 15


def test_blocks_of_sixteen():
    distinct = np.arange(16, dtype=np.uint32).reshape(4, 4) * 3 + 5
    assert np.array_equal(M.rep_map(distinct, 4), np.arange(16, dtype=np.uint8).reshape(4, 4))
    # later samples point at a representative that is neither sample 0 nor themselves: primitive 9 first wins sample 5
    block = np.array([[1, 1, 2, NO], [1, 9, 9, 2], [9, 3, NO, 9], [3, 3, 9, 1]], np.uint32)
    want = np.array([[0, 0, 2, 3], [0, 5, 5, 2], [5, 9, 10, 5], [9, 9, 5, 0]], np.uint8)
    got = M.rep_map(block, 4)
    assert np.array_equal(got, want) and got.ravel().tolist() == expected_rep(block.ravel().tolist())
    # two blocks side by side and one below do not see each other
    frame = np.full((8, 8), 7, np.uint32)
    frame[:4, 4:] = block
    got = M.rep_map(frame, 4)
    assert np.array_equal(got[:4, 4:], want) and not got[:4, :4].any() and not got[4:].any()
    values = np.arange(8 * 8 * 4, dtype=F).reshape(8, 8, 4)
    g = M.replicate(values, got, 4)
    assert np.array_equal(g[2, 4], values[1, 5]) and np.array_equal(g[3, 6], values[1, 5]) and np.array_equal(g[3, 4], values[2, 5])
    assert np.array_equal(g[5, 5], values[4, 4]) and np.array_equal(g[6, 1], values[4, 0])            # the blocks of one primitive
    assert np.array_equal(g[0, 7], values[0, 7]) and np.array_equal(g[2, 6], values[2, 6])          # uncovered: themselves


# ---------------------------------------------------------------------------------------------------------------------
# properties
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [2, 4])
def test_properties(n):
    rng = np.random.default_rng(n)
    prim = rng.integers(0, 3, (n * 5, n * 7)).astype(np.uint32)
    prim[rng.random(prim.shape) < 0.2] = NO
    fine = rng.standard_normal(prim.shape + (4,)).astype(F)
    rep = M.rep_map(prim, n)
    g = M.replicate(fine, rep, n)
    assert np.array_equal(M.replicate(g, rep, n), g)                       # idempotent
    own = M.representatives(rep, n)
    assert np.array_equal(g[own], fine[own]) and own[prim == NO].all()
    assert np.array_equal(M.merged(fine, prim, n), RR.resolve(g, n))
    one = np.zeros_like(prim)                                              # one primitive over the frame
    assert not M.rep_map(one, n).any()
    if n == 2:
        assert np.array_equal(M.merged(fine, one, 2).view(np.uint32), fine[::2, ::2].view(np.uint32))
    else:                                                                  # within the rounding of the sixteen additions
        assert np.allclose(M.merged(fine, one, 4), fine[::4, ::4], rtol=2.0 ** -20, atol=0)


# ---------------------------------------------------------------------------------------------------------------------
# census on the oracle
# ---------------------------------------------------------------------------------------------------------------------
MINIMUM = {"one": 256, "two": 16, "three or more": 128, "all distinct": 1, "partial": 32, "far representative": 32}


@pytest.mark.parametrize("n", [2, 4])
def test_census_of_the_scenes(n):
    count = dict.fromkeys(MINIMUM, 0)
    for name in ("triangle", "ball", "balls"):
        fine, prim = M.oracle(name, n * W, n * H, n)
        rep = M.rep_map(prim, n)
        own = M._blocks(M.representatives(rep, n), n)
        covered = M._blocks(prim != NO, n)
        # representatives among the covered samples of a pixel = the primitives in it
        reps = (own & covered).sum(axis=2)
        count["one"] += int((reps == 1).sum())
        count["two"] += int((reps == 2).sum())
        count["three or more"] += int((reps >= 3).sum())
        count["all distinct"] += int(((reps == n * n) & covered.all(axis=2)).sum())
        count["partial"] += int((covered.any(axis=2) & ~covered.all(axis=2)).sum())
        r = M._blocks(rep, n)
        count["far representative"] += int(((r != 0) & (r != np.arange(n * n))).any(axis=2).sum())   # (output pixels with one)
        differ = (M.merged(fine, prim, n).view(np.uint32) != RR.resolve(fine, n).view(np.uint32)).any(axis=2).sum()
        print(f"n = {n} {name}: merged differs from the per-sample resolve on {differ} pixels")
        if name != "triangle":
            assert differ >= 200, (name, differ)        # a library that ignores the option fails the GPU tests
    print(f"n = {n}: {count}")
    for kind, least in MINIMUM.items():
        assert count[kind] >= least, (kind, count[kind])


@pytest.mark.parametrize("n", [2, 4])
def test_partition_chart_shows_every_partition(n):
    _, prim = M.oracle("chart", n * W, n * H, n)
    assert (prim != NO).all()                                   # the base quad covers the frame
    if n == 2:
        blocks = M._blocks(prim, 2)
    else:                                                       # every 2 x 2 window of samples inside a block
        p4 = prim.reshape(H, 4, W, 4)
        blocks = np.concatenate([np.moveaxis(p4[:, oy:oy + 2, :, ox:ox + 2], 1, 2).reshape(-1, 4)
                                 for oy in range(3) for ox in range(3)])
    codes = np.unique(M.partition_code(blocks.reshape(-1, 4)))
    print(f"n = {n}: {len(codes)} partitions of four samples on the chart")
    assert len(codes) == 15
    rep = M.rep_map(prim, n)
    assert len(np.unique(M._blocks(rep, n).reshape(-1, n * n), axis=0)) >= 15
