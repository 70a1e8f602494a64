"""The TBN overlay's line rule on the CPU: the diamond-exit rule of OpenGL 4.6 section 14.5.1 on
1/256-pixel integers with the spec's perturbation p' = p - (eps, eps^2).  Hand-derived fragment sets, then the kernel's
form (major-axis candidates, separation along three axes) against an independent per-pixel symbolic Liang-Barsky form."""
import numpy as np
import pytest

import tbn_reference as tr
from bibim_renderer_amd.renderer import TBN_SEGMENT_DTYPE


def seg(x0, y0, x1, y1, key=0, za=0.5, zb=0.5):
    r = np.zeros(1, TBN_SEGMENT_DTYPE)
    r[0] = (x0, y0, x1, y1, za, zb, key, 0)
    return r


def c(p):  # centre of pixel p along one axis, 1/256 pixel
    return 256 * p + 128


# (x0, y0, x1, y1) -> the fragments the rule produces, derived by hand
HAND = [
    ((c(0), c(0), c(4), c(0)), {(0, 0), (1, 0), (2, 0), (3, 0)}),      # horizontal, centre to centre: start in, end out
    ((c(4), c(0), c(0), c(0)), {(4, 0), (3, 0), (2, 0), (1, 0)}),      # reversed
    ((c(2), c(0), c(2), c(4)), {(2, 0), (2, 1), (2, 2), (2, 3)}),      # vertical
    ((c(2), c(4), c(2), c(0)), {(2, 4), (2, 3), (2, 2), (2, 1)}),
    ((c(0), c(0), c(4), c(4)), {(0, 0), (1, 1), (2, 2), (3, 3)}),      # 45 degrees through the centres
    ((c(4), c(0), c(0), c(4)), {(4, 0), (3, 1), (2, 2), (1, 3)}),      # -45 degrees
    ((0, 128, 512, 128), {(0, 0)}),                                    # diamond vertex to vertex: pixel 1 holds the end
    ((512, 128, 0, 128), {(1, 0), (0, 0)}),                            # reversed: the end (-eps, -eps^2) is outside pixel 0
    ((192, 64, 192, 576), {(0, 0), (0, 1)}),                           # ends on diamond edges (x > centre: inside)
    ((64, 64, 64, 576), {(0, 0), (0, 1)}),                             # ends on diamond edges (x < centre: outside)
    ((c(1), c(1), c(1), c(1)), set()),                                 # zero length
    ((c(3) + 100, c(2), c(3) + 100, c(2)), set()),
    ((c(0), c(0), c(0) + 60, c(0) + 10), set()),                       # short, ends inside its own diamond
    ((c(0), c(0), c(0) + 200, c(0)), {(0, 0)}),                        # leaves its diamond, ends in no other
]


def hand_set():
    return np.concatenate([seg(*s, key=i) for i, (s, _) in enumerate(HAND)])


@pytest.mark.parametrize("i", range(len(HAND)))
def test_hand_derived_fragments(i):
    s, want = HAND[i]
    r = seg(*s)
    px, py = tr.fragments_brute(r[0], 16, 16)
    assert set(zip(px.tolist(), py.tolist())) == want, "brute-force form"
    _, px, py = tr.fragments(r, 16, 16)
    assert set(zip(px.tolist(), py.tolist())) == want, "kernel form"


def random_segments(n, seed, span=10):
    """random and boundary-heavy segments in a (span + 2)^2-pixel window: ends on pixel centres, diamond vertices and
    edges, pixel corners, axis-parallel, 45 degrees, one subpixel long, zero length"""
    rng = np.random.default_rng(seed)
    lo, hi = 256, 256 * (span + 1)
    kind = rng.integers(0, 6, n)
    P = rng.integers(lo, hi, (n, 4))
    grid = rng.integers(2, 2 * span + 2, (n, 4)) * 128                  # multiples of 128: centres, vertices, corners
    P = np.where((kind == 1)[:, None], grid, P)
    quarter = rng.integers(4, 4 * span + 4, (n, 4)) * 64                 # multiples of 64: points on diamond edges
    P = np.where((kind == 2)[:, None], quarter, P)
    d = rng.integers(-3 * 256, 3 * 256, n)
    P[kind == 3, 2] = P[kind == 3, 0] + d[kind == 3]                    # 45 degrees
    P[kind == 3, 3] = P[kind == 3, 1] + d[kind == 3] * rng.choice([-1, 1], int((kind == 3).sum()))
    ax = kind == 4                                                      # axis-parallel
    P[ax, 3] = P[ax, 1]
    vert = ax & (rng.random(n) < 0.5)
    P[vert, 2], P[vert, 3] = P[vert, 0], P[vert, 1] + d[vert]
    short = kind == 5                                                   # short: a few subpixels, some zero length
    P[short, 2:] = P[short, :2] + rng.integers(-3, 4, (int(short.sum()), 2))
    r = np.zeros(n, TBN_SEGMENT_DTYPE)
    r["x0"], r["y0"], r["x1"], r["y1"] = P[:, 0], P[:, 1], P[:, 2], P[:, 3]
    r["key"] = np.arange(n)
    return r


def test_the_two_forms_agree_on_20k_segments():
    W = H = 13
    segs = random_segments(20000, 7, span=10)
    # brute force: every pixel of the window for every segment
    PX, PY = np.meshgrid(np.arange(W), np.arange(H))
    fx, fy = (256 * PX.ravel() + 128)[None, :], (256 * PY.ravel() + 128)[None, :]
    X0, Y0, X1, Y1 = (segs[k].astype(np.int64)[:, None] for k in ("x0", "y0", "x1", "y1"))
    hit = tr.covers_brute(X0 - fx, Y0 - fy, X1 - fx, Y1 - fy)
    s_b, p_b = np.nonzero(hit)
    brute = set(zip(s_b.tolist(), PX.ravel()[p_b].tolist(), PY.ravel()[p_b].tolist()))
    s, px, py = tr.fragments(segs, W, H)
    fast = set(zip(s.tolist(), px.tolist(), py.tolist()))
    assert len(brute) > 40000
    assert fast == brute, (len(fast - brute), len(brute - fast), sorted(fast ^ brute)[:5])
    zero = (segs["x0"] == segs["x1"]) & (segs["y0"] == segs["y1"])
    assert zero.sum() > 50 and not np.isin(s, np.nonzero(zero)[0]).any()


def test_fmaf_is_correctly_rounded():
    from fractions import Fraction
    rng = np.random.default_rng(3)
    a = (rng.standard_normal(3000) * 1e3).astype(np.float32)
    b = (rng.standard_normal(3000) * 1e3).astype(np.float32)
    c = -(a.astype(np.float64) * b.astype(np.float64)).astype(np.float32)  # heavy cancellation
    c[::2] = (rng.standard_normal(1500) * 1e6).astype(np.float32)
    got = tr.fmaf(a, b, c)
    for x, y, z, g in zip(a[:600], b[:600], c[:600], got[:600]):
        exact = Fraction(float(x)) * Fraction(float(y)) + Fraction(float(z))
        lo = np.float32(float(exact))
        cands = [np.nextafter(lo, np.float32(-np.inf)), lo, np.nextafter(lo, np.float32(np.inf))]
        best = min(cands, key=lambda v: (abs(Fraction(float(v)) - exact), int(np.float32(v).view(np.uint32)) & 1))
        assert g == best, (x, y, z, g, best)
