"""Properties of the auto exposure model (tests/exposure_reference.py), which the GPU tests compare the device against.  No GPU."""
import numpy as np
import pytest

import exposure_reference as X

F32 = np.float32


def ramp(w=48, h=20, lo=-5.0, hi=5.0, seed=3):
    """a frame whose luminances lie in [2^lo, 2^hi] * (a colour factor below 4): well inside the bins"""
    rng = np.random.default_rng(seed)
    f = np.exp2(rng.uniform(lo, hi, (h, w, 1))).astype(F32) * rng.uniform(0.5, 1.5, (h, w, 4)).astype(F32)
    f[..., 3] = 1.0
    return f


def test_the_chart_holds_its_hazards():
    hz = X.hazards()
    y = X.luma(hz)
    assert np.isnan(y).sum() >= 3 and np.isposinf(y).sum() >= 1 and (y < 0).sum() >= 2 and (y == 0).sum() >= 2
    assert ((y > 0) & (y < F32(1.2e-38))).sum() >= 2                      # denormal luminances
    u = y.view(np.uint32).astype(np.int64)
    for e in [(X.FIRST + k) << 20 for k in (1, 2, 100, 128, 129, 255)] + [111 << 23, 143 << 23]:
        for d in (-1, 0, 1):
            assert (u == e + d).any(), (hex(e), d)
    hist, ignored = X.histogram(X.chart_frame(64, 64))
    assert ignored >= 7 and hist[0] >= 3 and hist[255] >= 3 and sum(hist) + ignored == 64 * 64
    hist, ignored = X.histogram(X.chart_frame(64, 64, "flat"))
    assert max(hist) >= 64 * 64 - len(hz)                                 # one bin holds almost every pixel
    hist, ignored = X.histogram(X.chart_frame(512, 256, "constant"))
    assert max(hist) == 512 * 256 and ignored == 0
    assert X.histogram(X.chart_frame(33, 9, "ignored")) == ([0] * 256, 33 * 9)
    for v in range(6):                                                    # the smallest frames see different hazards
        assert X.chart_frame(1, 1, v).shape == (1, 1, 4)
    assert len({X.chart_frame(1, 1, v).tobytes() for v in range(6)}) == 6


def test_bins_are_eighths_of_octaves():
    def bin_of(u):
        hist, ignored = X.histogram(np.array([[X.pixel_with_luma(u) + (F32(1.0),)]], F32))
        assert sum(hist) == 1 and ignored == 0
        return hist.index(1)
    for e in (-16, -15, -1, 0, 3, 15):
        u = (127 + e) << 23                                               # Y = 2^e exactly
        assert bin_of(u) == (e + 16) * 8
        assert bin_of(u - 1) == max((e + 16) * 8 - 1, 0)
        assert bin_of(u + (3 << 20)) == (e + 16) * 8 + 3
    assert bin_of(143 << 23) == 255 and bin_of((143 << 23) - 1) == 255 and bin_of(100 << 23) == 0


@pytest.mark.parametrize("k", [-3, -1, 1, 4])
def test_scaling_by_a_power_of_two_shifts_the_mean_exactly(k):
    f = ramp()
    g = f.copy()
    g[..., :3] = f[..., :3] * F32(2.0 ** k)
    for p in (X.DEFAULTS, X.params(lo=0, hi=1000), X.params(lo=100, hi=300, key=0.5)):
        a, _ = X.expose(f, p)
        b, _ = X.expose(g, p)
        assert a["counted"] == b["counted"] == f.shape[0] * f.shape[1]
        assert b["mean_bits"] - a["mean_bits"] == k << 23
        assert X.bits(b["target"]) == X.bits(F32(a["target"] * F32(2.0 ** -k)))
        assert np.array_equal(np.roll(a["hist"], 8 * k), b["hist"])


def test_permuting_the_pixels_changes_nothing():
    f = X.chart_frame(64, 64, 2)
    rng = np.random.default_rng(11)
    g = f.reshape(-1, 4)[rng.permutation(64 * 64)].reshape(32, 128, 4)
    a, ha = X.expose(f, X.DEFAULTS, F32(0.3))
    b, hb = X.expose(g, X.DEFAULTS, F32(0.3))
    assert X.same_record(a, b) is None and X.bits(ha) == X.bits(hb)


def test_something_is_always_kept():
    rng = np.random.default_rng(5)
    for n in range(1, 2001):
        cuts = np.sort(rng.integers(0, n + 1, 3))
        hist = [0] * 256
        hist[3], hist[100], hist[101], hist[255] = int(cuts[0]), int(cuts[1] - cuts[0]), int(cuts[2] - cuts[1]), int(n - cuts[2])
        for lo, hi in [(0, 1), (499, 500), (999, 1000)]:
            total, kept, s = X.trim(hist, lo, hi)
            assert total == n and kept == n - n * lo // 1000 - n * (1000 - hi) // 1000 and kept > 0
            assert 3 * kept <= s <= 255 * kept


def test_a_constant_frame_means_its_own_bin():
    for y in [2.0 ** -16, 1e-3, 0.18, 1.0, 7.3, 1000.0, 65535.0]:
        f = np.full((5, 7, 4), y, F32)
        rec, _ = X.expose(f, X.params(lo=0, hi=1000))
        yy = X.luma(f[0, 0])
        k = (X.bits(yy) >> 20) - 888
        assert rec["hist"][k] == 35 and rec["mean_bits"] >> 20 == 888 + k
        ybar = X.from_bits(rec["mean_bits"])
        assert X.from_bits((888 + k) << 20) < ybar < X.from_bits((889 + k) << 20)
        assert np.isfinite(ybar) and ybar >= F32(2.0 ** -16) and ybar < F32(2.0 ** 16)


def test_rate_one_returns_the_clamped_target_bit_for_bit():
    f = ramp(seed=9)
    for history in (None, F32(0.001), F32(77.0)):
        rec, after = X.expose(f, X.params(rate=1.0), history)
        assert X.bits(rec["applied"]) == X.bits(rec["clamped"]) == X.bits(after)
    rec, after = X.expose(f, X.params(rate=0.25), F32(8.0))
    assert rec["flags"] == 1 and rec["previous"] == F32(8.0)
    assert X.bits(after) == X.bits(F32(F32(8.0) + F32(F32(rec["clamped"] - F32(8.0)) * F32(0.25))))
    rec, _ = X.expose(f, X.params(rate=0.0), F32(8.0))
    assert rec["applied"] == F32(8.0)
    rec, _ = X.expose(f, X.params(rate=0.0))                              # no history: E_c whatever the rate
    assert X.bits(rec["applied"]) == X.bits(rec["clamped"]) and rec["flags"] == 0
    rec, _ = X.expose(f, X.params(e_min=3.0, e_max=3.0))
    assert rec["applied"] == F32(3.0) and rec["target"] != F32(3.0)


def test_nothing_counted():
    f = X.chart_frame(9, 4, "ignored")
    rec, after = X.expose(f, X.DEFAULTS, None, fallback=0.7)
    assert rec["applied"] == F32(0.7) and after is None and rec["flags"] == 2 and rec["previous"] == 0
    assert (rec["counted"], rec["kept"], rec["sum"], rec["mean_bits"], rec["ignored"]) == (0, 0, 0, 0, 36)
    rec, after = X.expose(f, X.params(rate=0.5), F32(2.5), fallback=0.7)
    assert rec["applied"] == F32(2.5) and after == F32(2.5) and rec["flags"] == 3 and rec["previous"] == F32(2.5)
