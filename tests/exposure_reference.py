"""The auto exposure rule (include/bibim_hip.h, "auto exposure"), restated in numpy and Python integers, and the chart of
frames the GPU tests present.  Written from the rule's text alone; nothing here knows the kernels.

Every floating-point operation is one np.float32 operation (one rounding to nearest even, denormals kept, nothing fused);
everything about the histogram is a Python integer.

    luma     Y = (0.2126f * r + 0.7152f * g) + 0.0722f * b
    count    !(Y > 0): ignored.  Else bin = clamp((bits(Y) >> 20) - 888, 0, 255);  N = sum hist;  ignored = W * H - N
    trim     skip_lo = N * lo // 1000, skip_hi = N * (1000 - hi) // 1000
             c_k = max(0, min(P_k + hist[k], N - skip_hi) - max(P_k, skip_lo));  N' = sum c_k;  S = sum k * c_k
    mean     mean_bits = (888 << 20) + (S << 20) // N' + (1 << 19)
    target   E* = key * (1 / Ybar);  E_c = min(max(E*, e_min), e_max)
    adapt    E = E_c if rate == 1 or there is no history, else E_prev + (E_c - E_prev) * rate;  the history becomes E
             N == 0: the history stays;  E = the history, else the caller's exposure
"""
import collections

import numpy as np

F32 = np.float32
BINS = 256
FIRST = (127 - 16) * 8                     # 888: bits >> 20 of 2^-16
KR, KG, KB = F32(0.2126), F32(0.7152), F32(0.0722)

Params = collections.namedtuple("Params", "key e_min e_max rate lo hi")
DEFAULTS = Params(F32(0.18), F32(2.0 ** -10), F32(2.0 ** 10), F32(1.0), 500, 950)
FIELDS = ("hist", "ignored", "counted", "kept", "sum", "mean_bits", "target", "clamped", "previous", "applied", "flags")


def params(key=0.18, e_min=2.0 ** -10, e_max=2.0 ** 10, rate=1.0, lo=500, hi=950):
    return Params(F32(key), F32(e_min), F32(e_max), F32(rate), int(lo), int(hi))


def bits(x):
    return int(np.asarray(x, F32).reshape(1).view(np.uint32)[0])


def from_bits(u):
    return np.array([u], np.uint32).view(F32)[0]


def luma(frame):
    """Y, float32, of an [..., 4] (or [..., 3]) array"""
    f = np.asarray(frame, F32)
    with np.errstate(invalid="ignore", over="ignore", under="ignore"):
        return ((KR * f[..., 0] + KG * f[..., 1]).astype(F32) + KB * f[..., 2]).astype(F32)


def histogram(frame):
    """(hist: 256 Python integers, ignored)"""
    y = luma(frame).reshape(-1)
    with np.errstate(invalid="ignore"):
        counted = y > 0
    u = y[counted].view(np.uint32).astype(np.int64)
    k = np.clip((u >> 20) - FIRST, 0, BINS - 1)
    hist = [int(v) for v in np.bincount(k, minlength=BINS)]
    return hist, int(y.size - counted.sum())


def trim(hist, lo, hi):
    """(N, N', S) in Python integers"""
    n = sum(hist)
    skip_lo, skip_hi = n * lo // 1000, n * (1000 - hi) // 1000
    below, kept, s = 0, 0, 0
    for k, v in enumerate(hist):
        c = max(0, min(below + v, n - skip_hi) - max(below, skip_lo))
        kept += c
        s += k * c
        below += v
    return n, kept, s


def mean_bits(s, kept):
    return (FIRST << 20) + ((s << 20) // kept) + (1 << 19)


def target(ybar, key):
    with np.errstate(over="ignore", under="ignore"):
        return F32(F32(key) * F32(F32(1.0) / F32(ybar)))


def expose(frame, p=DEFAULTS, history=None, fallback=1.0):
    """One presentation: (the record as a dict, the history afterwards).  history: None or a float32."""
    hist, ignored = histogram(frame)
    n, kept, s = trim(hist, p.lo, p.hi)
    rec = dict(hist=np.array(hist, np.uint32), ignored=ignored, counted=n, kept=kept, sum=s, mean_bits=0, target=F32(0), clamped=F32(0),
               previous=F32(0) if history is None else F32(history), flags=(0 if history is None else 1) | (0 if n else 2))
    if n == 0:
        rec["applied"] = F32(fallback) if history is None else F32(history)
        return rec, history
    rec["mean_bits"] = mean_bits(s, kept)
    rec["target"] = target(from_bits(rec["mean_bits"]), p.key)
    rec["clamped"] = F32(min(max(rec["target"], p.e_min), p.e_max))
    if history is None or p.rate == F32(1.0):
        e = rec["clamped"]
    else:
        with np.errstate(over="ignore", under="ignore"):
            e = F32(F32(history) + F32(F32(rec["clamped"] - F32(history)) * p.rate))
    rec["applied"] = F32(e)
    return rec, F32(e)


def same_record(got, want):
    """every field of a record read from the device equals the model's, floats bit for bit; returns the first difference"""
    for name in FIELDS:
        g, w = got[name], want[name]
        if name == "hist":
            if not np.array_equal(np.asarray(g, np.int64), np.asarray(w, np.int64)):
                k = np.flatnonzero(np.asarray(g, np.int64) != np.asarray(w, np.int64))[:5]
                return f"hist differs at bins {k.tolist()}: {np.asarray(g)[k].tolist()} against {np.asarray(w)[k].tolist()}"
        elif name in ("target", "clamped", "previous", "applied"):
            if bits(g) != bits(w):
                return f"{name}: {float(g)!r} ({bits(g):#x}) against {float(w)!r} ({bits(w):#x})"
        elif int(g) != int(w):
            return f"{name}: {int(g)} against {int(w)}"
    return None


# ---- the chart ----
CHART_FRAMES = [(1, 1), (2, 2), (3, 5), (64, 64), (257, 33), (512, 256)]   # (w, h)
VARIANTS = (0, 1, 2, 3, 4, 5, "flat", "constant", "ignored")


def pixel_with_luma(u):
    """(r, g, b) whose Y has exactly the bits u: a grey near the value, else a green"""
    y = from_bits(u)
    for make, centre in ((lambda v: (v, v, v), y), (lambda v: (F32(0), v, F32(0)), F32(y / KG))):
        v = F32(centre)
        for _ in range(16):
            v = np.nextafter(v, F32(0))
        for _ in range(33):
            if bits(luma(np.array(make(v), F32))) == u:
                return tuple(F32(t) for t in make(v))
            v = np.nextafter(v, F32(np.inf))
    raise AssertionError(f"no pixel with luma bits {u:#x}")


def hazards():
    """the planted pixels (r, g, b, a): each exercises one clause of the count or one edge of the bins"""
    nan, inf = F32(np.nan), F32(np.inf)
    out = [(nan, 1.0, 1.0, 1.0), (1.0, nan, 0.5, 1.0), (0.25, inf, 0.25, 1.0), (inf, 1.0, -inf, 1.0), (-inf, 1.0, 1.0, 1.0),
           (1e-40, 1e-40, 1e-40, 1.0), (0.0, 1e-45, 0.0, 1.0), (0.0, 0.0, 0.0, 1.0), (-0.0, -0.0, -0.0, 1.0), (-1.0, -1.0, -1.0, 1.0),
           (-1.0, 2.0, 0.0, 1.0), (3.0, -0.5, 1.0, nan), (3.0e38, 3.0e38, 3.0e38, 1.0), (0.5, 0.5, 0.5, -inf)]
    edges = [(FIRST + k) << 20 for k in (1, 2, 100, 128, 129, 255)]          # bin edges
    edges += [(127 - 16) << 23, (127 + 16) << 23]                              # 2^-16 and 2^16
    for e in edges:
        for u in (e - 1, e, e + 1):
            out.append(pixel_with_luma(u) + (F32(1.0),))
    return np.array(out, F32)


_HAZARDS = None


def chart_frame(w, h, variant=0):
    """[h, w, 4] float32.  Variants 0..5: a ramp over twelve octaves with the hazards planted at scattered pixels, rotated by
    the variant (a 1 x 1 frame holds one of them).  "flat": one bin holds almost every pixel, the hazards the rest.
    "constant": one value everywhere.  "ignored": nothing to count (zeros, negatives, NaN)."""
    global _HAZARDS
    if _HAZARDS is None:
        _HAZARDS = hazards()
    hz = _HAZARDS
    n = w * h
    f = np.empty((h, w, 4), F32)
    f[..., 3] = 1.0
    if variant == "constant":
        f[..., :3] = (0.5, 0.4, 0.3)
        return f
    if variant == "ignored":
        f[..., :3] = 0.0
        flat = f.reshape(-1, 4)
        flat[1::3, :3] = -2.5
        flat[2::3, 0] = np.nan
        flat[::7, 2] = -0.0
        return f
    if variant == "flat":
        f[..., :3] = (0.5, 0.4, 0.3)
        rot = 0
    else:
        x = np.arange(w, dtype=np.float64) / max(w - 1, 1)
        y = np.arange(h, dtype=np.float64) / max(h - 1, 1)
        level = np.exp2(12.0 * x[None, :] - 6.0 + 0.37 * y[:, None])
        f[..., 0] = level * (1.0 + 0.5 * y[:, None])
        f[..., 1] = level
        f[..., 2] = level * (1.5 - y[:, None])
        rot = int(variant)
    rng = np.random.default_rng(4099 * w + h + 7919 * rot)
    spots = rng.permutation(n)[:len(hz)]
    flat = f.reshape(-1, 4)
    for i, at in enumerate(spots):
        flat[at] = hz[(i + 7 * rot) % len(hz)]
    return f
