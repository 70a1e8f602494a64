"""The bloom rule (include/bibim_hip.h, "bloom"), restated in numpy on whole arrays, and the chart of frames the GPU tests
present.  Written from the rule's text alone; nothing here knows the kernels.

Every operation is one np.float32 operation on float32 arrays: numpy adds, subtracts and multiplies binary32 values with one
rounding to nearest even each, keeps denormals and never fuses a product into a sum.  tests/test_bloom_reference.py checks
that against exact rational arithmetic rounded operation by operation.

    sizes    w_0 = W, h_0 = H;  w_k = (w_{k-1} + 1) >> 1, h_k likewise, k = 1 .. L
    bright   e = min(max0(F - T), 65504)           max0(d) = d > 0 ? d : 0
    box      ((G(x0,y0) + G(x1,y0)) + (G(x0,y1) + G(x1,y1))) * 0.25     x0 = min(2x, w-1), x1 = min(2x+1, w-1)
    down     D_1 = box(e);  D_{k+1} = box(D_k)
    lerp4    a + (b - a) * 0.25
    up       px = x >> 1, qx = clamp(px + (x odd ? 1 : -1), 0, w'-1);  lerp4(lerp4(G(px,py), G(qx,py)), lerp4(G(px,qy), G(qx,qy)))
    sum      U_L = D_L;  U_k = D_k + up(U_{k+1})
    pixel    v = F + I * up(U_1)
"""
import numpy as np

from oracle import bbo

F32 = np.float32
QUARTER = F32(0.25)
BRIGHT_MAX = F32(65504.0)
MAX_LEVELS = 8


def level_sizes(w, h, levels):
    """[(w_0, h_0), (w_1, h_1), ..., (w_L, h_L)]"""
    out = [(int(w), int(h))]
    for _ in range(levels):
        out.append(((out[-1][0] + 1) >> 1, (out[-1][1] + 1) >> 1))
    return out


def bright(frame, threshold):
    """e: [H, W, 3] from the r, g, b of an [H, W, 4] frame"""
    with np.errstate(invalid="ignore", over="ignore"):
        d = np.asarray(frame, F32)[..., :3] - F32(threshold)
        e = np.where(d > 0, d, F32(0.0)).astype(F32)      # NaN -> +0, -0 -> +0, -inf -> 0
        return np.minimum(e, BRIGHT_MAX)                   # +inf -> 65504


def box(g):
    h, w = g.shape[:2]
    x, y = np.arange((w + 1) >> 1), np.arange((h + 1) >> 1)
    x0, x1 = np.minimum(2 * x, w - 1), np.minimum(2 * x + 1, w - 1)
    y0, y1 = np.minimum(2 * y, h - 1), np.minimum(2 * y + 1, h - 1)
    top = g[y0][:, x0] + g[y0][:, x1]
    bottom = g[y1][:, x0] + g[y1][:, x1]
    return ((top + bottom) * QUARTER).astype(F32)


def lerp4(a, b):
    return (a + (b - a) * QUARTER).astype(F32)


def up(g, wf, hf):
    """g: a level [h', w', 3]; the result has the next finer grid's extent [hf, wf, 3]"""
    h, w = g.shape[:2]
    x, y = np.arange(wf), np.arange(hf)
    px, py = x >> 1, y >> 1
    qx = np.clip(px + np.where(x & 1, 1, -1), 0, w - 1)
    qy = np.clip(py + np.where(y & 1, 1, -1), 0, h - 1)
    r0 = lerp4(g[py][:, px], g[py][:, qx])
    r1 = lerp4(g[qy][:, px], g[qy][:, qx])
    return lerp4(r0, r1)


def down_levels(frame, levels, threshold):
    """[None, D_1, ..., D_L]"""
    d = [None, box(bright(frame, threshold))]
    for _ in range(1, levels):
        d.append(box(d[-1]))
    return d


def pyramid(frame, levels, threshold):
    """[None, U_1, ..., U_L], each float32 [h_k, w_k, 3]"""
    d = down_levels(frame, levels, threshold)
    u = list(d)
    for k in range(levels - 1, 0, -1):
        u[k] = (d[k] + up(u[k + 1], d[k].shape[1], d[k].shape[0])).astype(F32)
    return u


def bloomed(frame, levels, threshold, intensity):
    """v: the frame with I * B added to r, g, b (alpha as it was); levels 0: the frame itself"""
    frame = np.asarray(frame, F32)
    if levels == 0:
        return frame.copy()
    h, w = frame.shape[:2]
    b = up(pyramid(frame, levels, threshold)[1], w, h)
    out = frame.copy()
    with np.errstate(invalid="ignore", over="ignore"):
        out[..., :3] = frame[..., :3] + F32(intensity) * b
    return out


def image(frame, levels, threshold, intensity, enable, exposure, hdr16=True):
    """the presented RGBA8 image [H, W, 4]"""
    v = bloomed(frame, levels, threshold, intensity)
    return bbo.present(v.reshape(-1, 4), enable, exposure, hdr16).reshape(v.shape[0], v.shape[1], 4)


# ---- the chart ----
CHART_FRAMES = [(1, 1), (2, 2), (3, 5), (33, 17), (64, 64), (257, 131)]   # (w, h)
CHART_LEVELS = [1, 2, 3, 8]
SMALL_FRAMES = [(1, 1), (2, 2), (3, 5), (7, 4)]                            # what the scalar restatement walks
CHART_THRESHOLD = F32(1.0)
CHART_INTENSITY = F32(0.25)


def hazards(threshold):
    """the planted values: each exercises one clause of the bright pass or one edge of binary32"""
    t = F32(threshold)
    return np.array([np.nan, np.inf, -np.inf, -0.0, -3.5, -1e30, 1e-45, 1e-39, -1e-40, t, np.nextafter(t, F32(np.inf)),
                     np.nextafter(t, F32(-np.inf)), 65504.0, F32(65505.0) + t, 1e30, 3.0e38], F32)


def chart_frame(w, h, threshold=CHART_THRESHOLD, variant=0):
    """[h, w, 4] float32: a smooth field around the threshold with the hazards planted at the corners, along the last (odd)
    column and row, and in the interior; `variant` rotates which hazard lands where (a 1 x 1 frame holds three of them)"""
    rng = np.random.default_rng(1000 * w + h + 7919 * variant)
    f = (rng.random((h, w, 4), dtype=F32) * F32(4.0) * F32(threshold)).astype(F32)
    f[..., 3] = 1.0
    hz = hazards(threshold)
    spots = [(0, 0), (w - 1, 0), (0, h - 1), (w - 1, h - 1), (w - 1, h // 2), (w // 2, h - 1), (w - 1, h // 3), (w // 3, h - 1),
             (w // 2, h // 2), (w // 3, h // 3), (2 * w // 3, h // 2), (w // 2, 2 * h // 3), (w // 4, 3 * h // 4), (3 * w // 4, h // 4),
             (w // 5, h // 2), (w // 2, h // 5)]
    for i, (x, y) in enumerate(spots):
        for c in range(3):
            f[y, x, c] = hz[(3 * i + c + variant) % len(hz)]
    if w > 8 and h > 8:
        f[h // 2 + 2, w // 2 + 1:w // 2 + 4, :3] = 50.0     # a light of intensity 50, three pixels wide
    return f


def same_bits(a, b):
    """equal as bit patterns (so +0 and -0 differ, and a NaN equals itself)"""
    a, b = np.ascontiguousarray(a, F32), np.ascontiguousarray(b, F32)
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))
