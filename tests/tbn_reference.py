"""CPU restatement of the TBN line overlay's rule, vectorised in numpy.

The parts other passes already pin come from the oracle: the vertex stage (bbo.vertex_stage: posWorld, N, T, B), the
sampler (bbo.sample) and P * V (bbo_proj_view).  Restated here: the fp32 steps specific to tbn.vert / tbn.geom, the
clipper, project_vertex, and the line rule in two independent forms:
  * covers_sat + fragments():  the kernel's form -- candidates along the major axis, separation along three axes;
  * covers_brute():            a per-pixel Liang-Barsky intersection of the perturbed segment with the open diamond,
                               every quantity a symbolic value n + a eps + b eps^2 compared lexicographically."""
from __future__ import annotations

import ctypes as C

import numpy as np

from bibim_renderer_amd.renderer import TBN_SEGMENT_DTYPE
from oracle import bbo

F = np.float32
GUARD = F(4.0)
LENGTH = F(0.05)
NO_KEY = 0xFFFFFFFF
COLOURS = np.array([[255, 0, 0, 255], [0, 255, 0, 255], [0, 0, 255, 255]], np.uint8)


# ---------------------------------------------------------------------------------------------------------------------
# fp32 helpers
# ---------------------------------------------------------------------------------------------------------------------

def fmaf(a, b, c):
    """fp32 fma: the product is exact in binary64; the sum is made error-free (TwoSum) and rounded to odd, from which
    the rounding to fp32 is correct"""
    a, b, c = (np.asarray(v, F).astype(np.float64) for v in (a, b, c))
    p = a * b
    s = p + c
    bb = s - p
    e = (p - (s - bb)) + (c - bb)
    bits = s.view(np.int64).copy()
    fix = (e != 0) & ((bits & 1) == 0)
    toward = np.where(np.signbit(e) == np.signbit(s), 1, -1)
    bits = np.where(fix, bits + toward, bits)
    return bits.view(np.float64).astype(F)


def cross(a, b):
    return np.stack([a[..., 1] * b[..., 2] - a[..., 2] * b[..., 1], a[..., 2] * b[..., 0] - a[..., 0] * b[..., 2],
                     a[..., 0] * b[..., 1] - a[..., 1] * b[..., 0]], -1)


def mean3(a, b, c):
    return ((a + b) + c) / F(3.0)


def normalize(v):
    with np.errstate(invalid="ignore", divide="ignore"):
        l = np.sqrt((v[..., 0] * v[..., 0] + v[..., 1] * v[..., 1]) + v[..., 2] * v[..., 2])
        return v / l[..., None]


def to_clip(m, p):
    """vCombined * (p, 1), m column-major [col][row]"""
    return np.stack([((m[0, i] * p[..., 0] + m[1, i] * p[..., 1]) + m[2, i] * p[..., 2]) + m[3, i] * F(1.0) for i in range(4)],
                    -1)


def proj_view(view):
    out = np.zeros((4, 4), F)
    bbo.lib().bbo_proj_view(bbo._p(view), out.ctypes.data_as(C.c_void_p))
    return out


def project(c, half_w, half_h):
    """project_vertex (bb_kernels.hip.h): 1/w, fmaf to the viewport, rintf(x 256)"""
    with np.errstate(all="ignore"):
        w = c[..., 3]
        ok = w > 0
        r = F(1.0) / w
        xs = fmaf(c[..., 0] * r, F(half_w), F(half_w))
        ys = fmaf(c[..., 1] * r, F(half_h), F(half_h))
        ok &= (np.abs(xs) <= F(4194304.0)) & (np.abs(ys) <= F(4194304.0))
        X = np.where(ok, np.rint(xs * F(256.0)), 0).astype(np.int64)
        Y = np.where(ok, np.rint(ys * F(256.0)), 0).astype(np.int64)
        z = c[..., 2] * r
    return ok, X, Y, z


def clip_segments(p0, p1):
    """Liang-Barsky against z <= w, z >= 0, |x|, |y| <= 4 w; returns (ok, q0, q1)"""
    with np.errstate(all="ignore"):
        ok = np.isfinite(p0).all(-1) & np.isfinite(p1).all(-1)
        t0 = np.zeros(len(p0), F)
        t1 = np.ones(len(p0), F)

        def planes(c):
            return [c[:, 3] - c[:, 2], c[:, 2], GUARD * c[:, 3] + c[:, 0], GUARD * c[:, 3] - c[:, 0], GUARD * c[:, 3] + c[:, 1],
                    GUARD * c[:, 3] - c[:, 1]]

        for d0, d1 in zip(planes(p0), planes(p1)):
            ok &= ~((d0 < 0) & (d1 < 0))
            t = d0 / (d0 - d1)
            t0 = np.where(d0 < 0, np.maximum(t0, t), t0)
            t1 = np.where(~(d0 < 0) & (d1 < 0), np.minimum(t1, t), t1)
        ok &= ~(t0 > t1)
        q0 = np.where((t0 > 0)[:, None], p0 + t0[:, None] * (p1 - p0), p0)
        q1 = np.where((t1 < 1)[:, None], p0 + t1[:, None] * (p1 - p0), p1)
    return ok, q0, q1


def make_segments(p0, p1, keys, width, height):
    """clip + snap strip segments (clip-space endpoints [n, 4]); records of the ones that survive"""
    ok, q0, q1 = clip_segments(p0, p1)
    o0, X0, Y0, z0 = project(q0, 0.5 * F(width), 0.5 * F(height))
    o1, X1, Y1, z1 = project(q1, 0.5 * F(width), 0.5 * F(height))
    ok &= o0 & o1 & ((X0 != X1) | (Y0 != Y1))
    r = np.zeros(int(ok.sum()), TBN_SEGMENT_DTYPE)
    r["x0"], r["y0"], r["x1"], r["y1"] = X0[ok], Y0[ok], X1[ok], Y1[ok]
    r["za"], r["zb"], r["key"] = z0[ok], z1[ok], keys[ok]
    return r


# ---------------------------------------------------------------------------------------------------------------------
# per-triangle stage (tbn.vert + tbn.geom)
# ---------------------------------------------------------------------------------------------------------------------

def _vertex_frames(view, inst, verts, used, nmap, enable):
    """posWorld, N, T, B of the vertices `used` for one instance"""
    pw = np.zeros((len(verts), 3), F)
    N = np.zeros((len(verts), 3), F)
    T = np.zeros((len(verts), 3), F)
    B = np.zeros((len(verts), 3), F)
    nt = np.zeros((len(verts), 3), F)
    for i in used:
        _, vary = bbo.vertex_stage(view, inst, verts[i:i + 1])
        pw[i], N[i], T[i], B[i] = vary[2:5], vary[5:8], vary[8:11], vary[11:14]
        if enable:
            nt[i] = bbo.sample(nmap, 4, verts[i]["uv"][0], verts[i]["uv"][1])[:3] * F(2.0) - F(1.0)
    if enable:
        n = (T * nt[:, 0:1] + B * nt[:, 1:2]) + N * nt[:, 2:3]
        bn = np.zeros_like(n)
        bn[:, 0] = 1.0
        same = (n[:, 0] == 1.0) & (n[:, 1] == 0.0) & (n[:, 2] == 0.0)
        bn[same] = (0.0, 0.0, 1.0)
        with np.errstate(all="ignore"):
            tn = cross(n, bn)
            bn = cross(n, tn)
        N, T, B = n, tn, bn
    return pw, N, T, B


def tbn_records(scene):
    """every segment record of the scene's TBN draw, in key order"""
    view = scene.view
    pv = proj_view(view)
    enable = int(view["enable_normal_map"]) != 0
    out = []
    first = 0
    for d in scene.draws:
        verts = d.vertices
        idx = d.indices if d.indices is not None else np.arange(len(verts), dtype=np.uint32)
        tris = len(idx) // 3
        idx = idx[:3 * tris].astype(np.int64)
        used = np.unique(idx)
        nmap = d.material.maps.get("normal")
        for ii in range(len(d.instances)):
            pw, N, T, B = _vertex_frames(view, d.instances[ii:ii + 1], verts, used, nmap, enable)
            tri = idx.reshape(tris, 3)
            with np.errstate(all="ignore"):
                Cn = mean3(pw[tri[:, 0]], pw[tri[:, 1]], pw[tri[:, 2]])
                ends = [normalize(mean3(V[tri[:, 0]], V[tri[:, 1]], V[tri[:, 2]])) * LENGTH for V in (T, B, N)]
                cc = to_clip(pv, Cn)
                ce = [to_clip(pv, Cn + e) for e in ends]
            strip = [cc, ce[0], cc, cc, ce[1], cc, cc, ce[2], cc]
            prim = (first + ii * tris + np.arange(tris, dtype=np.int64))
            for s in range(8):
                out.append(make_segments(strip[s], strip[s + 1], (prim * 8 + s).astype(np.uint32), scene.width, scene.height))
        first += tris * len(d.instances)
    r = np.concatenate(out) if out else np.zeros(0, TBN_SEGMENT_DTYPE)
    return r[np.argsort(r["key"], kind="stable")]


# ---------------------------------------------------------------------------------------------------------------------
# the line rule
# ---------------------------------------------------------------------------------------------------------------------

def covers_sat(ax, ay, bx, by):
    """kernel form (tbn_covers): endpoints relative to the fragment centre, 1/256 pixel, int64 arrays"""
    eb = np.abs(bx) + np.abs(by)
    ok = ~((eb < 128) | ((eb == 128) & (bx > 0)))
    au, bu = ax + ay, bx + by
    ok &= ~((np.maximum(au, bu) <= -128) | (np.minimum(au, bu) >= 129))
    av, bv = ax - ay, bx - by
    ok &= ~((np.maximum(av, bv) <= -128) | (np.minimum(av, bv) >= 129))
    dx, dy = bx - ax, by - ay
    c = dx * ay - dy * ax
    h = 128 * np.maximum(np.abs(dx), np.abs(dy))
    ok &= ~((c > h) | ((c == h) & ((dy > 0) | ((dy == 0) & (dx < 0)))))
    ok &= ~((c < -h) | ((c == -h) & ((dy < 0) | ((dy == 0) & (dx > 0)))))
    return ok


def _lexpos(n, a, b):
    """n + a eps + b eps^2 > 0"""
    return (n > 0) | ((n == 0) & ((a > 0) | ((a == 0) & (b > 0))))


def covers_brute(ax, ay, bx, by):
    """Independent form: the perturbed segment A' + t (B' - A'), t in [0, 1], meets the open diamond (four strict
    half-planes g_k > 0, pairwise Liang-Barsky conditions on symbolic values), and B' lies outside it"""
    dx, dy = bx - ax, by - ay
    hit = np.ones(np.broadcast(ax, bx).shape, bool)
    b_inside = np.ones_like(hit)
    g, q = [], []
    for s1, s2 in ((1, 1), (-1, -1), (1, -1), (-1, 1)):
        # g = 128 - s1 x - s2 y at A' = (ax - eps, ay - eps^2): (128 - s1 ax - s2 ay) + s1 eps + s2 eps^2
        gk = (128 - s1 * ax - s2 * ay, s1, s2)
        qk = -(s1 * dx + s2 * dy)
        g.append(gk)
        q.append(qk)
        at_b = _lexpos(gk[0] + qk, np.full_like(qk, s1), np.full_like(qk, s2))  # g at B'
        b_inside &= at_b
        hit &= np.where(qk == 0, _lexpos(gk[0], s1, s2), True)
        hit &= np.where(qk > 0, at_b, True)                           # lower bound below 1
        hit &= np.where(qk < 0, _lexpos(gk[0], s1, s2), True)          # upper bound above 0
    for k in range(4):
        for m in range(4):
            # lower bound -g_k / q_k (q_k > 0) below upper bound g_m / (-q_m) (q_m < 0):  g_m q_k - g_k q_m > 0
            n = g[m][0] * q[k] - g[k][0] * q[m]
            a = g[m][1] * q[k] - g[k][1] * q[m]
            b = g[m][2] * q[k] - g[k][2] * q[m]
            hit &= np.where((q[k] > 0) & (q[m] < 0), _lexpos(n, a, b), True)
    return hit & ~b_inside & ((dx != 0) | (dy != 0))


def fragments_brute(seg, width, height):
    """every pixel of the segment's bounding box (+1) tested with covers_brute: (px, py) arrays"""
    X0, Y0, X1, Y1 = (int(seg[k]) for k in ("x0", "y0", "x1", "y1"))
    px = np.arange(max((min(X0, X1) >> 8) - 1, 0), min((max(X0, X1) >> 8) + 2, width), dtype=np.int64)
    py = np.arange(max((min(Y0, Y1) >> 8) - 1, 0), min((max(Y0, Y1) >> 8) + 2, height), dtype=np.int64)
    PX, PY = np.meshgrid(px, py)
    fx, fy = 256 * PX + 128, 256 * PY + 128
    m = covers_brute(X0 - fx, Y0 - fy, X1 - fx, Y1 - fy)
    return PX[m], PY[m]


def fragments(segs, width, height):
    """kernel form over many segments: (segment index, px, py) of every fragment inside the target"""
    X0, Y0, X1, Y1 = (segs[k].astype(np.int64) for k in ("x0", "y0", "x1", "y1"))
    dx, dy = X1 - X0, Y1 - Y0
    xm = np.abs(dx) >= np.abs(dy)
    ma0, ma1, mi0 = np.where(xm, X0, Y0), np.where(xm, X1, Y1), np.where(xm, Y0, X0)
    dma, dmi = np.where(xm, dx, dy), np.where(xm, dy, dx)
    lima, limi = np.where(xm, width, height), np.where(xm, height, width)
    lo = np.maximum((np.minimum(ma0, ma1) >> 8) - 1, 0)
    hi = np.minimum((np.maximum(ma0, ma1) >> 8) + 1, lima - 1)
    cnt = np.where((dx != 0) | (dy != 0), np.maximum(hi - lo + 1, 0), 0)
    seg = np.repeat(np.arange(len(segs)), cnt)
    start = np.cumsum(cnt) - cnt
    i = lo[seg] + (np.arange(len(seg)) - start[seg])
    with np.errstate(all="ignore"):
        mc = mi0[seg].astype(np.float64) + (256 * i + 128 - ma0[seg]).astype(np.float64) * dmi[seg].astype(np.float64) / dma[seg].astype(np.float64)
    j0 = np.floor((mc - 128.0) / 256.0).astype(np.int64)
    out_s, out_x, out_y = [], [], []
    for off in (-1, 0, 1, 2):
        j = j0 + off
        keep = (j >= 0) & (j < limi[seg])
        s, ii, jj = seg[keep], i[keep], j[keep]
        px, py = np.where(xm[s], ii, jj), np.where(xm[s], jj, ii)
        fx, fy = 256 * px + 128, 256 * py + 128
        m = covers_sat(X0[s] - fx, Y0[s] - fy, X1[s] - fx, Y1[s] - fy)
        out_s.append(s[m]); out_x.append(px[m]); out_y.append(py[m])
    return np.concatenate(out_s), np.concatenate(out_x), np.concatenate(out_y)


def resolve(segs, width, height, depth, chunk=200_000):
    """[height, width] uint32: key + 1 of the largest-key fragment that passes z >= depth, 0 where none"""
    keys = np.zeros(height * width, np.uint32)
    for c0 in range(0, len(segs), chunk):
        sg = segs[c0:c0 + chunk]
        s, px, py = fragments(sg, width, height)
        X0, Y0 = sg["x0"].astype(np.int64)[s], sg["y0"].astype(np.int64)[s]
        dx, dy = sg["x1"].astype(np.int64)[s] - X0, sg["y1"].astype(np.int64)[s] - Y0
        num = (256 * px + 128 - X0) * dx + (256 * py + 128 - Y0) * dy
        t = num.astype(np.float64) / (dx * dx + dy * dy).astype(np.float64)
        z = ((1.0 - t) * sg["za"][s].astype(np.float64) + t * sg["zb"][s].astype(np.float64)).astype(F)
        ok = z >= depth[py, px]
        np.maximum.at(keys, (py * width + px)[ok], sg["key"][s][ok] + np.uint32(1))
    return keys.reshape(height, width)


def composite(base_rgba8, keys):
    """the lines over a presented image: pixels with a winning segment take its flat colour"""
    out = np.array(base_rgba8, np.uint8, copy=True)
    m = keys != 0
    out[m] = COLOURS[((keys[m] - 1) & 7) // 3]
    return out
