"""Vertex chart: two 160 x 128 frames whose primitives are a CHOSEN population of (instance, vertex) pairs for the vertex
stage (`k_geometry` / `k_tbn_segments`, csrc/bb_kernels.hip.h; oracle `vertex_stage`: forward_brdf.vert / gbuffer.vert).
TEST INFRASTRUCTURE ONLY.

  frame     8 x 8 pixel cells on a grid shifted by 4 pixels (19 x 15 cells), so that the columns at x = 28 and 60 and the
            rows at y = 28 and 60 lie across the 32- and 64-pixel tile borders; one small triangle per cell.  A cell's
            SCREEN position and clip w are chosen first, its object-space positions are solved for through model * view *
            proj in binary64 and rounded; the vertex order is the one that faces the camera.
  views     "main": perspective camera at the origin looking down +z, every class but the last.
            "near": the same camera moved along the translation of the last instance class, (1e6, 0, 0): that class'
            cells (the product (P*V) * posWorld cancels six digits there, V * posWorld does not) and the row NEAR_ROW whose
            triangles have their third vertex behind the camera -- they cross the near plane and go through the clipper.
            Each view sees only its own cells: the others lie 1e6 to the side, outside the frustum.
  classes   INSTANCE_CLASSES x VERTEX_CLASSES below; uv hazards cycle over the cells (UV_CLASSES).
  draws     twelve (past the three inline first_prim), indexed and not; draw 1's index buffer permutes its triangles and
            shares a vertex between two of them; draw 0 has seven instances of eight triangles; two materials alternate
            (one packed, one with maps of different sizes).

Census.  The squared length of a transformed normal / tangent decides what `normalize` does with it; `category` names it
in binary64 on the binary32 inputs, a factor 2 clear of every threshold (what is not clear is "borderline"):
    normal | denormal | zero (underflows, the vector is not zero) | inf | vzero (the vector is zero) | vinf (an infinite
    component) | nan
PATTERN states by hand what the contract's normalize (v * rsqrt(dot(v, v)), rsqrt(x) = 1 / sqrtf(x) outside the positive
normal numbers) makes of each; SCALE_LENGTH_CATEGORY states by hand where inv_model = s * rotation with |n| = l lands.

Bound of the binary64 comparison (cells whose six squared lengths are "normal"), u = 2^-24, first order in u with a
factor 1 + 2^-10 for the rest.  A k-term fmaf chain r = fl(sum a_i b_i) has |r - sum a_i b_i| <= k u sum |a_i b_i| (k
roundings, each relative to a partial sum bounded by sum |a_i b_i|).  Hence, with |.| taken entry by entry:
    posWorld   e_pw   = 4 u |pos| |model|
    P*V        e_PV   = 4 u |V| |P|                       (the host's binary32 product: one more such stage)
    forward    e_clip = 4 u |pw| |V| |P|  +  |pw| e_PV  +  e_pw |V| |P|          (|P*V| <= |V| |P|)
    deferred   e_view = 4 u |pw| |V| + e_pw |V|;   e_clip = 4 u |pv| |P| + e_view |P|
    v = normalMat * n   e_v = 3 u sum |inv_model_ij n_j|,  rho = ||e_v|| / ||v||
    normalize  every component of N = v / ||v|| moves by at most 2 rho (d N_c = d v_c / ||v|| - N_c (N . d v) / ||v||),
               and the evaluation adds 4 u (dot3 and the final product; bb_rsqrt is 1.1 ulp):  e_N = 2 rho + 4 u
    B = cross(N, T)   e_B_x = 2 u (|N_y T_z| + |N_z T_y|) + e_N (|T_z| + |T_y|) + e_T (|N_y| + |N_z|), cyclic
uv is a copy: its bits are compared."""
from __future__ import annotations

import functools
from types import SimpleNamespace

import numpy as np

from oracle import bbo, scenes

W, H = 160, 128
CELL, OFF, COLS, ROWS = 8, 4, 19, 15
NEAR_ROW = ROWS - 1
SEEDS = {"depth": 41, "material": 43, "shuffle": 47}
U = 2.0 ** -24
SLACK = 1.0 + 2.0 ** -10
F = np.float32
f64 = lambda a: np.asarray(a, np.float64)
NO_CLIP = 0xFFFFFFFF
FILL = 0xFFFFFFFF
FAR = 1.0e6                                        # the translation of the last class and of the "near" camera
VIEWS = ("main", "near")
CORNERS = ((1.3, 1.2), (6.9, 1.6), (1.7, 6.8))     # a cell's triangle, pixels from the cell's corner
NAN_A, NAN_B = 0x7FC12345, 0xFFC54321              # quiet NaNs with a payload


def _bits_to_f32(b):
    return np.array([b], np.uint32).view(F)[0]


# ---------------------------------------------------------------------------------------------------------------------
# classes
# ---------------------------------------------------------------------------------------------------------------------
VERTEX_CLASSES = ("unit", "short", "long", "parallel", "zero tangent", "denormal normal", "inf normal", "mixed")
UV_CLASSES = ("plain", "-0.0", "+-3e38", "denormal", "nan payload")
INV_SCALES = {"inv 1e-18": 1e-18, "inv 1e-22": 1e-22, "inv 1e-25": 1e-25, "inv 1e18": 1e18, "inv 1e20": 1e20}
ROTATED = ("rotated", "inv 1e-18", "inv 1e-22", "inv 1e-25", "inv 1e18", "inv 1e20", "nan inf outside")  # draw 0's instances
INSTANCE_CLASSES = ROTATED + ("identity", "scene", "nonuniform a", "nonuniform b", "mirrored", "identity inverse",
                              "rank 2", "rank 1", "w = 2", "projective", "translated 1e6")
HAZARDS = ("denormal", "zero", "inf", "vzero", "vinf", "nan")
# By hand: inv_model = s * (a rotation), |n| = l: the squared length (s l)^2 against binary32's normal range
# [1.18e-38, 3.4e38] and its smallest denormal 1.4e-45.
SCALE_LENGTH_CATEGORY = {
    ("inv 1e-18", "unit"): "normal",   ("inv 1e-18", "short"): "denormal", ("inv 1e-18", "long"): "normal",       # 1e-36 1e-42 1e-30
    ("inv 1e-22", "unit"): "denormal", ("inv 1e-22", "short"): "zero",     ("inv 1e-22", "long"): "borderline",   # 1e-44 1e-50 1e-38
    ("inv 1e-25", "unit"): "zero",     ("inv 1e-25", "short"): "zero",     ("inv 1e-25", "long"): "denormal",     # 1e-50 1e-56 1e-44
    ("inv 1e18", "unit"): "normal",    ("inv 1e18", "short"): "normal",    ("inv 1e18", "long"): "inf",           # 1e36 1e30 1e42
    ("inv 1e20", "unit"): "inf",       ("inv 1e20", "short"): "normal",    ("inv 1e20", "long"): "inf",           # 1e40 1e34 1e46
}
# By hand: what normalize(v) = v * rsqrt(dot(v, v)) is, per category of v (c: a component)
PATTERN = {
    "normal": "unit length (1e-5)",
    "borderline": "finite", "denormal": "finite",            # 1 / sqrtf of a denormal: finite, a few bits (length 0.9 .. 1.1)
    "zero": "c != 0: +-inf with c's sign; c == 0: NaN",      # rsqrt(0) = inf
    "inf": "+-0 with c's sign",                              # rsqrt(inf) = 0, v finite
    "vzero": "NaN",                                          # 0 * inf
    "vinf": "c infinite: NaN; else +-0 with c's sign",       # inf * 0
    "nan": "NaN",
}
# The cells left out of the binary64 comparison, planned by hand.  There are 19 rows of the 8 vertex classes (7 + 1 + 9 in the
# main view, 2 in the near view) and the two cells with the shared vertex.  In every row "zero tangent", "denormal normal", "inf
# normal" and "mixed" (its third vertex has a zero tangent) are hazards: 4 of 8, and both shared cells are "mixed".  The five
# scaled rows add what SCALE_LENGTH_CATEGORY does not call normal among their other four cells ("parallel" counts as "unit"):
# 1, 4, 4, 1 and 3.  "rank 2" / "rank 1" only remove a direction: none planned.
PLANNED_HAZARD_SHARE = (4 * 19 + 2 + (1 + 4 + 4 + 1 + 3)) / (8 * 19 + 2)


def _unit(a):
    a = f64(a)
    return a / np.sqrt((a * a).sum(-1))[..., None]


N0 = _unit((0.36, 0.48, -0.8))
T0 = _unit(np.cross(N0, (0.0, 1.0, 0.25)))


def vertex_attributes(vclass, k):
    """(normal, tangent) of vertex k of a triangle of class `vclass`, binary32; the normal differs from vertex to vertex"""
    n = _unit(N0 + 0.15 * np.eye(3)[k])
    t = _unit(np.cross(n, np.cross(T0, n)))
    kind = vclass if vclass != "mixed" else ("unit", "long", "zero tangent")[k]
    if kind == "short":
        n, t = n * 1e-3, t * 1e-3
    elif kind == "long":
        n, t = n * 1e3, t * 1e3
    elif kind == "parallel":
        t = n
    elif kind == "zero tangent":
        t = np.zeros(3)
    elif kind == "denormal normal":
        n = np.array([1e-40, 0.0, 0.0])
    elif kind == "inf normal":
        n = np.array([np.inf, 0.5, 0.25])
    return n.astype(F), t.astype(F)


def vertex_uv(uclass, k, cell):
    uv = (np.array([(0.125, 0.25), (0.75, 0.375), (0.5, 0.875)][k]) + 0.001 * cell).astype(F)
    if uclass == "-0.0" and k == 0:
        uv[0] = F(-0.0)
    elif uclass == "+-3e38" and k == 1:
        uv[:] = (3e38, -3e38)
    elif uclass == "denormal" and k == 2:
        uv[1] = F(1e-41)
    elif uclass == "nan payload" and k == 1:
        uv[0], uv[1] = _bits_to_f32(NAN_A), _bits_to_f32(NAN_B)
    return uv


def _rot(*steps):
    m = np.eye(4, dtype=F)
    for axis, deg in steps:
        m = bbo.mat_mul(m, {"x": bbo.mat_rotate_x, "y": bbo.mat_rotate_y, "z": bbo.mat_rotate_z}[axis](deg))
    return m


def instance_matrices(iclass):
    """(model, inv_model) of a class, binary32 [column][row]"""
    eye = np.eye(4, dtype=F)
    if iclass in ROTATED:
        m = bbo.mat_mul(bbo.mat_translate(0.25, -0.125, 0.5), _rot(("y", -90.0), ("x", -90.0)))
        inv = bbo.mat_inverse(m)
        if iclass in INV_SCALES:
            inv = inv.copy()
            inv[:3, :3] = (f64(inv[:3, :3]) * INV_SCALES[iclass]).astype(F)
        if iclass == "nan inf outside":           # must change nothing: the shader reads mat3(aInvModel)
            inv = inv.copy()
            inv[3, :] = (np.nan, np.inf, -np.inf, np.nan)
            inv[:3, 3] = (np.inf, np.nan, -np.inf)
        return m, inv
    if iclass == "identity":
        return eye, eye
    if iclass == "scene":                         # src/scene.cpp:180-187
        m = bbo.mat_mul(bbo.mat_mul(bbo.mat_mul(bbo.mat_translate(0.0, -1.0, 2.0), bbo.mat_rotate_y(-90.0)), bbo.mat_rotate_x(-90.0)),
                        bbo.mat_scale(0.01))
        return m, bbo.mat_inverse(m)
    if iclass in ("nonuniform a", "nonuniform b"):
        r = _rot(("y", 30.0), ("x", 20.0)) if iclass.endswith("a") else _rot(("z", -50.0), ("y", 70.0))
        m = bbo.mat_mul(r, bbo.mat_scale(1.0, 1e-3, 1e3))
        return m, bbo.mat_inverse(m)
    if iclass == "mirrored":
        m = bbo.mat_scale(-1.0, 1.0, 1.0)
        return m, bbo.mat_inverse(m)
    if iclass == "identity inverse":              # inv_model is NOT the inverse: the ABI takes it verbatim
        return _rot(("y", 40.0), ("x", -25.0)), eye
    if iclass in ("rank 2", "rank 1"):
        m = _rot(("y", 15.0))
        inv = bbo.mat_inverse(_rot(("z", 35.0), ("x", 50.0))).copy()
        inv[2, :3] = 0.0                          # (normalMat * n)_i = dot(inv_model column i, n): N.z = 0
        if iclass == "rank 1":
            inv[1, :3] = inv[0, :3]
        return m, inv
    if iclass == "w = 2":
        m = eye.copy(); m[3, 3] = 2.0
        return m, eye
    if iclass == "projective":
        m = eye.copy(); m[0, 3], m[1, 3] = 0.05, -0.03
        return m, eye
    if iclass == "translated 1e6":
        return bbo.mat_translate(FAR, 0.0, 0.0), bbo.mat_translate(-FAR, 0.0, 0.0)
    raise KeyError(iclass)


# ---------------------------------------------------------------------------------------------------------------------
# camera
# ---------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(None)
def view_uniforms(name, enable_normal_map=1):
    cam = (FAR, 0.0, 0.0) if name == "near" else (0.0, 0.0, 0.0)
    return scenes.view_uniforms(cam, 0.0, 0.0, W, H, enable_normal_map, 60.0, 0.1, 1000.0)


def _solve(C, sx, sy, w):
    """the point p with (p, 1) @ C projecting to screen (sx, sy) [pixels] at clip w; C = model @ view @ proj, binary64"""
    nx, ny = sx / (0.5 * W) - 1.0, sy / (0.5 * H) - 1.0
    cols = [C[:, 0] - nx * C[:, 3], C[:, 1] - ny * C[:, 3], C[:, 3]]
    A = np.stack([c[:3] for c in cols])
    b = np.array([-cols[0][3], -cols[1][3], w - cols[2][3]])
    return np.linalg.solve(A, b)


def _screen(C, p):
    c = np.append(f64(p), 1.0) @ C
    return np.array([(c[0] / c[3] + 1.0) * 0.5 * W, (c[1] / c[3] + 1.0) * 0.5 * H]), c


# ---------------------------------------------------------------------------------------------------------------------
# the plan
# ---------------------------------------------------------------------------------------------------------------------
def _materials():
    rng = np.random.Generator(np.random.PCG64(SEEDS["material"]))
    tex = lambda h, w: rng.integers(0, 256, (h, w, 4), dtype=np.uint8)
    packed = {k: tex(32, 32) for k in ("albedo", "metallic", "roughness", "ao", "normal")}
    mixed = {"albedo": tex(32, 32), "roughness": tex(16, 16), "ao": tex(24, 40), "normal": tex(64, 64)}
    for m in (packed, mixed):
        m["roughness"][..., 0] = np.maximum(m["roughness"][..., 0], 24)
    return bbo.MaterialData(packed), bbo.MaterialData(mixed)


@functools.lru_cache(None)
def plan():
    """the draws and, per primitive, where and what it is: .draws, .cells (list of SimpleNamespace in primitive order)"""
    rng = np.random.Generator(np.random.PCG64(SEEDS["depth"]))
    mats = _materials()
    VP = {v: f64(view_uniforms(v)["view"]) @ f64(view_uniforms(v)["proj"]) for v in VIEWS}
    draws, cells = [], []
    cell_no = [0]

    def triangle(C, col, row, w, corners, spread=0.004):
        """object-space positions [3, 3] (binary32) of a cell's triangle"""
        x0, y0 = OFF + CELL * col, OFF + CELL * row
        return np.stack([_solve(C, x0 + cx, y0 + cy, w * (1.0 + spread * k)) for k, (cx, cy) in enumerate(corners)]).astype(F)

    def faces_camera(C, p):
        c = np.stack([np.append(f64(q), 1.0) @ C for q in p])
        return np.linalg.det(c[:, [0, 1, 3]]) > 0          # the sign of the screen-space area of the part in front of the camera

    def mesh_for(C, specs):
        """specs: list of (col, row, w, vclass, near, corners) -> vertices [3 n], cell records"""
        v = np.zeros(3 * len(specs), bbo.VERTEX_DTYPE)
        out = []
        for j, (col, row, w, vclass, near, corners) in enumerate(specs):
            p = triangle(C, col, row, w, corners)
            if near:
                # The third vertex goes behind the camera: on the line from vertex 0 through a point of the plane w = 0 that
                # lies straight below the eye, so the part in front of the near plane runs from the cell down the screen.
                a = f64(p[0])
                xc, yc = OFF + CELL * col + 4.0, OFF + CELL * row + 4.0
                down = _solve(C, xc, yc + 1.0, w) - _solve(C, xc, yc, w)
                q0 = _eye_point(C) + down / np.linalg.norm(down) * 40.0
                p[2] = (a + 1.5 * (q0 - a)).astype(F)
            order = [0, 1, 2] if faces_camera(C, p) else [0, 2, 1]
            uclass = UV_CLASSES[cell_no[0] % len(UV_CLASSES)]
            for slot, k in enumerate(order):
                n, t = vertex_attributes(vclass, k)
                v[3 * j + slot] = (p[k], vertex_uv(uclass, k, cell_no[0]), n, t)
            out.append(SimpleNamespace(col=col, row=row, vclass=vclass, uclass=uclass, near=near, cell=cell_no[0], order=order))
            cell_no[0] += 1
        return v, out

    def _eye_point(C):
        # the point every line of sight passes through: (p, 1) @ C has x = y = w = 0 there
        A = np.stack([C[:3, 0], C[:3, 1], C[:3, 3]])
        return np.linalg.solve(A, -np.array([C[3, 0], C[3, 1], C[3, 3]]))

    def add(view, iclasses, specs, material, indexed=None, shifts=None):
        """one draw: mesh solved through the FIRST instance's model; instance i = that model shifted by shifts[i] rows"""
        m0, _ = instance_matrices(iclasses[0])
        C = f64(m0) @ VP[view]
        v, recs = mesh_for(C, specs)
        idx = None
        if indexed == "plain":
            idx = np.arange(len(v), dtype=np.uint32)
        elif indexed == "permuted":
            # triangles 8 and 9 share the vertex on their common cell border; the vertex buffer is shuffled and the triangles
            # are listed backwards
            tri = np.arange(len(v), dtype=np.uint32).reshape(-1, 3)
            tri[9, 0] = 3 * 8 + recs[8].order.index(1)           # (vertex 0 of a triangle always sits in its slot 0)
            perm = np.random.Generator(np.random.PCG64(SEEDS["shuffle"])).permutation(len(v))
            inv = np.empty_like(perm); inv[perm] = np.arange(len(v))
            v = v[perm]
            idx = inv[tri[::-1]].astype(np.uint32).ravel()
            recs = recs[::-1]
        inst = np.zeros(len(iclasses), bbo.INSTANCE_DTYPE)
        for i, ic in enumerate(iclasses):
            m, inv_m = instance_matrices(ic)
            m = m.copy()
            if shifts is not None and shifts[i]:
                w0 = specs[0][2]
                d = _solve(VP[view], 80.0, 64.0 + CELL * shifts[i], w0) - _solve(VP[view], 80.0, 64.0, w0)   # world shift of whole cells
                m[3, :3] = (f64(m[3, :3]) + d).astype(F)
            inst[i]["model"], inst[i]["inv_model"] = m, inv_m
        d_no = len(draws)
        draws.append(bbo.DrawData(v, idx, inst, material))
        for i, ic in enumerate(iclasses):
            for j, r in enumerate(recs):
                cells.append(SimpleNamespace(draw=d_no, inst=i, tri=j, col=r.col, row=r.row + (shifts[i] if shifts else 0), view=view,
                                             iclass=ic, vclass=r.vclass, uclass=r.uclass, near=r.near, indexed=idx is not None,
                                             material=d_no % 2))

    depth = lambda: float(rng.uniform(4.0, 8.0))
    row_of = lambda row, col0, w=None: [(col0 + j, row, w if w is not None else depth(), vc, False, CORNERS) for j, vc in enumerate(VERTEX_CLASSES)]
    w0 = 6.0
    add("main", list(ROTATED), row_of(0, 0, w0), mats[0], shifts=list(range(len(ROTATED))))
    ident = row_of(0, 8, 5.0)
    ident += [(16, 0, 5.0, "mixed", False, ((1.3, 1.2), (8.0, 4.0), (1.7, 6.8))), (17, 0, 5.0, "mixed", False, ((0.0, 4.0), (6.9, 1.6), (6.7, 6.9)))]
    add("main", ["identity"], ident, mats[1], indexed="permuted")
    singles = ["scene", "nonuniform a", "nonuniform b", "mirrored", "identity inverse", "rank 2", "rank 1", "w = 2", "projective"]
    for n, ic in enumerate(singles):
        add("main", [ic], row_of(1 + n, 8), mats[len(draws) % 2], indexed="plain" if n % 2 else None)
    far = row_of(0, 0, 100.0) + [(j, NEAR_ROW, 100.0, vc, True, CORNERS) for j, vc in enumerate(VERTEX_CLASSES)]
    add("near", ["translated 1e6"], far, mats[len(draws) % 2], indexed="plain")
    first = np.cumsum([0] + [d.n_prims for d in draws])
    for k, c in enumerate(cells):
        c.prim = k
    assert len(cells) == first[-1]
    return SimpleNamespace(draws=draws, cells=cells, first_prim=first[:-1], materials=mats)


def scene(view, enable_normal_map=1):
    p = plan()
    lights = [scenes.light(0, pos=(1.0, 2.0, 0.5), color=(1.0, 0.9, 0.8), intensity=60.0),
              scenes.light(2, dir=(0.25, -0.5, 1.0), color=(0.4, 0.5, 0.9), intensity=2.0),
              scenes.light(0, pos=(FAR - 20.0, 10.0, 60.0), color=(0.9, 1.0, 0.7), intensity=4000.0)]
    return bbo.Scene(scenes.frame_uniforms(lights), view_uniforms(view, enable_normal_map), p.draws, W, H, f"vertex chart {view}")


def cell_box(c):
    return OFF + CELL * c.col, OFF + CELL * c.row


def prim_vertices(c):
    """(instance record, the three vertex records) of a cell's primitive"""
    d = plan().draws[c.draw]
    vi = d.indices[3 * c.tri:3 * c.tri + 3] if d.indices is not None else np.arange(3 * c.tri, 3 * c.tri + 3)
    return d.instances[c.inst], [d.vertices[int(i)] for i in vi]


# ---------------------------------------------------------------------------------------------------------------------
# the oracle's vertex stage per primitive, and what the contract does with its clip positions
# ---------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(None)
def stage(view, deferred):
    """clip [n, 3, 4] and vary [n, 3, 14] (uv, posWorld, N, T, B) of every primitive: bbo.vertex_stage"""
    p = plan()
    vu = view_uniforms(view)
    clip = np.zeros((len(p.cells), 3, 4), F)
    vary = np.zeros((len(p.cells), 3, 14), F)
    memo = {}
    for c in p.cells:
        d = p.draws[c.draw]
        vi = d.indices[3 * c.tri:3 * c.tri + 3] if d.indices is not None else np.arange(3 * c.tri, 3 * c.tri + 3)
        for k, i in enumerate(vi):
            key = (c.draw, c.inst, int(i))
            if key not in memo:
                memo[key] = bbo.vertex_stage(vu, d.instances[c.inst:c.inst + 1], d.vertices[int(i):int(i) + 1], deferred=bool(deferred))
            clip[c.prim, k], vary[c.prim, k] = memo[key]
    return clip, vary


def fate(clip):
    """[n] of "rejected" / "clipped" / "unclipped": k_geometry's frustum test on binary32 clip positions (GUARD_BAND 32)"""
    with np.errstate(all="ignore"):
        x, y, z, w = (clip[..., i] for i in range(4))
        out = ((w + x < 0).all(-1) | (w - x < 0).all(-1) | (w + y < 0).all(-1) | (w - y < 0).all(-1) | (w - z < 0).all(-1) |
               (z < 0).all(-1))
        g = F(32.0)
        inside = ((w - z >= 0) & (z >= 0) & (g * w + x >= 0) & (g * w - x >= 0) & (g * w + y >= 0) & (g * w - y >= 0)).all(-1)
    return np.where(out, "rejected", np.where(inside, "unclipped", "clipped"))


def setup(clip):
    """The contract's projection and triangle setup of unclipped primitives, restated: project_vertex on each vertex, then
    setup_tri's binary64 expressions on int64 differences, rounded once.  Returns a namespace of arrays over the primitives:
    ok (projected, front-facing, a pixel centre in its box), X, Y [n, 3], rw [n, 3], z0, dzdx, dzdy, l1dx, l1dy, l2dx, l2dy."""
    import tbn_reference as tr
    ok, X, Y, z = tr.project(clip, 0.5 * F(W), 0.5 * F(H))
    with np.errstate(all="ignore"):
        rw = F(1.0) / clip[..., 3]
    ok = ok.all(-1)
    dx1, dy1 = X[:, 1] - X[:, 0], Y[:, 1] - Y[:, 0]
    dx2, dy2 = X[:, 2] - X[:, 0], Y[:, 2] - Y[:, 0]
    S = dx1 * dy2 - dx2 * dy1
    ok &= S > 0
    with np.errstate(all="ignore"):
        rS = 1.0 / S.astype(np.float64)
        d = lambda a: a.astype(np.float64)
        o = SimpleNamespace(X=X, Y=Y, rw=rw, z0=z[:, 0])
        o.l1dx, o.l1dy = (d(dy2) * rS).astype(F), (-d(dx2) * rS).astype(F)
        o.l2dx, o.l2dy = (-d(dy1) * rS).astype(F), (d(dx1) * rS).astype(F)
        dz1, dz2 = d(z[:, 1]) - d(z[:, 0]), d(z[:, 2]) - d(z[:, 0])
        o.dzdx = ((dz1 * d(dy2) - dz2 * d(dy1)) * rS).astype(F)
        o.dzdy = ((dz2 * d(dx1) - dz1 * d(dx2)) * rS).astype(F)
    px0 = np.maximum((X.min(1) - 128 + 255) >> 8, 0); px1 = np.minimum((X.max(1) - 128) >> 8, W - 1)
    py0 = np.maximum((Y.min(1) - 128 + 255) >> 8, 0); py1 = np.minimum((Y.max(1) - 128) >> 8, H - 1)
    o.ok = ok & (px0 <= px1) & (py0 <= py1)
    return o


def wins_in_own_cell(prim_map, view):
    """[n] bool: the primitive wins at least one pixel inside its own cell; and [n] pixels won anywhere"""
    cells = plan().cells
    own = np.zeros(len(cells), bool)
    for c in cells:
        if c.view == view:
            x0, y0 = cell_box(c)
            own[c.prim] = (prim_map[y0:y0 + CELL, x0:x0 + CELL] == c.prim).any()
    won = np.bincount(prim_map[prim_map != bbo.NO_PRIM].ravel(), minlength=len(cells))
    return own, won


# ---------------------------------------------------------------------------------------------------------------------
# census and the binary64 reference
# ---------------------------------------------------------------------------------------------------------------------
def category(v):
    """of a transformed vector v [3] in binary64 (computed from binary32 inputs), see the module's docstring"""
    v = f64(v)
    if np.isnan(v).any():
        return "nan"
    if np.isinf(v).any():
        return "vinf"
    if not v.any():
        return "vzero"
    sq = float((v * v).sum())
    if sq < 2.0 ** -151:
        return "zero"
    if 2.0 ** -148 <= sq < 2.0 ** -127:
        return "denormal"
    if 2.0 ** -125 < sq < 2.0 ** 127:
        return "normal"
    if sq > 2.0 ** 129:
        return "inf"
    return "borderline"


def transformed(inst, vertex):
    """normalMat * n and normalMat * t in binary64: (normalMat * n)_i = dot(inv_model column i, n)"""
    with np.errstate(all="ignore"):
        im = f64(inst["inv_model"])[:3, :3]
        return im @ f64(vertex["normal"]), im @ f64(vertex["tangent"])


@functools.lru_cache(None)
def categories():
    """per primitive: [(category of N's argument, of T's) for the three vertices]"""
    out = []
    for c in plan().cells:
        inst, vs = prim_vertices(c)
        out.append([tuple(category(v) for v in transformed(inst, vx)) for vx in vs])
    return out


def in_population(cats):
    return all(a == "normal" and b == "normal" for a, b in cats)


def check_pattern(cat, v, got):
    """assert PATTERN[cat] on normalize's result `got` [3] for the argument v [3] (binary64)"""
    got = np.asarray(got, F)
    if cat == "normal":
        assert abs(float(np.sqrt((f64(got) ** 2).sum())) - 1.0) <= 1e-5, (cat, got)
    elif cat in ("borderline", "denormal"):
        assert np.isfinite(got).all(), (cat, got)
    elif cat in ("vzero", "nan"):
        assert np.isnan(got).all(), (cat, got)
    elif cat == "zero":
        for c in range(3):
            if abs(v[c]) > 2.0 ** -148:
                assert np.isinf(got[c]) and np.signbit(got[c]) == np.signbit(v[c]), (cat, c, v, got)
            elif abs(v[c]) < 2.0 ** -151:
                assert np.isnan(got[c]), (cat, c, v, got)
    elif cat == "inf":
        assert (got == 0).all() and np.array_equal(np.signbit(got), np.signbit(v)), (cat, v, got)
    elif cat == "vinf":
        for c in range(3):
            if np.isinf(v[c]):
                assert np.isnan(got[c]), (cat, c, v, got)
            else:
                assert got[c] == 0 and np.signbit(got[c]) == np.signbit(v[c]), (cat, c, v, got)
    else:
        raise KeyError(cat)


def check_binormal_pattern(N, T, B):
    """B = cross(N, T): finite exactly when N and T are; all NaN when either is all NaN"""
    N, T, B = (np.asarray(a, F) for a in (N, T, B))
    assert np.isfinite(B).all() == (np.isfinite(N).all() and np.isfinite(T).all()), (N, T, B)
    if np.isnan(N).all() or np.isnan(T).all():
        assert np.isnan(B).all(), (N, T, B)


def glsl_f64(view, inst, vertex, deferred):
    """forward_brdf.vert:24-37 / gbuffer.vert:19-35 in binary64 (tests/test_oracle_contract.py's glsl_f64_vertex_stage;
    gbuffer.vert's order P * (V * posWorld) is the same product in binary64 up to its own rounding)"""
    from test_oracle_contract import glsl_f64_vertex_stage
    clip, vary = glsl_f64_vertex_stage(view, inst, vertex)
    if deferred:
        pw = np.append(f64(vertex["pos"]), 1.0) @ f64(inst["model"])
        clip = (pw @ f64(view["view"])) @ f64(view["proj"])
    return clip, vary


def bounds(view, inst, vertex, deferred):
    """forward error bounds (module docstring) of clip [4], posWorld [3], N, T, B [3] each, for a vertex of the population"""
    a = lambda m: np.abs(f64(m))
    model, V, P = a(inst["model"]), a(view["view"]), a(view["proj"])
    pos = np.append(a(vertex["pos"]), 1.0)
    pw = np.abs(np.append(f64(vertex["pos"]), 1.0) @ f64(inst["model"]))
    e_pw = 4 * U * (pos @ model)
    if deferred:
        pv = np.abs((np.append(f64(vertex["pos"]), 1.0) @ f64(inst["model"])) @ f64(view["view"]))
        e_view = 4 * U * (pw @ V) + e_pw @ V
        e_clip = 4 * U * (pv @ P) + e_view @ P
    else:
        e_clip = 4 * U * (pw @ V @ P) + pw @ (4 * U * (V @ P)) + e_pw @ V @ P
    im = a(inst["inv_model"])[:3, :3]
    out = {"clip": e_clip * SLACK, "pw": e_pw[:3] * SLACK}
    e_unit = {}
    for name, key in (("N", "normal"), ("T", "tangent")):
        v = f64(inst["inv_model"])[:3, :3] @ f64(vertex[key])
        e_v = 3 * U * (im @ a(vertex[key]))
        rho = np.sqrt((e_v ** 2).sum()) / np.sqrt((v ** 2).sum())
        e_unit[name] = 2 * rho + 4 * U
        out[name] = np.full(3, e_unit[name]) * SLACK
    n, t = (_unit(f64(inst["inv_model"])[:3, :3] @ f64(vertex[k])) for k in ("normal", "tangent"))
    n, t = np.abs(n), np.abs(t)
    eb = []
    for i in range(3):
        j, k = (i + 1) % 3, (i + 2) % 3
        eb.append(2 * U * (n[j] * t[k] + n[k] * t[j]) + e_unit["N"] * (t[k] + t[j]) + e_unit["T"] * (n[j] + n[k]))
    out["B"] = np.array(eb) * SLACK
    return out


def error_over_bound(view_name, deferred, prims):
    """worst |oracle - binary64| / bound over the vertices of the primitives `prims` (all in the population)"""
    view = view_uniforms(view_name)
    clip, vary = stage(view_name, deferred)
    cells = plan().cells
    worst = 0.0
    for p in prims:
        inst, vs = prim_vertices(cells[p])
        for k, vx in enumerate(vs):
            want_clip, want = glsl_f64(view, inst, vx, deferred)
            b = bounds(view, inst, vx, deferred)
            got = f64(vary[p, k])
            assert np.array_equal(vary[p, k, :2].view(np.uint32), np.asarray(vx["uv"], F).view(np.uint32))
            ratios = [np.abs(f64(clip[p, k]) - want_clip) / b["clip"], np.abs(got[2:5] - want[2:5]) / b["pw"],
                      np.abs(got[5:8] - want[5:8]) / b["N"], np.abs(got[8:11] - want[8:11]) / b["T"],
                      np.abs(got[11:14] - want[11:14]) / b["B"]]
            with np.errstate(all="ignore"):
                worst = max(worst, max(float(np.nanmax(r)) for r in ratios))
    return worst


@functools.lru_cache(None)
def oracle_frame(view, deferred, enable_normal_map=1):
    """the oracle's render of a view, computed once: namespace of frame, gbuf (deferred), prim, depth, stats -- read-only"""
    sc = scene(view, enable_normal_map)
    if deferred:
        frame, gbuf, prim, depth, st = bbo.render_deferred(sc)
    else:
        (frame, prim, depth, st), gbuf = bbo.render(sc), None
    for a in (frame, gbuf, prim, depth):
        if a is not None:
            a.setflags(write=False)
    return SimpleNamespace(scene=sc, frame=frame, gbuf=gbuf, prim=prim, depth=depth, stats=st)


def census(deferred):
    """{category: number of VISIBLE primitives (a pixel won, either view) with a vertex whose N or T argument is of it}"""
    cats = categories()
    won = sum(wins_in_own_cell(oracle_frame(v, deferred).prim, v)[1] for v in VIEWS)
    out = {k: 0 for k in ("normal", "borderline") + HAZARDS}
    for p in np.flatnonzero(won):
        for k in {x for ab in cats[p] for x in ab}:
            out[k] += 1
    return out


def oracle_worst():
    """{"<instance class> <pass>": worst error / bound of the oracle against the GLSL in binary64}, and the share left out"""
    cells, cats = plan().cells, categories()
    pop = [c for c in cells if in_population(cats[c.prim])]
    worst = {}
    for deferred in (0, 1):
        for c in pop:
            key = f"{c.iclass} {'deferred' if deferred else 'forward'}"
            worst[key] = max(worst.get(key, 0.0), error_over_bound(c.view, deferred, [c.prim]))
    return worst, 1.0 - len(pop) / len(cells)
