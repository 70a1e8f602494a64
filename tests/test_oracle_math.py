"""Row A0: the oracle's restatement of vector_math.cpp / camera.cpp is bit-identical to the reference's own
sources -- via the committed golden vectors (minted from oracle/_ref), among them 200 seeded random inputs per function, and,
when oracle/_ref is present, live on those inputs."""
import ctypes as C
import json
import os

import numpy as np
import pytest

from conftest import GOLDEN, ROOT
from oracle import bbo


def _bits(a):
    return [int(x) for x in np.ascontiguousarray(a, np.float32).view(np.uint32).ravel()]


def _from_bits(b):
    return np.array(b, np.uint32).view(np.float32).reshape(4, 4)


def _eval_case(m, c):
    op, a = c["op"], c["args"]
    if op == "perspective":
        return m.mat_perspective(*a)
    if op.startswith("rotate_"):
        return getattr(m, "mat_" + op)(a[0])
    if op == "camera_look":
        return m.camera_look(*a)
    if op == "camera_view":
        return m.camera_view(a[0], a[1], a[2])
    if op == "look_at":
        return m.mat_look_at(*a)
    if op == "mul":
        return m.mat_mul(_from_bits(a[0]), _from_bits(a[1]))
    if op == "inverse":
        return m.mat_inverse(_from_bits(a[0]))
    if op in ("instance_chain", "instance_chain_inverse"):
        t = m.mat_translate(*a)
        chain = m.mat_mul(m.mat_mul(m.mat_mul(t, m.mat_rotate_y(-90.0)), m.mat_rotate_x(-90.0)), m.mat_scale(0.01, 0.01, 0.01))
        return chain if op == "instance_chain" else m.mat_inverse(chain)
    if op in ("plane_model", "plane_model_inverse"):
        pm = m.mat_mul(m.mat_translate(0.0, -10.0, 0.0), m.mat_scale(100.0, 100.0, 100.0))
        return pm if op == "plane_model" else m.mat_inverse(pm)
    raise KeyError(op)


def golden_cases():
    return json.load(open(os.path.join(GOLDEN, "math_golden.json")))["cases"]


def test_oracle_matches_reference_golden_vectors():
    cases = golden_cases()
    assert len(cases) >= 80
    for c in cases:
        assert _bits(_eval_case(bbo, c)) == c["bits"], (c["op"], c["args"])


def test_survey_sample_values():
    # perspective(60, 16/9, 0.1, 1000)
    p = bbo.mat_perspective(60.0, 16.0 / 9.0, 0.1, 1000.0)
    assert p[0, 0] == np.float32(0.974278808) and p[1, 1] == np.float32(-1.73205125)
    assert p[2, 2] == np.float32(-0.000100010002) and p[3, 2] == np.float32(0.10001) and p[2, 3] == 1.0
    # pi32 = 3.141592f makes cos(-90 deg) tiny but non-zero: Model.M[0][0] = 3.139e-09 after scale(0.01)
    m = _eval_case(bbo, {"op": "instance_chain", "args": [0.0, -1.0, 2.0]})
    assert m[0, 0] == np.float32(3.13916471e-09)


def test_oracle_matches_compiled_reference_live():
    """200 seeded random inputs per function against what the reference's own vector_math.cpp / camera.cpp returned for them
    (tests/golden/math_random.npz, minted from oracle/_ref by tools/make_fixtures.py math_random) -- and, where oracle/_ref is
    built, against the compiled reference itself on the same inputs."""
    g = np.load(os.path.join(GOLDEN, "math_random.npz"))
    lib_path = os.path.join(ROOT, "oracle", "_ref", "libbb_ref.so")
    ref = C.CDLL(lib_path) if os.path.exists(lib_path) else None
    P, f = C.c_void_p, C.c_float
    if ref is not None:
        ref.ref_mat4_mul.argtypes = [P, P, P]; ref.ref_mat4_inverse.argtypes = [P, P]
        ref.ref_mat4_perspective.argtypes = [f, f, f, f, P]; ref.ref_camera_view.argtypes = [P, f, f, P]
        ref.ref_mat4_look_at.argtypes = [P, P, P, P]
        for n in "xyz":
            getattr(ref, f"ref_mat4_rotate_{n}").argtypes = [f, P]
    p = lambda a: a.ctypes.data_as(P)
    up = np.array([0, 1, 0], np.float32)
    assert g["in_a"].shape == (200, 4, 4)
    for i in range(200):
        a, b = np.ascontiguousarray(g["in_a"][i]), np.ascontiguousarray(g["in_b"][i])
        d, fov, asp = float(g["in_deg"][i]), float(g["in_fov"][i]), float(g["in_aspect"][i])
        pos, yaw, pitch = np.ascontiguousarray(g["in_pos"][i]), float(g["in_yaw"][i]), float(g["in_pitch"][i])
        eye, tgt = np.ascontiguousarray(g["in_eye"][i]), np.ascontiguousarray(g["in_target"][i])
        mine = {"mul": bbo.mat_mul(a, b), "inverse": bbo.mat_inverse(a), "perspective": bbo.mat_perspective(fov, asp, 0.1, 1000.0),
                "camera_view": bbo.camera_view(pos, yaw, pitch), "look_at": bbo.mat_look_at(eye, tgt, up),
                **{f"rotate_{n}": getattr(bbo, f"mat_rotate_{n}")(d) for n in "xyz"}}
        for name, m in mine.items():
            assert _bits(m) == _bits(g[f"out_{name}"][i]), (name, i)
        if ref is None:
            continue
        o = np.zeros((4, 4), np.float32)
        ref.ref_mat4_mul(p(a), p(b), p(o)); assert _bits(o) == _bits(mine["mul"])
        ref.ref_mat4_inverse(p(a), p(o)); assert _bits(o) == _bits(mine["inverse"])
        for n in "xyz":
            getattr(ref, f"ref_mat4_rotate_{n}")(d, p(o)); assert _bits(o) == _bits(mine[f"rotate_{n}"])
        ref.ref_mat4_perspective(fov, asp, 0.1, 1000.0, p(o)); assert _bits(o) == _bits(mine["perspective"])
        ref.ref_camera_view(p(pos), yaw, pitch, p(o)); assert _bits(o) == _bits(mine["camera_view"])
        ref.ref_mat4_look_at(p(eye), p(tgt), p(up), p(o)); assert _bits(o) == _bits(mine["look_at"])


def test_layout_sizes():
    L = bbo.lib()
    assert [L.bbo_sizeof(i) for i in range(6)] == [44, 128, 64, 6432, 144, 36]


def test_default_material_texels_match_reference_files():
    """resources/pbr/default/*.png decoded by the reference's stb_image (fixture) == the oracle's built-in defaults."""
    d = json.load(open(os.path.join(GOLDEN, "default_texels.json")))["maps"]
    for i, name in enumerate(("albedo", "metallic", "roughness", "ao", "normal", "height")):
        assert d[name]["uniform"]
        got = bbo.sample(None, i, 0.3, 0.7)
        want = np.array(d[name]["texel"], np.float32) * np.float32(1.0 / 255.0)
        assert np.array_equal(got, want), name
