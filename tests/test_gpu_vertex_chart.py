"""GPU: the vertex stage (`k_geometry`, `k_tbn_segments`; csrc/bb_kernels.hip.h) on hazard instances -- the vertex chart.

tests/vertex_chart.py builds two 160 x 128 frames whose primitives are a chosen population of (instance, vertex) pairs; per
pass and tile size both are rendered, and what k_geometry wrote per primitive is read back (bbr_read_records):
  1  the whole pipeline: frame, winning primitive, depth bits, n_shaded, n_clipped_prims (deferred: G-buffer too) equal the oracle's
  2  records: every primitive that wins a pixel, survives or is clipped has a record; its uv is the input's bit for bit, its
     posWorld, N, T, B are bbo.vertex_stage's ("equal": NaN in the same places, every other value bit-equal, signs of zero and
     infinities included), its material binding is its draw's, its clip_base says whether it was clipped
  3  setup: of the unclipped ones, snapped coordinates, 1/w, z0 and the five planes of head and triangle are the contract's
     projection and setup_tri of the oracle's clip position (the pass's own order of P, V), restated in numpy
  4  k_tbn_segments, the other caller of the expressions, against tests/tbn_reference.py on the same scenes
  5  the read-back is idempotent, survives the overlay pass and fails as documented
Each case is two frames of 20 480 pixels and 154 primitives; the file's wall time is recorded in tests/golden/vertex_chart.json."""
import ctypes as C
import functools
from types import SimpleNamespace

import numpy as np
import pytest

import surface_chart as SC
import tbn_reference as tr
import vertex_chart as VC
from bibim_renderer_amd import BibimError, Renderer
from bibim_renderer_amd.renderer import RECORD_DTYPE, TRIANGLE_DTYPE
from test_gpu_tbn_overlay import same_records

pytestmark = pytest.mark.gpu

W, H = VC.W, VC.H
equal = SC.equal_but_for_nan_payload
bits = SC.bits
pass_id = lambda d: "deferred" if d else "forward"
CASES = [(d, m) for d in (0, 1) for m in (0, 1)]
case_id = lambda c: f"{pass_id(c[0])} tile_mode {c[1]}"


@functools.lru_cache(None)
def gpu(view, deferred, tile_mode):
    """one frame of a view and its read-backs, rendered once per case and shared (read-only) by the checks"""
    sc = VC.scene(view)
    r = Renderer(W, H)
    r.set_option("render_pass", deferred)
    r.set_option("tile_mode", tile_mode)
    handles = r.render_scene(sc)
    g = SimpleNamespace(frame=r.read_framebuffer(), stats=r.stats())
    g.prim, g.depth = r.read_visibility()
    g.gbuf = r.read_gbuffer() if deferred else None
    g.recs, g.tris = r.read_records()
    again = r.read_framebuffer()                                   # the read-backs re-render the frame: the same bits
    r.close()
    assert equal(again, g.frame)
    g.material = [handles["mat"][id(m)] for m in VC.plan().materials]
    return g


def inspected(view, deferred):
    """what the oracle says of every primitive: fate, the contract's setup, pixels won; and which records are looked at"""
    o = VC.oracle_frame(view, deferred)
    clip, vary = VC.stage(view, deferred)
    fate = VC.fate(clip)
    st = VC.setup(clip)
    won = VC.wins_in_own_cell(o.prim, view)[1] > 0
    unclipped = (fate == "unclipped") & st.ok
    clipped = fate == "clipped"
    assert not (won & ~(unclipped | clipped)).any(), "the restated cull drops a primitive the oracle draws"
    return SimpleNamespace(clip=clip, vary=vary, setup=st, won=won, unclipped=unclipped, clipped=clipped, look=won | unclipped | clipped)


@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_1_frame_parity(case):
    deferred, tile_mode = case
    for view in VC.VIEWS:
        o, g = VC.oracle_frame(view, deferred), gpu(view, deferred, tile_mode)
        assert np.array_equal(g.prim, o.prim), f"{view}: {int((g.prim != o.prim).sum())} pixels pick another primitive"
        assert np.array_equal(bits(g.depth), bits(o.depth)), view
        assert g.stats["n_shaded"] == o.stats["n_shaded"] and g.stats["n_prims"] == o.stats["n_prims"]
        assert g.stats["n_clipped_prims"] == o.stats["n_clipped_prims"] == (8 if view == "near" else 0)
        if deferred:
            assert equal(g.gbuf, o.gbuf), f"{view}: G-buffer texels differ"
        ng, nw = np.isnan(g.frame), np.isnan(o.frame)
        diff = (ng != nw) | (~nw & ~ng & (bits(g.frame) != bits(o.frame)))
        assert equal(g.frame, o.frame), f"{view}: {int(diff.any(-1).sum())} pixels differ, primitives {np.unique(o.prim[diff.any(-1)])[:10]}"


@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_2_records(case):
    deferred, tile_mode = case
    p = VC.plan()
    packed_dims = [32 | 32 << 16, 0]
    for view in VC.VIEWS:
        g, q = gpu(view, deferred, tile_mode), inspected(view, deferred)
        assert g.recs.dtype == RECORD_DTYPE and g.tris.dtype == TRIANGLE_DTYPE and len(g.recs) == len(g.tris) == len(p.cells)
        n = int(q.look.sum())
        print(f"records {view} {pass_id(deferred)} tile_mode {tile_mode}: {n} inspected, {int(q.unclipped.sum())} unclipped, "
              f"{int(q.clipped.sum())} clipped")
        assert n == sum(c.view == view for c in p.cells)              # the view's own cells, none vacuously
        for c in p.cells:
            if not q.look[c.prim]:
                continue
            rec, want, who = g.recs[c.prim], q.vary[c.prim], (view, c.prim, c.iclass, c.vclass, c.uclass)
            assert rec["material"] != VC.FILL, ("no record", who)
            assert np.array_equal(bits(rec["uv"]), bits(want[:, 0:2])), ("uv", who, rec["uv"], want[:, 0:2])
            for name, lo in (("posWorld", 0), ("N", 3), ("T", 6), ("B", 9)):
                got = rec["vary"][lo:lo + 3].T                        # [varying][vertex] -> [vertex][component]
                assert equal(got, want[:, 2 + lo:5 + lo]), (name, who, got, want[:, 2 + lo:5 + lo])
            assert rec["material"] == g.material[c.material], ("material", who)
            assert rec["packed_dims"] == packed_dims[c.material] and (rec["packed"] != 0) == (c.material == 0), ("packing", who)
            assert (rec["clip_base"] == VC.NO_CLIP) == bool(q.unclipped[c.prim]), ("clip_base", who, hex(int(rec["clip_base"])))


@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_3_setup(case):
    deferred, tile_mode = case
    for view in VC.VIEWS:
        g, q = gpu(view, deferred, tile_mode), inspected(view, deferred)
        s, u = q.setup, q.unclipped
        assert u.sum() >= (8 if view == "near" else 138)
        rec, tri = g.recs[u], g.tris[u]
        for k, (fx, fy) in enumerate((("X0", "Y0"), ("X1", "Y1"), ("X2", "Y2"))):
            assert np.array_equal(tri[fx], s.X[u, k]) and np.array_equal(tri[fy], s.Y[u, k]), (view, "snapped vertex", k)
        assert np.array_equal(rec["X0"], s.X[u, 0]) and np.array_equal(rec["Y0"], s.Y[u, 0])
        assert np.array_equal(bits(rec["rw"]), bits(s.rw[u])) and np.array_equal(bits(tri["rw"]), bits(s.rw[u])), (view, "1 / w")
        assert np.array_equal(bits(tri["z0"]), bits(s.z0[u])), (view, "z0")
        for f in ("l1dx", "l1dy", "l2dx", "l2dy"):
            want = bits(getattr(s, f)[u])
            assert np.array_equal(bits(rec[f]), want) and np.array_equal(bits(tri[f]), want), (view, f)
        for f in ("dzdx", "dzdy"):
            assert np.array_equal(bits(tri[f]), bits(getattr(s, f)[u])), (view, f)
        # a clipped primitive: a zero head, no triangle (the fill)
        head = g.recs[q.clipped].view(np.uint32).reshape(-1, 56)[:, :9]
        assert q.clipped.sum() == (8 if view == "near" else 0) and not head.any()
        assert (g.tris[q.clipped].view(np.uint32) == VC.FILL).all()
        # what k_geometry culled keeps the fill in both
        culled = ~q.look
        assert (g.recs[culled].view(np.uint32) == VC.FILL).all() and (g.tris[culled].view(np.uint32) == VC.FILL).all()


@pytest.mark.parametrize("enable", [0, 1], ids=["EnableNormalMap 0", "EnableNormalMap 1"])
def test_4_tbn_segments(enable):
    for view in VC.VIEWS:
        sc = VC.scene(view, enable)
        want = tr.tbn_records(sc)
        r = Renderer(W, H)
        r.set_option("overlays", 1)
        r.set_option("tbn", 1)
        r.render_scene(sc)
        r.present()
        r.draw_overlays(0)
        got = r.read_tbn_segments()
        r.close()
        print(f"tbn {view} EnableNormalMap {enable}: {len(want)} segments")
        assert len(want) >= 16
        same_records(got, want)


def test_5_idempotence_overlay_pass_and_errors():
    sc = VC.scene("near")
    r = Renderer(W, H)
    with pytest.raises(BibimError) as e:
        r.read_records()                                           # before a first frame
    assert e.value.code == -6
    r.set_option("overlays", 1)
    r.render_scene(sc)
    a = r.read_records()
    b = r.read_records()
    assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes()
    assert (a[0]["material"] != VC.FILL).sum() == 16
    r.present()
    r.draw_overlays(0)                                             # (the markers go through k_geometry's overlay instantiation)
    c = r.read_records()
    assert a[0].tobytes() == c[0].tobytes() and a[1].tobytes() == c[1].tobytes()
    n = C.c_uint32()
    few = np.zeros(3, RECORD_DTYPE)
    assert r._L.bbr_read_records(r._ctx, few.ctypes.data, None, 3, C.byref(n)) == 0
    assert n.value == len(a[0]) and few.tobytes() == a[0][:3].tobytes()   # min(cap, n) records, either pointer may be NULL
    assert r._L.bbr_read_records(r._ctx, None, None, 0, None) == -1
    r.resize(96, 64)
    with pytest.raises(BibimError) as e:
        r.read_records()                                           # after bbr_resize
    assert e.value.code == -6
    r.close()
    r = Renderer(W, H)
    r.set_partition(0, 2)
    r.render_scene(sc)
    with pytest.raises(BibimError) as e:
        r.read_records()                                           # not on a partitioned context
    assert e.value.code == -1
    r.close()
