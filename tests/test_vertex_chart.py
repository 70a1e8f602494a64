"""CPU side of the vertex chart (tests/vertex_chart.py; the GPU side is tests/test_gpu_vertex_chart.py).

  * the chart is what it claims: every planned primitive wins a pixel of its own cell on the oracle's render, the near row
    is clipped, the draw list reaches the addressing it was built for
  * census: every hazard category of a squared length is present in a visible primitive, on both passes, and the hand-stated
    table of where a scaled inverse lands agrees with the binary64 count
  * the oracle's semantics per category (vertex_chart.PATTERN, stated by hand), on every vertex of the chart
  * the oracle against the GLSL in binary64 within a propagated forward error bound, on the cells whose squared lengths are
    normal numbers; the share of cells left out is a stated condition"""
import json
import os

import numpy as np
import pytest

import vertex_chart as VC
from conftest import GOLDEN
from oracle import bbo

RECORD = os.path.join(GOLDEN, "vertex_chart.json")
pass_id = lambda d: "deferred" if d else "forward"


@pytest.mark.parametrize("deferred", [0, 1], ids=pass_id)
@pytest.mark.parametrize("view", VC.VIEWS)
def test_chart_construction(view, deferred):
    p = VC.plan()
    o = VC.oracle_frame(view, deferred)
    own, won = VC.wins_in_own_cell(o.prim, view)
    mine = np.array([c.view == view for c in p.cells])
    assert o.stats["n_prims"] == len(p.cells) == 154
    assert own[mine].all(), [(c.prim, c.iclass, c.vclass) for c in p.cells if c.view == view and not own[c.prim]]
    assert not won[~mine].any(), "a cell of the other view is visible"
    for c in p.cells:                                            # a primitive's pixels lie in its own cell (the near row: and below)
        if c.view == view:
            ys, xs = np.nonzero(o.prim == c.prim)
            x0, y0 = VC.cell_box(c)
            assert (xs >= x0).all() and (xs < x0 + VC.CELL).all() and (ys >= y0).all() and (c.near or (ys < y0 + VC.CELL).all())
    near = [c for c in p.cells if c.near]
    assert len(near) == 8 and all(c.row == VC.NEAR_ROW and c.view == "near" for c in near)
    assert o.stats["n_clipped_prims"] == (8 if view == "near" else 0)
    fate = VC.fate(VC.stage(view, deferred)[0])
    assert all(fate[c.prim] == ("clipped" if c.near else "unclipped") for c in p.cells if c.view == view)
    assert (fate[~mine] == "rejected").all()
    assert VC.W <= 160 and VC.H <= 128


def test_the_draw_list_reaches_the_addressing():
    p = VC.plan()
    assert len(p.draws) >= 6 and len(p.first_prim) > 4                              # past the three inline first_prim
    assert any(d.indices is None for d in p.draws) and any(d.indices is not None for d in p.draws)
    assert any(len(d.instances) >= 3 and d.n_prims // len(d.instances) >= 2 for d in p.draws)
    d = p.draws[1]
    tri = d.indices.reshape(-1, 3)
    assert len(np.unique(d.indices)) < len(d.indices), "no shared vertex"
    assert not np.array_equal(np.sort(d.indices), d.indices) and (np.diff(tri[:, 0].astype(np.int64)) < 0).any()
    sizes = [{m.shape[:2] for m in mat.maps.values()} for mat in p.materials]
    assert len(sizes[0]) == 1 and len(p.materials[0].maps) == 5 and len(sizes[1]) > 1   # one packs, one does not
    assert {c.material for c in p.cells} == {0, 1}
    cols = {VC.OFF + VC.CELL * c.col for c in p.cells}
    rows = {VC.OFF + VC.CELL * c.row for c in p.cells}
    assert {28, 60} <= cols and {28, 60} <= rows                                    # cells across the 32- and 64-pixel borders
    assert {c.iclass for c in p.cells} == set(VC.INSTANCE_CLASSES) and {c.vclass for c in p.cells} == set(VC.VERTEX_CLASSES)
    assert {c.uclass for c in p.cells} == set(VC.UV_CLASSES)
    bits = lambda a: np.asarray(a, np.float32).view(np.uint32)
    for c in p.cells:                                           # uv hazards arrive in the vertex buffer bit for bit
        if c.uclass == "nan payload":
            uv = np.stack([v["uv"] for v in VC.prim_vertices(c)[1]])
            assert VC.NAN_A in bits(uv) and VC.NAN_B in bits(uv)
        if c.uclass == "-0.0":
            assert 0x80000000 in bits(np.stack([v["uv"] for v in VC.prim_vertices(c)[1]]))


def test_mirrored_cells_are_culled_in_the_unmirrored_order():
    """the chart picks the vertex order that faces the camera; under diag(-1, 1, 1) that is the reversed one: with the order
    of the identity row the oracle culls the cell"""
    p = VC.plan()
    k = next(i for i, d in enumerate(p.draws) if p.cells[int(p.first_prim[i])].iclass == "mirrored")
    d = p.draws[k]
    v = d.vertices.copy()
    v[1::3], v[2::3] = d.vertices[2::3], d.vertices[1::3]
    sc = VC.scene("main")
    swapped = bbo.Scene(sc.frame, sc.view, [bbo.DrawData(v, d.indices, d.instances, d.material) if i == k else x
                                            for i, x in enumerate(p.draws)], VC.W, VC.H)
    prim = bbo.render(swapped)[1]
    first = int(p.first_prim[k])
    assert not np.isin(prim, np.arange(first, first + d.n_prims)).any()
    assert np.isin(VC.oracle_frame("main", 0).prim, np.arange(first, first + d.n_prims)).any()


@pytest.mark.parametrize("deferred", [0, 1], ids=pass_id)
def test_census(deferred):
    c = VC.census(deferred)
    print(pass_id(deferred), c)
    for k in VC.HAZARDS:
        assert c[k] >= 1, f"no visible primitive with a {k} squared length"
    assert c["normal"] >= 100
    rec = json.load(open(RECORD))
    assert rec["seeds"] == VC.SEEDS and rec["frame"] == [VC.W, VC.H]
    assert rec["census"][pass_id(deferred)] == c, "tools/vertex_chart_record.py rewrites the record"


def test_scale_length_table_stated_by_hand():
    cats = VC.categories()
    seen = set()
    for c in VC.plan().cells:
        want = VC.SCALE_LENGTH_CATEGORY.get((c.iclass, c.vclass))
        if want is not None:
            assert {x for ab in cats[c.prim] for x in ab} == {want}, (c.iclass, c.vclass)
            seen.add((c.iclass, c.vclass))
    assert seen == set(VC.SCALE_LENGTH_CATEGORY)


@pytest.mark.parametrize("deferred", [0, 1], ids=pass_id)
def test_oracle_semantics_per_category(deferred):
    """every vertex of the chart: N and T are what PATTERN says of their category, B what cross makes of them"""
    cats = VC.categories()
    counted = {k: 0 for k in VC.PATTERN}
    for view in VC.VIEWS:
        _, vary = VC.stage(view, deferred)
        for c in VC.plan().cells:
            inst, vs = VC.prim_vertices(c)
            for k, vx in enumerate(vs):
                vn, vt = VC.transformed(inst, vx)
                VC.check_pattern(cats[c.prim][k][0], vn, vary[c.prim, k, 5:8])
                VC.check_pattern(cats[c.prim][k][1], vt, vary[c.prim, k, 8:11])
                VC.check_binormal_pattern(vary[c.prim, k, 5:8], vary[c.prim, k, 8:11], vary[c.prim, k, 11:14])
                counted[cats[c.prim][k][0]] += 1
                counted[cats[c.prim][k][1]] += 1
    assert all(counted.values()), counted


def test_what_lies_outside_the_3x3_changes_nothing():
    _, vary = VC.stage("main", 0)
    cells = VC.plan().cells
    plain = {c.vclass: c.prim for c in cells if c.iclass == "rotated"}
    n = 0
    for c in cells:
        if c.iclass == "nan inf outside":
            a, b = vary[c.prim, :, 5:], vary[plain[c.vclass], :, 5:]       # N, T, B (posWorld differs: another row of cells)
            assert np.array_equal(np.isnan(a), np.isnan(b)) and np.array_equal(a[~np.isnan(a)].view(np.uint32), b[~np.isnan(b)].view(np.uint32))
            n += 1
    assert n == 8


def test_oracle_against_the_glsl_in_binary64_within_the_propagated_bound():
    worst, left_out = VC.oracle_worst()
    print({k: round(v, 4) for k, v in worst.items()}, f"left out {left_out:.4f}")
    # the condition: the comparison covers everything but the planned hazards (vertex_chart.PLANNED_HAZARD_SHARE = 91 / 154)
    assert left_out <= VC.PLANNED_HAZARD_SHARE <= 0.6
    assert {k.rsplit(" ", 1)[0] for k in worst} == set(VC.INSTANCE_CLASSES) - {"inv 1e-22", "inv 1e-25"}
    assert max(worst.values()) <= 1.0, worst
    rec = json.load(open(RECORD))["oracle"]["worst_error_over_bound"]
    assert set(rec) == set(worst)
    for k, v in worst.items():
        assert abs(rec[k] - v) <= 0.05 * v + 1e-3, (k, rec[k], v)
