"""The step behind the frame on the exchange chart (tests/exchange_chart.py): k_pack_shard, k_pack_shard_half,
k_unpack_gathered<Form>, k_push_block<V>, k_tone_map and k_present on shards whose values are chosen by bit pattern, against
the chart's model (blocks, whole frames) and the oracle (bbo.present, bbo.tone_map).

How chosen values get into a frame: a frame without draws is rendered into a caller's buffer (bbr_set_output_device_ptr), and
once it is through the case's shard is copied over it.  From then on bbr_stage_shard, bbr_push_shard, bbr_tone_map,
bbr_present and bbr_read_shard act on that buffer; inject() asserts that bbr_read_shard returns the injected bits.

Comparison rule, no tolerance anywhere: copies (RGBA32F, RGBA8, the rgb of PACKED) are bit-equal, NaN payloads included; where
a value is computed (binary16 rounding, tone map) NaN sits in the same places and every other value is bit-equal, +-inf and
the sign of zero included (surface_chart.equal_but_for_nan_payload).

  1  pack      every case x form: bbr_stage_shard into a buffer of 0xAB leaves the model's block -- its padding bytes zero --
               and nothing behind it; bbr_pack_shard = bbr_stage_shard(PACKED)
  2  unpack    every case x form from a gather buffer the model made (for RGBA16F one the pack kernel could not have made: every
               binary16 bit pattern): bbr_unpack_whole and the three older names, on the first and the last rank
  3  present, tone map, RGBA8 form: bbr_present on the injected shard, bbr_tone_map and bbr_present_buffer at every exposure
               of the chart, against the oracle
  4  push, narrow form: gather buffers 8 (plain forms also 4) bytes off 16-byte alignment, both push modes, against aligned
               ones; the alignment rules of include/bibim_hip.h as status codes
  5  push among 17 ranks: the second launch of the push kernel and the wrap-around of its targets"""
import numpy as np
import pytest

from bibim_renderer_amd import Renderer, BibimError, _capi
from oracle import bbo, scenes
import exchange_chart as X
from surface_chart import equal_but_for_nan_payload

pytestmark = pytest.mark.gpu
GUARD = 256


def inject(name, rank, enable=0, exposure=1.0, push_mode=None):
    """a context of `rank` whose last frame IS the chart's shard: (renderer, the tensor that holds the frame -- keep it alive)"""
    import torch
    c = X.CASES[name]
    r = Renderer(c.width, c.height)
    r.set_option("tile_mode", c.tile_mode)
    if push_mode is not None:
        r.set_option("push_mode", push_mode)
    r.set_partition(rank, c.world, c.band_rows)
    assert r.shard_rows() == X.shard_rows(c)
    n = X.shard_pixels(c)
    frame = torch.zeros((n, 4), dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    r.set_output_device_ptr(frame.data_ptr(), n * 16)
    r.set_frame_uniforms(scenes.frame_uniforms([], enable, exposure))
    r.set_view_uniforms(scenes.view_uniforms((0.0, 0.0, 3.0), 0.0, 0.0, c.width, c.height, 0))
    r.begin_frame()
    r.end_frame()
    r.synchronize()
    refill(name, rank, frame)
    assert np.array_equal(r.read_shard().view(np.uint32), X.shard(name, rank)), "the library touched the injected frame"
    return r, frame


def refill(name, rank, frame):
    import torch
    bits = X.shard(name, rank).reshape(-1, 4).view(np.int32).copy()
    frame.view(torch.int32).copy_(torch.from_numpy(bits))
    torch.cuda.synchronize()          # torch fills on its own stream; the library does not wait for that one


def settle(*renderers):
    import torch
    for r in renderers:
        r.synchronize()
    torch.cuda.synchronize()


def filled(nbytes):
    import torch
    return torch.full((nbytes,), 0xAB, dtype=torch.uint8, device="cuda")


def upload(a):
    import torch
    t = torch.from_numpy(np.ascontiguousarray(a).reshape(-1).view(np.uint8).copy()).cuda()
    torch.cuda.synchronize()
    return t


def same_halves_but_for_nan_payload(a, b):
    a, b = (np.ascontiguousarray(x).reshape(-1).view("<u2") for x in (a, b))
    na, nb = (a & 0x7FFF) > 0x7C00, (b & 0x7FFF) > 0x7C00
    return a.size == b.size and np.array_equal(na, nb) and np.array_equal(a[~na], b[~na])


def block_is(got, want, form, c):
    """a staged or pushed block against the model's: bytes; for RGBA16F the decoded values under the rule, and the raw bytes
    wherever the value is not NaN"""
    if form != X.RGBA16F:
        return np.array_equal(got, want)
    rows = X.shard_rows(c)
    return (equal_but_for_nan_payload(X.decode_block(got, form, rows, c.width).view(np.float32),
                                      X.decode_block(want, form, rows, c.width).view(np.float32))
            and same_halves_but_for_nan_payload(got, want))


def whole_is(got, want, form):
    """a whole frame against the model's: RGBA32F, PACKED and RGBA8 are copies; RGBA16F is computed (widened)"""
    if form == X.RGBA16F:
        return equal_but_for_nan_payload(got, want.view(np.float32))
    return np.array_equal(np.ascontiguousarray(got).view(np.uint8), np.ascontiguousarray(want).view(np.uint8))


# ---- 1: pack ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", X.CASES)
def test_1_pack(name):
    c = X.CASES[name]
    for rank in X.test_ranks(name):
        r, frame = inject(name, rank)
        r.present()
        settle(r)
        assert np.array_equal(r.read_presented(), X.presented(name, rank))
        for form in X.FORMS:
            size = r.exchange_block_bytes(form)
            assert size == X.block_bytes(c, form)
            calls = [r.stage_shard] + ([lambda f, p: r.pack_shard(p)] if form == X.PACKED else [])
            for call in calls:
                buf = filled(size + GUARD)
                settle()
                call(form, buf.data_ptr())
                settle(r)
                got = buf.cpu().numpy()
                assert (got[size:] == 0xAB).all(), (form, rank, "written behind the block")
                assert block_is(got[:size], X.block(name, form, rank), form, c), (form, rank)
        if c.world == 1:
            assert r.packed_shard_bytes() == X.packed_layout(X.shard_pixels(c))[0]
        r.close()


# ---- 2: unpack --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", X.CASES)
def test_2_unpack(name):
    import torch
    c = X.CASES[name]
    source = {f: X.gathered16_hazard(name) if f == X.RGBA16F else X.gathered(name, f) for f in X.FORMS}
    want = {f: X.whole_frame(c, f, source[f]) for f in X.FORMS}
    dev = {f: upload(source[f]) for f in X.FORMS}
    older = {X.RGBA32F: Renderer.unpack_gathered, X.PACKED: Renderer.unpack_gathered_packed, X.RGBA8: Renderer.unpack_gathered_rgba8}
    for rank in X.test_ranks(name):
        r, frame = inject(name, rank)
        for form in X.FORMS:
            r.unpack_whole(form, dev[form].data_ptr())
            assert whole_is(r.read_whole_frame(form), want[form], form), (form, rank)
        r.close()
        bare = Renderer(c.width, c.height)                    # renders nothing
        bare.set_option("tile_mode", c.tile_mode)
        bare.set_partition(rank, c.world, c.band_rows)
        for form, call in older.items():
            out = filled(want[form].nbytes + GUARD)
            settle()
            call(bare, dev[form].data_ptr(), out.data_ptr())
            settle(bare)
            got = out.cpu().numpy()
            assert (got[want[form].nbytes:] == 0xAB).all(), (form, rank, "written behind the whole frame")
            assert np.array_equal(got[:want[form].nbytes], want[form].reshape(-1).view(np.uint8)), (form, rank)
        bare.close()


# ---- 3: present, tone map and the RGBA8 form --------------------------------------------------------------------------
@pytest.mark.parametrize("enable,exposure", X.PRESENT_SETTINGS)
@pytest.mark.parametrize("name", X.CASES)
def test_3_present_and_the_rgba8_block(name, enable, exposure):
    c = X.CASES[name]
    for rank in X.test_ranks(name):
        r, frame = inject(name, rank, enable, exposure)
        for hdr16 in (0, 1):
            r.present(hdr16=hdr16)
            settle(r)
            want = bbo.present(X.shard_f32(name, rank), enable, exposure, hdr16)
            got = r.read_presented()
            bad = np.nonzero((got != want).any(axis=-1).reshape(-1))[0]
            assert bad.size == 0, (rank, hdr16, bad[:4], X.shard(name, rank).reshape(-1, 4)[bad[:4]], got.reshape(-1, 4)[bad[:4]],
                                   want.reshape(-1, 4)[bad[:4]])
            size = X.block_bytes(c, X.RGBA8)
            buf = filled(size + GUARD)
            settle()
            r.stage_shard(X.RGBA8, buf.data_ptr())
            settle(r)
            got = buf.cpu().numpy()
            assert (got[size:] == 0xAB).all() and np.array_equal(got[:size], X.encode_block(want, X.RGBA8))
        r.close()


TONE_MAP_CASES = ("256x8", "64x65/4")      # one without a partition, one with: rank 0 owns every row of its shard, rank 3 none
TONE_SETTINGS = [("off", 0, 1.0)] + [(k, 1, e) for k, e in X.EXPOSURES.items()]


@pytest.mark.parametrize("name", TONE_MAP_CASES)
def test_3_tone_map_at_every_exposure(name):
    """bbr_tone_map in place on all shard_rows * width pixels, padding rows included; disabled it still forces alpha to 1"""
    failures = []
    for rank in X.test_ranks(name):
        r, frame = inject(name, rank)
        for key, enable, exposure in TONE_SETTINGS:
            refill(name, rank, frame)
            r.tone_map(enable, exposure)
            got = r.read_shard()
            want = bbo.tone_map(X.shard_f32(name, rank), enable, exposure)
            assert (want[..., 3] == 1.0).all()
            if not equal_but_for_nan_payload(got, want):
                g, w = got.reshape(-1).view(np.uint32), want.reshape(-1).view(np.uint32)
                bad = np.nonzero((np.isnan(got.reshape(-1)) != np.isnan(want.reshape(-1))) | (~np.isnan(want.reshape(-1)) & (g != w)))[0]
                src = X.shard(name, rank).reshape(-1)
                failures.append((key, rank, bad.size, [(hex(src[i]), hex(g[i]), hex(w[i])) for i in bad[:4]]))
        r.close()
    assert not failures, failures      # (exposure, rank, values that differ, [(input, GPU, oracle) bits])


@pytest.mark.parametrize("name", TONE_MAP_CASES)
def test_3_present_buffer_at_every_exposure(name):
    import torch
    failures = []
    n = X.shard_pixels(X.CASES[name])
    r = Renderer(64, 64)
    for rank in X.test_ranks(name):
        src = upload(X.shard(name, rank))
        out = torch.zeros((n, 4), dtype=torch.uint8, device="cuda")
        for key, enable, exposure in TONE_SETTINGS:
            for hdr16 in (0, 1):
                settle()
                r.present_buffer(src.data_ptr(), out.data_ptr(), n, enable, exposure, hdr16)
                settle(r)
                got = out.cpu().numpy()
                want = bbo.present(X.shard_f32(name, rank), enable, exposure, hdr16).reshape(-1, 4)
                bad = np.nonzero((got != want).any(axis=1))[0]
                if bad.size:
                    failures.append((key, hdr16, rank, bad.size, [(X.shard(name, rank).reshape(-1, 4)[i].tolist(), got[i].tolist(),
                                                                   want[i].tolist()) for i in bad[:3]]))
    r.close()
    assert not failures, failures


# ---- 4: push, narrow form ---------------------------------------------------------------------------------------------
def code_of(call, *args):
    with pytest.raises(BibimError) as e:
        call(*args)
    return _capi.STATUS[e.value.code]


@pytest.mark.parametrize("form", X.FORMS)
def test_4_push_into_buffers_off_16_byte_alignment(form):
    """64x65/4: every block is a multiple of 16 bytes, so only the gather pointers decide between k_push_block<uint4> and
    k_push_block<uint32_t>.  8 bytes off, every access of the pack kernels is still naturally aligned and the push must take
    the 4-byte form; 4 bytes off, only the plain forms may be pushed at all."""
    name = "64x65/4"
    c = X.CASES[name]
    world, size = c.world, X.block_bytes(c, form)
    total, want = world * size, X.gathered(name, form)
    rs = [inject(name, rank, push_mode=1) for rank in range(world)]
    for r, _ in rs:
        if form == X.RGBA8:
            r.present()
        assert r.exchange_block_bytes(form) == size
    settle(*[r for r, _ in rs])
    block_align, gather_align, whole_align = X.ALIGN[form]
    results = {}
    for push_mode in (1, 0):
        for offset in (8, 16, 4):
            if offset % block_align:
                continue
            bufs = [filled(offset + total + 8) for _ in range(world)]
            settle()
            assert all(b.data_ptr() % 16 == 0 for b in bufs)
            ptrs = [b.data_ptr() + offset for b in bufs]
            for r, _ in rs:
                r.set_option("push_mode", push_mode)
                r.push_shard(form, ptrs, [0] * world)
                assert r.push_was_direct() == bool(push_mode)
            settle(*[r for r, _ in rs])     # "all pushes have landed"
            host = [b.cpu().numpy() for b in bufs]
            for h in host:
                assert (h[:offset] == 0xAB).all() and (h[offset + total:] == 0xAB).all(), (push_mode, offset, "guard bytes")
                assert np.array_equal(h[offset:offset + total], host[0][offset:offset + total])
            results[push_mode, offset] = host[0][offset:offset + total].copy()
            if offset == 16:
                aligned = bufs
    first = results[1, 8]
    for r in range(world):
        assert block_is(first[r * size:(r + 1) * size], want[r * size:(r + 1) * size], form, c), r
    assert all(np.array_equal(v, first) for v in results.values()), [k for k, v in results.items() if not np.array_equal(v, first)]
    for rank in (0, world - 1):                                # unpack from an aligned copy
        r = rs[rank][0]
        r.unpack_whole(form, aligned[rank].data_ptr() + 16)
        assert whole_is(r.read_whole_frame(form), X.whole(name, form), form), rank

    # the alignment rules (include/bibim_hip.h, "Alignment") as status codes; nothing is launched on a rejected pointer
    r = rs[1][0]
    r.set_option("push_mode", 1)
    canary = [filled(16 + total + 16) for _ in range(world)]
    frame_out = filled(16 + X.whole(name, form).nbytes + 16)
    settle()
    base = [b.data_ptr() for b in canary]
    bad = "BBR_ERR_INVALID_ARGUMENT"
    for off in (1, 2, 4, 8):
        if off % block_align == 0:
            continue
        assert code_of(r.push_shard, form, [base[0] + 16, base[1] + 16, base[2] + 16, base[3] + off], [0] * world) == bad, off
        assert code_of(r.push_shard, form, [p + off for p in base], [0] * world) == bad, off
        assert code_of(r.stage_shard, form, base[0] + off) == bad, off
    for off in (1, 2, 4, 8):
        if off % gather_align:
            assert code_of(r.unpack_whole, form, base[0] + off, frame_out.data_ptr()) == bad, off
        if off % whole_align:
            assert code_of(r.unpack_whole, form, base[0], frame_out.data_ptr() + off) == bad, off
    older = {X.RGBA32F: r.unpack_gathered, X.PACKED: r.unpack_gathered_packed, X.RGBA8: r.unpack_gathered_rgba8}.get(form)
    if older:
        assert code_of(older, base[0] + gather_align // 2, frame_out.data_ptr()) == bad
        assert code_of(older, base[0], frame_out.data_ptr() + whole_align // 2) == bad
    if form == X.PACKED:
        assert code_of(r.pack_shard, base[0] + 4) == bad
    settle(*[r for r, _ in rs])
    assert all((b.cpu().numpy() == 0xAB).all() for b in canary + [frame_out]), "a rejected call wrote"
    for r, _ in rs:
        r.close()


# ---- 5: push among more ranks than one launch serves ------------------------------------------------------------------
def test_5_push_among_17_ranks():
    """1x544/17, PACKED (a block of 400 bytes: 384 of rgb, a half-used mask word, 8 bytes of padding).  One process, contexts
    for ranks 0, 9 and 16 only; each pushes into all 17 gather buffers: 15 targets in a first launch, the 16th in a second,
    (rank + k) % world wrapping in both.  Afterwards block r of EVERY buffer is rank r's for the three ranks that pushed, and
    every other byte is untouched."""
    name, form, ranks = "1x544/17", X.PACKED, (0, 9, 16)
    c = X.CASES[name]
    world, size = c.world, X.block_bytes(c, form)
    assert world == 17 and size == 400
    rs = {rank: inject(name, rank, push_mode=1) for rank in ranks}
    bufs = [filled(world * size + GUARD) for _ in range(world)]
    settle()
    ptrs = [b.data_ptr() for b in bufs]
    for rank in ranks:
        rs[rank][0].push_shard(form, ptrs, [0] * world)
        assert rs[rank][0].push_was_direct()
    settle(*[r for r, _ in rs.values()])
    want = np.full(world * size + GUARD, 0xAB, np.uint8)
    for rank in ranks:
        want[rank * size:(rank + 1) * size] = X.block(name, form, rank)
    for k, b in enumerate(bufs):
        got = b.cpu().numpy()
        wrong = sorted({int(i) // size for i in np.nonzero(got != want)[0]})
        assert not wrong, (f"buffer {k}: blocks", wrong)
    for r, _ in rs.values():
        r.close()
