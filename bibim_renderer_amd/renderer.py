"""Thin object wrapper over the C ABI.  Names follow the reference's vocabulary: a mesh is a vertex
(+ index) buffer, a material is the six-map PBRMaterial, a frame is begin -> draw* -> end."""
from __future__ import annotations

import ctypes as C
import weakref

import numpy as np

from . import _capi, partition
from ._capi import BbrImage, BbrStats, BbrUiDraw, BibimError, lib

MAP_NAMES = ("albedo", "metallic", "roughness", "ao", "normal", "height")
# bbr_tbn_segment (include/bibim_hip.h): endpoints in 1/256 pixel, z / w at both ends, key = primitive * 8 + segment
TBN_SEGMENT_DTYPE = np.dtype([("x0", "<i4"), ("y0", "<i4"), ("x1", "<i4"), ("y1", "<i4"), ("za", "<f4"), ("zb", "<f4"),
                              ("key", "<u4"), ("pad", "<u4")])

# one primitive record and one triangle of bbr_read_records (include/bibim_hip.h, "primitive-record read-back")
RECORD_DTYPE = np.dtype([("X0", "<i4"), ("Y0", "<i4"), ("l1dx", "<f4"), ("l1dy", "<f4"), ("l2dx", "<f4"), ("l2dy", "<f4"),
                         ("rw", "<f4", (3,)), ("uv", "<f4", (3, 2)), ("packed_dims", "<u4"), ("packed", "<u8"),
                         ("material", "<u4"), ("clip_base", "<u4"), ("vary", "<f4", (12, 3))])
TRIANGLE_DTYPE = np.dtype([("X0", "<i4"), ("Y0", "<i4"), ("X1", "<i4"), ("Y1", "<i4"), ("X2", "<i4"), ("Y2", "<i4"),
                           ("z0", "<f4"), ("dzdx", "<f4"), ("dzdy", "<f4"), ("l1dx", "<f4"), ("l1dy", "<f4"), ("l2dx", "<f4"),
                           ("l2dy", "<f4"), ("rw", "<f4", (3,))])
assert RECORD_DTYPE.itemsize == 224 and TRIANGLE_DTYPE.itemsize == 64


# bbr_ui_cmd and ImDrawVert (include/bibim_hip.h, "GUI pass")
UI_CMD_DTYPE = np.dtype([("clip_rect", "<f4", (4,)), ("texture", "<i4"), ("vtx_offset", "<u4"), ("idx_offset", "<u4"),
                         ("elem_count", "<u4")])
UI_VERTEX_DTYPE = np.dtype([("pos", "<f4", (2,)), ("uv", "<f4", (2,)), ("col", "<u4")])


def _ptr(a):
    return a.ctypes.data_as(C.c_void_p) if a is not None else None


class UiDrawData:
    """A bbr_ui_draw over numpy arrays (which it keeps alive): vertices UI_VERTEX_DTYPE [n], indices uint16 [m], commands
    UI_CMD_DTYPE [k] -- all command lists flattened in order, offsets made global."""

    def __init__(self, vertices, indices, cmds, display_pos, display_size, framebuffer_scale=(1.0, 1.0)):
        self.vertices = np.ascontiguousarray(vertices, UI_VERTEX_DTYPE).reshape(-1)
        self.indices = np.ascontiguousarray(indices, np.uint16).reshape(-1)
        self.cmds = np.ascontiguousarray(cmds, UI_CMD_DTYPE).reshape(-1)
        self.display_pos = tuple(float(x) for x in display_pos)
        self.display_size = tuple(float(x) for x in display_size)
        self.framebuffer_scale = tuple(float(x) for x in framebuffer_scale)

    def struct(self):
        d = BbrUiDraw()
        d.vertices, d.n_vertices = (self.vertices.ctypes.data if len(self.vertices) else None), len(self.vertices)
        d.indices, d.n_indices = (self.indices.ctypes.data if len(self.indices) else None), len(self.indices)
        d.cmds, d.n_cmds = (self.cmds.ctypes.data if len(self.cmds) else None), len(self.cmds)
        d.display_pos[:] = self.display_pos
        d.display_size[:] = self.display_size
        d.framebuffer_scale[:] = self.framebuffer_scale
        return d


def ui_validate(draw, fb_width, fb_height):
    """bbr_ui_validate (host only): (status, (x0, y0, x1, y1)) -- the union of the drawing commands' scissors in the frame"""
    box = (C.c_int32 * 4)()
    d = draw.struct()
    rc = lib().bbr_ui_validate(C.byref(d), int(fb_width), int(fb_height), box)
    return rc, tuple(box)


LIVE_RESOURCES = ("device_allocs", "device_bytes", "pinned_blocks", "events", "streams")


def live_resources():
    """bbr_debug_live_resources: what the library holds alive in this process, over all contexts (no GPU call)"""
    out = (C.c_uint64 * len(LIVE_RESOURCES))()
    rc = lib().bbr_debug_live_resources(out)
    assert rc == 0, rc
    return dict(zip(LIVE_RESOURCES, (int(x) for x in out)))


class Renderer:
    def __init__(self, width, height, device=0):
        self._L = lib()
        self._ctx = C.c_void_p()
        rc = self._L.bbr_create(width, height, device, C.byref(self._ctx))
        if rc != 0:
            raise BibimError(rc, (self._L.bbr_last_error(None) or b"").decode())
        self.width, self.height = int(width), int(height)
        self.supersample = 1  # option "supersample": the fine frame is supersample x the output extent
        self.shadow_map = 0   # option "shadow_map": the side of the map read_shadow_map returns
        self._scenes = weakref.WeakSet()  # host-shim scenes hold meshes of this context: they must go first

    # -- plumbing --
    def _check(self, rc):
        if rc != 0:
            raise BibimError(rc, (self._L.bbr_last_error(self._ctx) or b"").decode())

    def close(self):
        if self._ctx:
            for sc in list(self._scenes):
                sc.close()
            self._L.bbr_destroy(self._ctx)
            self._ctx = C.c_void_p()

    def resize(self, width, height):
        """onWindowResize: new extent, same meshes / materials / options."""
        self._check(self._L.bbr_resize(self._ctx, width, height))
        self.width, self.height = int(width), int(height)

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # -- resources --
    def upload_mesh(self, vertices, indices=None):
        v = np.ascontiguousarray(vertices)
        assert v.dtype.itemsize == 44 or (v.dtype == np.float32 and v.shape[-1] == 11)
        n = v.shape[0]
        idx = None if indices is None else np.ascontiguousarray(indices, np.uint32)
        out = C.c_int32()
        self._check(self._L.bbr_upload_mesh(self._ctx, _ptr(v), n, _ptr(idx), 0 if idx is None else len(idx), C.byref(out)))
        return out.value

    def upload_material(self, maps=None):
        maps = maps or {}
        arr = (BbrImage * 6)()
        keep = []
        for i, name in enumerate(MAP_NAMES):
            a = maps.get(name)
            if a is None:
                arr[i] = BbrImage(None, 0, 0)
            else:
                a = np.ascontiguousarray(a, np.uint8)
                assert a.ndim == 3 and a.shape[2] == 4
                keep.append(a)
                arr[i] = BbrImage(a.ctypes.data, a.shape[1], a.shape[0])
        out = C.c_int32()
        self._check(self._L.bbr_upload_material(self._ctx, arr, C.byref(out)))
        return out.value

    def free_mesh(self, mesh):
        self._check(self._L.bbr_free_mesh(self._ctx, mesh))

    def free_material(self, material):
        self._check(self._L.bbr_free_material(self._ctx, material))

    # -- frame --
    def set_frame_uniforms(self, block):
        b = np.ascontiguousarray(block)
        assert b.nbytes == 6432
        self._check(self._L.bbr_set_frame_uniforms(self._ctx, _ptr(b)))

    def set_view_uniforms(self, block):
        b = np.ascontiguousarray(block)
        assert b.nbytes == 144
        self._check(self._L.bbr_set_view_uniforms(self._ctx, _ptr(b)))

    def begin_frame(self):
        self._check(self._L.bbr_begin_frame(self._ctx))

    def draw(self, mesh, material, instances):
        inst = np.ascontiguousarray(instances)
        assert inst.nbytes % 128 == 0
        self._check(self._L.bbr_draw(self._ctx, mesh, material, _ptr(inst), inst.nbytes // 128))

    def end_frame(self):
        self._check(self._L.bbr_end_frame(self._ctx))

    def replay_frame(self):
        self._check(self._L.bbr_replay_frame(self._ctx))

    def synchronize(self):
        self._check(self._L.bbr_synchronize(self._ctx))

    # -- output --
    def read_framebuffer(self):
        out = np.empty((self.height, self.width, 4), np.float32)
        self._check(self._L.bbr_read_framebuffer(self._ctx, _ptr(out)))
        return out

    def read_samples(self):
        """the fine frame of the last frame (option "supersample" = n): [n*height, n*width, 4] float32"""
        n = self.supersample
        out = np.empty((n * self.height, n * self.width, 4), np.float32)
        self._check(self._L.bbr_read_samples(self._ctx, _ptr(out)))
        return out

    def read_sample_map(self):
        """rep(s) of every fine pixel of the last frame (option "sample_shading"): [n*height, n*width] uint8, each an index
        0 .. n*n - 1 into the sample's block; the identity with "sample_shading" 1 or n = 1"""
        n = self.supersample
        out = np.empty((n * self.height, n * self.width), np.uint8)
        self._check(self._L.bbr_read_sample_map(self._ctx, _ptr(out)))
        return out

    def read_visibility(self):
        prim = np.empty((self.height, self.width), np.uint32)
        depth = np.empty((self.height, self.width), np.float32)
        self._check(self._L.bbr_read_visibility(self._ctx, _ptr(prim), _ptr(depth)))
        return prim, depth

    def read_sample_visibility(self):
        """winner and depth of every fine pixel of the last frame (option "supersample" = n): two [n*height, n*width] arrays,
        uint32 and float32 -- the samples option "depth_resolve" chooses from; read_visibility() with n = 1"""
        n = self.supersample
        prim = np.empty((n * self.height, n * self.width), np.uint32)
        depth = np.empty((n * self.height, n * self.width), np.float32)
        self._check(self._L.bbr_read_sample_visibility(self._ctx, _ptr(prim), _ptr(depth)))
        return prim, depth

    def read_depth(self):
        """the depth the last frame kept for the overlay pass (option "overlays"; n >= 2: under option "depth_resolve"):
        [height, width] float32"""
        depth = np.empty((self.height, self.width), np.float32)
        self._check(self._L.bbr_read_depth(self._ctx, _ptr(depth)))
        return depth

    def stats(self):
        s = BbrStats()
        self._check(self._L.bbr_get_stats(self._ctx, C.byref(s)))
        return s.as_dict()

    def set_option(self, name, value):
        self._check(self._L.bbr_set_option(self._ctx, name.encode(), int(value)))
        if name == "supersample":
            self.supersample = int(value)
        if name == "shadow_map":
            self.shadow_map = int(value)

    def last_frame_time_ms(self):
        a, b = C.c_float(), C.c_float()
        self._check(self._L.bbr_last_frame_time_ms(self._ctx, C.byref(a), C.byref(b)))
        return a.value, b.value

    def timing_reset(self):
        self._check(self._L.bbr_timing_reset(self._ctx))

    def timing_summary(self):
        """(frames, avg frame ms, avg geometry ms, avg raster ms, avg shade ms) since timing_reset()."""
        n, f, g, r, t = C.c_uint32(), C.c_float(), C.c_float(), C.c_float(), C.c_float()
        self._check(self._L.bbr_timing_summary(self._ctx, C.byref(n), C.byref(f), C.byref(g), C.byref(r), C.byref(t)))
        return n.value, f.value, g.value, r.value, t.value

    def selftest_rcp(self, lo_bits=0, hi_bits=0x7FFFFFFF):
        n = C.c_uint64()
        self._check(self._L.bbr_selftest_rcp(self._ctx, lo_bits, hi_bits, C.byref(n)))
        return n.value

    def tone_map(self, enable, exposure):
        self._check(self._L.bbr_tone_map(self._ctx, int(enable), float(exposure)))

    def read_gbuffer(self):
        """deferred path only: [h, w, 4 attachments, 4] float32 (binary16 values)"""
        out = np.empty((self.height, self.width, 4, 4), np.float32)
        self._check(self._L.bbr_read_gbuffer(self._ctx, _ptr(out)))
        return out

    def read_surface(self):
        """what the fragment stage saw and produced per pixel, [h, w, 32] float32 (layout: include/bibim_hip.h,
        "surface read-back"); re-renders the last frame"""
        out = np.empty((self.height, self.width, 32), np.float32)
        self._check(self._L.bbr_read_surface(self._ctx, _ptr(out)))
        return out

    # -- shadow mapping (option "shadow_map" = S > 0; include/bibim_hip.h, "shadow mapping") --
    def render_shadow_map(self, light_index, light_view, bias=0.0):
        """render the S x S depth map of the recorded draws from `light_view` (a 144-byte view block: view and proj are used) and
        make light `light_index` the caster of every frame submitted from now on; synchronous.  Inside a frame after the draws,
        or after end_frame()"""
        b = np.ascontiguousarray(light_view)
        assert b.nbytes == 144
        self._check(self._L.bbr_render_shadow_map(self._ctx, int(light_index), _ptr(b), float(bias)))

    def read_shadow_map(self):
        """the shadow map, [S, S] float32"""
        s = max(int(self.shadow_map), 0)
        out = np.empty(max(s * s, 1), np.float32)  # (s = 0: the call refuses)
        self._check(self._L.bbr_read_shadow_map(self._ctx, _ptr(out)))
        return out.reshape(s, s)

    def render_shadow_faces(self, light_index, light_views, bias=0.0):
        """render_shadow_map with F = 1 .. 6 faces: `light_views` holds F consecutive 144-byte view blocks (cube_shadow_views
        gives the six of a point light).  The first face a fragment is not outside of decides it; one face is
        render_shadow_map"""
        b = np.ascontiguousarray(light_views)
        assert b.nbytes % 144 == 0
        self._check(self._L.bbr_render_shadow_faces(self._ctx, int(light_index), b.nbytes // 144, _ptr(b), float(bias)))

    def read_shadow_face(self, face):
        """the shadow map of one face, [S, S] float32"""
        s = max(int(self.shadow_map), 0)
        out = np.empty(max(s * s, 1), np.float32)  # (s = 0: the call refuses)
        self._check(self._L.bbr_read_shadow_face(self._ctx, int(face), _ptr(out)))
        return out.reshape(s, s)

    def read_shadow_face_index(self):
        """the face that decided every pixel of the last frame, [h, w] uint8: 255 where the pixel is not covered or outside
        every face; re-renders the last frame"""
        out = np.empty((self.height, self.width), np.uint8)
        self._check(self._L.bbr_read_shadow_face_index(self._ctx, _ptr(out)))
        return out

    def read_shadow_mask(self):
        """the shadow class of every pixel of the last frame, [h, w] uint8: 0 not covered, 1 lit, 2 shadowed, 3 outside the
        map, 4 partly lit (option "shadow_filter" >= 1); re-renders the last frame"""
        out = np.empty((self.height, self.width), np.uint8)
        self._check(self._L.bbr_read_shadow_mask(self._ctx, _ptr(out)))
        return out

    def read_shadow_taps(self):
        """k, the number of lit taps of every pixel of the last frame, [h, w] uint8: 0 .. (2R + 1)^2 under option "shadow_filter"
        = R (R = 0: 1 lit, 0 shadowed), 255 where the pixel is not covered or outside the map; re-renders the last frame"""
        out = np.empty((self.height, self.width), np.uint8)
        self._check(self._L.bbr_read_shadow_taps(self._ctx, _ptr(out)))
        return out

    # -- up to eight casters (include/bibim_hip.h, "Casters"): slot 0 is the caster of the calls above --
    def render_shadow_caster(self, caster, light_index, light_views, bias=0.0):
        """render_shadow_faces for caster slot `caster` (0 .. 7): light `light_index` is shadowed through the F = 1 .. 6 view
        blocks of `light_views`.  One slot per light"""
        b = np.ascontiguousarray(light_views)
        assert b.nbytes % 144 == 0
        self._check(self._L.bbr_render_shadow_caster(self._ctx, int(caster), int(light_index), b.nbytes // 144, _ptr(b), float(bias)))

    def queue_shadow_caster(self, caster, light_index, light_views, bias=0.0):
        """render_shadow_caster queued with the frame being recorded (between begin_frame and end_frame): the frame is the one
        with render_shadow_caster called in front of its end_frame, but nothing waits and no frame in flight is drained"""
        b = np.ascontiguousarray(light_views)
        assert b.nbytes % 144 == 0
        self._check(self._L.bbr_queue_shadow_caster(self._ctx, int(caster), int(light_index), b.nbytes // 144, _ptr(b), float(bias)))

    def shadow_queue_counts(self):
        """(queued passes submitted, drains of the context they caused) since the context was created; does not synchronise"""
        passes, drains = C.c_uint64(0), C.c_uint64(0)
        self._check(self._L.bbr_shadow_queue_counts(self._ctx, C.byref(passes), C.byref(drains)))
        return passes.value, drains.value

    def drop_shadow_caster(self, caster):
        """release the slot's maps and mark it not in use"""
        self._check(self._L.bbr_drop_shadow_caster(self._ctx, int(caster)))

    def shadow_casters(self):
        """(light index of every slot, -1 where it is not in use; number of faces of every slot), two int32 [8]"""
        light, faces = np.empty(8, np.int32), np.empty(8, np.int32)
        self._check(self._L.bbr_get_shadow_casters(self._ctx, _ptr(light), _ptr(faces)))
        return light, faces

    def read_shadow_caster_face(self, caster, face):
        """read_shadow_face for one slot"""
        s = max(int(self.shadow_map), 0)
        out = np.empty(max(s * s, 1), np.float32)  # (s = 0: the call refuses)
        self._check(self._L.bbr_read_shadow_caster_face(self._ctx, int(caster), int(face), _ptr(out)))
        return out.reshape(s, s)

    def _read_shadow_caster(self, call, caster):
        out = np.empty((self.height, self.width), np.uint8)
        self._check(call(self._ctx, int(caster), _ptr(out)))
        return out

    def read_shadow_caster_mask(self, caster):
        """read_shadow_mask for one slot; re-renders the last frame"""
        return self._read_shadow_caster(self._L.bbr_read_shadow_caster_mask, caster)

    def read_shadow_caster_face_index(self, caster):
        """read_shadow_face_index for one slot; re-renders the last frame"""
        return self._read_shadow_caster(self._L.bbr_read_shadow_caster_face_index, caster)

    def read_shadow_caster_taps(self, caster):
        """read_shadow_taps for one slot; re-renders the last frame"""
        return self._read_shadow_caster(self._L.bbr_read_shadow_caster_taps, caster)

    def read_material_level(self, material, map_index, level):
        """level `level` of one of a material's six maps (PBRMapType order), uint8 [h, w, 4] (option "mip_levels")"""
        w, h = C.c_int32(), C.c_int32()
        self._check(self._L.bbr_read_material_level(self._ctx, material, map_index, level, None, 0, C.byref(w), C.byref(h)))
        out = np.empty((h.value, w.value, 4), np.uint8)
        self._check(self._L.bbr_read_material_level(self._ctx, material, map_index, level, _ptr(out), out.nbytes, C.byref(w), C.byref(h)))
        return out

    def read_packed_level(self, material, level):
        """the packed form of one level of a material, uint8 [bytes] (empty for an unpacked material)"""
        n = C.c_uint64()
        self._check(self._L.bbr_read_packed_level(self._ctx, material, level, None, 0, C.byref(n)))
        out = np.empty(n.value, np.uint8)
        if n.value:
            self._check(self._L.bbr_read_packed_level(self._ctx, material, level, _ptr(out), out.nbytes, C.byref(n)))
        return out

    def read_records(self):
        """what k_geometry wrote per primitive of the last frame: (records RECORD_DTYPE [n], triangles TRIANGLE_DTYPE [n]);
        a culled primitive keeps the 0xFF fill (material == 0xFFFFFFFF); re-renders the last frame"""
        n = C.c_uint32()
        self._check(self._L.bbr_read_records(self._ctx, None, None, 0, C.byref(n)))
        recs, tris = np.zeros(n.value, RECORD_DTYPE), np.zeros(n.value, TRIANGLE_DTYPE)
        self._check(self._L.bbr_read_records(self._ctx, _ptr(recs), _ptr(tris), n.value, C.byref(n)))
        assert n.value == len(recs)
        return recs, tris

    # -- overlay subpass (light markers + corner gizmo over the presented image) --
    def upload_gizmo(self, vertices, indices=None):
        """vertices: float32 [n, 9] = pos, colour, normal (bb::GizmoVertex); indices: uint32 [m] or None"""
        v = np.ascontiguousarray(vertices, np.float32).reshape(-1, 9)
        i = None if indices is None else np.ascontiguousarray(indices, np.uint32)
        self._check(self._L.bbr_upload_gizmo(self._ctx, _ptr(v), v.shape[0], None if i is None else _ptr(i), 0 if i is None else i.size))

    def draw_overlays(self, gizmo_extent=100):
        self._check(self._L.bbr_draw_overlays(self._ctx, int(gizmo_extent)))

    # -- GUI pass (the back end's draw lists blended into the presented image; src/main.cpp:172) --
    def upload_ui_texture(self, rgba8):
        """uint8 [h, w, 4] -> the handle (>= 1) a bbr_ui_cmd names"""
        a = np.ascontiguousarray(rgba8, np.uint8)
        assert a.ndim == 3 and a.shape[2] == 4
        out = C.c_int32()
        self._check(self._L.bbr_upload_ui_texture(self._ctx, _ptr(a), a.shape[1], a.shape[0], C.byref(out)))
        return out.value

    def free_ui_texture(self, texture):
        self._check(self._L.bbr_free_ui_texture(self._ctx, int(texture)))

    def draw_ui(self, draw):
        """queue the GUI pass over the image of the last present (asynchronous); draw: UiDrawData"""
        d = draw.struct()
        self._check(self._L.bbr_draw_ui(self._ctx, C.byref(d)))

    # -- presentation (tone map + sRGB + UNORM8) --
    # -- TBN line overlay (option "tbn": bbr_draw_overlays draws the tangent frames of the last frame first) --
    def read_tbn_segments(self):
        """segment records of the last TBN draw, in key order (numpy structured array of TBN_SEGMENT_DTYPE)"""
        n = C.c_uint32()
        self._check(self._L.bbr_read_tbn_segments(self._ctx, None, 0, C.byref(n)))
        out = np.zeros(n.value, TBN_SEGMENT_DTYPE)
        self._check(self._L.bbr_read_tbn_segments(self._ctx, _ptr(out), len(out), C.byref(n)))
        assert n.value == len(out)
        return out

    def selftest_lines(self, segments, width, height, depth):
        """the pass's raster + resolve on caller-supplied segments: [height, width] uint32 of key + 1 (0: nothing passed)"""
        segs = np.ascontiguousarray(segments, TBN_SEGMENT_DTYPE)
        depth = np.ascontiguousarray(depth, np.float32)
        assert depth.shape == (height, width)
        keys = np.zeros((height, width), np.uint32)
        self._check(self._L.bbr_selftest_lines(self._ctx, _ptr(segs) if len(segs) else None, len(segs), int(width),
                                               int(height), _ptr(depth), _ptr(keys)))
        return keys

    def present(self, rgba8_device_ptr=None, hdr16=True):
        """queue k_present for the last frame; EnableToneMapping / Exposure come from its FrameUniformBlock"""
        self._check(self._L.bbr_present(self._ctx, C.c_void_p(rgba8_device_ptr) if rgba8_device_ptr else None, int(bool(hdr16))))

    def present_buffer(self, rgba32f_ptr, rgba8_ptr, n_pixels, enable, exposure, hdr16=True, stream=None):
        self._check(self._L.bbr_present_buffer(self._ctx, C.c_void_p(rgba32f_ptr), C.c_void_p(rgba8_ptr), int(n_pixels),
                                               int(enable), float(exposure), int(bool(hdr16)),
                                               C.c_void_p(stream) if stream else None))

    def read_presented(self):
        rows = self.shard_rows()
        out = np.empty((rows, self.width, 4), np.uint8)
        self._check(self._L.bbr_read_presented(self._ctx, _ptr(out)))
        return out

    def present_timing(self):
        """(launches, average k_present ms) since timing_reset(), option "timing" on"""
        n, t = C.c_uint32(), C.c_float()
        self._check(self._L.bbr_present_timing(self._ctx, C.byref(n), C.byref(t)))
        return n.value, t.value

    def resolve_timing(self):
        """(launches, average k_resolve ms) since timing_reset(), options "timing" on and "supersample" >= 2"""
        n, t = C.c_uint32(), C.c_float()
        self._check(self._L.bbr_resolve_timing(self._ctx, C.byref(n), C.byref(t)))
        return n.value, t.value

    # -- bloom (option "bloom" = L >= 1: a pyramid in front of k_present_bloom; the rule: bibim_hip.h "bloom") --
    def set_bloom(self, threshold, intensity):
        self._check(self._L.bbr_set_bloom(self._ctx, float(threshold), float(intensity)))

    def get_bloom(self):
        """(levels, threshold, intensity) as stored"""
        n, t, i = C.c_int32(), C.c_float(), C.c_float()
        self._check(self._L.bbr_get_bloom(self._ctx, C.byref(n), C.byref(t), C.byref(i)))
        return n.value, t.value, i.value

    def present_buffer_bloom(self, rgba32f_ptr, rgba8_ptr, width, height, enable, exposure, hdr16=True, stream=None):
        """the bloom rule + presentation on any width x height RGBA32F device frame (asynchronous)"""
        self._check(self._L.bbr_present_buffer_bloom(self._ctx, C.c_void_p(rgba32f_ptr), C.c_void_p(rgba8_ptr), int(width),
                                                     int(height), int(enable), float(exposure), int(bool(hdr16)),
                                                     C.c_void_p(stream) if stream else None))

    def read_bloom_level(self, level, source=0):
        """U_level, float32 [h_k, w_k, 3], of the last frame's presentation (source 0) or the last buffer call (source 1)"""
        w, h = C.c_int32(), C.c_int32()
        self._check(self._L.bbr_read_bloom_level(self._ctx, int(source), int(level), None, 0, C.byref(w), C.byref(h)))
        out = np.empty((h.value, w.value, 3), np.float32)
        self._check(self._L.bbr_read_bloom_level(self._ctx, int(source), int(level), _ptr(out), out.nbytes, C.byref(w), C.byref(h)))
        return out

    def bloom_timing(self):
        """(chains, average ms of one) since timing_reset(), option "timing" on"""
        n, t = C.c_uint32(), C.c_float()
        self._check(self._L.bbr_bloom_timing(self._ctx, C.byref(n), C.byref(t)))
        return n.value, t.value

    # -- auto exposure (option "auto_exposure" = 1: the exposure is metered on the device; the rule: bibim_hip.h "auto exposure") --
    # bbr_exposure_record, field for field
    EXPOSURE_RECORD = np.dtype([("hist", np.uint32, 256), ("ignored", np.uint32), ("counted", np.uint32), ("kept", np.uint32),
                                ("mean_bits", np.uint32), ("sum", np.uint64), ("target", np.float32), ("clamped", np.float32),
                                ("previous", np.float32), ("applied", np.float32), ("flags", np.uint32), ("reserved", np.uint32)])

    def set_auto_exposure(self, key=0.18, e_min=2.0 ** -10, e_max=2.0 ** 10, rate=1.0, lo_permille=500, hi_permille=950):
        self._check(self._L.bbr_set_auto_exposure(self._ctx, float(key), float(e_min), float(e_max), float(rate), int(lo_permille),
                                                  int(hi_permille)))

    def get_auto_exposure(self):
        """(key, e_min, e_max, rate, lo_permille, hi_permille) as stored"""
        k, a, b, r, lo, hi = C.c_float(), C.c_float(), C.c_float(), C.c_float(), C.c_int32(), C.c_int32()
        self._check(self._L.bbr_get_auto_exposure(self._ctx, C.byref(k), C.byref(a), C.byref(b), C.byref(r), C.byref(lo), C.byref(hi)))
        return k.value, a.value, b.value, r.value, lo.value, hi.value

    def reset_exposure(self):
        self._check(self._L.bbr_reset_exposure(self._ctx))

    def present_buffer_auto(self, rgba32f_ptr, rgba8_ptr, width, height, enable, exposure, hdr16=True, stream=None):
        """the auto exposure rule (and option "bloom") + presentation on any width x height RGBA32F device frame (asynchronous)"""
        self._check(self._L.bbr_present_buffer_auto(self._ctx, C.c_void_p(rgba32f_ptr), C.c_void_p(rgba8_ptr), int(width),
                                                    int(height), int(enable), float(exposure), int(bool(hdr16)),
                                                    C.c_void_p(stream) if stream else None))

    def read_exposure(self, source=0):
        """the record of the last presentation of bbr_present (source 0) or bbr_present_buffer_auto (source 1): a dict of numpy values"""
        rec = np.zeros(1, self.EXPOSURE_RECORD)
        self._check(self._L.bbr_read_exposure(self._ctx, int(source), _ptr(rec)))
        return {name: rec[name][0] for name in self.EXPOSURE_RECORD.names if name != "reserved"}

    def luminance_timing(self):
        """(k_luminance launches, average ms of one) since timing_reset(), option "timing" on"""
        n, t = C.c_uint32(), C.c_float()
        self._check(self._L.bbr_luminance_timing(self._ctx, C.byref(n), C.byref(t)))
        return n.value, t.value

    def presented_device_ptr(self):
        p, n = C.c_void_p(), C.c_uint64()
        self._check(self._L.bbr_presented_device_ptr(self._ctx, C.byref(p), C.byref(n)))
        return p.value, n.value

    def unpack_gathered_rgba8(self, gathered_ptr, frame_ptr, stream=None):
        self._check(self._L.bbr_unpack_gathered_rgba8(self._ctx, C.c_void_p(gathered_ptr), C.c_void_p(frame_ptr),
                                                      C.c_void_p(stream) if stream else None))

    def stream_layout_state(self):
        """(layout in use, decided?, [ms of the timed spans per layout])"""
        lay, dec, ms = C.c_int32(), C.c_int32(), (C.c_float * 3)()
        self._check(self._L.bbr_stream_layout_state(self._ctx, C.byref(lay), C.byref(dec), ms))
        return lay.value, bool(dec.value), [float(x) for x in ms]

    # -- multi-GPU partition --
    def set_partition(self, rank, world, band_rows=0):
        self._check(self._L.bbr_set_partition(self._ctx, rank, world, band_rows))

    def shard_rows(self):
        r = C.c_int32()
        self._check(self._L.bbr_shard_rows(self._ctx, C.byref(r)))
        return r.value

    def tile_height(self):
        r = C.c_int32()
        self._check(self._L.bbr_tile_height(self._ctx, C.byref(r)))
        return r.value

    def read_shard(self):
        out = np.empty((self.shard_rows(), self.width, 4), np.float32)
        self._check(self._L.bbr_read_shard(self._ctx, _ptr(out)))
        return out

    def set_output_device_ptr(self, ptr, nbytes):
        self._check(self._L.bbr_set_output_device_ptr(self._ctx, C.c_void_p(ptr), nbytes))

    def set_stream(self, stream_handle):
        self._check(self._L.bbr_set_stream(self._ctx, C.c_void_p(stream_handle)))

    def framebuffer_device_ptr(self):
        p, n = C.c_void_p(), C.c_uint64()
        self._check(self._L.bbr_framebuffer_device_ptr(self._ctx, C.byref(p), C.byref(n)))
        return p.value, n.value

    def unpack_gathered(self, gathered_ptr, frame_ptr, stream_handle=None):
        self._check(self._L.bbr_unpack_gathered(self._ctx, C.c_void_p(gathered_ptr), C.c_void_p(frame_ptr),
                                                C.c_void_p(stream_handle) if stream_handle else None))

    def packed_shard_bytes(self):
        n = C.c_uint64()
        self._check(self._L.bbr_packed_shard_bytes(self._ctx, C.byref(n)))
        return n.value

    def pack_shard(self, packed_ptr, stream_handle=None):
        """the last frame's shard as rgb[n][3] float + one alpha bit per pixel (lossless, 12.1 B per pixel)"""
        self._check(self._L.bbr_pack_shard(self._ctx, C.c_void_p(packed_ptr), C.c_void_p(stream_handle) if stream_handle else None))

    def unpack_gathered_packed(self, gathered_ptr, frame_ptr, stream_handle=None):
        self._check(self._L.bbr_unpack_gathered_packed(self._ctx, C.c_void_p(gathered_ptr), C.c_void_p(frame_ptr),
                                                       C.c_void_p(stream_handle) if stream_handle else None))

    # -- native exchange (include/bibim_hip.h, "native exchange") --
    def comm_unique_id(self) -> bytes:
        buf = (C.c_uint8 * _capi.COMM_ID_BYTES)()
        self._check(self._L.bbr_comm_unique_id(self._ctx, buf))
        return bytes(buf)

    def comm_init(self, rank, world, unique_id: bytes):
        assert len(unique_id) == _capi.COMM_ID_BYTES
        buf = (C.c_uint8 * _capi.COMM_ID_BYTES).from_buffer_copy(unique_id)
        self._check(self._L.bbr_comm_init(self._ctx, rank, world, buf))

    def comm_destroy(self):
        self._check(self._L.bbr_comm_destroy(self._ctx))

    def comm_probe(self):
        """can this process load librccl?  Not collective: ranks vote on it before they enter comm_init together."""
        self._check(self._L.bbr_comm_probe(self._ctx))

    def comm_count(self):
        """ranks in the context's communicator, as RCCL reports them (ncclCommCount)"""
        n = C.c_int32()
        self._check(self._L.bbr_comm_count(self._ctx, C.byref(n)))
        return int(n.value)

    def stage_shard(self, form, block_ptr, stream_handle=None):
        """this rank's block of the last frame in `form` -> block_ptr (exchange_block_bytes(form) bytes)"""
        self._check(self._L.bbr_stage_shard(self._ctx, form, C.c_void_p(block_ptr), C.c_void_p(stream_handle) if stream_handle else None))

    def exchange_block_bytes(self, form):
        n = C.c_uint64()
        self._check(self._L.bbr_exchange_block_bytes(self._ctx, form, C.byref(n)))
        return n.value

    def allgather_frame(self, form, gathered_ptr=None, whole_ptr=None, stream_handle=None):
        self._check(self._L.bbr_allgather_frame(self._ctx, form, C.c_void_p(gathered_ptr) if gathered_ptr else None,
                                                C.c_void_p(whole_ptr) if whole_ptr else None,
                                                C.c_void_p(stream_handle) if stream_handle else None))

    def push_shard(self, form, peer_gathered_ptrs, peer_devices, stream_handle=None):
        n = len(peer_gathered_ptrs)
        ptrs = (C.c_void_p * n)(*[C.c_void_p(p) for p in peer_gathered_ptrs])
        devs = (C.c_int32 * n)(*peer_devices)
        self._check(self._L.bbr_push_shard(self._ctx, form, ptrs, devs, C.c_void_p(stream_handle) if stream_handle else None))

    def capacity_growths(self):
        """capacity growths since the context was created (host-side counter: no synchronisation)"""
        n = C.c_uint32()
        self._check(self._L.bbr_capacity_growths(self._ctx, C.byref(n)))
        return int(n.value)

    def static_record_counts(self):
        """option static_records since the context was created (host-side counters: no synchronisation): k_record_static launches,
        draws submitted on the geometry kernel's light path"""
        fills, light = C.c_uint64(), C.c_uint64()
        self._check(self._L.bbr_static_record_counts(self._ctx, C.byref(fills), C.byref(light)))
        return {"fills": int(fills.value), "light_draws": int(light.value)}

    def view_keep_counts(self):
        """option view_keep since the context was created (host-side counters: no synchronisation): main frames kept (shading
        only), main frames rendered in full"""
        kept, full = C.c_uint64(), C.c_uint64()
        self._check(self._L.bbr_view_keep_counts(self._ctx, C.byref(kept), C.byref(full)))
        return {"kept": int(kept.value), "full": int(full.value)}

    def surface_keep_counts(self):
        """option surface_keep since the context was created (host-side counters: no synchronisation): storing frames, frames
        shaded from a kept surface (the storing ones included)"""
        stored, lit = C.c_uint64(), C.c_uint64()
        self._check(self._L.bbr_surface_keep_counts(self._ctx, C.byref(stored), C.byref(lit)))
        return {"stored": int(stored.value), "lit": int(lit.value)}

    def read_surface_keep(self, slot):
        """option surface_keep, frame slot `slot`: (values float32 [items * 64, 12], index uint32 [items * 64]) of its kept surface
        (include/bibim_hip.h); raises BibimError when the slot holds none.  Synchronises, renders nothing."""
        n = C.c_uint32()
        self._check(self._L.bbr_read_surface_keep(self._ctx, int(slot), None, None, 0, C.byref(n)))
        values = np.empty((int(n.value) * 64, 12), np.float32)
        index = np.empty(int(n.value) * 64, np.uint32)
        self._check(self._L.bbr_read_surface_keep(self._ctx, int(slot), _ptr(values), _ptr(index), index.size, C.byref(n)))
        return values, index

    def read_sky_tiles(self):
        """option sky_keep, the most recently submitted frame: a uint8 per tile, (tiles_y * tiles_x,) row-major -- 0 not a
        background tile (or a frame that could not keep), 1 background and filled, 2 background and kept.  Synchronises."""
        n = C.c_uint32()
        self._check(self._L.bbr_read_sky_tiles(self._ctx, None, 0, C.byref(n)))
        out = np.zeros(int(n.value), dtype=np.uint8)
        self._check(self._L.bbr_read_sky_tiles(self._ctx, out.ctypes.data_as(C.POINTER(C.c_uint8)), out.size, C.byref(n)))
        return out

    def host_timing(self):
        """host side of the frame loop since host_timing_reset (no GPU call): frames submitted, ns inside the submit calls, ns of
        that spent blocked on a frame slot still in flight, frames in which the host was blocked"""
        f, sub, blk, nb = C.c_uint64(), C.c_uint64(), C.c_uint64(), C.c_uint64()
        self._check(self._L.bbr_host_timing(self._ctx, C.byref(f), C.byref(sub), C.byref(blk), C.byref(nb)))
        return {"frames": int(f.value), "submit_ns": int(sub.value), "blocked_ns": int(blk.value), "blocked_frames": int(nb.value)}

    def host_timing_reset(self):
        self._check(self._L.bbr_host_timing_reset(self._ctx))

    def push_was_direct(self):
        """True if the last push_shard stored through the one-kernel direct form (option push_mode 1 and every peer mapped)"""
        d = C.c_int32()
        self._check(self._L.bbr_push_state(self._ctx, C.byref(d)))
        return bool(d.value)

    def unpack_whole(self, form, gathered_ptr, whole_ptr=None, stream_handle=None):
        self._check(self._L.bbr_unpack_whole(self._ctx, form, C.c_void_p(gathered_ptr), C.c_void_p(whole_ptr) if whole_ptr else None,
                                             C.c_void_p(stream_handle) if stream_handle else None))

    def whole_frame_device_ptr(self):
        p, n = C.c_void_p(), C.c_uint64()
        self._check(self._L.bbr_whole_frame_device_ptr(self._ctx, C.byref(p), C.byref(n)))
        return p.value, n.value

    def read_whole_frame(self, form=0):
        out = np.empty((self.height, self.width, 4), partition.FORMS[form].whole)
        self._check(self._L.bbr_read_whole_frame(self._ctx, _ptr(out)))
        return out

    def ipc_export(self, device_ptr) -> bytes:
        buf = (C.c_uint8 * _capi.IPC_HANDLE_BYTES)()
        self._check(self._L.bbr_ipc_export(self._ctx, C.c_void_p(device_ptr), buf))
        return bytes(buf)

    def ipc_open(self, handle: bytes):
        buf = (C.c_uint8 * _capi.IPC_HANDLE_BYTES).from_buffer_copy(handle)
        p = C.c_void_p()
        self._check(self._L.bbr_ipc_open(self._ctx, buf, C.byref(p)))
        return p.value

    def ipc_close(self, ptr):
        self._check(self._L.bbr_ipc_close(self._ctx, C.c_void_p(ptr)))

    def wait_event(self, event_handle):
        self._check(self._L.bbr_wait_event(self._ctx, C.c_void_p(event_handle)))

    def stream_wait_frame(self, stream_handle):
        self._check(self._L.bbr_stream_wait_frame(self._ctx, C.c_void_p(stream_handle)))

    # -- convenience: submit a scene description made of numpy inputs --
    def render_scene(self, scene, handles=None):
        """scene: object with .frame, .view and .draws, each draw having .vertices, .indices, .instances and
        .material.maps (dict name -> uint8 [h, w, 4]).  Returns handles so that repeated frames reuse the
        uploaded meshes / materials."""
        if handles is None:
            handles = {"mesh": {}, "mat": {}}
        self.set_frame_uniforms(scene.frame)
        self.set_view_uniforms(scene.view)
        self.begin_frame()
        for d in scene.draws:
            mk = id(d.vertices)
            if mk not in handles["mesh"]:
                handles["mesh"][mk] = self.upload_mesh(d.vertices, d.indices)
            tk = id(d.material)
            if tk not in handles["mat"]:
                handles["mat"][tk] = self.upload_material(d.material.maps)
            self.draw(handles["mesh"][mk], handles["mat"][tk], d.instances)
        self.end_frame()
        return handles
