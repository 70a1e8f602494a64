/*
 * bibim_hip.h -- C ABI of the MI355X-native forward PBR path (libbibim_hip.so).
 *
 * The reference (chromedays/bibim-renderer) has no plugin / FFI layer: its forward path is reached
 * through SceneBase::drawScene(const Frame&) (src/scene.h:84) and the DATA it hands to Vulkan.  Each
 * entry point below replaces one of those hand-offs and consumes the reference's byte layouts unchanged:
 *
 *   bbr_upload_mesh          createVertexBuffer / createIndexBuffer            src/scene.h:86-108
 *                            (bb::Vertex 44 B, src/render.h:112-117; VK_INDEX_TYPE_UINT32, src/scene.cpp:209)
 *   bbr_upload_material      createPBRMaterialSet + set 2 binding               src/render.cpp:1243-1336,
 *                            (6 RGBA8 images in PBRMapType order)               src/shaders/standard_sets.glsl:45-50
 *   bbr_set_frame_uniforms   FrameUniformBlock map/memcpy (6432 B)              src/main.cpp:1288-1327
 *   bbr_set_view_uniforms    ViewUniformBlock map/memcpy (144 B)                src/main.cpp:1329-1342
 *   bbr_begin_frame          vkCmdBeginRenderPass, all clears = 0               src/main.cpp:78-86
 *   bbr_draw                 updateInstanceBufferMemory + vkCmdDraw[Indexed]    src/scene.h:120-132,
 *                            (bb::InstanceBlock 128 B, src/render.h:96-99)      src/scene.cpp:203-210
 *   bbr_end_frame            vkCmdEndRenderPass + vkQueueSubmit                 src/main.cpp:174,1364
 *   bbr_read_framebuffer     the HDR colour attachment (kept fp32 RGBA)         src/main.cpp:463-472
 *   pipeline state           createPipeline + forward params (fixed here)       src/render.cpp:1044-1178,
 *                                                                               src/main.cpp:332-350
 *
 * Conventions: every call returns BBR_OK (0) or a negative bbr_status; bbr_last_error() gives text.
 * A context is externally synchronised (one thread at a time), as the reference's single render thread.
 * Caller-owned host memory is copied before the call returns (as createDeviceLocalBufferFromMemory does,
 * src/render.cpp:706-726).  All device work is queued on one HIP stream; bbr_end_frame does not block.
 * There is NO CPU fallback: without a HIP device every compute entry point fails with BBR_ERR_NO_DEVICE.
 */
#ifndef BIBIM_HIP_H
#define BIBIM_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct bbr_context bbr_context;

typedef enum bbr_status {
  BBR_OK = 0,
  BBR_ERR_INVALID_ARGUMENT = -1,
  BBR_ERR_NO_DEVICE = -2,
  BBR_ERR_HIP = -3,
  BBR_ERR_OUT_OF_MEMORY = -4,
  BBR_ERR_BAD_HANDLE = -5,
  BBR_ERR_NOT_IN_FRAME = -6,
  BBR_ERR_TOO_MANY_PRIMITIVES = -7,
  BBR_ERR_CAPACITY = -8
} bbr_status;

/* One RGBA8 image, stb_image STBI_rgb_alpha layout (src/resource.cpp:159-160).
 * rgba == NULL selects the `default` material's map for that slot (src/render.cpp:1328-1336). */
typedef struct bbr_image {
  const uint8_t *rgba;
  int32_t width;
  int32_t height;
} bbr_image;

/* PBRMapType order (src/render.h:235-243) */
enum { BBR_MAP_ALBEDO = 0, BBR_MAP_METALLIC, BBR_MAP_ROUGHNESS, BBR_MAP_AO, BBR_MAP_NORMAL, BBR_MAP_HEIGHT, BBR_MAP_COUNT };

/* Byte sizes the ABI accepts verbatim */
#define BBR_SIZEOF_VERTEX 44
#define BBR_SIZEOF_INSTANCE_BLOCK 128
#define BBR_SIZEOF_LIGHT 64
#define BBR_SIZEOF_FRAME_UNIFORM_BLOCK 6432
#define BBR_SIZEOF_VIEW_UNIFORM_BLOCK 144
#define BBR_MAX_NUM_LIGHTS 100

typedef struct bbr_stats {
  uint64_t n_prims;        /* triangles submitted this frame */
  uint64_t n_raster_tris;  /* (sub-)triangles that survived clip + cull + "covers a pixel centre" */
  uint64_t n_clipped_prims;
  uint64_t n_bin_refs;     /* (tile, triangle) pairs written to bins */
  uint64_t n_broad_tris;   /* triangles routed to the every-tile list */
  uint64_t n_shaded;       /* pixels of the owned rows whose winning fragment is geometry */
  uint32_t bin_overflow;   /* non-zero if a capacity was exceeded (frame is re-rendered transparently) */
  uint32_t tile_w, tile_h;
  uint32_t n_tiles;
} bbr_stats;

/* ---- lifetime ---- */
int bbr_create(int32_t width, int32_t height, int32_t device, bbr_context **out_ctx);
int bbr_destroy(bbr_context *ctx);
/* onWindowResize (src/main.cpp:1042-1061: vkDeviceWaitIdle, cleanupReloadableResources, initReloadableResources): waits
 * for the frames in flight, drops every buffer whose size follows the extent and continues with the new one.  Meshes,
 * materials, options, the partition and the grown capacities stay.  There is no current frame afterwards (read-backs
 * fail with BBR_ERR_NOT_IN_FRAME until one is rendered) and a caller-owned output buffer has to be set again.
 * Not allowed between bbr_begin_frame and bbr_end_frame.  Option "supersample" stays: BBR_ERR_INVALID_ARGUMENT, with the
 * context unchanged, when supersample x width or supersample x height exceeds 32768. */
int bbr_resize(bbr_context *ctx, int32_t width, int32_t height);
const char *bbr_last_error(const bbr_context *ctx); /* ctx may be NULL: last creation error */
int bbr_device_count(void);

/* ---- resources ---- */
int bbr_upload_mesh(bbr_context *ctx, const void *vertices, uint32_t n_vertices, const uint32_t *indices_or_null,
                    uint32_t n_indices, int32_t *out_mesh);
int bbr_upload_material(bbr_context *ctx, const bbr_image maps[BBR_MAP_COUNT], int32_t *out_material);
/* What bbr_upload_material does with the five shaded maps, on the host alone (no context, no device): whether they pack
 * (every supplied one of the same size; a supplied map of another size, 1 x 1 included, leaves the material unpacked), the
 * packed size, the bytes of the packed form and -- with out_or_null of at least that capacity -- the bytes themselves.
 * Not packable: *out_width = *out_height = 0, *out_bytes = 0. */
int bbr_pack_material(const bbr_image maps[BBR_MAP_COUNT], int32_t *out_packable, int32_t *out_width, int32_t *out_height,
                      uint64_t *out_bytes, uint8_t *out_or_null, uint64_t capacity);
int bbr_free_mesh(bbr_context *ctx, int32_t mesh);
int bbr_free_material(bbr_context *ctx, int32_t material);

/* ---- per-frame state ---- */
int bbr_set_frame_uniforms(bbr_context *ctx, const void *frame_uniform_block /* 6432 B */);
int bbr_set_view_uniforms(bbr_context *ctx, const void *view_uniform_block /* 144 B */);

/* ---- frame ---- */
int bbr_begin_frame(bbr_context *ctx);
int bbr_draw(bbr_context *ctx, int32_t mesh, int32_t material, const void *instance_blocks, uint32_t n_instances);
/* Capacities that depend on the scene (tile bins, every-tile list, clip arena) grow by themselves.  A synchronising
 * call (bbr_synchronize, bbr_get_stats, any read-back) that finds the last frame overflowed re-renders it with larger
 * buffers before returning.  A host that only streams frames is covered too: every frame stores its overflow bits
 * into pinned host memory (two words, from the raster kernel) and the next frame that reuses its slot grows the
 * capacities first -- the overflowed
 * frames themselves (at most frames_in_flight + 1 of them) are incomplete and stay so. */
int bbr_end_frame(bbr_context *ctx);   /* queues the kernels; asynchronous */
int bbr_replay_frame(bbr_context *ctx); /* re-submit the last recorded frame (same draws and uniforms) */
int bbr_synchronize(bbr_context *ctx);

/* ---- output ---- */
/* Full frame: height*width*4 floats, row-major, RGBA.  On a partitioned context (world > 1) this fails with
 * BBR_ERR_INVALID_ARGUMENT: the output is a compact shard, use bbr_read_shard. */
int bbr_read_framebuffer(bbr_context *ctx, float *rgba32f_host);
/* The fine frame of the last frame (option "supersample" = n): n*height * n*width * 4 floats, row-major -- the samples
 * k_resolve averaged.  Synchronises.  BBR_ERR_NOT_IN_FRAME before a frame, BBR_ERR_INVALID_ARGUMENT on a partitioned context.
 * With n = 1 it is bbr_read_framebuffer; with "present_fused" and n >= 2 it works (the fine frame exists). */
int bbr_read_samples(bbr_context *ctx, float *rgba32f_host);
/* With option "sample_shading" 0 (and n >= 2) bbr_read_samples returns g: every sample holds the value of its
 * representative (replicated on the host from the fine frame and the sample map).
 * bbr_read_sample_map: rep(s) of every fine pixel of the last frame, n*width * n*height bytes, row-major over the fine frame,
 * each an index 0 .. n^2 - 1 into the sample's block (k = j * n + i).  The identity (each sample its own index) with
 * "sample_shading" 1 or n = 1.  Synchronises.  BBR_ERR_NOT_IN_FRAME before a frame, BBR_ERR_INVALID_ARGUMENT on a
 * partitioned context. */
int bbr_read_sample_map(bbr_context *ctx, uint8_t *out);
int bbr_framebuffer_device_ptr(bbr_context *ctx, void **out_device_ptr, uint64_t *out_bytes);
/* Render into caller-provided device memory instead (e.g. a torch tensor that RCCL all-gathers);
 * NULL restores the internal buffer.  bytes must cover the frame (or the shard when partitioned). */
int bbr_set_output_device_ptr(bbr_context *ctx, void *device_ptr, uint64_t bytes);
/* By default a context owns four HIP streams and keeps two frames in flight, like the reference (numFrames,
 * src/main.cpp:38): every frame slot has its own buffers, counter block and stream ("stream_layout" 2, the default: all
 * kernels of a frame on the stream of its slot, so whole frames overlap and nothing inside a frame needs an event); the
 * host blocks in bbr_end_frame only when the slot it wants to reuse is still on the GPU (bbr_host_timing counts that).
 * Options "frames_in_flight" 1..4 and "stream_layout" change this.  bbr_read_framebuffer / bbr_framebuffer_device_ptr refer
 * to the most recently submitted frame.
 * bbr_set_stream(stream != NULL) puts ALL of the context's work on the caller's stream instead (one frame in flight,
 * plain stream ordering with the caller's other work); NULL returns to the context's own streams. */
int bbr_set_stream(bbr_context *ctx, void *hip_stream);
/* Cross-stream hand-offs for callers that pipeline frames against their own streams (e.g. an RCCL all-gather of
 * frame N overlapping the rendering of frame N+1):
 *   bbr_wait_event        device work submitted after this call waits for `hip_event` (a hipEvent_t the caller recorded,
 *                         e.g. "the consumer of the output buffer has finished with it");
 *   bbr_stream_wait_frame `hip_stream` (a hipStream_t) waits until the most recently submitted frame is complete. */
int bbr_wait_event(bbr_context *ctx, void *hip_event);
int bbr_stream_wait_frame(bbr_context *ctx, void *hip_stream);

/* ---- screen-band partition across GPUs (no reference counterpart) ---- */
/* Band b (band_rows framebuffer rows, a multiple of the tile height) belongs to rank b % world.  The
 * rank's output becomes a compact shard [local band][row in band][x][rgba]; every rank's shard is padded
 * to bbr_shard_rows() rows so that an all-gather of equal-sized shards reassembles the frame. */
int bbr_set_partition(bbr_context *ctx, int32_t rank, int32_t world, int32_t band_rows);
int bbr_shard_rows(const bbr_context *ctx, int32_t *out_rows);
int bbr_read_shard(bbr_context *ctx, float *rgba32f_host); /* shard_rows*width*4 floats */
/* Device-side un-interleave of an all-gathered buffer [world][shard_rows][width][4] into a row-major frame, queued on
 * `hip_stream` (NULL = the context's shading stream).  = bbr_unpack_whole(BBR_SHARD_RGBA32F) into the caller's frame; like
 * its _packed and _rgba8 siblings it needs no rendered frame and leaves bbr_read_whole_frame's state alone. */
int bbr_unpack_gathered(bbr_context *ctx, const void *gathered_device, void *frame_device, void *hip_stream);
/* The same exchange with a quarter less payload, lossless: alpha is 1.0 on shaded pixels and 0.0 on cleared ones
 * (forward_brdf.frag:75, clear colour src/main.cpp:84; the deferred path writes 1 everywhere), so a shard travels as
 * rgb[n][3] float + one bit per pixel, n = shard_rows * width: bbr_packed_shard_bytes() bytes per rank.
 *   bbr_pack_shard              the last frame's shard -> `packed_device`, queued on `hip_stream` (NULL = the stream the
 *                               frame was shaded on; a caller's stream must already wait for the frame, bbr_stream_wait_frame)
 *   bbr_unpack_gathered_packed  [world] packed blocks -> the row-major RGBA32F frame, bit for bit what bbr_unpack_gathered
 *                               makes of the RGBA32F shards */
int bbr_packed_shard_bytes(const bbr_context *ctx, uint64_t *out_bytes);                 /* = bbr_exchange_block_bytes(BBR_SHARD_PACKED) */
int bbr_pack_shard(bbr_context *ctx, void *packed_device, void *hip_stream);             /* = bbr_stage_shard(BBR_SHARD_PACKED) */
int bbr_unpack_gathered_packed(bbr_context *ctx, const void *gathered_device, void *frame_device, void *hip_stream); /* BBR_SHARD_PACKED */
int bbr_tile_height(const bbr_context *ctx, int32_t *out_tile_h);

/* ---- diagnostics ---- */
/* (with option "supersample" = n >= 2 the counts are those of the render extent: n_shaded counts fine samples, n_tiles,
 *  n_bin_refs and n_broad_tris fine tiles and their references; with option "sample_shading" 0 n_shaded counts the
 *  representatives, i.e. the fragments that were shaded) */
int bbr_get_stats(bbr_context *ctx, bbr_stats *out);                            /* synchronises (and re-renders an overflowed frame) */
/* How often a capacity (bins, every-tile list, clip arena) has been grown since bbr_create (= bbr_stats.bin_overflow), without
 * synchronising or touching the GPU: a host that times frames can tell afterwards whether one of them overflowed. */
int bbr_capacity_growths(const bbr_context *ctx, uint32_t *out_count);          /* host-side counter: does NOT synchronise */
/* Option "static_records" since bbr_create, without synchronising or touching the GPU: how often the camera-independent part
 * of a draw's records was written (one k_record_static launch per draw and frame slot), and how many draws were submitted
 * on the geometry kernel's light path.  Either pointer may be NULL. */
int bbr_static_record_counts(const bbr_context *ctx, uint64_t *out_fills, uint64_t *out_light_draws);
/* Option "sky_keep", the most recently submitted frame: one byte per tile, row-major over the tile grid (*out_count tiles;
 * `out` may be NULL to ask for the count, else `cap` must cover it).  BBR_SKY_TILE_FILLED: a background tile whose pixels
 * this frame stored; BBR_SKY_TILE_KEPT: a background tile whose pixels the frame found in place and did not store;
 * BBR_SKY_TILE_NONE: every other tile, and every tile of a frame that could not keep (see the option).  Synchronises; a frame
 * that is rendered again here after a capacity growth reports the second rendering. */
enum { BBR_SKY_TILE_NONE = 0, BBR_SKY_TILE_FILLED = 1, BBR_SKY_TILE_KEPT = 2 };
int bbr_read_sky_tiles(bbr_context *ctx, uint8_t *out, uint32_t cap, uint32_t *out_count);
/* Option "view_keep" since bbr_create, without synchronising or touching the GPU: main frames submitted that were kept (their
 * visibility was in the frame slot: shading only) and main frames rendered in full (re-renders included).  Either pointer
 * may be NULL. */
int bbr_view_keep_counts(const bbr_context *ctx, uint64_t *out_kept, uint64_t *out_full);
/* Option "surface_keep" since bbr_create, without synchronising or touching the GPU: storing frames (k_surface_store ran), and
 * frames shaded from a slot's kept surface (k_shade_lit; the storing frames are among them).  Every such frame is a kept frame
 * of bbr_view_keep_counts.  Either pointer may be NULL. */
int bbr_surface_keep_counts(const bbr_context *ctx, uint64_t *out_stored, uint64_t *out_lit);
/* For tests: the kept surface of frame slot `slot` (0 .. frames in flight - 1) and its item count.  Fragment slot e = item * 64 +
 * lane, e < 64 * *out_items, gets out_values[12 e ..] = P.xyz, the shading normal, albedo.rgb, metallic, roughness, ao (what
 * bbr_read_surface reports as floats 6..17 of the pixel's record) and out_index[e] = the pixel's index y * width + x, or
 * 0xFFFFFFFF for a lane without a fragment.  `capacity`: the fragment slots both arrays have room for; both may be NULL to ask
 * for the count.  Synchronises; renders nothing and forgets nothing.  BBR_ERR_NOT_IN_FRAME if the slot holds no valid surface. */
int bbr_read_surface_keep(bbr_context *ctx, int32_t slot, float *out_values, uint32_t *out_index, uint64_t capacity, uint32_t *out_items);
/* The host's side of the frame loop since bbr_host_timing_reset, kept without touching the GPU (steady_clock around the
 * submit): frames submitted by bbr_end_frame / bbr_replay_frame, nanoseconds spent inside those calls, and the part of
 * it the host was BLOCKED because the frame slot it wanted to reuse was still on the GPU (and in how many frames).  A
 * host that is never blocked is the bottleneck itself; one that is blocked every frame is waiting for the GPU.  This is
 * the frame loop the reference paces with a fence per frame in flight (src/main.cpp:1277-1279). */
int bbr_host_timing(const bbr_context *ctx, uint64_t *out_frames, uint64_t *out_submit_ns, uint64_t *out_blocked_ns,
                    uint64_t *out_blocked_frames);
int bbr_host_timing_reset(bbr_context *ctx);
/* What the library itself holds alive in this process, over all contexts, without touching the GPU: out[0] device allocations
 * and out[1] their bytes, out[2] pinned host blocks, out[3] events, out[4] streams.  Memory the caller owns (bbr_device_alloc,
 * the IPC calls) and the RCCL communicator are not counted.  Every count returns to its earlier value when a context is
 * destroyed: a host, or a test, can tell from it that nothing leaked. */
int bbr_debug_live_resources(uint64_t out[5]);
/* winning primitive (global API-order index, 0xFFFFFFFF = none) and depth per pixel; synchronises.
 * Re-runs the frame once with the visibility dump enabled. */
int bbr_read_visibility(bbr_context *ctx, uint32_t *prim_host, float *depth_host);
/* With option "supersample" = n >= 2 and a rule in option "depth_resolve", bbr_read_visibility returns the RESOLVED winner and
 * depth, width x height (the option's rule; the dump path of k_resolve_depth).  Its siblings:
 *   bbr_read_sample_visibility  the winners and depths of the render extent, n*height * n*width values each, row-major -- the
 *                               samples the rule chooses from, whatever the option's value; in the family of bbr_read_samples.
 *                               With n = 1 it is bbr_read_visibility.  Re-runs the frame once, synchronises.
 *   bbr_read_depth              the depth the last frame KEPT for the overlay pass (option "overlays"), width x height: with
 *                               n = 1 the bits of bbr_read_visibility's depth, with n >= 2 what k_resolve_depth wrote behind
 *                               k_raster.  Nothing is rendered again.  INVALID_ARGUMENT when the frame was rendered without
 *                               "overlays", or with n >= 2 and "depth_resolve" 0.
 * Both: BBR_ERR_NOT_IN_FRAME before a frame, BBR_ERR_INVALID_ARGUMENT on a partitioned context. */
int bbr_read_sample_visibility(bbr_context *ctx, uint32_t *prim_host, float *depth_host);
int bbr_read_depth(bbr_context *ctx, float *depth_host);
/* device time of the last bbr_end_frame/bbr_replay_frame in ms, and of its dominant kernel (k_shade); synchronises */
int bbr_last_frame_time_ms(bbr_context *ctx, float *out_frame_ms, float *out_shade_kernel_ms);
/* With option "timing" = 1 every frame records HIP events on the context's stream (frame start, geometry kernel
 * done, raster kernel done, shade kernel done) into a ring of 512 frames.  bbr_timing_summary averages the frames
 * recorded since bbr_timing_reset: whole frame, geometry (incl. the H2D of instances/lights), raster, shade.
 * With option "supersample" >= 2 the frame interval (here and in bbr_last_frame_time_ms) ends behind the frame's k_resolve;
 * the shade interval does not include it (bbr_resolve_timing has the kernel's own). */
int bbr_timing_reset(bbr_context *ctx);
int bbr_timing_summary(bbr_context *ctx, uint32_t *out_frames, float *out_avg_frame_ms, float *out_avg_geometry_ms,
                       float *out_avg_raster_ms, float *out_avg_shade_ms);
/* Options (all but "render_pass" drain the context first):
 *   "timing" 0|1|2           1: five HIP events per frame (frame start, geometry, raster, shade start, shade done);
 *                            2: only the two around k_shade (frame/geometry/raster averages read 0); restarts the ring
 *   "timing_stride" n        with "timing" on, only every n-th frame carries events (default 1): the events themselves
 *                            perturb a pipelined frame stream (two per frame: ~4 % of the C3 frame rate)
 *   "frames_in_flight" 1..4  default 2 (the reference's numFrames); bench.py runs 4K with 3 and 1080p with 4
 *   "tile_mode" 0|1          1 (default): 32x32 screen tiles; 0: 64x64 tiles -- kept for frames beyond 8192 x 8192 pixels
 *                            (65 536 tile slots), slower everywhere else (k_raster 120 vs 65 us at 4K, round 1)
 *   "bin_cap" n              initial references per (tile, raster class); grows by itself on overflow
 *   "broad_threshold" n      triangles touching more than n tiles go to the every-tile list
 *   "broad_cap" n            initial entries of the every-tile list (default 4096); doubles when a frame overflows it
 *   "clip_cap" n             initial sub-triangle slots of the clip arena (default 4096); doubles likewise
 *   "gbuffer_view" -1..3      deferred path only: instead of brdf.frag, buffer_visualize.frag shows the rgb of one G-buffer
 *                            attachment (GBufferVisualizingOption, src/scene.h:27-35; recordCommand src/main.cpp:96-121):
 *                            0 position, 1 normal, 2 albedo, 3 metallic / roughness / ao; -1 (default) the lit scene.
 *                            The frame then goes through presentation like any other
 *   "render_pass" 0|1        0: forward path (default, the path BASELINE measures), 1: deferred path
 *   "max_anisotropy" 1..16   texture filtering of the fragment stages (src/render.cpp:1349-1350: the reference's sampler has
 *                            anisotropyEnable, maxAnisotropy = 16).  1 (default): one bilinear tap at LOD 0, the kernels and
 *                            pixels of every earlier release.  2..16: up to that many bilinear taps along the long axis of
 *                            the pixel's footprint, averaged (the Vulkan specification's example scheme; the rule is
 *                            spelled out in DESIGN.md section 3 and under "surface read-back" below).  The TBN overlay's
 *                            vertex-stage fetch has no derivatives and stays one tap.  Anything else: INVALID_ARGUMENT
 *   "mip_levels" 1..15       mip chains and the trilinear half of the reference's sampler (src/render.cpp:1363-1365:
 *                            mipmapMode LINEAR, which the reference pins to its images' single level).  1 (default): no
 *                            chain exists; the kernels, statements and pixels of "max_anisotropy" alone.  n >= 2: a map of
 *                            w x h texels gets L = min(n, 1 + floor(log2 max(w, h))) levels, level k of max(1, w >> k) x
 *                            max(1, h >> k) texels (15: the full chain of a 16384 map), built on the GPU -- of every live
 *                            material when the option goes above 1, by bbr_upload_material while it is, freed by
 *                            bbr_free_material and when it returns to 1.  The extra memory is a third of the maps' own
 *                            bytes, plus what placement adds: every level starts on a multiple of 256 bytes (a 2 x 2 map
 *                            of 16 bytes gets a 256-byte level), and a packed level's 4 x 4 blocks round its extents up
 *                            (a 16384 x 3 set: half again, not a third).  Frames are then
 *                            shaded by k_shade_mip, whatever "max_anisotropy" is (the rule: "mip chains" below).  The TBN
 *                            overlay's vertex-stage fetch and the GUI sampler have no derivatives and stay on level 0.
 *                            Anything else: INVALID_ARGUMENT.  Refused (INVALID_ARGUMENT) at >= 2 while "shadow_map" > 0
 *   "shadow_map" 0..8192     shadow mapping, up to eight casters per context ("shadow mapping" below).  0 (default): off -- no kernel
 *                            of the option runs, no buffer of it exists.  S >= 1: the side of a square binary32 depth map
 *                            that bbr_render_shadow_map renders; until it has, frames are rendered by the unshadowed
 *                            kernels exactly as with 0, afterwards by k_shade_shadow.  Changing the value drains the
 *                            context and drops the map and its pass buffers.  Anything else: INVALID_ARGUMENT, the option
 *                            unchanged.  Refused (INVALID_ARGUMENT) at > 0 while "mip_levels" >= 2, in whichever order the
 *                            two are set: k_shade_shadow has no trilinear form
 *   "shadow_filter" 0..2     percentage-closer filtering of the shadow test ("shadow mapping" below, "Filtering").  0
 *                            (default): the hard compare -- the kernels, launches and bits of "shadow_map" alone.  R >= 1: a
 *                            (2R+1) x (2R+1) box of compares, 9 or 25 taps; frames under a map are shaded by
 *                            k_shade_shadow_pcf, whatever the number of faces.  Stored at any "shadow_map" (in effect once a
 *                            map exists); setting it drains the context, leaves no current frame and keeps the map.
 *                            Anything else: INVALID_ARGUMENT, the option unchanged.  "mip_levels" >= 2 stays refused
 *   "supersample" 1..4       n x n supersampling: rasterizationSamples = n^2 on a regular grid, sampleShadingEnable with
 *                            minSampleShading = 1 and VK_RESOLVE_MODE_AVERAGE (the reference pins 1 sample,
 *                            src/render.cpp:1104-1112).  1 (default): nothing changes, no kernel of the option runs.
 *                            n >= 2: a context of W x H renders the FINE frame of nW x nH -- by definition what the same
 *                            calls produce on a context created as nW x nH with "supersample" 1 (same uniforms, draws and
 *                            options, the same 1/256 snap of the fine pixel grid, texture differences per fine pixel) --
 *                            and k_resolve writes the W x H output.  Output pixel (x, y), all four channels, in binary32
 *                            without contraction:
 *                              acc = f(nx, ny)
 *                              for j in 0..n-1, i in 0..n-1, (i, j) != (0, 0), row-major (i fastest): acc = acc + f(nx+i, ny+j)
 *                              out = acc * R[n]    R[2] = 0.25f, R[3] = the binary32 nearest 1/9, R[4] = 0.0625f
 *                            Alpha is averaged like the colours (forward: the covered fraction; deferred: 1); NaN and inf go
 *                            through the additions as they are.  The resolve happens in linear HDR: bbr_present,
 *                            bbr_tone_map, the exchange forms and bbr_draw_ui act on the resolved W x H values.  width /
 *                            height everywhere else in this header stay the OUTPUT extent (outputs, shards, presented
 *                            images, caller buffers); tiles, bins, the "tile_mode" limit of 65 536 tile slots and
 *                            bbr_get_stats follow the render extent.  The fine frame is always library-owned.
 *                            Setting it acts like a resize of the render extent: extent-sized buffers are dropped and
 *                            there is no current frame afterwards; a caller's output buffer stays (the output size did
 *                            not change).  INVALID_ARGUMENT, context unchanged, outside 1..4 or when n x width or
 *                            n x height exceeds 32768.
 *                            With "present_fused" and n >= 2 the fine frame is rendered by the fp32 kernels and k_resolve
 *                            writes the presented RGBA8 image directly (binary16 stage included: the bytes of the unfused
 *                            route with hdr16 = 1); there is no W x H fp32 frame and no k_present pass.
 *                            Partition: bbr_set_partition keeps its meaning in OUTPUT rows (bands are n x band_rows fine
 *                            rows); a rank's resolved shard is the shard of the resolved whole frame.  BBR_SHARD_PACKED
 *                            keeps one alpha bit per pixel and is refused with n >= 2: bbr_stage_shard, bbr_pack_shard,
 *                            bbr_allgather_frame and bbr_push_shard return INVALID_ARGUMENT for it and launch nothing.
 *                            Also refused with n >= 2 (INVALID_ARGUMENT): bbr_draw_overlays, TBN included, and
 *                            bbr_read_visibility (both need a depth resolve rule: while option "depth_resolve" is 0),
 *                            bbr_read_gbuffer, bbr_read_surface and bbr_read_records (their buffers have the output
 *                            extent), whatever "depth_resolve" is
 *   "depth_resolve" 0|1|4|8  with "supersample" n >= 2: which sample of an output pixel's block gives the pixel its depth and
 *                            its winning primitive.  The values are VkResolveModeFlagBits (pass (int)depthResolveMode):
 *                              0  NONE         default: no depth is kept while n >= 2, and bbr_draw_overlays, bbr_read_visibility
 *                                              and bbr_read_depth are refused as above
 *                              1  SAMPLE_ZERO  k* = 0
 *                              4  MIN          k* = the first k, in index order, whose depth bit pattern is smallest
 *                              8  MAX          k* = the first k, in index order, whose depth bit pattern is largest
 *                            The block of output pixel (x, y) is the fine pixels (nx + i, ny + j) and k = j * n + i, as in
 *                            the colour resolve; bit patterns are compared as unsigned 32-bit integers.  The resolved depth
 *                            is the bit pattern of sample k*, the resolved primitive the winner of sample k* (0xFFFFFFFF
 *                            where that sample is uncovered).  Stored depths lie in [0, 1] and an uncovered sample holds
 *                            the cleared 0.0, so the order of the bit patterns is the order of the values, and it is the
 *                            comparison the rasteriser's keys make.  Depth is reverse-Z (the larger value wins): MAX is
 *                            the nearest sample, MIN the farthest, and one uncovered sample makes MIN return 0.  With
 *                            "sample_shading" 0 the samples keep their own depth: the rule is the same.
 *                            k_resolve_depth runs behind k_raster in every frame that keeps its depth ("overlays" 1), and in
 *                            bbr_read_visibility's re-render.  bbr_draw_overlays then draws the markers, the gizmo and the
 *                            TBN lines one sample per OUTPUT pixel into the presented width x height image, depth-tested
 *                            against the resolved depth.  Deviation: a multisampled Vulkan pass would rasterise them at n^2
 *                            samples and resolve their colour with the scene's.
 *                            2 (AVERAGE: an averaged depth has no winner) and every other value: INVALID_ARGUMENT.  The
 *                            value is stored at any "supersample"; at n = 1 it changes nothing and no kernel of it runs.
 *                            Setting a new value while n >= 2 leaves no current frame; the fine depth is dropped.  A
 *                            partition refuses all of these calls as before
 *   "sample_shading" 0|1     with "supersample" n >= 2: 1 (default) shades every sample (sampleShadingEnable = VK_TRUE, the
 *                            rule above, bit for bit; no kernel of this option runs).  0 is multisampling
 *                            (sampleShadingEnable = VK_FALSE): one fragment is shaded per primitive and output pixel.
 *                            The block of output pixel (x, y) is the fine pixels (nx + i, ny + j), indexed k = j * n + i;
 *                            P(s) is the primitive that wins fine pixel s (the sub-triangles of a clipped primitive are one
 *                            primitive):
 *                              rep(s) = the first s' of s's block, in index order, with P(s') == P(s)   (covered s)
 *                              rep(s) = s                                                               (uncovered s)
 *                              g(s)   = f(rep(s))                                                       all four channels
 *                              out    = the resolve rule of "supersample" applied to g
 *                            Only the samples with rep(s) == s, the representatives, are shaded, each as the fine pixel it
 *                            is (its own planes, clip slot and per-fine-pixel texture differences): its value is the fine
 *                            frame's, bit for bit.  A representative is a covered sample; nothing is extrapolated outside
 *                            its primitive.  An interior pixel returns its representative's bits at n = 2 and comes back
 *                            within the rounding of the sixteen additions at n = 4; forward alpha stays the covered
 *                            fraction.  Deviations from Vulkan multisampling: the shading position is sample 0's of the
 *                            primitive in the pixel, not the pixel centre, and the texture footprint stays the fine
 *                            pixel's (not differences over n fine pixels).  k_sample_merge thins the fragment lists behind
 *                            k_raster (the frame always takes the k_shade_items route, whatever "no_tail_items" says) and
 *                            k_resolve_merged replaces k_resolve, also under "present_fused".  bbr_get_stats' n_shaded is
 *                            then the number of representatives.  With "timing" the merge falls into the raster interval.
 *                            The value is stored at any "supersample" and takes effect with n >= 2.  "supersample" 3 with
 *                            "sample_shading" 0 is refused (a 3 x 3 block straddles the tiles): whichever call would
 *                            complete the pair returns INVALID_ARGUMENT and leaves the context unchanged.  Values other
 *                            than 0 and 1: INVALID_ARGUMENT.  Setting it leaves no current frame; only the sample maps
 *                            are dropped.  Everything "supersample" >= 2 refuses stays refused
 *   "present_fused" 0|1      frames are produced as presented RGBA8 pixels directly (binary16 stage, tone map and sRGB
 *                            encode fused into the raster / shade kernels): no fp32 frame, no k_present pass; bbr_present
 *                            then only marks (or copies to a caller buffer), bbr_read_framebuffer / bbr_read_shard fail
 *   "overlays" 0|1           keep every frame's resolved depth for bbr_draw_overlays (default 0; with "supersample" >= 2 only
 *                            under a rule of "depth_resolve": with its value 0 nothing is kept and bbr_draw_overlays is refused)
 *   "tbn" 0|1                bbr_draw_overlays first draws the TBN lines of the last frame (default 0; see below)
 *   "stream_layout" 0|1|2    how the kernels of the frames in flight are spread over HIP streams.  Same pixels in every
 *                            layout.  0: geometry + raster on one stream, shade on a second, present on a third.
 *                            1: as 0 with k_raster on a stream of its own (the geometry of frame N+1 overlaps the
 *                            raster of frame N).  2 (default): every kernel of a frame on the stream of its frame slot
 *                            (frames share nothing, whole frames overlap).  Three frames in flight, us per frame for
 *                            0 / 1 / 2: 1080p, one ShaderBall 84.5 / 67.1 / 37.3; 4K, sixteen 191.5 / 153.6 / 148.6.
 *   "push_mode" 0|1          bbr_push_shard: 1 (default) one kernel storing to every peer at once, 0 peer copies one after
 *                            the other (see "native exchange" below)
 *   "no_tail_items" n        (default 40000) what counts as a SHORT frame: at most n item slots (tiles x 64-fragment chunks
 *                            per tile: 1080p has 32 640).  A long frame's shading work list is built by a scan kernel
 *                            (k_shade_items, screen order), its main launch is sized from the item count the frame slot
 *                            produced one frame earlier and a small tail launch covers what that estimate misses.  A
 *                            short frame is a chain of dependent kernels whose length is its rate: its raster tiles append
 *                            their items themselves (no k_shade_items launch) and it is shaded at full coverage without
 *                            the tail launch (C2: chain 95 -> 85 us, 27.3 -> 24.6 us per frame with four in flight)
 *   "heavy_tiles" n          long frames: the raster kernel starts the tiles one of whose bins holds at least n triangle
 *                            references before the screen-ordered rest.  Same pixels.  0: plain screen order; -1 (default):
 *                            64 while one frame is in flight, 0 otherwise -- it shortens a single frame (C3: k_raster alone
 *                            61.9 -> 51.0 us, frame latency 177 -> 167 us) and costs 1-2 % of the pipelined frame rate
 *   "static_records" 0|1     1 (default): 184 of the 224 bytes of a primitive's record -- texture coordinates, material binding,
 *                            world-space position, normal, tangent, bitangent -- do not depend on the camera.  A draw whose
 *                            mesh, material binding, place in the frame and instance blocks (compared byte for byte) are
 *                            those of the frame that used the same frame slot before has them written once per slot, for
 *                            every primitive (k_record_static); from then on the geometry kernel stores only the 40 bytes
 *                            that follow the camera.  Same records, same pixels.  A draw whose instances change pays the
 *                            comparison and is processed as with 0; it comes back one frame after its key has repeated.
 *                            Uploading or freeing a mesh or a material, a change of "mip_levels", bbr_read_records and a
 *                            growth of the record buffer make every draw start over.  0: every frame writes whole records.
 *                            The overlay pass and the shadow-map pass always write whole records.
 *   "sky_keep" 0|1           1 (default): a 32 x 32 (64 x 64) tile that no triangle touches gets the clear colour in every pixel,
 *                            and the frame goes into the frame slot's own buffer -- so a tile that was background when the
 *                            slot rendered last, and is background again, already holds those bytes and is not stored
 *                            again (C3: 61.9 of the 86.4 MB the raster kernel writes per frame).  Same pixels.  The library
 *                            keeps one word per tile and slot; a tile that turns background is filled once and kept from the
 *                            slot's next frame on.  Only forward frames of the whole image with one sample per pixel into the
 *                            library's fp32 frame keep: not "render_pass" 1, "present_fused", "supersample" >= 2,
 *                            "overlays", a partition or a caller's output buffer.  Every slot starts over (one frame that
 *                            fills every background tile) after bbr_tone_map, bbr_draw_overlays, bbr_draw_ui, bbr_resize,
 *                            bbr_set_partition, bbr_set_output_device_ptr, bbr_framebuffer_device_ptr, the bbr_unpack_*
 *                            calls, any bbr_set_option that waits for the GPU, and a read-back that renders the frame again
 *                            (visibility, G-buffer, surface, shadow mask).  The pointer of bbr_framebuffer_device_ptr is
 *                            good for what the call has always promised, the most recently submitted frame: a caller who
 *                            writes through it later, behind frames the library has rendered since, must set 0.
 *                            0: every frame stores every background pixel.  bbr_read_sky_tiles says what happened.
 *   "view_keep" 0|1          1 (default): what the geometry and raster kernels produce -- triangles, records, bins, fragment
 *                            lists, the shading work list, the background pixels -- depends on the view, the draws and the
 *                            frame's geometry parameters only, not on lights, tone mapping, the normal-map switch, the
 *                            filtering options or a shadow map.  A frame whose view matrices, draws (as "static_records"
 *                            compares them: every draw on the light path, nothing to fill), capacities, parameters and
 *                            buffers are those its frame slot rendered last finds all of that in the slot and launches
 *                            its staging copy and its shading only (and a one-workgroup kernel for the light table when
 *                            the lights changed).  Shading itself is never kept.  Same pixels, same read-backs, same
 *                            bbr_get_stats.  Kept from the slot's third frame of a kind on; the conditions of "sky_keep" apply,
 *                            and so does its list of calls that make every slot start over -- except that of the options only
 *                            those that can change the parameters, the mode or a buffer do (not "max_anisotropy",
 *                            "mip_levels", "shadow_map", "shadow_filter", "timing", "static_records", "sky_keep").  Not kept:
 *                            a frame under "timing" 1 (every stage is timed), "static_records" 0, a frame that carries a
 *                            queued shadow caster or follows one, a frame behind a capacity growth or an overflowed frame.
 *                            bbr_read_sky_tiles reports a kept frame's background tiles as kept.  0: every frame runs every
 *                            stage.  bbr_view_keep_counts counts both kinds.
 *   "surface_keep" 0|n       n (default 64): under a kept view the part of shading in front of the light loop -- barycentrics,
 *                            varyings, texel taps, the filter, the TBN product -- does not change either: it depends on the
 *                            slot's visibility, the draws, the materials and the normal-map switch, not on lights, exposure
 *                            or tone mapping.  A slot's n-th kept frame in a row that takes the plain shading kernel on the
 *                            long route (no shadow map, "mip_levels" 1, "max_anisotropy" 1, "timing" 0 or 2, more item slots
 *                            than "no_tail_items") stores that surface (k_surface_store: 52 bytes per fragment slot, allocated
 *                            then); it and every such frame behind it run the light loop alone on it (k_shade_lit).  Same
 *                            pixels, same read-backs, same bbr_get_stats, same bbr_view_keep_counts.  A full frame, a kept frame
 *                            that cannot be lit, a change of the normal-map switch and whatever makes the slots forget their
 *                            visibility start the run again; setting the option itself forgets the surfaces only.  0: off,
 *                            nothing is allocated.  n follows from what a storing frame costs: DESIGN.md section 5.
 *                            bbr_surface_keep_counts counts storing and lit frames.
 *   "bloom" 0..8             0 (default): bbr_present launches k_present; no kernel or buffer of the option exists.  L = 1..8:
 *                            a bloom pyramid of L levels in front of k_present_bloom (the rule and the calls: "bloom" below).
 *                            Setting it waits for the GPU like "max_anisotropy": the slots keep their visibility, the last
 *                            frame stays current, an image already presented is not redone.  Refused with a partition of
 *                            world > 1 and with "present_fused" non-zero, in either order.
 *   "auto_exposure" 0|1      0 (default): presentation uses the frame's own Exposure; no kernel or buffer of the option exists.
 *                            1: bbr_present meters the frame on the device and converts it with the exposure that follows (the
 *                            rule and the calls: "auto exposure" below).  Setting it waits for the GPU like "bloom": the slots
 *                            keep their visibility and their kept surfaces, the last frame stays current, an image already
 *                            presented is not redone.  Setting 0 forgets the histories and frees the buffers.  Refused with a
 *                            partition of world > 1 and with "present_fused" non-zero, in either order.
 *   "ablate" bits          diagnostic builds only (make EXTRA=-DBB_ABLATE): skip parts of the pipeline */
int bbr_set_option(bbr_context *ctx, const char *name, int64_t value);
/* The stream layout in use (option "stream_layout"; 0 while only one frame is in flight).  *out_decided is always 1 and
 * out_ms[3] all zero: the layout is a plain option, nothing is timed at run time (round 1 did). */
int bbr_stream_layout_state(const bbr_context *ctx, int32_t *out_layout, int32_t *out_decided, float *out_ms);
/* Self-test of the arithmetic contract on this device: the shader's reciprocal (v_rcp_f32 + one Newton step) against
 * the IEEE division for +x and -x of every float with bit pattern in [lo_bits, hi_bits); 0 mismatches expected.
 * The whole positive range 0 .. 0x7FFFFFFF takes about half a second. */
int bbr_selftest_rcp(bbr_context *ctx, uint32_t lo_bits, uint32_t hi_bits, uint64_t *out_mismatches);

/* ---- deferred variant ----
 * bbr_set_option(ctx, "render_pass", 1) renders with the reference's deferred path, its default
 * (SceneBase::SceneRenderPassType, src/scene.h:77; recordCommand src/main.cpp:89-104): gbuffer.vert/.frag into four
 * R16G16B16A16_SFLOAT attachments (src/main.cpp:443), then brdf.frag on every pixel.  The two subpasses are fused
 * (the G-buffer texel of a pixel is only read by the same pixel), so the G-buffer is not stored unless asked for:
 * bbr_read_gbuffer re-renders the last frame and returns width*height*16 floats, per pixel
 * position.xyz 1 | normal.xyz 0 | albedo.rgb 0 | metallic roughness ao height (binary16 values widened); synchronises. */
int bbr_read_gbuffer(bbr_context *ctx, float *gbuffer_host);

/* ---- surface read-back ----
 * What the fragment stage saw and produced at every pixel, before lighting: a diagnostic in the family of
 * bbr_read_visibility / bbr_read_gbuffer.  Re-renders the last frame with a dumping instantiation of the shading kernel
 * and synchronises; BBR_ERR_NOT_IN_FRAME before a first frame and after bbr_resize, BBR_ERR_INVALID_ARGUMENT on a
 * partitioned context.  Both passes, any "max_anisotropy" (1 included).  `out` holds height*width*32 floats; an uncovered
 * pixel is 32 zeros, a covered one
 *   [0..1]   vUV                        [2..5]   dudx dvdx dudy dvdy
 *   [6..8]   vPosWorld                  [9..11]  the normal handed to the light loop, before its normalize (deferred:
 *                                                before the binary16 rounding)
 *   [12..14] albedo   [15] metallic   [16] roughness   [17] ao   [18] height (deferred only, else 0)
 *   [19..21] the normal-map sample s*2-1 (0 when EnableNormalMap is 0)
 *   [22..27] taps N used for each map, PBRMapType order (0: a map the pass did not sample)
 *   [28..31] 0 with "mip_levels" 1; otherwise the level choice (see "mip chains"): [28] d and [29] delta of the packed set, or
 *            of the albedo map of an unpacked material; [30] d and [31] delta of the height map (deferred pass, else 0)
 * all filtered values before any binary16 rounding.  The differences and N follow the filter rule of "max_anisotropy":
 *   dudx = u(x+1, y) - u(x, y), dudy = u(x, y+1) - u(x, y) (v likewise), u(X, Y) being the fragment's own planes
 *   evaluated at that pixel centre, whatever wins there; per map of w x h texels px2 = (dudx w)^2 + (dvdx h)^2, py2
 *   likewise, long axis x iff px2 > py2; N = 1 + #{n in 1..15: n^2 min < max}, capped by the option, 1 when max <= 1 (a
 *   footprint of at most one texel) or a difference is not finite; tap i of N >= 2 at uv + (i / (N + 1) - 1/2) * (the long
 *   axis' differences); the taps are summed in order and multiplied by 1 / N.  A packed material (five maps of one size)
 *   has one N, a material whose maps differ in size one per map. */
int bbr_read_surface(bbr_context *ctx, float *out);

/* ---- mip chains (option "mip_levels" >= 2) ----
 * The rule, in binary32, without contraction, in this operand order (tests/mip_reference.py):
 *   chain    level k + 1, per channel byte of all six maps: texel (x, y) = (s + 2) >> 2, s the integer sum of the four
 *            level-k bytes at columns min(2x, w_k - 1), min(2x + 1, w_k - 1) and the same two rows.  A defaulted (NULL)
 *            map is 1 x 1 and has one level.  A packed material's level k is what bbr_pack_material makes of the five
 *            level-k maps: the same 9-byte block-linear records, the same tail padding, per level.
 *   N        the footprint and tap count of "max_anisotropy" (1 included) on the map's LEVEL-0 size; mx its long axis
 *   level    P = mx * R2[N], R2[k] the binary32 nearest to 1 / k^2.  A difference not finite, or !(P > 1): d = 0, delta = 0.
 *            Otherwise, b the bits of P: e = (b >> 23) - 127, d = e >> 1, delta = 0.5f * ((float)(e & 1) + (float)(b &
 *            0x7FFFFF) * 2^-23), all exact.  d >= L - 1 (+inf included): d = L - 1, delta = 0 -- so a footprint that is
 *            huge but finite (a steep, nearly edge-on or degenerate primitive) samples the LAST level; only differences
 *            that are not finite, and footprints of at most a texel, stay on level 0.  This is lambda = 1/2 log2 P with
 *            log2(1 + t) taken as t: it reads low by at most 0.043 level (slightly sharp), a documented deviation
 *   value    hi = the taps and average of "max_anisotropy" on level d's size (tap offsets are in uv: the same on every
 *            level; wrapping and the 2^30 cutoff per level).  delta == 0: value = hi and nothing else happens -- a
 *            magnified pixel and a one-level map keep the bits of the "max_anisotropy" path.  Otherwise lo = the same on
 *            level d + 1 and value = fmaf(delta, lo - hi, hi) per channel; the normal sample is fmaf(value, 2, -1) as ever.
 *            A packed material has one (N, d, delta), a material with maps of different sizes one per map.
 * Chain read-back, in the family of the other diagnostics; both synchronise and return BBR_ERR_INVALID_ARGUMENT for a
 * level the chain does not have (with "mip_levels" 1 every map has level 0 alone), BBR_ERR_BAD_HANDLE for a material
 * that is not live, BBR_ERR_CAPACITY when `capacity` (bytes) is too small; `out` may be NULL to ask for the size:
 *   bbr_read_material_level  the row-major RGBA8 level of one of the six maps (PBRMapType order) and its size
 *   bbr_read_packed_level    the packed form of that level and its bytes; 0 bytes for an unpacked material */
int bbr_read_material_level(bbr_context *ctx, int32_t material, int32_t map, int32_t level, uint8_t *out_rgba8, uint64_t capacity,
                            int32_t *out_width, int32_t *out_height);
int bbr_read_packed_level(bbr_context *ctx, int32_t material, int32_t level, uint8_t *out, uint64_t capacity, uint64_t *out_bytes);

/* ---- shadow mapping (option "shadow_map" = S > 0) ----
 * Up to eight shadow-casting lights per context ("Casters" below; what follows states the rule for one, the caster of slot
 * 0): a depth map of the recorded draws from a view the caller supplies, and a depth test in front of that light's
 * iteration of the light loop.  The rule, in binary32, without contraction, in this operand order
 * (tests/shadow_reference.py):
 *   map      texel (i, j) is the depth the rasteriser keeps for pixel (i, j) of an S x S frame of the recorded draws under
 *            gl_Position = (L.proj * L.view) * posWorld -- the forward order, whatever "render_pass" is -- with the frame's
 *            own fixed-function state (clipper, back-face cull, 1/256 snap, top-left rule, GREATER_OR_EQUAL, depth clamp).
 *            An uncovered texel holds the clear value 0.  The map ignores the partition: every rank renders all of it.
 *   test     per fragment, on the position P the light loop receives (deferred: P rounded to binary16).  M = L.proj *
 *            L.view as the vertex stage evaluates it (column j = proj * view[j], an fma chain); c = M * (P, 1) in the same
 *            chain.  !(c.w > 0): OUTSIDE.  r = the correctly rounded 1 / c.w, h = 0.5f * S, xs = fmaf(c.x * r, h, h), ys =
 *            fmaf(c.y * r, h, h).  !(xs >= 0 && xs < S && ys >= 0 && ys < S): OUTSIDE (NaN lands here).  i = (int)xs, j =
 *            (int)ys, t = c.z * r + bias.  SHADOWED iff map[j][i] > t (a NaN t is not shadowed); otherwise LIT.
 *   classes  as bbr_read_shadow_mask reports them: 0 not covered, 1 LIT, 2 SHADOWED, 3 OUTSIDE (4 PARTIAL: "Filtering")
 *   loop     the iteration of light `light_index` of a SHADOWED fragment contributes nothing, like a light of unknown type;
 *            everything else is the light loop's.  A light_index >= NumLights shadows nothing.
 * Deviations: a hard compare unless option "shadow_filter" is set ("Filtering" below), one caster per light ("Casters"
 * below), and the deferred background colour is evaluated without the test.
 *
 * Faces.  The caster has an ordered list of F = 1 .. 6 frusta (bbr_render_shadow_faces; bbr_render_shadow_map is F = 1), each
 * with a map of its own, for ONE light_index and ONE bias:
 *   maps     map_f is the map above for L_f; every rank renders all of them
 *   test     for f = 0 .. F - 1 in this order: cls_f = the test above with M_f = L_f.proj * L_f.view and map_f.  The first
 *            cls_f != OUTSIDE is the fragment's class and f its face.  None: OUTSIDE, face 255
 * Six 90-degree-class frusta at a point light's position are a cube map (bb::cubeShadowViews / bbs_cube_shadow_views,
 * include/bibim_scene.h: +X, -X, +Y, -Y, +Z, -Z); two or three nested orthographic ones are cascades of a directional light.
 *   overlap  where frusta overlap, the earlier face wins; the later face's map is not read there
 *   seams    a fragment OUTSIDE every face is lit.  With faces of exactly 90 degrees that happens ON the seam planes (both
 *            neighbours reject a coordinate that lands on xs == S or ys == S): give a cube a few degrees over 90 (96 is what
 *            the tests use; the overlap rule then decides the doubly covered rim)
 *   memory   F * S * S * 4 bytes of maps; the pass's buffers are shared by the faces.  A later call with fewer faces keeps
 *            the larger buffer
 *
 * Filtering (option "shadow_filter" = R in 1 .. 2; tests/shadow_filter_reference.py).  K = (2R+1)^2 compares instead of one:
 *   face, texel, t   exactly the rules above: the deciding face f is the first face the fragment is not OUTSIDE of (with one
 *            face, that face); i, j and t = c.z * r + bias are taken on the P the light loop receives (deferred: after the
 *            binary16 rounding).  OUTSIDE and "not covered" are unchanged and decided before any tap is read
 *   taps     for dj = -R .. R and di = -R .. R, tap (di, dj) reads map_f[clamp(j + dj, 0, S - 1)][clamp(i + di, 0, S - 1)].
 *            A tap is lit iff !(texel > t) -- the hard rule's compare, so a NaN t makes every tap lit.  k is the number of
 *            lit taps, 0 .. K: an integer count, the tap order has no meaning.  Taps never leave the deciding face's map; on a
 *            cube they clamp at the face's edge
 *   classes  0, 1 LIT (k = K), 2 SHADOWED (k = 0) and 3 OUTSIDE as above; 4 PARTIAL (0 < k < K)
 *   loop     k = K: the caster's iteration is untouched.  k = 0: it contributes nothing.  0 < k < K: it runs with the caster's
 *            cooked colour replaced, per channel, by color[c] * (intensity * v), v = (float)k * RK, RK[9] and RK[25] the
 *            binary32 values nearest 1/9 and 1/25 (the device of R[3] in the resolve rule): the light loop with the caster's
 *            intensity replaced by the binary32 product intensity * v, everything else unchanged.  A light_index >=
 *            NumLights shadows and scales nothing
 *   hence    with S = 1 every tap is texel (0, 0), k is 0 or K and the frame is the hard rule's, bit for bit; the same holds
 *            wherever all K taps agree
 * Deviations: a box, not bilinear weights; one t for all taps (no receiver-plane bias); no fetch across cube faces; the
 * deferred background stays untested.
 *
 * Casters (bbr_render_shadow_caster; tests/shadow_casters_reference.py).  A context has kMaxShadowCasters = 8 caster SLOTS,
 * 0 .. 7.  A slot in use holds a light index, F = 1 .. 6 view blocks, their F maps of S x S and a bias; S ("shadow_map") and R
 * ("shadow_filter") stay context-wide.  The caster of bbr_render_shadow_map / bbr_render_shadow_faces is slot 0.
 *   maps     slot s, face f: exactly the map rule above for that view block.  Every rank renders all of them
 *   test     for every slot in use, independently of the others: (class_s, face_s, k_s) is the rule above evaluated with that
 *            slot's matrices, maps and bias.  R = 0: the first face not OUTSIDE and the hard compare, K = 1 and k is 0 or 1.
 *            R >= 1: the box of K = 9 or 25 compares clamped inside the deciding face.  It runs on the P the light loop
 *            receives (deferred: after the binary16 rounding); no operation of it changes.  Slots do not see each other
 *   loop     iteration li looks for the slot in use whose light index is li; there is at most one.  No such slot, or class
 *            OUTSIDE, or k = K: the iteration is untouched.  k = 0: it contributes nothing, the `continue` of an unknown type.
 *            0 < k < K: it runs with the cooked colour color[c] * (intensity * ((float)k * RK)), RK as above.  The lights'
 *            order, every other operation and the accumulation order are the light loop's.  A slot whose light index is >=
 *            NumLights changes nothing
 *   hence    a frame with one slot in use, whichever slot it is, is bit for bit the frame of that caster in slot 0; which slot
 *            a caster sits in has no meaning: permuting the casters over the slots changes no bit; a caster at bias 2
 *            (nothing shadowed), or on a light beyond the frame's lights, leaves the frame of the other casters alone
 *   kernels  with only slot 0 in use a frame runs the kernels, launches and bits described above; with any other slot in use,
 *            k_shade_shadow_casters, one kernel for every number of casters, every F and R = 0 .. 2
 *   memory   per slot its F * S * S * 4 bytes of maps, allocated when the slot is first rendered; the pass's buffers are
 *            shared by the slots; a 3.6 KB table from the first use of a slot other than 0
 * Deviations kept: the deferred background stays untested; a box, one t per window, no fetch across faces.  New: one slot per
 * light -- two slots naming the same light are refused, not combined.
 *
 * bbr_render_shadow_map renders the map from `light_view_block` (144 bytes in ViewUniformBlock layout; view and proj are
 * used, the rest is ignored).  It renders the recorded draws and is valid inside a frame after the bbr_draw calls (the draws
 * recorded so far) and after bbr_end_frame (the last recorded frame's); otherwise BBR_ERR_NOT_IN_FRAME.  It is synchronous,
 * like bbr_draw_overlays: it drains the frames in flight, grows a capacity that overflows and renders again, and returns
 * when the map is complete.  From then on every submitted frame (bbr_end_frame, bbr_replay_frame, the re-renders of the
 * read-backs) uses the map, the index and the bias, until the next call, a change of the option or bbr_destroy; bbr_resize
 * keeps them.  BBR_ERR_INVALID_ARGUMENT: the option is 0, light_index outside [0, 100), a NULL block, a NaN bias.
 * bbr_render_shadow_faces is the same call with `n_faces` consecutive view blocks (n_faces outside 1 .. 6:
 * BBR_ERR_INVALID_ARGUMENT): one drain, one upload of the draws, the faces back to back, one wait; if a capacity overflows
 * in any face, it grows and all faces are rendered again.  With n_faces = 1 it is bbr_render_shadow_map, bit for bit.
 * bbr_render_shadow_caster is bbr_render_shadow_faces for one slot: the same validity, the same synchronous pass and growth,
 * the same refusals; also BBR_ERR_INVALID_ARGUMENT for `caster` outside 0 .. 7 and for a light_index that another slot in use
 * already holds.  A refused call leaves every slot as it was, the slot named included.  bbr_render_shadow_map / _faces are
 * this call with caster 0, bit for bit (the duplicate-light refusal included).  bbr_drop_shadow_caster drains, releases the
 * slot's maps and marks it not in use; on a slot not in use it is BBR_OK.  With no slot left in use, frames are rendered by
 * the unshadowed kernels, as before a map exists.  bbr_get_shadow_casters fills eight light indices (-1: not in use) and
 * eight face counts (0: not in use).  Changing "shadow_map" drops every slot; "shadow_filter" applies to every slot.
 * Works with both tile modes, both render passes, "present_fused", "max_anisotropy", "supersample" with either
 * "sample_shading" (the test runs per fine fragment), a partition, up to four frames in flight and bbr_replay_frame.
 *
 * Read-backs, in the family of the other diagnostics:
 *   bbr_read_shadow_map   the S x S map, row-major.  INVALID_ARGUMENT while the option is 0, BBR_ERR_NOT_IN_FRAME before a
 *                         map has been rendered
 *   bbr_read_shadow_mask  width*height bytes: the class of every pixel of the last frame.  Re-renders it like
 *                         bbr_read_surface, with the same refusals ("supersample" >= 2, a partition), and INVALID_ARGUMENT
 *                         while no map is in use.  With F >= 2: the class of the deciding face
 *   bbr_read_shadow_face  the S x S map of face `face`; as bbr_read_shadow_map (which reads face 0), and INVALID_ARGUMENT
 *                         for a face outside 0 .. F - 1
 *   bbr_read_shadow_face_index  width*height bytes: the deciding face of every pixel of the last frame, 255 where the class
 *                         is 0 or OUTSIDE.  The same re-render and the same refusals as bbr_read_shadow_mask
 *   bbr_read_shadow_taps  width*height bytes: k of every pixel of the last frame, 255 where the class is 0 or OUTSIDE.  With
 *                         "shadow_filter" 0 it is K = 1: 1 where LIT, 0 where SHADOWED.  The same re-render and the same
 *                         refusals as bbr_read_shadow_mask
 *   bbr_read_shadow_caster_face / _mask / _face_index / _taps  what the namesake above does, for one slot (the calls above
 *                         are slot 0): the same re-render -- one re-render dumps one slot --, the same refusals, the same
 *                         fill values; INVALID_ARGUMENT for a slot outside 0 .. 7 or not in use
 * bbr_read_surface and bbr_read_gbuffer keep working while a map is in use: the re-rendered frame is the shadowed one.
 *
 * The queued pass (bbr_queue_shadow_caster): for a caster that moves every frame.  Valid between bbr_begin_frame and
 * bbr_end_frame only (BBR_ERR_NOT_IN_FRAME elsewhere); it judges its arguments as bbr_render_shadow_caster does, with the same
 * codes, and also refuses a light_index that another slot queued in this frame holds.  It copies the view blocks and returns:
 * nothing is launched, nothing waits, the frames in flight stay in flight.  A second call for a slot in one frame replaces the first.
 * The rule: any sequence of calls with bbr_queue_shadow_caster(args) inside a frame gives, bit for bit in every output, what the
 * same sequence gives with bbr_render_shadow_caster(args) directly in front of that frame's bbr_end_frame, once per queued slot
 * in slot order.  So the maps show every draw the frame has recorded by bbr_end_frame, wherever in the frame the call stood; the
 * caster stays the context's for later frames; a later synchronous call or bbr_drop_shadow_caster replaces or drops it; the
 * read-backs work afterwards (they drain).  The maps are rendered on the frame's own stream in front of its geometry, into a
 * generation of the slot's maps that no frame on the GPU reads.  A capacity that overflows in the pass overflows the frame and
 * is found where a frame's overflow is found: by a synchronising call (any of them, also when later frames have been recorded
 * since), by the next frame that goes into the frame's slot, and by bbr_free_mesh / bbr_free_material.  There the capacities
 * grow and the pass -- and every queued pass submitted behind it -- is rendered again, synchronously, from its own frame's
 * draws, unless a later call has replaced the slot's caster; a synchronising call also renders the last frame again.  Frames
 * shaded in between with the incomplete maps keep their pixels, as frames queued behind an overflowed frame do.
 * A slot keeps up to one copy of its maps (F x S x S floats) per frame in flight once it has been queued; a synchronous call
 * for the slot, a drop or a change of "shadow_map" releases the extra ones.
 * bbr_replay_frame renders the recorded frame's queued passes again.
 * bbr_shadow_queue_counts: host-side counters, does NOT synchronise -- queued passes submitted since bbr_create (one per queued
 * slot and submission of its frame), and how often a frame had to drain the whole context because of one (an overflowed pass
 * found by a host that only streams frames).  Waiting for one frame slot to become idle is not a drain. */
#define BBR_MAX_SHADOW_CASTERS 8
int bbr_render_shadow_map(bbr_context *ctx, int32_t light_index, const void *light_view_block /* 144 B */, float bias);
int bbr_read_shadow_map(bbr_context *ctx, float *out);
int bbr_read_shadow_mask(bbr_context *ctx, uint8_t *out);
int bbr_render_shadow_faces(bbr_context *ctx, int32_t light_index, int32_t n_faces, const void *light_view_blocks /* n_faces x 144 B */,
                            float bias);
int bbr_read_shadow_face(bbr_context *ctx, int32_t face, float *out);
int bbr_read_shadow_face_index(bbr_context *ctx, uint8_t *out);
int bbr_read_shadow_taps(bbr_context *ctx, uint8_t *out);
int bbr_render_shadow_caster(bbr_context *ctx, int32_t caster, int32_t light_index, int32_t n_faces,
                             const void *light_view_blocks /* n_faces x 144 B */, float bias);
int bbr_queue_shadow_caster(bbr_context *ctx, int32_t caster, int32_t light_index, int32_t n_faces,
                            const void *light_view_blocks /* n_faces x 144 B */, float bias);
int bbr_shadow_queue_counts(const bbr_context *ctx, uint64_t *out_queued_passes, uint64_t *out_drains);
int bbr_drop_shadow_caster(bbr_context *ctx, int32_t caster);
int bbr_get_shadow_casters(bbr_context *ctx, int32_t *out_light_index /* 8, -1 = not in use */, int32_t *out_faces /* 8 */);
int bbr_read_shadow_caster_face(bbr_context *ctx, int32_t caster, int32_t face, float *out);
int bbr_read_shadow_caster_mask(bbr_context *ctx, int32_t caster, uint8_t *out);
int bbr_read_shadow_caster_face_index(bbr_context *ctx, int32_t caster, uint8_t *out);
int bbr_read_shadow_caster_taps(bbr_context *ctx, int32_t caster, uint8_t *out);

/* ---- primitive-record read-back ----
 * What the vertex stage (k_geometry: forward_brdf.vert / gbuffer.vert, clip test, viewport, snap, triangle setup) wrote
 * for every primitive of the last frame: a diagnostic in the family of bbr_read_visibility / bbr_read_gbuffer /
 * bbr_read_surface.  Fills the last frame slot's record and triangle buffers with 0xFF bytes (k_geometry writes nothing for
 * a primitive it culls, so what they hold after a frame is partly an earlier frame's), re-renders the last frame and synchronises.  *out_count = the frame's
 * primitives n; min(cap, n) records of 224 bytes and triangles of 64 bytes are copied (either pointer may be NULL), in
 * primitive order (API order of the draws, instance-major inside a draw).  BBR_ERR_NOT_IN_FRAME before a first frame and
 * after bbr_resize, BBR_ERR_INVALID_ARGUMENT on a partitioned context.
 * A primitive that was culled (outside the frustum, back-facing, no pixel centre in its box) keeps the fill in both: its
 * `material` reads 0xFFFFFFFF.  A primitive that goes through the clipper has a record whose head [0..8] is zero (its
 * sub-triangles carry their own planes) and no triangle (the fill).
 * One record, by dword (float unless said otherwise):
 *   [0..1]   X0 Y0 (int32): vertex 0 in 1/256 pixel, pixel (px, py) has its centre at (256 px + 128, 256 py + 128)
 *   [2..5]   l1dx l1dy l2dx l2dy: the screen-space planes of the barycentrics of vertices 1 and 2, per 1/256 pixel,
 *            relative to vertex 0 (binary64 expressions rounded once)
 *   [6..8]   rw0 rw1 rw2: 1 / w of gl_Position at the three vertices
 *   [9..14]  uv[3][2]: aUV of vertex 0, 1, 2 (copies: every bit of the input, a NaN's payload included)
 *   [15]     packed_dims (uint32): width | height << 16 of a packed material, 0 otherwise
 *   [16..17] packed (a device pointer; only "is it null" has a meaning for the caller)
 *   [18]     material (uint32): the draw's material handle
 *   [19]     clip_base (uint32): 0xFFFFFFFF unless the clipper produced sub-triangles for the primitive
 *   [20..55] vary[12][3], varying-major ([varying][vertex]): vPosWorld.xyz, then N.xyz, T.xyz, B.xyz of vTBN
 *            (forward_brdf.vert:25,31-35)
 * One triangle (unclipped survivors only), by dword:
 *   [0..5]   X0 Y0 X1 Y1 X2 Y2 (int32), 1/256 pixel        [6..8]   z0 dzdx dzdy: z / w at vertex 0 and its plane per
 *   [9..12]  l1dx l1dy l2dx l2dy as in the record                   1/256 pixel
 *   [13..15] rw0 rw1 rw2 */
int bbr_read_records(bbr_context *ctx, void *records, void *triangles, uint32_t cap, uint32_t *out_count);

/* ---- overlay subpass ----
 * The reference draws its light markers and the corner gizmo into the swapchain image after tone mapping, depth-tested
 * against the scene (recordCommand, src/main.cpp:128-171; light.vert/.frag on generateUVSphereMesh(0.1, 16, 16), one
 * instance per light; gizmo.vert/.frag in a gizmo_extent^2 viewport at the top-right whose depth is cleared first).
 *   bbr_set_option(ctx, "overlays", 1)   frames keep their resolved depth (4 bytes per pixel) from now on
 *   bbr_upload_gizmo                     the gizmo mesh: 36-byte bb::GizmoVertex records (Pos, Color, Normal,
 *                                        src/render.h:122-126), optional uint32 indices (see bba_load_obj_gizmo)
 *   bbr_draw_overlays                    after bbr_present of the last frame: draws markers (the frame's own lights) and,
 *                                        if gizmo_extent > 0 and a gizmo was uploaded, the gizmo (the reference uses
 *                                        100) over the presented image.  Synchronous: a debugging aid, not part of the
 *                                        hot path.  Not available with a partition. */
int bbr_upload_gizmo(bbr_context *ctx, const void *gizmo_vertices, uint32_t n_vertices, const uint32_t *indices,
                     uint32_t n_indices);
int bbr_draw_overlays(bbr_context *ctx, int32_t gizmo_extent);

/* ---- TBN line overlay ("Enable TBN", src/main.cpp:1309-1310; pipeline src/main.cpp:788-822) ----
 * With option "tbn" = 1, bbr_draw_overlays first draws, for every triangle of the last frame's draws, the tangent frame
 * of tbn.vert / tbn.geom (src/shaders/tbn.vert:18-41, src/shaders/tbn.geom:14-73): a 9-vertex line strip C,T,C, C,B,C,
 * C,N,C from the centroid, 0.05 long, red / green / blue, depth-tested (>=) against the scene without writing depth,
 * over the presented image; then the markers and the gizmo as above.  Same preconditions as bbr_draw_overlays; it also
 * runs with no lights and gizmo_extent = 0.  The line rule: clip-space Liang-Barsky against
 * 0 <= z <= w and |x|, |y| <= 4 w, snapped to 1/256 pixel like the triangles, diamond-exit fragments (OpenGL 4.6
 * section 14.5.1) on those integers, at each pixel the passing fragment with the largest key wins.
 * One segment record (32 bytes): */
typedef struct bbr_tbn_segment {
  int32_t x0, y0, x1, y1; /* endpoints in 1/256 pixel, pixel (px, py) has its centre at (256 px + 128, 256 py + 128) */
  float za, zb;           /* z / w at the two endpoints */
  uint32_t key;           /* global primitive index * 8 + strip segment s (0..7); colour s / 3 = red, green, blue */
  uint32_t pad;
} bbr_tbn_segment;
/* The segment records of the last TBN draw, in key order (a strip segment that was clipped away, not finite or of zero
 * length once snapped has none).  *out_count = their number; min(cap, count) are copied to out (out may be NULL).
 * Synchronises.  BBR_ERR_NOT_IN_FRAME before the first TBN draw and after bbr_resize. */
int bbr_read_tbn_segments(bbr_context *ctx, bbr_tbn_segment *out, uint32_t cap, uint32_t *out_count);
/* Self-test of the line rule: the pass's own binning, raster and resolve kernels on n caller-supplied segments over a
 * width x height depth buffer (row-major floats).  out_keys[width * height] receives key + 1 of the winning segment per
 * pixel, 0 where no fragment passed.  Coordinates within +-2^25, key != 0xFFFFFFFF.  Synchronises. */
int bbr_selftest_lines(bbr_context *ctx, const bbr_tbn_segment *segs, uint32_t n, int32_t width, int32_t height,
                       const float *depth, uint32_t *out_keys);

/* ---- GUI pass: the last statement of the overlay subpass (src/main.cpp:172) ----
 * ImGui_ImplVulkan_RenderDrawData(ImGui::GetDrawData(), cmdBuffer) blends the GUI's draw lists into the swapchain image
 * inside the render pass this library replaces.  The window system, input and widget logic stay the host's; the library
 * takes the DRAW DATA the GUI code hands to Vulkan: ImDrawVert / ImDrawIdx arrays and the ImDrawCmd records without their
 * pointers, all command lists flattened in order with their offsets made global (INTEGRATION.md has the loop).
 *   bbr_upload_ui_texture   ImGui_ImplVulkan_CreateFontsTexture / ImGui_ImplVulkan_AddTexture: an RGBA8 image, row-major;
 *                           the handle (>= 1) is what the host stores as ImTextureID.  At most 16384 x 16384 texels
 *   bbr_free_ui_texture     drains the context first.  The handle is dead at once and the lowest dead handle is what the next
 *                           bbr_upload_ui_texture returns, so a host that rebuilds its atlas keeps a bounded table
 *   bbr_draw_ui             blends the draw data into the image the last bbr_present wrote -- after bbr_draw_overlays if the
 *                           host calls that: the same image, a caller's buffer and option "present_fused" included.  With
 *                           both (a fused frame that bbr_present copied to a caller's buffer) the pass blends into the slot's
 *                           image and copies the rows of the union box to the caller's buffer again behind itself, so the
 *                           buffer and bbr_presented_device_ptr hold the same bytes.
 *                           BBR_ERR_NOT_IN_FRAME before a frame, before a present and after bbr_resize;
 *                           BBR_ERR_INVALID_ARGUMENT on a partitioned context, when (int)(display_size * framebuffer_scale)
 *                           is not the context's extent, when bbr_ui_validate fails, or when a command that draws
 *                           (elem_count > 0) names a texture that is not alive.  Nothing is launched in any of these cases.
 *                           ASYNCHRONOUS, unlike the debugging overlays (a host draws its GUI every frame): the draw data
 *                           is copied into pinned staging owned by the frame slot before the call returns and the kernels are
 *                           queued behind the presentation on the slot's stream.  The call blocks only to grow a buffer (or,
 *                           called again for the same frame, until the earlier call's copy has left the staging).
 *                           It never re-renders, and a re-render does not repeat it: a frame that is resubmitted (capacity
 *                           growth found by a synchronising call, a diagnostic read such as bbr_read_visibility) or
 *                           presented again has no GUI until the host calls bbr_draw_ui again.
 *   bbr_ui_validate         host only -- no context, no device: everything bbr_draw_ui requires of the draw data itself.
 *                           BBR_ERR_INVALID_ARGUMENT for elem_count % 3 != 0, idx_offset + elem_count > n_indices, any
 *                           vtx_offset + index >= n_vertices, a non-finite pos or uv (of any vertex in the array), a position
 *                           whose snapped coordinate leaves +-2^23 (1/256 pixel), display_size <= 0, a non-finite
 *                           display_pos / framebuffer_scale, a NULL array with a non-zero count, a frame beyond 32768.
 *                           out_box (may be NULL): the union of the scissors of the commands that draw, cut to the frame,
 *                           x0 y0 x1 y1 with exclusive ends (all 0: nothing to draw); only its tiles are launched.
 * The rule, binary32 without contraction, in this operand order:
 *   vertex    scale = 2.0f / display_size, translate = -1.0f - display_pos * scale, ndc = pos * scale + translate (a multiply,
 *             then an add), w = 1 (external/imgui/imgui_impl_vulkan.cpp:122-126, 301-306); viewport transform and 1/256 snap
 *             as for scene triangles
 *   coverage  pixel centres at + 0.5, integer edge functions on the snapped coordinates, top-left rule; cullMode NONE
 *             (external/imgui/imgui_impl_vulkan.cpp:716): a triangle of negative area has vertices 1 and 2 exchanged WITH their
 *             attributes before setup, zero area draws nothing
 *   scissor   external/imgui/imgui_impl_vulkan.cpp:406-425: r = (clip_rect - display_pos) * framebuffer_scale; the command is
 *             skipped unless r.x < fb_w && r.y < fb_h && r.z >= 0 && r.w >= 0; negative r.x / r.y become 0; offset =
 *             (int32)r.x, extent = (uint32)(r.z - r.x) -- the difference is truncated, not the ends (a negative difference:
 *             extent 0); a fragment passes iff offset <= p < offset + extent on both axes
 *   attribute l1 = fmaf(l1dx, dx, l1dy * dy), l2 likewise, from planes set up once per triangle in binary64 and rounded once,
 *             (dx, dy) the pixel centre minus snapped vertex 0 in 1/256 pixel; a = fmaf(l2, a2 - a0, fmaf(l1, a1 - a0, a0))
 *             for u, v and the four colour channels, a colour channel being (float)byte * (1.0f / 255.0f)
 *   fragment  src = colour * texel per channel (external/imgui/imgui_impl_vulkan.cpp:181-183), texel = one bilinear tap at
 *             LOD 0, REPEAT (sampler external/imgui/imgui_impl_vulkan.cpp:610-618), the sampler of "max_anisotropy" 1
 *   blend     external/imgui/imgui_impl_vulkan.cpp:724-732 on the sRGB UNORM8 image: the pixel's BYTES are the destination,
 *             d = dec[byte] ((float) of the binary64 EOTF of byte / 255.0), ia = 1.0f - sa, o = fmaf(s, sa, d * ia), byte =
 *             the sRGB encode of o as in bbr_present; alpha oa = sa * ia (factors ONE_MINUS_SRC_ALPHA and ZERO, as the back end
 *             sets them), byte = rintf(255.0f * clamp01(oa)).  Requantised to bytes after EVERY fragment
 *   order     the fragments of a pixel are blended in command order and, within a command, in index order */
typedef struct bbr_ui_cmd {            /* one ImDrawCmd without its pointers; 32 bytes */
  float    clip_rect[4];               /* x1 y1 x2 y2, as ImDrawCmd::ClipRect */
  int32_t  texture;                    /* handle from bbr_upload_ui_texture */
  uint32_t vtx_offset, idx_offset, elem_count;
} bbr_ui_cmd;
typedef struct bbr_ui_draw {
  const void     *vertices;  uint32_t n_vertices;  /* ImDrawVert, 20 B: pos f32x2 @0, uv f32x2 @8, col RGBA8 @16 (R = low byte) */
  const uint16_t *indices;   uint32_t n_indices;   /* ImDrawIdx = unsigned short in the reference's build */
  const bbr_ui_cmd *cmds;    uint32_t n_cmds;      /* all command lists flattened in order, offsets made global */
  float display_pos[2], display_size[2], framebuffer_scale[2];
} bbr_ui_draw;
int bbr_upload_ui_texture(bbr_context *ctx, const uint8_t *rgba8, int32_t w, int32_t h, int32_t *out_texture);
int bbr_free_ui_texture(bbr_context *ctx, int32_t texture);
int bbr_draw_ui(bbr_context *ctx, const bbr_ui_draw *draw);
int bbr_ui_validate(const bbr_ui_draw *draw, int32_t fb_width, int32_t fb_height, int32_t *out_box /* x0 y0 x1 y1 */);

/* ---- presentation: the step after the path ----
 * Replaces the tone-map subpass + swapchain write (src/main.cpp:123-126, src/shaders/hdr_tone_mapping.frag:9-18,
 * HDR attachment R16G16B16A16_SFLOAT src/render.h:94, sRGB swapchain format src/render.cpp:242-254):
 * per pixel of the last frame  rgb -> [binary16 round, if hdr16] -> EnableToneMapping ? 1 - exp(-rgb * Exposure) : rgb
 * -> sRGB encode -> UNORM8, alpha = 255; EnableToneMapping / Exposure are the ones of the FrameUniformBlock the frame
 * was rendered with.  Asynchronous, queued behind the frame's shading.  `rgba8_device` = NULL writes a buffer owned by
 * the context (bbr_presented_device_ptr / bbr_read_presented); with a partition the image is this rank's shard
 * (bbr_shard_rows() rows), gathered with ncclAllGather + bbr_unpack_gathered_rgba8 at a quarter of the fp32 payload. */
int bbr_present(bbr_context *ctx, void *rgba8_device, int32_t hdr16);
int bbr_read_presented(bbr_context *ctx, uint8_t *rgba8_host); /* rows*width*4 bytes; synchronises */
/* the same conversion on any device buffer of n_pixels RGBA32F pixels (e.g. an all-gathered frame), queued on
 * `hip_stream` (NULL = the context's shading stream) */
int bbr_present_buffer(bbr_context *ctx, const void *rgba32f_device, void *rgba8_device, uint64_t n_pixels,
                       int32_t enable_tone_mapping, float exposure, int32_t hdr16, void *hip_stream);
int bbr_presented_device_ptr(bbr_context *ctx, void **out_ptr, uint64_t *out_bytes);
int bbr_unpack_gathered_rgba8(bbr_context *ctx, const void *gathered_device, void *frame_device, void *hip_stream); /* BBR_SHARD_RGBA8 */
/* with option "timing" on: launches of k_present since bbr_timing_reset and their average duration (HIP events) */
int bbr_present_timing(bbr_context *ctx, uint32_t *out_launches, float *out_avg_ms);
/* its sibling for option "supersample" >= 2: the k_resolve launches of the timed frames since bbr_timing_reset (one per frame
 * that carries events, see "timing_stride") and their average duration */
int bbr_resolve_timing(bbr_context *ctx, uint32_t *out_launches, float *out_avg_ms);
/* hdr_tone_mapping.frag:9-18 alone on the fp32 frame, in place (no quantisation) */
int bbr_tone_map(bbr_context *ctx, int32_t enable_tone_mapping, float exposure);

/* ---- bloom (option "bloom" = L in 1..8; no reference counterpart: the reference clips a bright light to a white disc) ----
 * Between the linear HDR frame and the presented image: what exceeds a threshold is filtered down L levels and back up,
 * and the sum is added to the frame's value in front of the conversion of bbr_present.  The fp32 frame is only read.
 * The rule.  All operations are binary32, round to nearest even, denormals kept, no contraction: every + - * below is one
 * IEEE operation, there is no fma.  Inputs: L; the threshold T and the intensity I of bbr_set_bloom; the source F, the
 * W x H RGBA32F frame bbr_present reads (the slot's output, the resolved frame under "supersample" >= 2, a caller's output
 * buffer).  Only r, g and b take part.
 *   sizes    w_0 = W, h_0 = H;  w_k = (w_{k-1} + 1) >> 1, h_k likewise, k = 1 .. L   (never below 1: all L levels always exist)
 *   bright   e(x,y)[c] = min(max0(F(x,y)[c] - T), 65504.0f)    max0(d) = d > 0 ? d : 0  (NaN -> +0, -0 -> +0, -inf -> 0, +inf -> 65504)
 *   box      box(G,w,h)(x,y) = ((G(x0,y0) + G(x1,y0)) + (G(x0,y1) + G(x1,y1))) * 0.25f
 *            x0 = min(2x, w-1), x1 = min(2x+1, w-1), y0, y1 likewise
 *   down     D_1 = box(e, W, H);   D_{k+1} = box(D_k, w_k, h_k)
 *   lerp4    lerp4(a,b) = a + (b - a) * 0.25f
 *   up       up(G,w',h')(x,y), (x,y) a texel of the next finer grid:  px = x >> 1, py = y >> 1,
 *            qx = clamp(px + ((x & 1) ? 1 : -1), 0, w'-1), qy likewise,
 *            r0 = lerp4(G(px,py), G(qx,py)), r1 = lerp4(G(px,qy), G(qx,qy)), up = lerp4(r0, r1)     (weights 9 3 3 1 / 16)
 *   sum      U_L = D_L;   U_k = D_k + up(U_{k+1}, w_{k+1}, h_{k+1}),  k = L-1 .. 1
 *   pixel    B(x,y) = up(U_1, w_1, h_1)(x,y);   v[c] = F(x,y)[c] + I * B(x,y)[c]    (the product, then the sum)
 *   image    the byte triple of bbr_present's conversion of v (binary16 stage if hdr16, tone map, sRGB byte); alpha 255
 * So every D, U and B is finite and >= +0 whatever F holds; a NaN or inf of F reaches only its own pixel, as without bloom;
 * with I = 0, or T >= every finite channel of F, the bytes are those of "bloom" 0; and a constant bright-pass value e gives
 * U_1 = L * e: the levels add and nothing is normalised -- I is the user's scale.
 * Deviations from the usual effect, on purpose: a hard per-channel threshold (no soft knee, no luminance weighting), a box
 * down-filter and a tent up-filter, an fp32 pyramid.
 *   bbr_set_option(ctx, "bloom", L)   see the option list.  With L >= 1 bbr_present queues the chain (k_bloom_first,
 *             k_bloom_down, k_bloom_up) and k_present_bloom in k_present's place, on the same stream; whatever presents a frame
 *             again (a capacity growth, the read-backs that render again) runs the chain again.  hdr16 0 and 1, a caller's
 *             rgba8_device or output buffer, "supersample" 2..4 with either "sample_shading", both render passes, up to four
 *             frames in flight (a pyramid per frame slot); bbr_draw_overlays and bbr_draw_ui act on the bloomed image.
 *   bbr_set_bloom     T and I: both finite and >= 0, else BBR_ERR_INVALID_ARGUMENT and nothing changes.  Defaults 1.0f and 0.05f.
 *             Stored at any L.  Waits for the GPU like the option; in effect from the next presentation.
 *   bbr_get_bloom     the stored L, T and I (any pointer may be NULL).
 *   bbr_present_buffer_bloom   the rule on any W x H device frame, with a pyramid owned by the context: how a host blooms the
 *             all-gathered whole frame of a partition.  With L = 0 it is bbr_present_buffer(n = width * height), bit for bit.
 *             BBR_ERR_INVALID_ARGUMENT, and nothing launched, for a NULL pointer, a source not 16-byte or an output not 4-byte
 *             aligned, an extent outside 1..32768.  Asynchronous on `hip_stream` (NULL = the context's shading stream); calls on
 *             different streams are ordered one behind the other by the library (an event), since they share the pyramid.
 *   bbr_read_bloom_level   U_level, w_k * h_k * 3 floats (r, g, b; row-major), of the last frame's presentation (source 0)
 *             or of the last bbr_present_buffer_bloom (source 1).  Synchronises.  `out_rgb` may be NULL to ask for the size;
 *             `capacity` is in bytes, BBR_ERR_CAPACITY when too small.  BBR_ERR_NOT_IN_FRAME before such a run under the
 *             option's current value and after bbr_resize; BBR_ERR_INVALID_ARGUMENT for a level outside 1..L (every level at L = 0).
 *   bbr_bloom_timing  sibling of bbr_present_timing: with option "timing" on, the chains since bbr_timing_reset and the
 *             average duration of one (first launch to last, in front of k_present_bloom, which bbr_present_timing times).
 * Refused, by whichever call would complete the pair, with the context unchanged: "bloom" >= 1 on a partition of world > 1
 * (bbr_set_option / bbr_set_partition: the chain needs the rows the neighbours own) and with "present_fused" non-zero (there
 * is no fp32 frame).
 * Memory: per frame slot the sum of w_k * h_k texels of 16 bytes (about a third of W * H), from the slot's first bloomed
 * presentation until the option returns to 0, bbr_resize or bbr_destroy; counted by bbr_debug_live_resources. */
int bbr_set_bloom(bbr_context *ctx, float threshold, float intensity);
int bbr_get_bloom(bbr_context *ctx, int32_t *out_levels, float *out_threshold, float *out_intensity);
int bbr_present_buffer_bloom(bbr_context *ctx, const void *rgba32f_device, void *rgba8_device, int32_t width, int32_t height,
                             int32_t enable_tone_mapping, float exposure, int32_t hdr16, void *hip_stream);
int bbr_read_bloom_level(bbr_context *ctx, int32_t source, int32_t level, float *out_rgb, uint64_t capacity, int32_t *out_w,
                         int32_t *out_h);
int bbr_bloom_timing(bbr_context *ctx, uint32_t *out_launches, float *out_avg_ms);

/* ---- auto exposure (option "auto_exposure" = 1; no reference counterpart: the reference's Exposure is a slider) ----
 * The exposure of a presentation follows from the pixels of the frame it presents, on the device: nothing is read back and
 * the frames in flight stay in flight.  The fp32 frame is only read.
 * The rule.  Every floating-point operation is one binary32 IEEE operation: round to nearest even, denormals kept, no
 * contraction, no fma.  Everything about the histogram is integer arithmetic, so the result does not depend on the order in
 * which pixels are counted and can be checked with no tolerance.  Source: F, the W x H RGBA32F frame bbr_present reads (the
 * slot's output, the resolved frame under "supersample" >= 2, a caller's output buffer): the fp32 values in front of the
 * binary16 stage and before bloom is added.  Alpha takes no part.
 *   luma     Y = (0.2126f * r + 0.7152f * g) + 0.0722f * b
 *   count    !(Y > 0)  (NaN, +-0, negative, -inf): the pixel is IGNORED.  Otherwise, u the bits of Y:
 *            bin = clamp((int)(u >> 20) - 888, 0, 255)      8 bins per octave over [2^-16, 2^16);  888 = (127 - 16) * 8
 *            denormals and everything below 2^-16 go to bin 0, everything >= 2^16, +inf included, to bin 255
 *            hist[k] = the pixels in bin k;  N = sum hist[k];  ignored = W * H - N
 *   trim     lo, hi in permille, 0 <= lo < hi <= 1000
 *            skip_lo = floor(N * lo / 1000), skip_hi = floor(N * (1000 - hi) / 1000), in 64 bits
 *            P_k = sum_{j<k} hist[j];   c_k = max(0, min(P_k + hist[k], N - skip_hi) - max(P_k, skip_lo))
 *            N' = sum c_k  (= N - skip_lo - skip_hi, > 0 whenever N > 0);   S = sum k * c_k
 *   mean     mean_bits = (888 << 20) + floor((S << 20) / N') + (1 << 19), in 64 bits: the centre of a bin, the fraction
 *            carried into the mantissa.  Ybar = the binary32 with those bits: always normal, in [2^-16, 2^16).  This is the
 *            log-average with log2(1 + t) taken as t, the device "mip_levels" already uses for lambda.
 *   target   E* = key * r, r the correctly rounded 1 / Ybar;   E_c = min(max(E*, e_min), e_max)
 *   adapt    with a history E_prev:  E = (rate == 1.0f) ? E_c : E_prev + (E_c - E_prev) * rate;   without one: E = E_c
 *            The history becomes E.
 *            N == 0: the history is left as it is, and E = the history if there is one, else the frame's own Exposure
 *            (the caller's `exposure` in the buffer call); the record's mean_bits, target and clamped are 0 then.
 *   image    the bytes of bbr_present's conversion with E in Exposure's place; under "bloom" L >= 1 of v = F + I * B as
 *            without the option.  EnableToneMapping and hdr16 are as without it; with tone mapping off E is computed and unused.
 * Histories and presentations.  A context has two histories, as bloom has two pyramids: source 0 is the frames bbr_present
 * presents, source 1 is bbr_present_buffer_auto.  Every bbr_present call the host makes is one presentation, in call order:
 * it meters, adapts and advances history 0.  Presentations of frames in different slots run on different streams; the adapt
 * step of each is ordered behind that of the one before it on the device (an event; the host never waits).  A presentation the
 * library repeats -- the re-render behind a capacity growth, the read-backs that render the frame again -- does not meter
 * again: it converts with the E the slot's frame was first presented with and leaves the history alone.  Deviation, on
 * purpose: a frame that overflowed a capacity was metered incomplete, and that E stays.
 *   bbr_set_option(ctx, "auto_exposure", 0|1)   see the option list.  Both render passes, "supersample" 2..4 with either
 *             "sample_shading", "bloom" 0..8, a caller's rgba8_device or output buffer, hdr16 0 and 1, one to four frames in
 *             flight, every "stream_layout", bbr_set_stream and bbr_replay_frame; bbr_draw_overlays and bbr_draw_ui act on the
 *             image as before.
 *   bbr_set_auto_exposure   key, e_min, e_max, rate, lo and hi (permille).  Defaults 0.18f, 2^-10, 2^10, 1.0f, 500, 950.  Every
 *             float finite, key > 0, 0 < e_min <= e_max, 0 <= rate <= 1, 0 <= lo < hi <= 1000; else BBR_ERR_INVALID_ARGUMENT
 *             and nothing changes.  Stored at either value of the option.  Does not wait for the GPU and touches no slot: a
 *             presentation takes the values stored when it is queued, so presentations in flight keep theirs and the next
 *             call of bbr_present / bbr_present_buffer_auto has the new ones -- cheap enough to call every frame.
 *             `rate` is per presentation: the host owns the clock and passes 1 - exp(-dt * speed).
 *   bbr_get_auto_exposure   the six stored values (any pointer may be NULL).
 *   bbr_reset_exposure      forgets both histories (the next presentation of each source applies its E_c).  Waits for the
 *             GPU like the option.
 *   bbr_present_buffer_auto   the rule on any W x H device frame, with history 1: how a host exposes the all-gathered whole
 *             frame of a partition.  Honours option "bloom" exactly as bbr_present_buffer_bloom does, with the same
 *             alignment and extent refusals; asynchronous on `hip_stream` (NULL = the context's shading stream), calls on
 *             different streams ordered one behind the other by the library (an event).  `exposure` is used only when nothing
 *             is counted and there is no history.  BBR_ERR_INVALID_ARGUMENT while the option is 0.
 *   bbr_read_exposure   synchronises and returns the record of that source's last presentation.  BBR_ERR_NOT_IN_FRAME before
 *             such a presentation under the option, and after bbr_resize for source 0; BBR_ERR_INVALID_ARGUMENT for a source
 *             outside 0..1 or while the option is 0.
 *   bbr_luminance_timing   sibling of bbr_present_timing.  With option "timing" on, k_luminance has a ring of its own: the
 *             launches since bbr_timing_reset and the average duration of one.  k_exposure (and its wait for the adapt step of
 *             the presentation before) falls into the interval bbr_present_timing reports.
 * Refused, by whichever call would complete the pair, with the context unchanged: "auto_exposure" 1 with "present_fused"
 * non-zero (the exposure would be needed before the frame exists) and on a partition of world > 1 (bbr_set_option /
 * bbr_set_partition: metering needs the whole frame; the host meters the gathered frame with the buffer call).
 * Memory: five histograms of 257 words, five records and two history words, from the option's set to 1 until it returns to 0
 * or bbr_destroy; counted by bbr_debug_live_resources. */
typedef struct bbr_exposure_record {
  uint32_t hist[256];                       /* the pixels counted per bin */
  uint32_t ignored, counted, kept;          /* W * H - N, N, N' */
  uint32_t mean_bits;                       /* the bits of Ybar */
  uint64_t sum;                             /* S */
  float target, clamped, previous, applied; /* E*, E_c, E_prev (0 without a history), E */
  uint32_t flags;                           /* bit 0: a history existed; bit 1: N == 0 */
  uint32_t reserved;
} bbr_exposure_record;
int bbr_set_auto_exposure(bbr_context *ctx, float key, float e_min, float e_max, float rate, int32_t lo_permille, int32_t hi_permille);
int bbr_get_auto_exposure(bbr_context *ctx, float *out_key, float *out_e_min, float *out_e_max, float *out_rate,
                          int32_t *out_lo_permille, int32_t *out_hi_permille);
int bbr_reset_exposure(bbr_context *ctx);
int bbr_present_buffer_auto(bbr_context *ctx, const void *rgba32f_device, void *rgba8_device, int32_t width, int32_t height,
                            int32_t enable_tone_mapping, float exposure, int32_t hdr16, void *hip_stream);
int bbr_read_exposure(bbr_context *ctx, int32_t source, bbr_exposure_record *out);
int bbr_luminance_timing(bbr_context *ctx, uint32_t *out_launches, float *out_avg_ms);

/* ---- native exchange: every rank gets the whole frame (BASELINE config #4) ----
 * The reference renders on one GPU; with a partition (bbr_set_partition) each rank holds a compact shard and the frame
 * is completed by one exchange step.  Two native forms, both queued on the stream of the frame's slot right behind its
 * shading (with stream layout 2 that stream carries nothing else: the next frame of the slot is ordered behind the
 * exchange without an event, the other slots render meanwhile), or on `hip_stream` when one is given (made to wait for
 * the frame first):
 *   collective  bbr_comm_unique_id on rank 0 -> the 128 bytes reach every rank by the host's own means ->
 *               bbr_comm_init on every rank (ncclCommInitRank; one process per GPU) -> per frame bbr_allgather_frame:
 *               [pack into this rank's slot of `gathered`] -> ncclAllGather in place (ring over xGMI) -> un-interleave into
 *               `whole`.  librccl is opened with dlopen at the first of these calls; a single-GPU host never loads it.
 *   peer        bbr_push_shard: this rank's block goes into every rank's gather buffer -- for one process driving several
 *               GPUs (one context each) or processes that exchanged bbr_ipc_export handles.  Option "push_mode" 1
 *               (default): ONE kernel loads the block once and stores it to all world - 1 peers, every xGMI link of the
 *               full mesh busy at the same time (the direct pattern: block / link bandwidth); peer access to the other
 *               devices is enabled on first use, and a peer that cannot be mapped falls back to mode 0.  "push_mode" 0:
 *               hipMemcpyPeerAsync copies queued one behind the other, nearest rank first -- one link at a time, i.e.
 *               ring timing.  bbr_push_state says which form the last push took.  The host orders "all pushes have
 *               landed" (events or a barrier) before bbr_unpack_whole, and must not let a rank push frame n + 1 into a
 *               buffer a peer is still un-interleaving frame n from: two gather buffers per rank, used in turn.
 * Block forms (what travels per rank; bbr_exchange_block_bytes): BBR_SHARD_RGBA32F the fp32 shard (16 B/pixel),
 * BBR_SHARD_PACKED rgb + one alpha bit per pixel (12.1 B, lossless: alpha is 0 or 1; = bbr_pack_shard), BBR_SHARD_RGBA8
 * the presented shard (4 B; needs bbr_present), BBR_SHARD_RGBA16F the shard rounded to binary16 (8 B, lossy: a separate
 * output, see the define).  `gathered` / `whole` = NULL use buffers owned by the frame's slot
 * (bbr_whole_frame_device_ptr, bbr_read_whole_frame).  An exchange never re-renders (one rank alone must not repeat a
 * collective): let the capacities settle with one synchronised frame first, as after any scene change.
 * BBR_SHARD_PACKED in full: rgb[n][3] float (n = shard_rows * width), padding to 8 bytes, one little-endian 64-bit mask per
 * 64 pixels (bit k of word w = pixel 64 w + k, set where alpha has the bits of 1.0f; unused bits of the last word clear),
 * padding to 16 bytes.  The padding bytes are written as zero: a block depends on the shard alone.
 * Alignment.  Every pointer below is accessed by a kernel at the width given (bytes); a call whose pointer is not a
 * multiple of it returns BBR_ERR_INVALID_ARGUMENT and launches nothing.  Every block size is a multiple of its form's
 * figures (with a partition, of 16), so block r of an aligned gather buffer is aligned as well.
 *                                                                      RGBA32F  PACKED  RGBA8  RGBA16F
 *   block written: bbr_stage_shard / bbr_pack_shard `block_device`,
 *     bbr_push_shard every peer_gathered[], bbr_allgather_frame gathered      4       8      4        8
 *   gather buffer read: bbr_unpack_whole, bbr_unpack_gathered*,
 *     bbr_allgather_frame `gathered_device`                                  16       8      4        8
 *   whole frame written: `whole_device` / `frame_device` of the same         16      16      4       16
 * (the mask words and a binary16 pixel are 8-byte accesses, an RGBA32F pixel a 16-byte one; a plain block is copied, and
 * stored by bbr_push_shard in 16-byte pieces when every gather buffer is 16-byte aligned, in 4-byte words otherwise).
 * Not yet run on more than one GPU: see DESIGN.md section 5. */
#define BBR_COMM_ID_BYTES 128
#define BBR_IPC_HANDLE_BYTES 64
#define BBR_SHARD_RGBA32F 0
#define BBR_SHARD_PACKED 1
#define BBR_SHARD_RGBA8 2
#define BBR_SHARD_RGBA16F 3 /* every channel rounded to binary16 -- the reference's own HDR attachment format, R16G16B16A16_SFLOAT
                             * (src/render.h:94, src/main.cpp:463-472): 8 B/pixel, LOSSY; the whole frame is widened back to RGBA32F */
int bbr_comm_unique_id(bbr_context *ctx, uint8_t *out_id /* BBR_COMM_ID_BYTES */);
int bbr_comm_init(bbr_context *ctx, int32_t rank, int32_t world, const uint8_t *unique_id /* BBR_COMM_ID_BYTES */);
int bbr_comm_destroy(bbr_context *ctx);
/* opens librccl (dlopen + symbol lookup) and nothing else: NOT collective.  Hosts vote on this before they enter
 * bbr_comm_init together -- a rank that cannot load the library must not leave the others waiting inside ncclCommInitRank */
int bbr_comm_probe(bbr_context *ctx);
/* ranks in the context's communicator as RCCL itself reports them (ncclCommCount) */
int bbr_comm_count(bbr_context *ctx, int32_t *out_ranks);
/* this rank's block of the last frame in `form`, written to `block_device` (bbr_exchange_block_bytes bytes) on `hip_stream`
 * (NULL = the frame's own stream): what bbr_allgather_frame / bbr_push_shard do first, for hosts that run the collective
 * themselves and finish with bbr_unpack_whole */
int bbr_stage_shard(bbr_context *ctx, int32_t form, void *block_device, void *hip_stream);
int bbr_exchange_block_bytes(const bbr_context *ctx, int32_t form, uint64_t *out_bytes);
int bbr_allgather_frame(bbr_context *ctx, int32_t form, void *gathered_device /* world blocks, or NULL */,
                        void *whole_device /* height*width pixels, or NULL */, void *hip_stream);
int bbr_push_shard(bbr_context *ctx, int32_t form, void *const *peer_gathered /* [world] device pointers */,
                   const int32_t *peer_devices /* [world] HIP device of each */, void *hip_stream);
/* 1 if the last bbr_push_shard stored through the one-kernel direct form, 0 if it queued copies */
int bbr_push_state(const bbr_context *ctx, int32_t *out_direct);
int bbr_unpack_whole(bbr_context *ctx, int32_t form, const void *gathered_device, void *whole_device, void *hip_stream);
int bbr_whole_frame_device_ptr(bbr_context *ctx, void **out_ptr, uint64_t *out_bytes);
int bbr_read_whole_frame(bbr_context *ctx, void *host /* height*width*16 bytes (RGBA8 form: *4); synchronises */);
/* plain device memory on the context's GPU (zero-filled), for hosts that do not link HIP themselves: gather buffers */
int bbr_device_alloc(bbr_context *ctx, uint64_t bytes, void **out_ptr);
int bbr_device_free(bbr_context *ctx, void *ptr);
int bbr_copy_to_host(bbr_context *ctx, void *host, const void *device_ptr, uint64_t bytes); /* drains the context first */
int bbr_ipc_export(bbr_context *ctx, void *device_ptr, uint8_t *out_handle /* BBR_IPC_HANDLE_BYTES */);
int bbr_ipc_open(bbr_context *ctx, const uint8_t *handle, void **out_ptr);
int bbr_ipc_close(bbr_context *ctx, void *ptr);

#ifdef __cplusplus
}
#endif
#endif
