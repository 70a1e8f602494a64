// bibim_hip.hip -- C-ABI (include/bibim_hip.h) over the HIP kernels in bb_kernels.hip.h.
//
// One context = one GPU, one HIP stream, all buffers resident in HBM for the context's lifetime.
// A frame is: [H2D of lights + draw descriptors + instances, one async copy from pinned staging] -> k_geometry
// (all draws) -> k_raster (per tile) -> k_shade (per visible pixel).  No host synchronisation inside a frame; capacities (bins, broad list, clip arena) are
// checked lazily at the next synchronising call and the frame is re-rendered once after growing them.
#include <hip/hip_runtime.h>
#include <rccl/rccl.h>  // types and prototypes only: the library is opened at bbr_comm_init (see the exchange section)

#include <dlfcn.h>

#include <algorithm>
#include <array>
#include <chrono>
#include <cmath>
#include <limits>
#include <memory>
#include <mutex>
#include <unordered_set>
#include <cstdio>
#include <cstring>
#include <string>
#include <tuple>
#include <vector>

#include "../../include/bibim_hip.h"
#ifdef BB_ABLATE  // a diagnostic build (make EXTRA=-DBB_ABLATE)?  Asked here: bb_kernels.hip.h defines the macro's function form in every build
constexpr bool kAblateBuild = true;
#else
constexpr bool kAblateBuild = false;
#endif
#include "bb_kernels.hip.h"
#include "bb_own.h"
#include "bb_pack.h"
#include "bb_ui_kernels.hip.h"

using namespace bbr;

namespace {

std::string g_create_error;

// RCCL, opened once per process at the first bbr_comm_unique_id / bbr_comm_init and never closed (it owns threads): the
// single-GPU path loads and runs without it.
struct Rccl {
  void *lib = nullptr;
  decltype(&ncclGetUniqueId) get_unique_id = nullptr;
  decltype(&ncclCommInitRank) comm_init_rank = nullptr;
  decltype(&ncclAllGather) all_gather = nullptr;
  decltype(&ncclCommDestroy) comm_destroy = nullptr;
  decltype(&ncclCommCount) comm_count = nullptr;
  decltype(&ncclGetErrorString) error_string = nullptr;
};
Rccl g_rccl;
std::mutex g_rccl_mutex;

// (Mesh, Material: move-only through their buffers; `m = Mesh()` frees a handle)
struct Mesh {
  DeviceBuffer<Vertex> d_vertices;
  DeviceBuffer<uint32_t> d_indices;
  uint32_t n_vertices = 0, n_indices = 0;
  bool alive = false;
};

struct Material {
  DeviceBuffer<uint8_t> d_texels[kMapCount];
  DeviceBuffer<uint8_t> d_packed;
  DeviceBuffer<uint8_t> d_chain;  // option "mip_levels" >= 2: levels >= 1 of every supplied map and of the packed form, one allocation
  MipTable mip = {};           // where every level of every set starts (valid while "mip_levels" >= 2)
  MaterialDesc desc = {};
  bool alive = false;
};

struct RecordedDraw {
  int32_t mesh, material;
  uint32_t n_instances, first_instance, first_prim, tris_per_instance;
};
// A draw list on the device as k_geometry takes it: the descriptors (fill_draw_descs), how many, first_prim of draws 1 .. 3, the primitives of all
struct DeviceDraws {
  const DrawDesc *d = nullptr;
  uint32_t n = 0;
  FirstPrims first_prims = {};
  uint32_t n_prims = 0;
};

// Where a transfer of draws keeps its parts, computed once from the counts: [lights | draw descriptors | instances | item head |
// caster table] in a frame's staging (`frame`), [descriptors | instances] alone in a synchronous pass's.  The accessors give the
// typed view of one part of a block laid out so: the pinned staging or its device copy.
struct StagingLayout {
  size_t draws_offset, inst_offset, inst_bytes, head_offset, table_offset, total;
  // [item head: one zero word, 16-byte slot]: k_raster's tiles count a short frame's items through it.  [caster table]: once a queued pass has
  // changed a slot: the context's table is written only while nothing is in flight, and the frames in flight differ in the generations they read
  StagingLayout(size_t n_descs, size_t n_instances, bool frame = false, bool carries_table = false) {
    draws_offset = frame ? sizeof(Light) * kMaxNumLights : 0;
    inst_offset = draws_offset + ((sizeof(DrawDesc) * n_descs + 127) & ~(size_t)127);
    inst_bytes = sizeof(InstanceBlock) * n_instances;
    head_offset = (inst_offset + inst_bytes + 15) & ~(size_t)15;
    table_offset = (head_offset + 16 + 255) & ~(size_t)255;
    total = carries_table ? table_offset + sizeof(ShadowCasterTable) : frame ? head_offset + 16 : inst_offset + inst_bytes;
  }
  Light *lights(uint8_t *block) const { return reinterpret_cast<Light *>(block); }
  DrawDesc *descs(uint8_t *block) const { return reinterpret_cast<DrawDesc *>(block + draws_offset); }
  InstanceBlock *instances(uint8_t *block) const { return reinterpret_cast<InstanceBlock *>(block + inst_offset); }
  uint32_t *item_head(uint8_t *block) const { return reinterpret_cast<uint32_t *>(block + head_offset); }
  ShadowCasterTable *caster_table(uint8_t *block) const { return reinterpret_cast<ShadowCasterTable *>(block + table_offset); }
};

// Host -> device copies that kernels on the (non-blocking) context streams read right afterwards: completed on the
// NULL stream before returning, for the reason given at zero_fill_sync (bb_own.h).
inline hipError_t upload_sync(void *dst, const void *src, size_t bytes) {
  hipError_t e = hipMemcpy(dst, src, bytes, hipMemcpyHostToDevice);
  if (e == hipSuccess) e = hipStreamSynchronize(nullptr);
  return e;
}

// What the options in force mean for a frame: decided in frame_mode (below) and nowhere else.  ensure_slot_buffers allocates
// from it, launch_frame takes its pointers from it, and the slot keeps it for the read-backs.  The default is "no frame".
struct FrameMode {
  int n = 1;             // option "supersample": samples per output pixel along each axis
  bool resolve = false;  // n >= 2: the kernels up to shading write the fine frame (library-owned), k_resolve the output
  bool merged = false;   // ... with option "sample_shading" 0: a sample map, k_sample_merge, k_resolve_merged
  bool depth = false;    // option "overlays": the frame keeps its depth for bbr_draw_overlays (whole frame; n >= 2: a rule)
  int depth_rule = 0;    // n >= 2: option "depth_resolve" (0: no depth is kept; else k_resolve_depth's MODE, VkResolveModeFlagBits)
  bool shadow = false;   // option "shadow_map" > 0 and a map has been rendered (bbr_render_shadow_map): k_shade_shadow shades
  bool shadow_faces = false;  // ... two or more of them (bbr_render_shadow_faces): k_shade_shadow_faces
  int shadow_filter = 0;      // ... and option "shadow_filter" R >= 1: k_shade_shadow_pcf, whatever the number of faces
  bool shadow_casters = false;  // ... a caster slot other than 0 is in use (bbr_render_shadow_caster): k_shade_shadow_casters, whatever F and R
  bool fused = false;    // option "present_fused": the frame is written as presented RGBA8 (the slot's d_present) ...
  bool shade_presents() const { return fused && !resolve; }   // ... by k_raster / k_shade
  bool resolve_presents() const { return fused && resolve; }  // ... by k_resolve (a presented byte cannot be averaged): then
  bool frame32() const { return !resolve_presents(); }        //     there is no W x H fp32 frame at all
  size_t out_rows = 0, fine_pixels = 0, map_words = 0;  // output rows (a shard's padding included); resolve: fine pixels; merged: the map in 8-byte words
};
inline size_t sample_map_word_bytes(int n) { return n == 2 ? sizeof(SampleMap<2>::Word) : sizeof(SampleMap<4>::Word); }

// A ring of (start, stop) event pairs around one kind of launch while option "timing" is on, with the number of launches
// since the last reset.  The events are made on demand and live as long as the context.
constexpr uint32_t kRingCap = 512;
// `n` timing events in `events`, made where there are fewer (plain ones, as hipEventCreate makes them)
inline hipError_t ensure_events(std::vector<Event> &events, size_t n) {
  events.reserve(n);
  for (Event e; events.size() < n; events.push_back(std::move(e)))
    if (hipError_t err = e.ensure()) return err;
  return hipSuccess;
}
struct PairRing {
  std::vector<Event> events;
  uint32_t launches = 0;
  hipError_t ensure() { return ensure_events(events, 2 * kRingCap); }
  hipEvent_t start(uint32_t i) const { return events[2 * (i % kRingCap)]; }
  hipEvent_t stop(uint32_t i) const { return events[2 * (i % kRingCap) + 1]; }
  hipError_t begin(hipStream_t st) { return hipEventRecord(start(launches), st); }
  hipError_t end(hipStream_t st) { return hipEventRecord(stop(launches++), st); }
  void reset() { launches = 0; }
};

// A run-time choice as a compile-time constant: f(std::true_type or std::false_type), f(std::integral_constant<int, n>)
template <class F> void with_bool(bool b, F &&f) { b ? f(std::true_type{}) : f(std::false_type{}); }
template <class F> void with_samples(int n, F &&f) {  // n = 2, 3 or 4
  n == 2 ? f(std::integral_constant<int, 2>{}) : n == 3 ? f(std::integral_constant<int, 3>{}) : f(std::integral_constant<int, 4>{});
}
template <class F> void with_tile(int tile_mode, F &&f) {  // option "tile_mode": the side of the square tiles, 64 or 32
  tile_mode == 0 ? f(std::integral_constant<int, 64>{}) : f(std::integral_constant<int, 32>{});
}

template <class F> void with_depth_rule(int rule, F &&f) {  // option "depth_resolve": 1, 4 or 8
  rule == kDepthZero ? f(std::integral_constant<int, kDepthZero>{})
                     : rule == kDepthMin ? f(std::integral_constant<int, kDepthMin>{}) : f(std::integral_constant<int, kDepthMax>{});
}

}  // namespace

// A group of members stated once, at its declaration: dropping the group is assigning a fresh one, so a new buffer needs its
// declaration and nothing else.
template <class Group, class Whole> void drop(Whole &w) { static_cast<Group &>(w) = Group(); }

// What a slot holds that is sized by the tile grid: option "tile_mode" drops it (bins and fragment lists are laid out per
// tile, and ensure() zeroes the fresh counters), and so does whatever drops the ExtentSized group.
struct TileSized {
  DeviceBuffer<uint32_t> d_tile_count;
  DeviceBuffer<uint32_t> d_bins;
  DeviceBuffer<unsigned long long> d_frags;  // per tile: compacted (pixel << 32 | primitive ref) of covered pixels
  DeviceBuffer<uint32_t> d_frag_count;       // per tile; behind the counts, option "sky_keep": k_raster's word per tile (sky_words)
  DeviceBuffer<uint32_t> d_items;       // k_shade's work list: [0] = count, then slot << 6 | chunk of 64 fragments
  DeviceBuffer<CookedLight> d_cooked;   // the frame's light table as the light loop consumes it (k_shade_items -> k_shade)
  DeviceBuffer<uint32_t> d_heavy;       // the frame's heavy-tile list (k_geometry -> k_raster; option "heavy_tiles")
  DeviceBuffer<uint32_t> d_item_groups; // 64-fragment chunks per group of 256 launch slots (k_raster -> k_shade_items)
  DeviceBuffer<float4> d_surface_keep;  // option "surface_keep": the slot's kept surface (k_surface_store -> k_shade_lit), from its first storing frame
};

// Option "sky_keep": what a slot remembers about the background in its d_frame.  While `stamp` is non-zero, a tile whose word
// behind the slot's fragment counts carries it holds the clear colour in every pixel of the buffer described by the other members (k_raster's
// light-tile path establishes that, and nothing else).  The stamp is kept from frame to frame only while the next frame goes
// into that same buffer in a mode that may keep (sky_stamp_for); forgetting is asking for a fresh one, which no word holds.
struct SkyKeep {
  uint32_t stamp = 0;        // 0: nothing is remembered
  uint32_t used = 0;         // the stamp the slot's last frame ran under (0: it kept nothing and marked nothing): bbr_read_sky_tiles
  const void *out = nullptr, *state = nullptr;  // the frame and the state buffer the stamp speaks of
  int32_t width = 0, height = 0, tiles_x = 0, tiles_y = 0, tile_mode = -1;
};
// What k_record_static, k_geometry, k_raster, k_sample_merge and k_shade_items make a main frame's visibility from, beside the
// slot's buffers: stated here and nowhere else.  submit_frame_body builds one per frame (frame_shape), launch_visibility takes every
// geometry-side value from it, and option "view_keep" compares it with the slot's (same_inputs): a new input is a new member.
struct FrameInputs {
  Mat4 pv = {}, view = {};
  FrameParams fp = {};  // the final ones (capacities, heavy rows)
  DeviceDraws draws;    // (their contents: plan_static_records' keys)
  int tile_mode = -1, grid_y = 0;  // (the rows of k_raster's screen-ordered grid)
  uint32_t max_items = 0;     // the item slots of the frame
  bool short_frame = false;   // no k_shade_items launch: k_raster's tiles append their items through the head word
  uint32_t *item_head = nullptr;  // that word, in the slot's device staging
};
// Option "view_keep": what a slot remembers about the visibility in its buffers.  While `valid`, the slot's geometry-side
// buffers (tris, records, bins, every-tile list, clip slots, fragment lists and counts, items, item count) and the background
// pixels of its d_frame are those of a complete frame rendered from exactly the inputs below: a frame with the same inputs
// launches its shading only (launch_frame's kept branch).  Set by every full frame that may be kept behind (submit_frame_body),
// left alone by a kept one; whatever touches the image or the lists outside launch_frame forgets (FrameSlot::forget_visibility).
struct VisKeep {
  bool valid = false;
  bool kept_last = false;  // the slot's last frame was a kept one (bbr_read_sky_tiles: it stored into no background tile)
  FrameInputs in;          // what the visibility was made from beside the draws' contents (those: plan_static_records' keys)
  std::array<const void *, 15> buffers = {};  // the buffers that hold it
};

// Option "surface_keep": what a slot remembers about the surface in its d_surface_keep (TileSized: dropped with the lists it
// mirrors).  While `valid`, entry [item * 64 + lane] of the buffer holds what light_surface receives for the fragment slot
// k_shade's wave `item` shades in lane `lane`, for all `items` items of the visibility in the slot's buffers (VisKeep), filtered
// under `normal_map` and `all_packed`: a kept frame under the same two launches k_shade_lit on it in place of k_shade.  `run`:
// the kept frames in a row that could have been lit, under one `normal_map`: the n-th of them is the storing frame
// (submit_frame_body).  Whatever forgets the visibility forgets the surface (FrameSlot::forget_visibility); so does a kept frame
// that takes another shading kernel, and a full frame.
constexpr int kSurfaceKeepDefault = 64;
struct SurfaceKeep {
  bool valid = false;
  uint32_t run = 0;
  int32_t normal_map = 0;   // enable_normal_map of the slot's last frame: what the run counts under, and the surface was made with
  bool all_packed = true;   // ... and bbr_context::all_packed
  const void *buffer = nullptr;  // where it lives (d_surface_keep.ptr when it was stored)
  uint32_t items = 0;       // the exact item count it was stored for, and the buffer's item capacity
  void forget() { valid = false, run = 0; }
};

// ... by the render or the output extent: bbr_resize and option "supersample" drop it (drop_extent_buffers)
struct ExtentSized {
  DeviceBuffer<float4> d_frame;
  DeviceBuffer<float4> d_fine;        // option "supersample" >= 2: the fine frame k_resolve reads (always library-owned)
  DeviceBuffer<unsigned long long> d_sample_map;  // option "sample_shading" 0: the frame's sample map (k_sample_merge ->
                                      // k_resolve_merged), one word of 2 (n = 2) or 8 (n = 4) bytes per output pixel
  DeviceBuffer<float> d_depth;        // option "overlays": the frame's resolved depth, for bbr_draw_overlays
  DeviceBuffer<float> d_fine_depth;   // ... with n >= 2 and a rule: k_raster's depth of the render extent (k_resolve_depth -> d_depth)
  DeviceBuffer<uint32_t> d_present;   // RGBA8 presented image of this slot's frame (bbr_present)
  DeviceBuffer<float4> d_bloom;       // option "bloom" >= 1: the slot's pyramid, levels 1 .. L one behind the other (from its first bloomed present)
};

// Option "static_records": what a slot knows about the camera-independent part of the records in its d_attrs.  One entry
// per live draw of the frame last submitted to the slot, in draw order: the descriptor k_geometry was given (its instance
// blocks are still in the slot's pinned staging, where `key.instances` points in the device copy) and whether k_record_static
// has written the draw's static part since.  Whatever destroys or replaces record bytes forgets the entries.
struct StaticRecords {
  struct Draw {
    DrawDesc key;  // (flags 0)
    bool filled;
  };
  std::vector<Draw> draws;
  uint64_t epoch = 0;  // bbr_context::resource_epoch the keys were taken under
  // capacities of d_attrs and of the staging the keys speak of: both buffers only ever grow, and growing loses what they held
  size_t attrs_cap = 0, staging_cap = 0;
  void forget() { draws.clear(); }
};

// What a call asks for in one caster slot (check_caster_request): the synchronous calls render it at once.
// bbr_queue_shadow_caster keeps it as what the recorded frame asked for (ShadowOwned::queued): it belongs to the recorded frame like
// its draws: bbr_begin_frame forgets it, every submission of the frame (bbr_end_frame, a replay, a re-render) renders it again.
struct CasterRequest {
  bool on = false;  // (queued)
  int32_t light = 0, faces = 0;
  float bias = 0.f;
  ViewUniformBlock view[kMaxShadowFaces];
};
// A queued pass as the frame in a slot carried it: which caster slot, the request, and the stamp the slot got from it (the
// slot still holds this request while its stamp is this one).  Kept so that the pass can be rendered again from the frame's
// draws, which stay in the slot's device staging until its next frame (settle_queued_passes).
struct CarriedPass {
  int caster = 0;
  uint32_t stamp = 0;
  CasterRequest q;
};

// Everything one frame in flight owns.  What is in neither group survives an option change and a resize.
struct FrameSlot : TileSized, ExtentSized {
  StaticRecords statics;
  PinnedBlock<uint8_t> h_staging;  // pinned: lights, draw descriptors, instances
  PinnedBlock<uint32_t> h_flags;   // pinned, device-visible: the kHostFlagWords words of HostFlagWord (bb_types.h), stored by the kernels
                                   // of the frame last rendered in this slot and read when the slot's next frame is submitted
  DeviceBuffer<uint8_t> d_staging;
  DeviceBuffer<RasterTri> d_tris;
  DeviceBuffer<ShadeRec> d_attrs;
  DeviceBuffer<ClipSlot> d_clip;
  int ctr_index = 0;                        // the slot's counter block (slot index; the overlay slot has the last one)
  DeviceBuffer<BlockStats> d_block_stats;  // one record per k_geometry wave
  DeviceBuffer<BroadTri> d_broad;
  DeviceBuffer<float4> d_background;  // deferred path: colour of the pixels no geometry covers
  FrameMode mode;                     // of the frame in this slot: which of the buffers above hold it (fused: d_present, d_frame nothing)
  FrameUniformBlock frame_u = {};     // the uniforms the frame in this slot was rendered with (overlays need them)
  ViewUniformBlock view_u = {};
  struct {
    bool active = false;  // bbr_present was queued for the frame in this slot (re-queued if the frame is replayed)
    uint32_t *out = nullptr;
    void *copy_to = nullptr;  // fused presentation: the caller's buffer the image was copied to
    int32_t enable = 0, hdr16 = 1;
    float exposure = 1.f;
    // option "auto_exposure": the presentation was queued under it (the image is made with the exposure in the slot's record),
    // and the frame has been metered (a presentation the library repeats converts with that exposure again and meters nothing)
    bool auto_e = false, metered = false;
  } present;
  int bloom_ran = 0;  // the levels of the chain that last ran on d_bloom for the frame in this slot (0: none; bbr_read_bloom_level)
  Event ev_geom_done, ev_raster_done, ev_tail_done;  // edges between the streams of a frame
  // Everything queued on this slot's image so far: the frame's k_shade, then whatever was put behind it (presentation, the
  // GUI pass, a copy to the caller's buffer, the exchange).  Work on the image goes between follow() and busy_until().
  Event ev_done;
  // `st` follows everything queued on the slot so far.  (Also needed on the slot's own stream once something ran elsewhere:
  // a separate presentation pass may have run on another stream and moved the event there.)
  hipError_t follow(hipStream_t st) const { return hipStreamWaitEvent(st, ev_done, 0); }
  // the slot is busy until what `st` holds now
  hipError_t busy_until(hipStream_t st) { return hipEventRecord(ev_done, st); }
  bool idle() const { return hipEventQuery(ev_done) == hipSuccess; }  // (hipErrorNotReady: still on the GPU)
  hipError_t wait_idle() const { return hipEventSynchronize(ev_done); }  // the host waits
  // GUI pass (bbr_draw_ui) of the frame in this slot: pinned staging [commands | vertices | indices], its device copy and
  // the per-triangle records; ev_copied says the staging may be written again
  struct {
    PinnedBlock<uint8_t> h_staging;
    DeviceBuffer<uint8_t> d_staging;
    DeviceBuffer<UiTri> d_tris;
    DeviceBuffer<UiBox> d_boxes;
    Event ev_copied;
    bool copy_pending = false;
  } ui;
  bool in_flight = false;
  // per caster slot, the map generation the frame in this slot reads (ShadowSlot::cur at its submission), -1: none.  While
  // the frame is on the GPU no queued pass writes that generation (pick_generation).
  int8_t shadow_gen[kMaxShadowCasters] = {-1, -1, -1, -1, -1, -1, -1, -1};
  bool had_pass = false;       // the frame in this slot carried a queued shadow pass (its overflow words include the pass's)
  std::vector<CarriedPass> carried;  // ... these
  // The draw list of the frame in this slot, in d_staging: valid only until the slot's next submission replaces the staging (until
  // then the carried passes can be rendered again from it, settle_queued_passes; `d` is null once that staging was reallocated)
  DeviceDraws draws;
  uint64_t serial = 0;         // the order of submission among the context's frames
  float4 *out_used = nullptr;  // where the frame in this slot wrote its pixels
  hipStream_t stream_used = nullptr;  // the stream its k_shade ran on

  // The flag words describe frames rendered with the old capacities (apply_growth) / the old extent (bbr_resize).  Two sets,
  // kept apart as they were; the heavy-tile count survives both (a list that does not fit its rows is merely not used).
  void forget_capacities() {
    if (uint32_t *f = h_flags.ptr)
      f[kFlagOverflow] = f[kFlagBinNeed] = f[kFlagItemCount] = f[kFlagBroadNeed] = f[kFlagClipNeed] = f[kFlagPassBroadNeed] = f[kFlagPassClipNeed] = 0u;
  }
  void forget_extent() {
    if (uint32_t *f = h_flags.ptr) f[kFlagOverflow] = f[kFlagBinNeed] = f[kFlagItemCount] = 0u;
  }
  // Option "sky_keep": something other than this slot's own k_raster / k_shade may have written its frame, or the frame or
  // the state words are not the ones the stamp speaks of.  The rule for every entry point that touches a slot's image or its
  // buffers outside launch_frame: call this (forget_image(c) does it for every slot, with what stands below).  Touches no memory: the slot's next
  // frame runs under a fresh stamp, fills every sky tile and keeps again from the frame after.
  SkyKeep sky;
  void forget_sky() { sky.stamp = 0; }
  // Option "view_keep": the same rule, and besides for whatever touches, frees or re-reads under other inputs the slot's
  // geometry-side buffers (a capacity growth, a diagnostic re-render, a dropped buffer group): the slot's next frame is
  // rendered in full.  An entry point that touches the image forgets both (forget_image).
  VisKeep vis;
  SurfaceKeep surf;  // option "surface_keep": rests on `vis`
  void forget_visibility() { vis.valid = false, surf.forget(); }
  void forget_image() { forget_sky(), forget_visibility(); }
  // native exchange (bbr_allgather_frame / bbr_push_shard) with library-owned buffers: every rank's block, the whole frame
  DeviceBuffer<uint8_t> d_gathered, d_whole;
};

// The streams the kernels of one frame run on (bbr_context::frame_streams).
struct FrameStreams {
  hipStream_t geom, raster, shade;
};

// Live contexts: a scene object (bb::SceneBase, bbs_scene) frees its meshes through the context it was created on; if
// the host destroys the context first (garbage collectors do), those late calls must fail cleanly instead of touching
// freed memory.
namespace {
std::mutex g_live_mutex;
std::unordered_set<const bbr_context *> g_live;
bool is_live(const bbr_context *c) {
  std::lock_guard<std::mutex> lock(g_live_mutex);
  return g_live.count(c) != 0;
}
}  // namespace

// The context's buffers of the output or the render extent: the dumps of the read-backs.  drop_extent_buffers drops the group.
struct ExtentDumps {
  DeviceBuffer<uint32_t> d_vis_prim;  // bbr_read_visibility's dump, width x height (n >= 2: resolved by k_resolve_depth from ...
  DeviceBuffer<float> d_vis_depth;
  DeviceBuffer<uint32_t> d_vis_fine_prim;  // ... k_raster's dump of the render extent: bbr_read_sample_visibility)
  DeviceBuffer<float> d_vis_fine_depth;
  DeviceBuffer<uint2> d_gbuffer;  // width*height*4 (four RGBA16F texels per pixel), only while bbr_read_gbuffer runs
  DeviceBuffer<uint8_t> d_shadow_mask;  // width*height classes, only while bbr_read_shadow_mask runs
  DeviceBuffer<uint8_t> d_shadow_face;  // width*height deciding faces, only while bbr_read_shadow_face_index runs (F >= 2)
  DeviceBuffer<uint8_t> d_shadow_taps;  // width*height lit-tap counts, only while bbr_read_shadow_taps runs ("shadow_filter" >= 1)
};

// Option "shadow_map": everything the feature owns.  Changing the option's value drops the group; at 0 nothing of it exists.
// One caster slot (bbr_render_shadow_caster): its maps and what the shading kernels get of it.
// What a slot publishes to the frames: everything a submission may change of it (publish), and what a failed one puts back
// by assignment (submit_frame_into).  A member that a submission changes belongs here.
struct CasterPublished {
  bool valid = false;             // in use: the maps have been rendered since the option was set, and not dropped
  int cur = 0;                    // the generation args.map points to
  uint32_t stamp = 0;             // a new value with every request that makes the slot valid (bbr_context::caster_stamp): CarriedPass
  ShadowFacesArgs args = {};      // what every frame's k_shade_shadow (F = 1: its first matrix) or k_shade_shadow_faces gets:
                                  // M_f, the maps, S, F, the caster's index, the bias
};
struct ShadowSlot : CasterPublished {
  CasterPublished &published() { return *this; }
  DeviceBuffer<float> d_map;      // the maps: F x S x S depths, face f row-major at f * S * S (k_raster's depth store)
  // Queued passes (bbr_queue_shadow_caster): further GENERATIONS of the maps, d_map being generation 0.  A frame reads the
  // generation that was current when it was submitted (FrameSlot::shadow_gen); a queued pass writes one no frame on the GPU
  // reads (pick_generation), which then is the current one.  The synchronous pass writes generation 0: nothing is in flight.
  static constexpr int kGenerations = 4;  // the frame slots: of n frames in flight, n - 1 can hold a generation against the n-th
  DeviceBuffer<float> d_more[kGenerations - 1];
  DeviceBuffer<float> &generation(int g) { return g == 0 ? d_map : d_more[g - 1]; }
};
struct ShadowOwned {
  FrameSlot pass;                 // the map pass's own little frame (k_geometry -> k_raster at S x S), like the overlay pass's
  ShadowSlot slot[kMaxShadowCasters];  // slot 0: the caster of bbr_render_shadow_map / bbr_render_shadow_faces
  CasterRequest queued[kMaxShadowCasters];
  // The queued passes of all frames share `pass`, the sink and the counter blocks: ev_pass is recorded behind each (its
  // k_shadow_pass_retire), the next one waits for it on its stream, and so does the shading of every frame from then on -- a
  // frame that queues nothing may read maps that the pass of the frame before it, on another stream, is still writing.
  Event ev_pass;
  bool pass_queued = false;       // a queued pass has been submitted since the group was made: ev_pass is recorded
  bool table_stale = false;       // ... and has changed a slot since d_table was written: frames carry the table in their staging
  struct { uint32_t n_prims = 0, bin_cap = 0, broad_cap = 0, clip_cap = 0; int tile_mode = -1; } pass_sized;  // what `pass` was last sized for
  DeviceBuffer<uint32_t> d_sink;  // S x S words k_raster's background stores go to; nothing reads them (one for all faces)
  DeviceBuffer<Counters> d_ctr;   // a counter block per face (of every queued slot: kShadowPassBlocks): the faces run back to back and are read after one wait
  // what k_shade_shadow_casters reads: every slot's entry and the light -> slot lookup.  It exists from the first use of a slot
  // other than 0, and is written by the synchronous render / drop calls only, while no frame is in flight.
  DeviceBuffer<ShadowCasterTable> d_table;
  bool any() const {
    for (const ShadowSlot &s : slot) if (s.valid) return true;
    return false;
  }
  bool beyond_first() const {     // a slot other than 0 is in use: k_shade_shadow_casters
    for (int s = 1; s < kMaxShadowCasters; ++s) if (slot[s].valid) return true;
    return false;
  }
  ShadowArgs one_face() const {   // (slot 0 alone, F = 1)
    const ShadowFacesArgs &args = slot[0].args;
    ShadowArgs a = {};
    a.m = args.m[0], a.map = args.map, a.side = args.side, a.light = args.light, a.half = args.half, a.bias = args.bias;
    return a;
  }
};

struct bbr_context : ExtentDumps {
  int device = 0;
  int32_t width = 0, height = 0;  // the OUTPUT extent: what every output, shard, present, exchange, GUI and caller buffer is sized by
  // option "supersample": everything up to and including shading (tiles, bins, fragment lists, items, the viewport, the flag
  // words) works on the render extent n * width x n * height; k_resolve brings the fine frame to the output extent
  int supersample = 1;
  // option "sample_shading": 1 = every sample of the fine frame is shaded; 0 = one fragment per primitive and output pixel
  // (k_sample_merge, k_resolve_merged).  Stored at any "supersample", in effect with n >= 2; the pair (3, 0) is refused.
  int sample_shading = 1;
  // option "depth_resolve": which sample of a block gives the output pixel its depth and winner (VkResolveModeFlagBits: 0 none,
  // 1 SAMPLE_ZERO, 4 MIN, 8 MAX).  Stored at any "supersample", in effect with n >= 2 (frame_mode).
  int depth_resolve = 0;
  int32_t render_width() const { return width * supersample; }
  int32_t render_height() const { return height * supersample; }
  Stream s_geom, s_raster, s_shade, s_present;  // context-owned streams (declared first, so destroyed last: behind every event and buffer)
  hipStream_t user_stream = nullptr;                 // bbr_set_stream: everything on the caller's stream, 1 frame in flight
  std::string last_error;

  std::vector<Mesh> meshes;
  std::vector<Material> materials;
  DeviceBuffer<uint8_t> d_default_texels;  // 6 x RGBA8 (1x1 default maps)
  DeviceBuffer<MaterialDesc> d_materials;
  bool materials_dirty = true;
  bool all_packed = true;  // every live material has a packed form (k_shade's MIXED = false instantiation may be used)

  FrameUniformBlock frame_u = {};
  ViewUniformBlock view_u = {};

  bool in_frame = false, have_frame = false;
  std::vector<RecordedDraw> draws;
  std::vector<InstanceBlock> host_instances;
  uint32_t n_prims = 0;

  static constexpr int kMaxSlots = 4;
  // one per frame slot + one for the overlay pass + a spare one: what the shading of a kept frame (option "view_keep") retires
  // in place of its slot's block, whose retired copy stays the full frame's
  static constexpr int kCounterBlocks = kMaxSlots + 2;
  static constexpr int kSpareCounterBlock = kMaxSlots + 1;
  FrameSlot slots[kMaxSlots];
  DeviceBuffer<Counters> d_counters;       // zero between frames: a frame's k_shade clears its slot's block ...
  DeviceBuffer<Counters> d_counters_done;  // ... after copying it here (statistics, overflow check)
  int frames_in_flight = 2;
  uint64_t frame_counter = 0;
  int last_slot = -1;

  DeviceBuffer<SrgbTables> d_srgb_tables;  // thresholds t_k (linear value at which the sRGB byte becomes k) + the keyed table
  struct UiTexture {
    DeviceBuffer<uint32_t> d_texels;  // RGBA8, row-major
    int32_t w = 0, h = 0;
  };
  std::vector<UiTexture> ui_textures;  // bbr_upload_ui_texture: handle = index + 1, a freed one has no texels
  DeviceBuffer<float> d_ui_dec;        // the blend's decode table (ui_dec_table)
  void *ext_out = nullptr;
  uint64_t ext_out_bytes = 0;

  int tile_mode = 1;  // 0: 64x64, 1: 32x32 (default: finer tiles balance better; 16x16 with one-wave workgroups measured slower)
  uint32_t bin_cap = 512, broad_cap = 4096, clip_cap = 4096, broad_threshold = 16;
  int32_t rank = 0, world = 1, band_rows = 0;
  bool dump_vis = false;
  bool present_fused = false;  // option "present_fused": frames are written as presented RGBA8, no fp32 frame
  bool overlays = false;  // option "overlays": frames keep their depth so that bbr_draw_overlays can test against it
  Mesh marker_mesh, gizmo_mesh;  // generateUVSphereMesh(0.1, 16, 16) and the caller's gizmo, both as Vertex meshes
  FrameSlot ov;           // buffers of the overlay pass (its own little frame)
  bool tbn = false;       // option "tbn": bbr_draw_overlays first draws the TBN lines of the last frame (tbn.vert/.geom/.frag)
  struct TbnRecords {  // what drop_extent_buffers drops of the pass (its records were snapped to the old extent)
    DeviceBuffer<uint8_t> d_staging;   // the frame's draw descriptors + instances
    DeviceBuffer<TbnSeg> d_segs;       // eight slots per primitive (slot = key)
    DeviceBuffer<uint32_t> d_tile_count, d_bins, d_ctr;
    DeviceBuffer<uint32_t> d_keys;     // per pixel: key + 1 of the winning segment, 0 = none
    uint32_t n_slots = 0;
    bool valid = false;                // d_segs holds the records of the last TBN draw
  };
  struct TbnPass : TbnRecords {
    uint32_t bin_cap = 1024;           // bin entries per 32 x 32 tile (grows on overflow)
  } tbn_pass;
  int gbuffer_view = -1;  // option "gbuffer_view": GBufferVisualizingOption (src/scene.h:27-35) while the deferred path runs
  bool deferred = false;  // option "render_pass": the reference's deferred path (its default) instead of the forward one
  bool dump_gbuffer = false;
  int max_anisotropy = 1;         // option "max_anisotropy": 1 = k_shade's bilinear tap, 2..16 = k_shade_aniso
  int mip_levels = 1;             // option "mip_levels": 1 = no chain, the kernels above; 2..15 = chains of up to that many levels, k_shade_mip
  DeviceBuffer<MipTable> d_mip_tables;  // one per material slot, beside d_materials (only while "mip_levels" >= 2)
  int shadow_map = 0;             // option "shadow_map": 0 = off, 1..8192 = the side S of the map (k_shade_shadow once a map exists)
  ShadowOwned shadow;
  int shadow_filter = 0;          // option "shadow_filter": 0 = the hard compare, 1..2 = the radius R of the box (k_shade_shadow_pcf)
  bool dump_shadow_mask = false;  // (bbr_read_shadow_mask: together with dump_surface, the DUMP form of k_shade_shadow)
  int dump_shadow_slot = 0;       // (... the caster slot k_shade_shadow_casters' DUMP form dumps)
  bool dump_surface = false;
  DeviceBuffer<float> d_surface;  // width*height*32 floats, only while bbr_read_surface runs
  // option "static_records": 1 = a draw whose key repeats in a slot has the camera-independent part of its records written
  // once (k_record_static) and k_geometry's light path from then on; 0 = always the full path
  bool static_records = true;
  // option "sky_keep": 1 = a tile that was background when its frame slot rendered last, and is background again, is not
  // filled again (k_raster's light-tile path, SkyKeep); 0 = every frame stores every background pixel
  bool sky_keep = true;
  // option "view_keep": 1 = a frame whose view, draws and geometry parameters are those its frame slot rendered last launches
  // its shading only (VisKeep, launch_frame's kept branch); 0 = every frame runs every stage
  bool view_keep = true;
  uint64_t view_kept_frames = 0, view_full_frames = 0;  // bbr_view_keep_counts: main frames submitted either way
  // option "surface_keep": 0 = off; n >= 1 = a slot's n-th kept frame in a row that takes the plain k_shade stores the slot's
  // surface (k_surface_store), and it and every such frame behind it are shaded from it (k_shade_lit; SurfaceKeep).  The default
  // is the smallest power of two for which a stop of the camera that ends right behind its stores loses at most 5 %: DESIGN.md section 5
  int surface_keep = kSurfaceKeepDefault;
  uint64_t surface_stored_frames = 0, surface_lit_frames = 0;  // bbr_surface_keep_counts: storing frames; frames k_shade_lit shaded (those included)
  bool dump_records = false;    // (bbr_read_records: its frame shows what k_geometry's full path writes, and what it leaves alone)
  // Bumped by every call that can change what a mesh or material handle, or a pointer taken from one, means (upload and free
  // of either, the material table, the mip chains): a freed and reused address never compares equal to its former self.
  uint64_t resource_epoch = 1;
  uint64_t static_fills = 0, static_light_draws = 0;  // k_record_static launches; draws submitted on the light path
  // bbr_shadow_queue_counts: queued passes submitted (one per queued slot and submission of its frame), and how often a
  // frame had to drain the context because of one (an overflowed pass seen in a slot's pinned words).  They outlive `shadow`.
  uint64_t shadow_queue_passes = 0, shadow_queue_drains = 0;
  uint32_t caster_stamp = 0;   // ShadowSlot::stamp's source
  uint64_t frame_serial = 0;   // FrameSlot::serial's source
  uint32_t ablate = 0;
  int n_cus = 256;         // compute units of the device (hipDeviceProp_t::multiProcessorCount)
  int timing = 0;  // 0 off, 1 five events per frame, 2 only the two events around k_shade
  int timing_stride = 1;  // option "timing_stride": events on every n-th frame only (two events a frame cost ~4 % at C3)
  uint64_t timing_tick = 0;
  // timing ring: (frame start, geometry done, raster done, shade start, shade done) per frame since the last reset
  std::vector<Event> ring;
  uint32_t ring_frames = 0;
  PairRing present_ring;  // around each k_present (k_present_bloom) while timing is on
  // option "bloom": 0 = k_present; 1..8 = the levels of the pyramid in front of k_present_bloom (the rule: bibim_hip.h "bloom")
  int bloom = 0;
  float bloom_threshold = 1.0f, bloom_intensity = 0.05f;  // bbr_set_bloom: stored at any "bloom"
  // bbr_present_buffer_bloom's pyramid: one for the context, so its calls are ordered one behind the other through ev_used
  // whatever their streams.  Dropped with the option's return to 0 and with the extent buffers.
  struct BloomBuffer {
    DeviceBuffer<float4> d_levels;
    Event ev_used;     // behind the last call's k_present_bloom
    bool used = false; // ... recorded
    int32_t w = 0, h = 0;
    int ran = 0;       // extent and levels of the last call's chain (0: none; bbr_read_bloom_level source 1)
  } bloom_buffer;
  PairRing bloom_ring;  // around each chain (k_bloom_first .. the last k_bloom_up) while timing is on
  // option "auto_exposure" (the rule: bibim_hip.h "auto exposure"): 1 = bbr_present meters the frame (k_luminance, k_exposure)
  // and converts it with the exposure that leaves on the device (k_present_auto / k_present_bloom_auto)
  int auto_exposure = 0;
  ExposureParams exposure_params = {0.18f, 0.0009765625f, 1024.0f, 1.0f, 500, 950};  // bbr_set_auto_exposure: stored at either value
  // Everything of the option on the device, alive while it is 1.  A "unit" is what one presentation in flight owns: a
  // histogram (zero between uses: k_exposure leaves it so) and a record; one per frame slot, and one (kBufferUnit) for
  // bbr_present_buffer_auto.  The two histories are shared by the presentations of a source, so their k_exposure are
  // ordered one behind the other on the device through an event, whatever their streams.
  struct ExposureOwned {
    static constexpr int kBufferUnit = kMaxSlots, kUnits = kMaxSlots + 1;
    DeviceBuffer<uint32_t> d_hist;            // kUnits x kLumaWords
    DeviceBuffer<ExposureRecord> d_records;   // kUnits
    DeviceBuffer<ExposureHistory> d_history;  // source 0 (bbr_present), source 1 (bbr_present_buffer_auto)
    Event ev_adapted;       // behind the k_exposure of source 0's last presentation
    bool adapted = false;   // ... recorded
    Event ev_buffer;        // behind the present kernel of the last bbr_present_buffer_auto (its unit is free again)
    bool buffer_used = false;
    int last_slot = -1;     // the slot of source 0's last presentation (bbr_read_exposure), -1: none
    uint32_t *hist(int unit) const { return d_hist.ptr + (size_t)unit * kLumaWords; }
    ExposureRecord *record(int unit) const { return d_records.ptr + unit; }
  } exposure;
  PairRing luminance_ring;  // around each k_luminance while timing is on (k_exposure falls into present_ring's interval)
  PairRing resolve_ring;  // around the k_resolve of each timed frame: pair i is ring frame i's (the two counts are reset together)
  static constexpr uint32_t kRingCap = ::kRingCap;
  static constexpr uint32_t kRingEvents = 5;
  int retries = 0;
  // host side of the frame loop since the last bbr_host_timing_reset (steady_clock; no GPU call is made to keep them):
  // frames submitted, time inside the submit (bbr_end_frame / bbr_replay_frame), and the part of it spent blocked because
  // the frame slot's previous frame had not left the GPU yet
  uint64_t host_frames = 0, host_submit_ns = 0, host_blocked_ns = 0, host_blocked_frames = 0;

  ncclComm_t comm = nullptr;
  int comm_rank = -1, comm_world = 0;
  int exchange_slot = -1, exchange_form = -1;  // where the last exchange left the whole frame (library-owned buffers)
  void *exchange_whole = nullptr;
  int push_mode = 1;  // option "push_mode": 1 one kernel storing to every peer (all links at once), 0 copies one after the other
  std::unordered_set<int> peer_mapped;  // devices whose memory this context's device can store to (peer access enabled)
  bool last_push_direct = false;
  int64_t no_tail_items = 40000;  // option "no_tail_items": frames with at most this many item slots get no tail launch
  // option "heavy_tiles": k_raster starts the tiles one of whose bins holds at least this many references before the
  // screen-ordered rest (long frames only; 0: plain screen order; -1, the default: 64 while ONE frame is in flight, 0
  // otherwise).  Measured at C3: k_raster alone 61.9 -> 51.0 us and a frame's latency 177 -> 167 us with 64 (48: the same;
  // 96 / 128 / 256: 58.7 / 61.0 / 61.4; 1 / 16 / 32: 55 / 54 / 53.5 and k_geometry +9 / +10 / +6 us for its appends) -- and
  // with three frames in flight the frame period 1-2 % LONGER (32: 7 %): the other frames' kernels fill the tail that
  // the order removes, and the light tiles' background stores then come in one burst instead of spread over the launch.
  int64_t heavy_tiles = -1;
  std::vector<hipEvent_t> pending_waits;  // bbr_wait_event: applied to the first stream of the next frame
  static constexpr int kLayouts = 3;
  int layout_mode = 2;  // option "stream_layout"
  bool pipelined() const { return !user_stream && frames_in_flight > 1; }
  hipStream_t slot_stream(int i) const { return i == 0 ? s_raster : (i == 1 ? s_shade : (i == 2 ? s_present : s_geom)); }
  // Outside a frame (synchronous passes, self-tests, waiting): the context's first stream, and the one shading runs on
  hipStream_t geom_stream() const { return user_stream ? user_stream : s_geom; }
  hipStream_t shade_stream() const { return user_stream ? user_stream : (frames_in_flight > 1 ? s_shade : s_geom); }
  // k_present is bandwidth-bound, k_shade issue-bound: on its own stream the presentation of frame N overlaps the
  // shading of frame N+1 instead of delaying it
  hipStream_t present_stream() const { return (user_stream || frames_in_flight == 1) ? shade_stream() : s_present; }
  // Stream layout of the frames in flight (option "stream_layout"), decided here and in slot_present_stream, nowhere else.
  // A caller's stream (bbr_set_stream) or one frame in flight: everything on one stream.  Otherwise all three render the
  // same bits:
  //   0  geometry + raster on s_geom, shade on s_shade, present on s_present          (stage streams)
  //   1  as 0, but k_raster on s_raster: geometry of frame N+1 need not wait for the raster of frame N.  At 1080p that
  //      chain -- not the GPU -- set the frame rate (C2: 72 -> 41 us per frame)
  //   2  every kernel of a frame (copy, geometry, raster, shade, present) on the stream of its slot: frames share
  //      nothing (each slot has its own buffers and counter block), so whole frames overlap and no event is needed
  //      inside a frame.  The four context streams double as the slot streams: a process that owns more than a
  //      handful of HIP streams gets slower as a whole -- with seven streams every layout lost 60 %
  // A plain option with a fixed default, 2: measured with three frames in flight (us per frame, layouts 0 / 1 / 2) it is
  // the fastest everywhere -- C2 1080p 84.5 / 67.1 / 37.3, C3 4K 191.5 / 153.6 / 148.6 -- because a frame's chain of
  // dependent kernels (copy -> geometry -> raster -> items -> shade) then only waits for itself.  (Round 1 timed the
  // layouts on the first ~500 frames of every workload and switched by itself; the measurement was fragile and made
  // the frame rate a function of history.)
  FrameStreams frame_streams(int slot) const {
    if (!pipelined()) return {geom_stream(), geom_stream(), geom_stream()};
    if (layout_mode == 2) return {slot_stream(slot), slot_stream(slot), slot_stream(slot)};
    return {s_geom, layout_mode == 1 ? s_raster : s_geom, s_shade};
  }
  // The stream the presentation and the GUI pass of the frame in `s` run on.  Layout 2: the slot's own stream, behind its
  // k_shade (the other slots' streams keep the GPU busy meanwhile); otherwise the presentation stream.
  hipStream_t slot_present_stream(const FrameSlot &s) const {
    return (pipelined() && s.stream_used && s.stream_used != shade_stream()) ? s.stream_used : present_stream();
  }
  int n_slots() const { return user_stream ? 1 : frames_in_flight; }
  int tile_w() const { return tile_mode == 0 ? 64 : 32; }
  int tile_h() const { return tile_mode == 0 ? 64 : 32; }
  int tiles_x() const { return (render_width() + tile_w() - 1) / tile_w(); }
  int tiles_y() const { return (render_height() + tile_h() - 1) / tile_h(); }
  // The partition is stated in output rows; a band is `supersample` times as many fine rows, so the band count, the
  // ownership and the shard's layout are those of the output, and the fine shard is n x the output shard.
  int eff_band_rows() const { return band_rows > 0 ? band_rows : tile_h(); }
  int band_tiles() const { return supersample * eff_band_rows() / tile_h(); }  // tile rows of one band of the render extent
  size_t fine_pixels() const { return (size_t)render_width() * ((size_t)supersample * std::max(height, shard_rows())); }
  int n_bands() const { return (height + eff_band_rows() - 1) / eff_band_rows(); }
  int local_bands() const { return world > 1 ? (n_bands() - rank + world - 1) / world : n_bands(); }
  int shard_rows() const { return world > 1 ? ((n_bands() + world - 1) / world) * eff_band_rows() : height; }
  size_t shard_pixels() const { return (size_t)width * shard_rows(); }  // pixels of this rank's output (world 1: the frame)
};

namespace {

int fail(bbr_context *ctx, int code, const std::string &msg) {
  if (ctx) ctx->last_error = msg;
  else g_create_error = msg;
  return code;
}

// Every entry point that can allocate, copy or launch makes the context's device current first: a process that drives
// several GPUs (one context each) may call with another device current.
#define BBR_ON_DEVICE(ctx)                                                                                     \
  do {                                                                                                         \
    hipError_t _e = hipSetDevice((ctx)->device);                                                               \
    if (_e != hipSuccess) return fail(ctx, BBR_ERR_HIP, std::string("hipSetDevice: ") + hipGetErrorString(_e)); \
  } while (0)

#define HIP_TRY(ctx, expr)                                                                                     \
  do {                                                                                                         \
    hipError_t _e = (expr);                                                                                    \
    if (_e != hipSuccess)                                                                                      \
      return fail(ctx, _e == hipErrorOutOfMemory ? BBR_ERR_OUT_OF_MEMORY : BBR_ERR_HIP,                        \
                  std::string(#expr) + ": " + hipGetErrorString(_e));                                          \
  } while (0)

// The mode of the next frame: what the options in force imply, stated here and nowhere else.
FrameMode frame_mode(const bbr_context *c) {
  FrameMode m;
  m.n = c->supersample;
  m.resolve = c->supersample > 1;
  m.merged = m.resolve && c->sample_shading == 0;
  m.fused = c->present_fused;
  m.shadow = c->shadow_map > 0 && c->shadow.any();
  m.shadow_casters = m.shadow && c->shadow.beyond_first();
  m.shadow_faces = m.shadow && !m.shadow_casters && c->shadow.slot[0].args.faces > 1;
  m.shadow_filter = m.shadow ? c->shadow_filter : 0;
  m.depth_rule = m.resolve ? c->depth_resolve : 0;
  // (bbr_draw_overlays is refused on a partition, and with n >= 2 unless option "depth_resolve" names a rule)
  m.depth = c->overlays && c->world == 1 && (!m.resolve || m.depth_rule != 0);
  m.out_rows = (size_t)std::max(c->height, c->shard_rows());
  if (m.resolve) m.fine_pixels = c->fine_pixels();
  if (m.merged) m.map_words = ((size_t)c->width * m.out_rows * sample_map_word_bytes(m.n) + 7) / 8;
  return m;
}

// What has the output extent (the overlay pass's depth, the dumps, the records) does not exist with n >= 2.
int refuse_supersampled(bbr_context *c, const char *who, const char *why = "its buffers have the output extent") {
  if (!frame_mode(c).resolve) return BBR_OK;
  return fail(c, BBR_ERR_INVALID_ARGUMENT, std::string(who) + ": not available with option supersample >= 2 (" + why + ")");
}
// ... unless option "depth_resolve" names the rule that gives an output pixel its depth and its winner
int refuse_without_depth_rule(bbr_context *c, const char *who, const char *why) {
  return frame_mode(c).depth_rule ? BBR_OK : refuse_supersampled(c, who, why);
}
// the pair of options that is refused, in whichever order it is asked for: a 3 x 3 block straddles the tiles
bool refused_pair(int64_t supersample, int64_t sample_shading) { return supersample == 3 && sample_shading == 0; }
// ... and the other one: pairing them would double the instantiations of the largest kernel (k_shade_mip)
bool refused_shadow_pair(int64_t mip_levels, int64_t shadow_map) { return mip_levels >= 2 && shadow_map > 0; }
// ... and option "bloom"'s two: a rank's shard lacks the rows its neighbours own, and a fused frame is no fp32 frame
bool refused_bloom_partition(int64_t bloom, int64_t world) { return bloom >= 1 && world > 1; }
bool refused_bloom_fused(int64_t bloom, int64_t present_fused) { return bloom >= 1 && present_fused != 0; }
// ... and option "auto_exposure"'s two: metering needs the whole frame, and a fused frame needs its exposure before it exists
bool refused_auto_partition(int64_t auto_exposure, int64_t world) { return auto_exposure != 0 && world > 1; }
bool refused_auto_fused(int64_t auto_exposure, int64_t present_fused) { return auto_exposure != 0 && present_fused != 0; }
// the render extent n * width x n * height has the limit of the output extent (bbr_create)
constexpr int32_t kMaxExtent = 32768;
constexpr int32_t kMaxShadowMap = 8192;  // option "shadow_map": 256 x 256 tiles of 32 x 32, the launch-slot limit of a frame
int check_render_extent(bbr_context *c, const char *who, int64_t n, int32_t width, int32_t height) {
  if (n * width <= kMaxExtent && n * height <= kMaxExtent) return BBR_OK;
  return fail(c, BBR_ERR_INVALID_ARGUMENT, std::string(who) + ": supersample x width/height exceeds 32768");
}
// there is no current frame any more, and no whole frame of an exchange
void forget_current_frame(bbr_context *c) {
  c->exchange_slot = c->last_slot = -1;
  c->exchange_whole = nullptr;
  c->have_frame = false;
}

// Option "sky_keep": the slot's word per tile stands behind the `tiles` fragment counts in d_frag_count, zeroed with them when
// the buffer is made (0 is no stamp) and dropped with them (the tile group: no allocation of its own)
#ifdef BB_STAMPS
constexpr size_t kFragCountWords = 18;  // diagnostic build: counts, 8 x u64 raster stamps per tile, the sky words
#else
constexpr size_t kFragCountWords = 2;   // counts, sky words
#endif
uint32_t *sky_words(const FrameSlot &s, size_t tiles) {
  return s.d_frag_count.cap >= tiles * kFragCountWords ? s.d_frag_count.ptr + tiles * (kFragCountWords - 1) : nullptr;
}
// Options "sky_keep" and "view_keep": every slot forgets what it holds (FrameSlot::forget_sky has the rule)
void forget_image(bbr_context *c) {
  for (FrameSlot &s : c->slots) s.forget_image();
}
// The stamp a main frame about to be launched into slot `s` runs under (0: it keeps nothing and marks nothing; k_raster then
// gets no state words at all).  A frame may keep while it is a forward frame of the whole image, one sample per pixel, into
// the slot's own fp32 frame, and k_raster's light-tile path is in use (no depth or visibility store); the slot's stamp lives
// on while such a frame follows such a frame into the same buffer under the same tile grid with the same state words.
// Everything else gets, or leaves behind, a fresh stamp from a process-wide counter: bit 30 set, bit 0 (kSkyKept) and bit 31
// clear, so it is never 0, k_raster's words of earlier stamps cannot equal it, and neither can the zeros of a new buffer
// or a fragment count (at most a tile's pixels, with or without kFullTile = bit 31).
// What options "sky_keep" and "view_keep" both rest on: the frame about to go into slot `s` is a forward frame of the whole
// image, one sample per pixel, into the slot's own fp32 frame, and k_raster's light-tile path is in use (no depth or
// visibility store).  Only such a frame leaves pixels behind that the slot's next frame may rely on, and only such a frame may.
bool keeps_own_image(const bbr_context *c, const FrameSlot &s, const FrameMode &mode, const float4 *out) {
  return !c->ablate && !c->deferred && !c->ext_out && c->world == 1 && !c->dump_vis && !mode.fused && !mode.resolve && !mode.depth &&
         out && out == s.d_frame.ptr;
}
// Option "view_keep": the same inputs, member by member (the structs have padding; those compared byte for byte have none)
bool same_inputs(const FrameInputs &a, const FrameInputs &b) {
  static_assert(sizeof(FrameParams) == 27 * 4 && sizeof(Mat4) == 64 && sizeof(FirstPrims) == 4 * kInlineFirstPrims, "no padding");
  auto same_bytes = [](const auto &x, const auto &y) { return std::memcmp(&x, &y, sizeof x) == 0; };
  return same_bytes(a.pv, b.pv) && same_bytes(a.view, b.view) && same_bytes(a.fp, b.fp) && a.draws.d == b.draws.d &&
         a.draws.n == b.draws.n && same_bytes(a.draws.first_prims, b.draws.first_prims) && a.draws.n_prims == b.draws.n_prims &&
         a.tile_mode == b.tile_mode && a.grid_y == b.grid_y && a.max_items == b.max_items && a.short_frame == b.short_frame &&
         a.item_head == b.item_head;
}
uint32_t sky_stamp_for(const bbr_context *c, FrameSlot &s, const FrameMode &mode, const float4 *out) {
  const uint32_t *state = sky_words(s, (size_t)c->tiles_x() * c->tiles_y());
  const bool may_keep = c->sky_keep && keeps_own_image(c, s, mode, out) && state;
  const SkyKeep now = {s.sky.stamp, 0u, out, state, c->width, c->height, c->tiles_x(), c->tiles_y(), c->tile_mode};
  const SkyKeep &was = s.sky;
  if (!may_keep || was.out != now.out || was.state != now.state || was.width != now.width || was.height != now.height ||
      was.tiles_x != now.tiles_x || was.tiles_y != now.tiles_y || was.tile_mode != now.tile_mode)
    s.forget_sky();
  const uint32_t kept_stamp = s.sky.stamp;
  s.sky = now;
  s.sky.stamp = kept_stamp;
  if (may_keep && !s.sky.stamp) {
    static std::atomic<uint32_t> counter{0};
    s.sky.stamp = 0x40000000u | ((counter.fetch_add(1u) << 1) & 0x3FFFFFFEu);
  }
  if (!may_keep) s.sky.stamp = 0;
  s.sky.used = s.sky.stamp;
  return s.sky.stamp;
}

// P*V exactly as the vertex stage's contract evaluates it (column j = P * V[j], fmaf chain)
Mat4 proj_view(const ViewUniformBlock &v) {
  Mat4 r;
  for (int c = 0; c < 4; ++c) {
    const float *col = v.view.M[c];
    for (int i = 0; i < 4; ++i)
      r.M[c][i] = std::fmaf(v.proj.M[3][i], col[3],
                            std::fmaf(v.proj.M[2][i], col[2], std::fmaf(v.proj.M[1][i], col[1], v.proj.M[0][i] * col[0])));
  }
  return r;
}

FrameParams make_params(const bbr_context *c) {
  FrameParams fp = {};  // (the overlay fields stay 0 for the main pass)
  fp.width = c->render_width();
  fp.height = c->render_height();
  fp.half_w = 0.5f * (float)c->render_width();
  fp.half_h = 0.5f * (float)c->render_height();
  fp.tiles_x = c->tiles_x();
  fp.tiles_y = c->tiles_y();
  fp.bin_cap = c->bin_cap;
  fp.broad_cap = c->broad_cap;
  fp.clip_cap = c->clip_cap;
  fp.broad_threshold = c->broad_threshold;
  fp.rank = c->rank;
  fp.world = c->world;
  fp.band_tiles = c->band_tiles();
  fp.shard_rows = c->supersample * c->shard_rows();
  fp.ablate = c->ablate;
  fp.deferred = c->deferred ? 1 : 0;
  fp.gbuffer_view = c->deferred ? c->gbuffer_view : -1;
  return fp;
}
// The overlay pass draws one sample per OUTPUT pixel into the presented image (whole frame only): with n >= 2 its extent,
// half extents, tile grid and rows are the output's, not the render extent's.  At n = 1 this is make_params.
FrameParams make_output_params(const bbr_context *c) {
  FrameParams fp = make_params(c);
  fp.width = c->width;
  fp.height = c->height;
  fp.half_w = 0.5f * (float)c->width;
  fp.half_h = 0.5f * (float)c->height;
  fp.tiles_x = (c->width + c->tile_w() - 1) / c->tile_w();
  fp.tiles_y = (c->height + c->tile_h() - 1) / c->tile_h();
  fp.band_tiles = c->eff_band_rows() / c->tile_h();
  fp.shard_rows = c->shard_rows();
  return fp;
}

// Wait for everything this context has queued.
int drain(bbr_context *c) {
  HIP_TRY(c, hipStreamSynchronize(c->geom_stream()));
  if (c->shade_stream() != c->geom_stream()) HIP_TRY(c, hipStreamSynchronize(c->shade_stream()));
  if (c->s_raster) HIP_TRY(c, hipStreamSynchronize(c->s_raster));

  if (c->s_present) HIP_TRY(c, hipStreamSynchronize(c->s_present));
  for (FrameSlot &s : c->slots) s.in_flight = false;
  return BBR_OK;
}

int ensure_srgb_tables(bbr_context *c);

// The buffers of one binned pass (k_geometry -> k_raster) over `n_prims` primitives at the context's tile grid and
// capacities (`tiles`: the pass's grid -- the render extent's, or the output extent's for an overlay pass over a resolved frame).
// The main pass (ensure_slot_buffers) adds its items, item groups, cooked lights, heavy list, frame, present,
// depth and dump buffers; the overlay pass (bbr_draw_overlays) passes n_prims > 0 and needs none of those.
int ensure_pass_buffers(bbr_context *c, FrameSlot &s, uint32_t n_prims, size_t tiles) {
  HIP_TRY(c, s.d_tris.ensure(std::max<size_t>(n_prims, 1)));
  HIP_TRY(c, s.d_attrs.ensure(std::max<size_t>(n_prims, 1)));
#ifdef BB_STAMPS
  HIP_TRY(c, s.d_clip.ensure(c->clip_cap + 8192));  // diagnostic build: room for per-workgroup time stamps
#else
  HIP_TRY(c, s.d_clip.ensure(c->clip_cap));
#endif
  HIP_TRY(c, c->d_counters.ensure(bbr_context::kCounterBlocks, true));
  HIP_TRY(c, s.d_block_stats.ensure(std::max<size_t>((n_prims + 255) / 256, 1) * 4, true));
  HIP_TRY(c, s.d_tile_count.ensure(tiles * kBinClasses, true));
  HIP_TRY(c, s.d_bins.ensure(tiles * kBinClasses * c->bin_cap));
  // (at least kBroadSpec entries: k_raster's light-tile path reads that many before it knows how many the frame wrote)
  HIP_TRY(c, s.d_broad.ensure(std::max<size_t>(c->broad_cap, kBroadSpec), true));
  HIP_TRY(c, s.d_frags.ensure(tiles * (size_t)(c->tile_w() * c->tile_h())));
  HIP_TRY(c, s.d_frag_count.ensure(tiles * kFragCountWords, true));  // (the counts and what stands behind them: sky_words)
  return BBR_OK;
}

int ensure_slot_buffers(bbr_context *c, FrameSlot &s, const FrameMode &m) {
  size_t tiles = (size_t)c->tiles_x() * c->tiles_y();
  int rc = ensure_pass_buffers(c, s, c->n_prims, tiles);
  if (rc) return rc;
  HIP_TRY(c, c->d_counters_done.ensure(bbr_context::kCounterBlocks, true));
  // (+ kShadeWaves: the last workgroup of k_shade's main launch reads the item words of all its waves before it knows the count)
  HIP_TRY(c, s.d_items.ensure(1 + tiles * (size_t)(c->tile_w() * c->tile_h() / 64) + kShadeWaves, true));
  if (tiles > (size_t)kItemGroupSlots * kItemGroups)  // 65536 launch slots: 8192 x 8192 pixels at 32 x 32 tiles
    return fail(c, BBR_ERR_INVALID_ARGUMENT, "frame too large for this tile size: set option tile_mode to 0 (64 x 64 tiles)");
  HIP_TRY(c, s.d_item_groups.ensure((size_t)kItemGroups * kItemGroupStride, true));
  HIP_TRY(c, s.d_cooked.ensure(kMaxNumLights));
  HIP_TRY(c, s.d_heavy.ensure(tiles * kBinClasses, true));
  if (c->deferred) HIP_TRY(c, s.d_background.ensure(2));
  if (m.depth) HIP_TRY(c, s.d_depth.ensure((size_t)c->width * c->height));
  if (m.depth && m.resolve) HIP_TRY(c, s.d_fine_depth.ensure((size_t)c->render_width() * c->render_height()));
  // (zero filled: the padding rows of a fine shard are never written, and k_resolve reads them)
  if (m.resolve) HIP_TRY(c, s.d_fine.ensure(m.fine_pixels, true));
  // (zero filled like the fine frame: rep 0 for every sample of a shard's padding rows, which no tile writes)
  if (m.merged) HIP_TRY(c, s.d_sample_map.ensure(m.map_words, true));
  if (m.fused) {
    HIP_TRY(c, s.d_present.ensure((size_t)c->width * m.out_rows));
    int rc_t = ensure_srgb_tables(c);
    if (rc_t) return rc_t;
  }
  if (c->dump_gbuffer) HIP_TRY(c, c->d_gbuffer.ensure((size_t)c->width * c->height * 4, true));
  if (c->dump_surface) HIP_TRY(c, c->d_surface.ensure((size_t)c->width * c->height * kSurfaceFloats, true));
  if (c->dump_shadow_mask) HIP_TRY(c, c->d_shadow_mask.ensure((size_t)c->width * c->height, true));
  if (!c->ext_out && m.frame32()) HIP_TRY(c, s.d_frame.ensure(m.out_rows * c->width));
  if (c->dump_vis) {  // (n >= 2: k_raster dumps the render extent; the output extent exists where a rule resolves it)
    if (m.resolve) {
      HIP_TRY(c, c->d_vis_fine_prim.ensure((size_t)c->render_width() * c->render_height()));
      HIP_TRY(c, c->d_vis_fine_depth.ensure((size_t)c->render_width() * c->render_height()));
    }
    if (!m.resolve || m.depth_rule) {
      HIP_TRY(c, c->d_vis_prim.ensure((size_t)c->width * c->height));
      HIP_TRY(c, c->d_vis_depth.ensure((size_t)c->width * c->height));
    }
  }
  if (!s.h_flags.ptr) {
    HIP_TRY(c, s.h_flags.ensure(kHostFlagWords * sizeof(uint32_t)));
    for (int i = 0; i < kHostFlagWords; ++i) s.h_flags.ptr[i] = 0u;
  }
  for (Event *e : {&s.ev_geom_done, &s.ev_raster_done, &s.ev_done, &s.ev_tail_done}) HIP_TRY(c, e->ensure(hipEventDisableTiming));
  return BBR_OK;
}

// The timing ring's events (option "timing": made there, not in the first timed frame -- 2560 hipEventCreate calls take
// half a millisecond)
int ensure_timing_ring(bbr_context *c, bool resolve_pairs) {
  HIP_TRY(c, ensure_events(c->ring, bbr_context::kRingEvents * bbr_context::kRingCap));
  if (resolve_pairs) HIP_TRY(c, c->resolve_ring.ensure());  // around k_resolve, one pair per ring frame
  return BBR_OK;
}

// The event that ends the interval of ring frame `i`: behind the frame's k_resolve if it has one -- the stop event of its resolve
// pair -- and behind its shading otherwise.  (The ring holds frames of one kind: option "supersample" empties it.)
hipEvent_t frame_end_event(const bbr_context *c, uint32_t i) {
  return frame_mode(c).resolve ? c->resolve_ring.stop(i) : c->ring[bbr_context::kRingEvents * (i % bbr_context::kRingCap) + 4];
}

// An edge between two streams of a frame: `to` goes on behind what `from` holds now.  Nothing to do on one stream.
void stream_edge(hipStream_t from, hipStream_t to, hipEvent_t ev) {
  if (from == to) return;
  (void)hipEventRecord(ev, from);
  (void)hipStreamWaitEvent(to, ev, 0);
}

// ---- mip chains (option "mip_levels" >= 2) ----
// L of a w x h map under the option's value n: min(n, 1 + floor(log2 max(w, h)))
int mip_level_count(int w, int h, int n) {
  int levels = 1;
  for (int m = std::max(w, h); m > 1; m >>= 1) ++levels;
  return std::min(levels, n);
}
int mip_extent(int n, int level) { return std::max(1, n >> level); }
size_t packed_level_bytes(int w, int h) { return (((size_t)w + 3) / 4) * (((size_t)h + 3) / 4) * 16 * kPackedTexelBytes + kPackedTexelPad; }

void free_chain(Material &m) {
  m.d_chain.release();
  m.mip = MipTable{};
}

// Levels >= 1 of every supplied map (k_mip_reduce, each from the level above) and, for a packed material, of the packed form
// (k_mip_pack, from the level-k maps), in one allocation -- every level starts on a multiple of 256 bytes, so a third of the
// material's own bytes plus at most 255 per level; and the level table.
// The context is drained and the material's level 0 is on the device.  Synchronises.
int build_chain(bbr_context *c, Material &m) {
  free_chain(m);
  const int n = c->mip_levels;
  auto aligned = [](size_t bytes) { return (bytes + 255) & ~(size_t)255; };
  size_t total = 0, offset[kMipSets][kMaxMipLevels] = {};
  for (int i = 0; i < kMapCount; ++i) {
    const TexDesc &td = m.desc.maps[i];
    MipSet &ms = m.mip.set[i];
    ms.levels = m.d_texels[i].ptr ? mip_level_count(td.w, td.h, n) : 1;  // (a defaulted map is 1 x 1)
    ms.level[0] = td.texels;
    for (int k = 1; k < ms.levels; ++k) {
      offset[i][k] = total;
      total += aligned((size_t)mip_extent(td.w, k) * mip_extent(td.h, k) * 4);
    }
  }
  MipSet &ps = m.mip.set[kMapCount];
  ps.levels = m.desc.packed ? mip_level_count(m.desc.pw, m.desc.ph, n) : 1;
  ps.level[0] = m.desc.packed;
  for (int k = 1; k < ps.levels; ++k) {
    offset[kMapCount][k] = total;
    total += aligned(packed_level_bytes(mip_extent(m.desc.pw, k), mip_extent(m.desc.ph, k)));
  }
  if (!total) return BBR_OK;
  HIP_TRY(c, m.d_chain.ensure(total));
  for (int i = 0; i < kMipSets; ++i)
    for (int k = 1; k < m.mip.set[i].levels; ++k) m.mip.set[i].level[k] = m.d_chain.ptr + offset[i][k];
  for (int i = 0; i < kMapCount; ++i) {
    const TexDesc &td = m.desc.maps[i];
    const MipSet &ms = m.mip.set[i];
    for (int k = 1; k < ms.levels; ++k) {
      const int w0 = mip_extent(td.w, k - 1), h0 = mip_extent(td.h, k - 1), w1 = mip_extent(td.w, k), h1 = mip_extent(td.h, k);
      hipLaunchKernelGGL(k_mip_reduce, dim3((unsigned)(((size_t)w1 * h1 + kMipThreads - 1) / kMipThreads)), dim3(kMipThreads), 0, nullptr,
                         (const uint32_t *)ms.level[k - 1], w0, h0, (uint32_t *)(m.d_chain.ptr + offset[i][k]), w1, h1);
    }
  }
  for (int k = 1; k < ps.levels; ++k) {
    // (the supplied shaded maps of a packed material have its size, so each has this level)
    MipPackMaps maps;
    for (int j = 0; j < 5; ++j) maps.map[j] = m.d_texels[j].ptr ? m.mip.set[j].level[k] : nullptr;
    const int w = mip_extent(m.desc.pw, k), h = mip_extent(m.desc.ph, k);
    const size_t slots = std::max<size_t>((((size_t)w + 3) / 4) * (((size_t)h + 3) / 4) * 16, kPackedTexelPad);
    hipLaunchKernelGGL(k_mip_pack, dim3((unsigned)((slots + kMipThreads - 1) / kMipThreads)), dim3(kMipThreads), 0, nullptr, maps,
                       (const uint8_t *)c->d_default_texels.ptr, w, h, m.d_chain.ptr + offset[kMapCount][k]);
  }
  HIP_TRY(c, hipGetLastError());
  HIP_TRY(c, hipStreamSynchronize(nullptr));
  return BBR_OK;
}

int upload_material_table(bbr_context *c) {
  if (!c->materials_dirty) return BBR_OK;
  size_t n = std::max<size_t>(c->materials.size(), 1);
  std::vector<MaterialDesc> h(n);
  c->all_packed = true;
  for (size_t i = 0; i < c->materials.size(); ++i) {
    h[i] = c->materials[i].desc;
    if (c->materials[i].alive && !c->materials[i].desc.packed) c->all_packed = false;
  }
  int rc = drain(c);
  if (rc) return rc;
  HIP_TRY(c, c->d_materials.ensure(n));
  HIP_TRY(c, upload_sync(c->d_materials.ptr, h.data(), n * sizeof(MaterialDesc)));
  if (c->mip_levels > 1) {
    std::vector<MipTable> t(n);
    for (MipTable &m : t)
      for (MipSet &ms : m.set) ms.levels = 1;  // (a slot without a live material: never sampled)
    for (size_t i = 0; i < c->materials.size(); ++i)
      if (c->materials[i].alive) t[i] = c->materials[i].mip;
    HIP_TRY(c, c->d_mip_tables.ensure(n));
    HIP_TRY(c, upload_sync(c->d_mip_tables.ptr, t.data(), n * sizeof(MipTable)));
  }
  c->materials_dirty = false;
  ++c->resource_epoch;
  return BBR_OK;
}

// ---- the bin pass: k_geometry -> k_raster through a slot's pass buffers (ensure_pass_buffers), counting in `ctr` ----
// The frame, a shadow face and the overlay pass (OVERLAY) each launch the pair through these two, which hold the only launch
// of their kernel.
template <int TW, int TH, bool OVERLAY = false>
void launch_geometry(const bbr_context *c, FrameSlot &s, hipStream_t st, Counters *ctr, const FrameParams &fp, const DeviceDraws &draws,
                     const Mat4 &pv, const Mat4 &view, uint32_t *heavy = nullptr) {
  if (!draws.n_prims) return;
  hipLaunchKernelGGL((k_geometry<TW, TH, OVERLAY>), dim3((draws.n_prims + 255) / 256), dim3(256), 0, st, draws.d, draws.n, draws.n_prims, draws.first_prims,
                     s.d_tris.ptr, s.d_attrs.ptr, s.d_tile_count.ptr, s.d_bins.ptr, ctr, pv, view, fp, s.d_clip.ptr, s.d_broad.ptr,
                     c->d_materials.ptr, s.d_block_stats.ptr, heavy);
}

// What a pass asks of k_raster beside the slot's own buffers: its optional inputs and outputs, null / 0 where the pass names none
struct RasterIO {
  int rows = 0;                   // of the grid: heavy_rows + grid_y for a frame, tiles_y for a pass
  float4 *out = nullptr;          // the background pixels' colour, or (out8) their presented words
  uint32_t *out8 = nullptr;
  uint32_t *vis_prim = nullptr;   // bbr_read_visibility's dump
  float *vis_depth = nullptr;
  const float4 *background = nullptr;
  float *depth_io = nullptr;      // a frame or a shadow face stores its depth here; the overlay pass tests against it
  uint32_t *host_flags = nullptr, *item_groups = nullptr, *item_head = nullptr, *items = nullptr;
  const Light *lights = nullptr;  // what a short frame's first workgroup cooks
  int num_lights = 0;
  CookedLight *cooked = nullptr;
  const uint32_t *heavy = nullptr;
  uint32_t *sky_state = nullptr;  // option "sky_keep": the slot's word per tile and the frame's stamp (sky_stamp_for)
  uint32_t sky_stamp = 0;
};
template <int TW, int TH, bool OVERLAY = false>
void launch_raster(FrameSlot &s, hipStream_t st, Counters *ctr, const FrameParams &fp, const RasterIO &io) {
  hipLaunchKernelGGL((k_raster<TW, TH, OVERLAY>), dim3(fp.tiles_x, io.rows), dim3(kTileThreads), 0, st, s.d_tile_count.ptr, ctr, s.d_broad.ptr,
                     s.d_frag_count.ptr, s.d_frags.ptr, io.out, fp, s.d_tris.ptr, s.d_clip.ptr, s.d_bins.ptr, io.vis_prim, io.vis_depth,
                     io.background, io.depth_io, io.host_flags, io.out8, io.item_groups, io.item_head, io.items, io.lights, io.num_lights,
                     io.cooked, io.heavy, io.sky_state, io.sky_stamp);
}

// What a main frame's launches are sized by, decided once in front of them: the final parameters, the rows of k_raster's
// screen-ordered grid, the item slots and whether it is a short frame.  The caller adds the view, the draws and the item head.
FrameInputs frame_shape(const bbr_context *c, const FrameSlot &s, const FrameMode &mode, const FrameParams &fp_in) {
  FrameInputs z;
  z.tile_mode = c->tile_mode;
  FrameParams &fp = z.fp = fp_in;
  // a rank without bands (more ranks than bands) still launches one row: its blocks fall off tiles_y and exit
  z.grid_y = std::max(1, c->world > 1 ? c->local_bands() * fp.band_tiles : fp.tiles_y);
  // A SHORT frame (at most option "no_tail_items" item slots: 1080p has 32 640) has no k_shade_items launch: k_raster's tiles
  // append their items themselves through the head word the staging copy has just zeroed, and its first workgroup cooks
  // the lights.  One kernel and one kernel boundary less on the frame's chain of dependent kernels; such a frame is also
  // shaded at full coverage, without the tail launch (launch_frame).
  z.max_items = (uint32_t)(fp.tiles_x * z.grid_y) * (uint32_t)(c->tile_w() * c->tile_h() / 64);
  // option "sample_shading" 0 (n >= 2): always the long route -- k_sample_merge thins the lists behind k_raster and does the
  // accounting of the items, which k_raster therefore leaves alone (both of its pointers are guarded)
  z.short_frame = !mode.merged && z.max_items <= (uint32_t)c->no_tail_items;
  // Heavy tiles first (long frames; k_raster): the heavy rows in front of the launch are sized from the length of the list
  // the slot's previous frame produced (pinned word kFlagHeavyTiles) + 1/8 + 8.  A list that does not fit them is not
  // used by that frame at all (plain screen order), so the first frame of a slot, or one after a jump, is merely slower.
  const int64_t heavy_tiles = c->heavy_tiles >= 0 ? c->heavy_tiles : (c->pipelined() ? 0 : 64);
  if (!z.short_frame && heavy_tiles > 0 && !c->dump_vis) {
    fp.heavy_threshold = (uint32_t)heavy_tiles;
    const uint32_t seen_heavy = s.h_flags.ptr ? s.h_flags.ptr[kFlagHeavyTiles] : 0u;
    if (seen_heavy) fp.heavy_rows = (int32_t)((seen_heavy + seen_heavy / 8u + 8u + (uint32_t)fp.tiles_x - 1u) / (uint32_t)fp.tiles_x);
  }
  return z;
}

// What shading alone needs of a main frame beside the slot's buffers (k_raster stores the background through the same pointers)
struct ShadeInputs {
  ShadeParams sp = {};
  const Light *lights = nullptr;             // the frame's, in the slot's device staging
  const ShadowCasterTable *table = nullptr;  // the frame's own caster table in its staging, or nullptr: the context's
  // Where the kernels write.  With a resolve `out` is the fine frame and k_resolve (at the end) writes `final_out`, the W x H fp32
  // frame (nullptr if the mode has none); with fused presentation k_raster / k_shade write presented pixels into the slot's RGBA8
  // image (`out8`), unless there is a resolve (a fine frame is fp32: a presented byte cannot be averaged, k_resolve presents)
  float4 *final_out = nullptr, *out = nullptr;
  uint32_t *out8 = nullptr;
  const SrgbTables *tables = nullptr;
  // option "view_keep" (submit_frame_body decides).  `kept`: the slot's buffers hold this frame's visibility already: nothing is
  // launched in front of the shading but, where `cook` says the lights are not the ones the slot's table was cooked from, k_cook_lights.
  bool kept = false, cook = false;
  // option "surface_keep" (submit_frame_body decides): `lit`: k_shade_lit on `surface` (`surface_items` items) in place of k_shade
  // and its tail; `store`: k_surface_store in front of it
  bool lit = false, store = false;
  float4 *surface = nullptr;
  uint32_t surface_items = 0;
};

// Everything in front of the shading: the frame's visibility, from `in`, into the slot's buffers.  `ev`: as for launch_frame.
template <int TW, int TH>
void launch_visibility(bbr_context *c, FrameSlot &s, const FrameMode &mode, const FrameStreams &st, const Event *ev, const FrameInputs &in,
                       const ShadeInputs &sh, const DrawDesc *h_draws, const std::vector<uint32_t> &fills) {
  const FrameParams &fp = in.fp;
  const bool resolve = mode.resolve, merged = mode.merged, short_frame = in.short_frame;
  const int grid_y = in.grid_y;
  const hipStream_t sg = st.geom, sr = st.raster;
  Counters *const ctr = c->d_counters.ptr + s.ctr_index;
  // (with a resolve k_raster stores the depth, and dumps, at the render extent; k_resolve_depth, behind it, the output's)
  float *depth = !mode.depth ? nullptr : (resolve ? s.d_fine_depth.ptr : s.d_depth.ptr);
  uint32_t *vis_prim = !c->dump_vis ? nullptr : (resolve ? c->d_vis_fine_prim.ptr : c->d_vis_prim.ptr);
  float *vis_depth = !c->dump_vis ? nullptr : (resolve ? c->d_vis_fine_depth.ptr : c->d_vis_depth.ptr);
  // option "static_records": the draws whose key has just repeated in this slot (plan_static_records; `h_draws`: the host's
  // copy of the descriptors) get the camera-independent part of their records first, once; k_geometry then stores the rest
  for (const uint32_t d : fills) {
    const uint32_t n = h_draws[d].n_instances * h_draws[d].tris_per_instance;
    hipLaunchKernelGGL(k_record_static, dim3((n + kRecordStaticThreads - 1) / kRecordStaticThreads), dim3(kRecordStaticThreads), 0, sg,
                       in.draws.d, d, s.d_attrs.ptr);
    ++c->static_fills;
  }
  launch_geometry<TW, TH>(c, s, sg, ctr, fp, in.draws, in.pv, in.view, s.d_heavy.ptr);
  if (ev && c->timing == 1) (void)hipEventRecord(ev[1], sg);
  stream_edge(sg, sr, s.ev_geom_done);
  // k_raster writes the background pixels of `out`: if the frame still shading on the other stream writes the
  // same buffer (single external output), raster has to wait for it; geometry above still overlapped
  // (every frame still in flight, not just the previous one: with one stream per slot, or while the layout is being
  //  switched, "after the previous frame" no longer implies "after the one before")
  for (const FrameSlot &o : c->slots)
    if (&o != &s && o.in_flight && sh.final_out && o.out_used == sh.final_out && o.stream_used != sr) (void)o.follow(sr);
  if (fp.deferred)
    hipLaunchKernelGGL(k_deferred_background, dim3(1), dim3(kBackgroundThreads), 0, sr, sh.sp, sh.lights, s.d_background.ptr, sh.tables, fp.gbuffer_view);
  RasterIO io;
  io.rows = fp.heavy_rows + grid_y;
  io.out = sh.out, io.out8 = sh.out8, io.vis_prim = vis_prim, io.vis_depth = vis_depth, io.depth_io = depth, io.host_flags = s.h_flags.ptr;
  io.background = fp.deferred ? s.d_background.ptr : nullptr;
  io.item_groups = (short_frame || merged) ? nullptr : s.d_item_groups.ptr, io.item_head = short_frame ? in.item_head : nullptr, io.items = s.d_items.ptr;
  io.lights = sh.lights, io.num_lights = sh.sp.num_lights, io.cooked = s.d_cooked.ptr, io.heavy = s.d_heavy.ptr;
  // option "sky_keep": the stamp this frame's light tiles keep and mark under, if the frame may (k_raster writes the fp32 frame then)
  io.sky_stamp = sky_stamp_for(c, s, mode, sh.final_out);
  io.sky_state = io.sky_stamp ? sky_words(s, (size_t)fp.tiles_x * fp.tiles_y) : nullptr;
  launch_raster<TW, TH>(s, sr, ctr, fp, io);
  if (merged)
    with_samples(mode.n, [&](auto n) {
      constexpr int N = decltype(n)::value;
      if constexpr (N != 3)  // (refused_pair)
        hipLaunchKernelGGL((k_sample_merge<TW, TH, N>), dim3((unsigned)fp.tiles_x, (unsigned)grid_y), dim3(kMergeThreads), 0, sr, fp, s.d_frag_count.ptr,
                           s.d_frags.ptr, reinterpret_cast<typename SampleMap<N>::Word *>(s.d_sample_map.ptr), s.d_item_groups.ptr);
    });
  // k_shade's work list (64 fragments per item), built from the per-tile fragment counts as soon as k_raster is done; the
  // same launch cooks the frame's light table
  if (!short_frame)
    hipLaunchKernelGGL((k_shade_items<TW, TH>), dim3((unsigned)((fp.tiles_x * grid_y + kItemsThreads - 1) / kItemsThreads)), dim3(kItemsThreads), 0, sr, fp, s.d_frag_count.ptr, s.d_item_groups.ptr, s.d_items.ptr,
                       fp.tiles_x, grid_y, s.h_flags.ptr ? s.h_flags.ptr + kFlagItemCount : nullptr, sh.lights, sh.sp.num_lights, s.d_cooked.ptr,
                       s.d_tile_count.ptr, ctr, s.d_heavy.ptr);
  if (mode.depth_rule && (depth || vis_prim)) {
    // k_resolve_depth, on k_raster's stream behind it and in front of the edge to the shading stream: the slot's ev_done, recorded
    // behind shading, covers it in every stream layout.  The plain form for the overlay pass's depth, the PRIM form for the dump.
    const dim3 grid((unsigned)((c->width + kResolveThreads - 1) / kResolveThreads), (unsigned)c->height);
    auto launch = [&](auto n, auto rule, auto prim, const float *fine_depth, const uint32_t *fine_prim, float *to_depth, uint32_t *to_prim) {
      hipLaunchKernelGGL((k_resolve_depth<decltype(n)::value, decltype(rule)::value, decltype(prim)::value>), grid, dim3(kResolveThreads), 0, sr,
                         reinterpret_cast<const uint32_t *>(fine_depth), fine_prim, reinterpret_cast<uint32_t *>(to_depth), to_prim, c->width);
    };
    with_samples(mode.n, [&](auto n) { with_depth_rule(mode.depth_rule, [&](auto rule) {
      if (depth) launch(n, rule, std::false_type{}, depth, nullptr, s.d_depth.ptr, nullptr);
      if (vis_prim) launch(n, rule, std::true_type{}, vis_depth, vis_prim, c->d_vis_depth.ptr, c->d_vis_prim.ptr);
    }); });
  }
}

// The launches of a main frame.  `ev`: the frame's five timing events, or nullptr.
template <int TW, int TH>
void launch_frame(bbr_context *c, FrameSlot &s, const FrameMode &mode, const FrameStreams &st, const Event *ev, const FrameInputs &in,
                  const ShadeInputs &sh, const DrawDesc *h_draws, const std::vector<uint32_t> &fills) {
  const FrameParams &fp = in.fp;
  const ShadeParams &sp = sh.sp;
  const Light *d_lights = sh.lights;
  const bool resolve = mode.resolve, merged = mode.merged, kept = sh.kept, short_frame = in.short_frame;
  const uint32_t max_items = in.max_items;
  const hipStream_t sg = st.geom, sr = st.raster, ss = st.shade;
  // (a kept frame: the slot's block is zero already and its retired copy holds the full frame's statistics, which stay: the
  //  frame's shading retires the spare block, and finds the chunk totals cleared)
  const int ctr_block = kept ? bbr_context::kSpareCounterBlock : s.ctr_index;
  Counters *ctr = c->d_counters.ptr + ctr_block, *ctr_done = c->d_counters_done.ptr + ctr_block;
  uint32_t *item_head = short_frame ? in.item_head : nullptr;
  if (kept) {
    // on the stream the slot's table was cooked on, in front of the edge to the shading stream, like the kernels it stands for
    stream_edge(sg, sr, s.ev_geom_done);
    if (sh.cook) hipLaunchKernelGGL(k_cook_lights, dim3(1), dim3(kItemsThreads), 0, sr, d_lights, sp.num_lights, s.d_cooked.ptr);
  } else {
    launch_visibility<TW, TH>(c, s, mode, st, ev, in, sh, h_draws, fills);
  }
  const uint32_t *item_count = short_frame ? item_head : s.d_items.ptr;   // where k_shade finds the number of items
  if (ev && c->timing == 1) (void)hipEventRecord(ev[2], sr);
  stream_edge(sr, ss, s.ev_raster_done);
  // (ev[3], the start of the shading interval, is recorded in front of the MAIN launch below -- behind the tail launch when
  //  both are on one stream: the interval is then the dominant kernel's own, which the kernel trace can be held against)
  // the maps a shadowed frame reads may come from a queued pass on another frame's stream (ShadowOwned::ev_pass)
  if (mode.shadow && c->shadow.pass_queued) (void)hipStreamWaitEvent(ss, c->shadow.ev_pass, 0);
  uint2 *gbuf = (fp.deferred && c->dump_gbuffer) ? c->d_gbuffer.ptr : nullptr;
  // Main launch: one item (64 fragments) per wave, four per workgroup, sized from the item count of the frame this slot
  // rendered last (k_shade_items leaves it in pinned host memory) plus 3 %; tail launch: a small persistent grid for
  // whatever lies behind that (a scene that suddenly grew; normally nothing, and its workgroups exit at once).
  const uint32_t seen = s.h_flags.ptr ? s.h_flags.ptr[kFlagItemCount] : 0u;
  uint32_t est = seen ? seen + seen / 32u + 64u : max_items;
  if (est > max_items) est = max_items;
  // A small frame is launched at full coverage instead: workgroups without an item leave after one scalar load, and a few
  // thousand of them cost less than the tail launch's kernel boundary on the frame's chain of dependent kernels (at
  // 1080p the chain's length over the frames in flight IS the frame rate).
  if (short_frame) est = max_items;
  const uint32_t main_wgs = std::max(1u, (est + kShadeWaves - 1) / kShadeWaves);
  // The tail runs on the raster stream, beside the main launch (their items are disjoint): in front of or behind it on
  // one stream an empty tail would still cost the frame a kernel boundary (~4 us).
  const bool tail = main_wgs * kShadeWaves < max_items;
  auto shade = [&](auto deferred, auto present) {
    constexpr bool DEFERRED = decltype(deferred)::value, PRESENT = decltype(present)::value;
    // The shading kernels' arguments, stated once.  A launch names its kernel, grid and stream, k_shade's `first_item` word (a
    // tuple: k_shade_aniso and k_shade_mip take none), the item groups, and what its kernel takes behind those.
    auto launch = [&](auto kernel, uint32_t wgs, hipStream_t stream, auto first_item, uint32_t *item_groups, auto... trailing) {
      std::apply([&](auto... first) {
        hipLaunchKernelGGL(kernel, dim3(wgs), dim3(kShadeThreads), 0, stream, s.d_items.ptr, item_count, first..., s.d_frags.ptr,
                           s.d_frag_count.ptr, s.d_attrs.ptr, s.d_clip.ptr, fp, sp, s.d_cooked.ptr, c->d_materials.ptr, sh.out, gbuf, sh.tables,
                           sh.out8, ctr, ctr_done, item_groups, trailing...);
      }, first_item);
    };
    uint32_t *groups = (short_frame || kept) ? nullptr : s.d_item_groups.ptr;
    if (mode.shadow || c->mip_levels > 1 || c->max_anisotropy > 1 || c->dump_surface) {
      // a valid shadow map: k_shade_shadow_casters, or k_shade_shadow, k_shade_shadow_faces, k_shade_shadow_pcf (never together with "mip_levels" >= 2: refused_shadow_pair); option "mip_levels":
      // k_shade_mip; option "max_anisotropy" / bbr_read_surface (the kernels' DUMP forms): k_shade_aniso.
      // Each is one launch whose waves walk the whole item list.
      if (ev) (void)hipEventRecord(ev[3], ss);
      float *surface = c->dump_surface ? c->d_surface.ptr : nullptr;
      with_bool(c->mip_levels > 1, [&](auto mip) { with_bool(c->dump_surface, [&](auto dump) {
        constexpr bool DUMP = decltype(dump)::value;
        if (mode.shadow_casters) {
          ShadowCastersArgs sa = {};
          sa.table = sh.table ? sh.table : c->shadow.d_table.ptr, sa.lights = d_lights, sa.num_lights = sp.num_lights, sa.radius = mode.shadow_filter;
          sa.side = c->shadow_map, sa.half = 0.5f * (float)c->shadow_map, sa.dump_slot = c->dump_shadow_slot;
          if (DUMP && c->dump_shadow_mask) sa.mask = c->d_shadow_mask.ptr, sa.face = c->d_shadow_face.ptr, sa.taps = c->d_shadow_taps.ptr;
          launch(k_shade_shadow_casters<TW, TH, DEFERRED, PRESENT, DUMP>, main_wgs, ss, std::tuple<>{}, groups, c->max_anisotropy, surface, sa);
        } else if (mode.shadow_filter) {
          ShadowPcfArgs sa = {c->shadow.slot[0].args, d_lights, nullptr, sp.num_lights, mode.shadow_filter};
          if (DUMP && c->dump_shadow_mask) sa.f.mask = c->d_shadow_mask.ptr, sa.f.face = c->d_shadow_face.ptr, sa.taps = c->d_shadow_taps.ptr;
          launch(k_shade_shadow_pcf<TW, TH, DEFERRED, PRESENT, DUMP>, main_wgs, ss, std::tuple<>{}, groups, c->max_anisotropy, surface, sa);
        } else if (mode.shadow_faces) {
          ShadowFacesArgs sa = c->shadow.slot[0].args;
          sa.mask = (DUMP && c->dump_shadow_mask) ? c->d_shadow_mask.ptr : nullptr;
          sa.face = (DUMP && c->dump_shadow_mask) ? c->d_shadow_face.ptr : nullptr;
          launch(k_shade_shadow_faces<TW, TH, DEFERRED, PRESENT, DUMP>, main_wgs, ss, std::tuple<>{}, groups, c->max_anisotropy, surface, sa);
        } else if (mode.shadow) {
          ShadowArgs sa = c->shadow.one_face();
          sa.mask = (DUMP && c->dump_shadow_mask) ? c->d_shadow_mask.ptr : nullptr;
          launch(k_shade_shadow<TW, TH, DEFERRED, PRESENT, DUMP>, main_wgs, ss, std::tuple<>{}, groups, c->max_anisotropy, surface, sa);
        } else if constexpr (decltype(mip)::value) launch(k_shade_mip<TW, TH, DEFERRED, PRESENT, DUMP>, main_wgs, ss, std::tuple<>{}, groups, c->max_anisotropy, c->d_mip_tables.ptr, surface);
        else launch(k_shade_aniso<TW, TH, DEFERRED, PRESENT, DUMP>, main_wgs, ss, std::tuple<>{}, groups, c->max_anisotropy, surface);
      }); });
      return;
    }
    if constexpr (!DEFERRED && !PRESENT) {
      if (sh.lit) {
        // option "surface_keep": the grid from the exact item count; the storing frame fills the surface first, on the same stream
        const uint32_t wgs = (sh.surface_items + kShadeWaves - 1) / kShadeWaves;
        if (sh.store)
          hipLaunchKernelGGL((k_surface_store<TW, TH>), dim3(std::min(wgs, 8u * (uint32_t)c->n_cus)), dim3(kShadeThreads), 0, ss, s.d_items.ptr, item_count,
                             sh.surface_items, s.d_frags.ptr, s.d_frag_count.ptr, s.d_attrs.ptr, s.d_clip.ptr, fp, sp.enable_normal_map,
                             c->d_materials.ptr, sh.surface);
        if (ev) (void)hipEventRecord(ev[3], ss);
        hipLaunchKernelGGL(k_shade_lit<false>, dim3(wgs), dim3(kShadeThreads), 0, ss, (const float4 *)sh.surface, item_count, sh.surface_items, sp,
                           s.d_cooked.ptr, sh.out, sh.tables, sh.out8, ctr, ctr_done, groups);
        return;
      }
    }
    if (tail) launch(k_shade<TW, TH, DEFERRED, PRESENT, true, true>, 32u, sr, std::make_tuple(main_wgs * (uint32_t)kShadeWaves), nullptr);
    if (ev) (void)hipEventRecord(ev[3], ss);
    // (the main launch without the per-map sampling path when every material is packed: k_shade, MIXED)
    with_bool(c->all_packed, [&](auto packed) { launch(k_shade<TW, TH, DEFERRED, PRESENT, false, !decltype(packed)::value>, main_wgs, ss, std::make_tuple(0u), groups); });
    if (tail) stream_edge(sr, ss, s.ev_tail_done);  // (nothing else went onto sr since the tail launch)
  };
  with_bool(fp.deferred, [&](auto deferred) { with_bool(sh.out8 != nullptr, [&](auto present) { shade(deferred, present); }); });
  if (resolve) {
    // k_resolve, right behind k_shade (and the tail launch, whose edge `ss` already follows) on the frame's own stream.  The
    // shading interval ends in front of it, the frame's interval behind it (the stop event of its own pair).
    if (ev) (void)hipEventRecord(ev[4], ss);
    if (ev) (void)c->resolve_ring.begin(ss);
    const int32_t rows = c->world > 1 ? c->shard_rows() : c->height;
    const dim3 grid((unsigned)((c->width + kResolveThreads - 1) / kResolveThreads), (unsigned)rows);
    // One launch over (merged, n, present).  It writes `final_out` or, presenting, the slot's RGBA8 image (`final_out` is nullptr
    // then; only the PRESENT forms read the tables, tone mapping and exposure); k_resolve_merged reads the sample map besides.
    uint32_t *present_to = mode.resolve_presents() ? s.d_present.ptr : nullptr;
    const SrgbTables *present_tables = present_to ? c->d_srgb_tables.ptr : nullptr;
    with_bool(merged, [&](auto merged_c) { with_samples(mode.n, [&](auto n) { with_bool(present_to != nullptr, [&](auto present) {
      constexpr int N = decltype(n)::value;
      constexpr bool PRESENT = decltype(present)::value;
      if constexpr (!decltype(merged_c)::value)
        hipLaunchKernelGGL((k_resolve<N, PRESENT>), grid, dim3(kResolveThreads), 0, ss, (const float4 *)sh.out, sh.final_out, present_to, c->width,
                           present_tables, sp.tone_enable, sp.exposure);
      else if constexpr (N != 3)  // (refused_pair)
        hipLaunchKernelGGL((k_resolve_merged<N, PRESENT>), grid, dim3(kResolveThreads), 0, ss, (const float4 *)sh.out,
                           reinterpret_cast<const typename SampleMap<N>::Word *>(s.d_sample_map.ptr), sh.final_out, present_to, c->width,
                           present_tables, sp.tone_enable, sp.exposure);
    }); }); });
    if (ev) (void)c->resolve_ring.end(ss);
  }
  (void)s.busy_until(ss);
  s.stream_used = ss;
  if (ev) {
    if (!resolve) (void)hipEventRecord(ev[4], ss);
    ++c->ring_frames;
  }
}

// what a growth loop reports when its eighth growth was not enough (sync_and_fix, run_pass_sync)
constexpr char kStillExceeded[] = "capacity still exceeded after 8 growth steps";
// A capacity overflowed (bit0 bins, bit1 every-tile list, bit2 clip arena): grow it.  Everything must have left the GPU.
int apply_growth(bbr_context *c, uint32_t overflow, uint32_t bin_need, uint32_t broad_need, uint32_t clip_need) {
  if (getenv("BBR_DEBUG"))
    fprintf(stderr, "[bbr] capacity growth: overflow bits %u, bin_need %u (bin_cap %u, broad_cap %u, clip_cap %u), frame %llu\n", overflow,
            bin_need, c->bin_cap, c->broad_cap, c->clip_cap, (unsigned long long)c->frame_counter);
  if (overflow & 1u) {
    // bin_need is exact for the frame that overflowed; round up with headroom so small scene changes do not re-trigger
    uint32_t need = std::max(bin_need + bin_need / 4u, c->bin_cap * 2u);
    c->bin_cap = (need + 255u) & ~255u;
    for (FrameSlot &s : c->slots) s.d_bins.release();
  }
  // the every-tile list and the clip arena: what the overflowed frame asked for (a lower bound: primitives dropped by a
  // full clip arena asked for no list entry) with headroom, at least double
  auto grown = [](uint32_t cap, uint32_t need) { return std::max(cap * 2u, (need + need / 4u + 255u) & ~255u); };
  if (overflow & 2u) c->broad_cap = grown(c->broad_cap, broad_need);
  if (overflow & 4u) c->clip_cap = grown(c->clip_cap, clip_need);
  ++c->retries;
  for (FrameSlot &s : c->slots) {
    s.forget_capacities();
    s.forget_visibility();  // (option "view_keep": the lists were cut short, and are laid out for the old capacities)
    // tile counters may hold residue of references that did not fit
    if (s.d_tile_count.ptr) HIP_TRY(c, zero_fill_sync(s.d_tile_count.ptr, s.d_tile_count.cap * sizeof(uint32_t)));
  }
  // (a queued shadow pass overflows as part of its frame, and leaves the same residue in the pass slot)
  if (FrameSlot &p = c->shadow.pass; p.d_tile_count.ptr) HIP_TRY(c, zero_fill_sync(p.d_tile_count.ptr, p.d_tile_count.cap * sizeof(uint32_t)));
  return BBR_OK;
}

// The recorded frame's draw descriptors as k_geometry reads them, into the host block `host` laid out as `lay`, for its device copy
// `device` (where the instance data will be too).  Returns the list: empty draws would break the first_prim search and get none.
DeviceDraws fill_draw_descs(const bbr_context *c, const StagingLayout &lay, uint8_t *host, uint8_t *device) {
  DrawDesc *const hd = lay.descs(host);
  const InstanceBlock *const d_inst_base = lay.instances(device);
  FirstPrims first_prims = {};
  uint32_t k = 0;
  for (const RecordedDraw &rd : c->draws) {
    if (!rd.n_instances || !rd.tris_per_instance) continue;
    const Mesh &m = c->meshes[rd.mesh];
    DrawDesc d;
    d.vertices = m.d_vertices.ptr;
    d.indices = m.d_indices.ptr;
    d.instances = d_inst_base + rd.first_instance;
    d.n_instances = rd.n_instances;
    d.tris_per_instance = rd.tris_per_instance;
    d.first_prim = rd.first_prim;
    d.material = (uint32_t)rd.material;
    const MaterialDesc &md = c->materials[rd.material].desc;
    d.packed = md.packed;
    d.packed_dims = md.packed ? ((uint32_t)md.pw | ((uint32_t)md.ph << 16)) : 0u;
    d.flags = 0;  // (the full path; a main frame's static draws: plan_static_records)
    if (k >= 1 && k <= (uint32_t)kInlineFirstPrims) first_prims.v[k - 1] = d.first_prim;
    hd[k++] = d;
  }
  for (uint32_t q = std::max(k, 1u); q <= (uint32_t)kInlineFirstPrims; ++q) first_prims.v[q - 1] = 0xFFFFFFFFu;
  return {lay.descs(device), k, first_prims, c->n_prims};
}

// The recorded draws for a synchronous pass: [draw descriptors | instances] in `staging`, as the frame's staging holds them,
// uploaded at once.  (A frame's own transfer is another job: pinned, asynchronous, one copy with its lights, head and table.)
int upload_recorded_draws(bbr_context *c, DeviceBuffer<uint8_t> &staging, DeviceDraws &up) {
  const StagingLayout lay(std::max<size_t>(c->draws.size(), 1), c->host_instances.size());
  HIP_TRY(c, staging.ensure(std::max<size_t>(lay.total, lay.inst_offset + 1)));
  std::vector<uint8_t> descs(lay.inst_offset);
  up = fill_draw_descs(c, lay, descs.data(), staging.ptr);
  if (up.n) HIP_TRY(c, upload_sync(lay.descs(staging.ptr), descs.data(), up.n * sizeof(DrawDesc)));
  if (lay.inst_bytes) HIP_TRY(c, upload_sync(lay.instances(staging.ptr), c->host_instances.data(), lay.inst_bytes));
  return BBR_OK;
}

// Option "static_records", a main frame's `n_draws` descriptors `hd` (fill_draw_descs) about to go into slot `s`: which of
// the draws find the camera-independent part of their records in the slot's d_attrs.  A draw's key is its descriptor (mesh
// pointers, instance count and place, triangle count, first primitive, material binding), its place in the frame and its
// instance blocks byte for byte, under one resource epoch and one allocation of d_attrs.  Per draw:
//   key new or changed    the full path; the key is remembered
//   key repeated          k_record_static is queued for the draw (`fills`), then the light path
//   key repeated, filled  the light path
// so a draw whose instances move every frame never causes a fill and pays the comparison only.  The descriptors are in the slot's
// pinned staging, laid out as `lay`, whose instance part is still as the slot's previous frame left it; the instance blocks of
// this frame are still in c->host_instances.  Called before that part is overwritten.
void plan_static_records(bbr_context *c, FrameSlot &s, const StagingLayout &lay, uint32_t n_draws, std::vector<uint32_t> &fills) {
  DrawDesc *const hd = lay.descs(s.h_staging.ptr);
  const InstanceBlock *const old_inst = lay.instances(s.h_staging.ptr), *const d_inst_base = lay.instances(s.d_staging.ptr);
  StaticRecords &sr = s.statics;
  if (!c->static_records || c->dump_records || c->ablate) return sr.forget();
  if (sr.epoch != c->resource_epoch || sr.attrs_cap != s.d_attrs.cap || sr.staging_cap != s.h_staging.cap) sr.forget();
  sr.epoch = c->resource_epoch;
  sr.attrs_cap = s.d_attrs.cap;
  sr.staging_cap = s.h_staging.cap;
  sr.draws.resize(n_draws, StaticRecords::Draw{DrawDesc{}, false});  // (a fresh entry's null pointers equal no live draw's)
  for (uint32_t k = 0; k < n_draws; ++k) {
    StaticRecords::Draw &e = sr.draws[k];
    const size_t inst_bytes = sizeof(InstanceBlock) * hd[k].n_instances;
    // (equal descriptors point at the same place of the device staging: the previous frame's blocks are at that place of the pinned one)
    const bool same = std::memcmp(&e.key, &hd[k], sizeof(DrawDesc)) == 0 &&
                      std::memcmp(old_inst + (hd[k].instances - d_inst_base), c->host_instances.data() + (hd[k].instances - d_inst_base), inst_bytes) == 0;
    if (!same) {
      e.key = hd[k];
      e.filled = false;
      continue;
    }
    if (!e.filled) fills.push_back(k);
    e.filled = true;
    hd[k].flags = kDrawStaticPresent;
    ++c->static_light_draws;
  }
}

// ---- shadow map passes: what the synchronous call (render_shadow_faces) and a frame's queued pass share ----

// The pass's frame: S x S whatever "supersample" is, the whole map on every rank, the forward order whatever "render_pass" is,
// the context's capacities as they are now.
FrameParams shadow_pass_params(const bbr_context *c) {
  const int32_t S = c->shadow_map;
  FrameParams fp = make_params(c);
  fp.width = fp.height = S;
  fp.half_w = fp.half_h = 0.5f * (float)S;
  fp.tiles_x = (S + c->tile_w() - 1) / c->tile_w();
  fp.tiles_y = (S + c->tile_h() - 1) / c->tile_h();
  fp.rank = 0;
  fp.world = 1;  // every rank renders the whole map
  fp.band_tiles = fp.tiles_y;
  fp.shard_rows = S;
  fp.deferred = 0;
  fp.gbuffer_view = -1;
  return fp;
}

// The faces of `q` on `st`, back to back through the pass slot: the frame's own k_geometry and k_raster, face f counting in
// `ctr[f]` (zero before), the depth of every texel into the f-th S x S map at `map`.
void launch_shadow_faces(bbr_context *c, hipStream_t st, const FrameParams &fp, const DeviceDraws &draws, const CasterRequest &q,
                         Counters *ctr, float *map) {
  FrameSlot &s = c->shadow.pass;
  const size_t texels = (size_t)c->shadow_map * (size_t)c->shadow_map;
  with_tile(c->tile_mode, [&](auto tile) {
    constexpr int T = decltype(tile)::value;
    for (int f = 0; f < q.faces; ++f) {
      RasterIO io;  // the depth into the map; the background's presented words into the sink
      io.rows = fp.tiles_y, io.depth_io = map + (size_t)f * texels, io.out8 = c->shadow.d_sink.ptr;
      // gl_Position = (L.proj * L.view) * posWorld: the forward order, whatever "render_pass" is
      launch_geometry<T, T>(c, s, st, ctr + f, fp, draws, proj_view(q.view[f]), q.view[f].view);
      launch_raster<T, T>(s, st, ctr + f, fp, io);
    }
  });
}

// What the shading kernels get of caster slot `cs` once its maps are (being) rendered as `q` asks: into generation `cs.cur`
void set_caster_args(const bbr_context *c, ShadowSlot &cs, const CasterRequest &q) {
  const int32_t S = c->shadow_map;
  for (int f = 0; f < kMaxShadowFaces; ++f) cs.args.m[f] = f < q.faces ? proj_view(q.view[f]) : Mat4{};
  cs.args.map = cs.generation(cs.cur).ptr;
  cs.args.mask = nullptr;
  cs.args.face = nullptr;
  cs.args.side = S;
  cs.args.light = q.light;
  cs.args.faces = q.faces;
  cs.args.half = 0.5f * (float)S;
  cs.args.bias = q.bias;
}
// The slot becomes valid: the frames from here on are shaded with `q`'s maps in `generation` (rendered, or about to be on the
// frame's own stream), under a stamp of its own
void publish(bbr_context *c, ShadowSlot &cs, int generation, const CasterRequest &q) {
  cs.cur = generation;
  set_caster_args(c, cs, q);
  cs.stamp = ++c->caster_stamp;
  cs.valid = true;
}

// The table k_shade_shadow_casters reads, from the slots in use
void fill_caster_table(const ShadowOwned &sh, ShadowCasterTable &t) {
  std::memset(&t, 0, sizeof t);
  for (int32_t &s : t.slot_of_light) s = -1;
  for (int s = 0; s < kMaxShadowCasters; ++s) {
    if (!sh.slot[s].valid) continue;
    const ShadowFacesArgs &a = sh.slot[s].args;
    ShadowCasterEntry &e = t.slot[s];
    for (int f = 0; f < kMaxShadowFaces; ++f) e.m[f] = a.m[f];
    e.map = a.map, e.light = a.light, e.faces = a.faces, e.bias = a.bias;
    t.slot_of_light[a.light] = s;  // (0 .. 99, and no other slot in use names it: render_shadow_faces, bbr_queue_shadow_caster)
  }
}

// ---- the queued pass (bbr_queue_shadow_caster) ----
// The rule: a frame that queued casters is the frame with bbr_render_shadow_caster called for each of them, in slot order,
// directly in front of its bbr_end_frame.  So the queued slots become the context's casters when the frame is submitted
// (apply_queued_casters, in front of frame_mode: the frame is shaded with them), and their maps are rendered from the frame's own
// draws on the frame's own stream in front of its k_geometry (launch_queued_passes).  Nothing waits and nothing is drained.

// The generation of slot `caster`'s maps a pass in front of the frame going into `into` may write: one that no frame on the
// GPU reads.  The frames in flight beside `into` are at most kMaxSlots - 1 and read one generation each, so there is one
// and nothing ever waits; finding none is an error.
static_assert(ShadowSlot::kGenerations >= bbr_context::kMaxSlots, "a free generation for every frame in flight");
int pick_generation(bbr_context *c, int caster, const FrameSlot &into, int *out) {
  auto read_on_gpu = [&](int g) {
    for (const FrameSlot &o : c->slots)
      if (&o != &into && o.in_flight && o.shadow_gen[caster] == g && !o.idle()) return true;
    return false;
  };
  for (int g = 0; g < ShadowSlot::kGenerations; ++g)
    if (!read_on_gpu(g)) return *out = g, BBR_OK;
  return fail(c, BBR_ERR_HIP, "queued shadow pass: every generation of the slot's maps is read by a frame in flight");
}

// The recorded frame's queued casters become the context's, each on a generation of its own.  Returns through `n_queued` how many.
int apply_queued_casters(bbr_context *c, const FrameSlot &into, int *n_queued) {
  ShadowOwned &sh = c->shadow;
  *n_queued = 0;
  if (c->shadow_map <= 0) return BBR_OK;
  const size_t texels = (size_t)c->shadow_map * (size_t)c->shadow_map;
  for (int k = 0; k < kMaxShadowCasters; ++k) {
    CasterRequest &q = sh.queued[k];
    if (!q.on) continue;
    // (a synchronous call since has put the light into another slot: the call in front of bbr_end_frame would be refused)
    for (int o = 0; o < kMaxShadowCasters; ++o)
      if (o != k && sh.slot[o].valid && sh.slot[o].args.light == q.light) q.on = false;
    if (!q.on) continue;
    ShadowSlot &cs = sh.slot[k];
    int g = 0;
    if (int rc = pick_generation(c, k, into, &g)) return rc;
    HIP_TRY(c, cs.generation(g).ensure(texels * (size_t)q.faces));  // (growing frees a buffer nothing on the GPU reads)
    publish(c, cs, g, q);
    sh.table_stale = true;
    ++*n_queued;
  }
  return BBR_OK;
}

// The queued casters' faces on `st` -- the frame's geometry stream, behind its staging transfer, whose descriptors and instance
// blocks the pass reads (`draws`: a static draw's light path stores less of a record the pass never reads, and the same
// triangle) -- then k_shadow_pass_retire, which folds the faces' counters into the frame's (`frame_ctr`, `into.h_flags`).
// The pass slot is the context's one (ShadowOwned::pass), shared by all frames behind ev_pass.  It never holds records a later
// frame relies on, unlike the frame slot's own buffers under "static_records".
int launch_queued_passes(bbr_context *c, FrameSlot &into, hipStream_t st, const DeviceDraws &draws, Counters *frame_ctr) {
  ShadowOwned &sh = c->shadow;
  FrameSlot &p = sh.pass;
  const FrameParams fp = shadow_pass_params(c);
  const size_t texels = (size_t)c->shadow_map * (size_t)c->shadow_map;
  auto &z = sh.pass_sized;
  const bool fits = p.d_tile_count.ptr && p.d_bins.ptr && p.d_broad.ptr && p.d_clip.ptr && sh.d_sink.cap >= texels &&
                    sh.d_ctr.cap >= (size_t)kShadowPassBlocks && draws.n_prims <= z.n_prims && c->bin_cap == z.bin_cap &&
                    c->broad_cap == z.broad_cap && c->clip_cap == z.clip_cap && c->tile_mode == z.tile_mode;
  if (!fits) {
    // the pass slot may be reallocated: the pass on the GPU leaves it first (the host waits for that one event)
    if (sh.pass_queued) HIP_TRY(c, hipEventSynchronize(sh.ev_pass));
    HIP_TRY(c, sh.d_sink.ensure(texels));
    HIP_TRY(c, sh.d_ctr.ensure(kShadowPassBlocks, true));
    if (int rc = ensure_pass_buffers(c, p, draws.n_prims, (size_t)fp.tiles_x * fp.tiles_y)) return rc;
    z.n_prims = std::max(z.n_prims, draws.n_prims), z.bin_cap = c->bin_cap, z.broad_cap = c->broad_cap, z.clip_cap = c->clip_cap;
    z.tile_mode = c->tile_mode;
  }
  HIP_TRY(c, sh.ev_pass.ensure(hipEventDisableTiming));
  if (sh.pass_queued) HIP_TRY(c, hipStreamWaitEvent(st, sh.ev_pass, 0));  // behind the pass of the frame before
  uint32_t block = 0;
  for (int k = 0; k < kMaxShadowCasters; ++k) {
    const CasterRequest &q = sh.queued[k];
    if (!q.on) continue;
    ShadowSlot &cs = sh.slot[k];
    launch_shadow_faces(c, st, fp, draws, q, sh.d_ctr.ptr + block, cs.generation(cs.cur).ptr);
    block += (uint32_t)q.faces;
    ++c->shadow_queue_passes;
  }
  hipLaunchKernelGGL(k_shadow_pass_retire, dim3(1), dim3(kPassRetireThreads), 0, st, sh.d_ctr.ptr, block, frame_ctr, into.h_flags.ptr);
  HIP_TRY(c, hipGetLastError());
  HIP_TRY(c, hipEventRecord(sh.ev_pass, st));
  sh.pass_queued = true;
  return BBR_OK;
}

// A synchronous bin pass over `n_prims` primitives through the pass slot `s`, on the context's shading stream, until it fits.
// Nothing of the context is on the GPU.  An attempt takes its parameters from `params()` (the capacities: again after a growth),
// sizes the slot's pass buffers for them, and `launch(fp, stream)` queues it; it counts in the `n_blocks` counter blocks at
// `d_blocks` (zero before, not a frame slot's: the pass is synchronous, so they are cleared here and not by a kernel).  One
// wait, one read of the blocks, one clear; a capacity that overflowed in any block is grown by the largest need among them and
// the whole attempt runs again.
template <class Params, class Launch>
int run_pass_sync(bbr_context *c, FrameSlot &s, uint32_t n_prims, Params &&params, Counters *d_blocks, int n_blocks, const std::string &who,
                  Launch &&launch) {
  for (int attempt = 0; attempt < 8; ++attempt) {
    const FrameParams fp = params();
    int rc = ensure_pass_buffers(c, s, n_prims, (size_t)fp.tiles_x * fp.tiles_y);
    if (rc) return rc;
    s.ctr_index = bbr_context::kMaxSlots;
    hipStream_t st = c->shade_stream();
    launch(fp, st);
    HIP_TRY(c, hipGetLastError());
    HIP_TRY(c, hipStreamSynchronize(st));
    Counters h[kMaxShadowFaces] = {};
    HIP_TRY(c, hipMemcpy(h, d_blocks, sizeof(Counters) * (size_t)n_blocks, hipMemcpyDeviceToHost));
    HIP_TRY(c, zero_fill_sync(d_blocks, sizeof(Counters) * (size_t)n_blocks));
    Counters need = {};
    for (int b = 0; b < n_blocks; ++b) {
      need.overflow |= h[b].overflow;
      need.bin_need = std::max(need.bin_need, h[b].bin_need);
      need.n_broad = std::max(need.n_broad, h[b].n_broad);
      need.n_clip_slots = std::max(need.n_clip_slots, h[b].n_clip_slots);
    }
    if (!need.overflow) return BBR_OK;
    rc = apply_growth(c, need.overflow, need.bin_need, need.n_broad, need.n_clip_slots);
    if (rc) return rc;
    if (s.d_tile_count.ptr) HIP_TRY(c, zero_fill_sync(s.d_tile_count.ptr, s.d_tile_count.cap * sizeof(uint32_t)));
  }
  return fail(c, BBR_ERR_CAPACITY, who + ": " + kStillExceeded);
}

// The faces of one caster, synchronously, through the pass slot: `q.faces` maps of S x S at `map` from the primitives of
// `draws`, a counter block per face (run_pass_sync: an overflow in any face renders ALL faces again).  Shared by the
// synchronous call (render_shadow_faces) and by the repair of a queued pass that overflowed (settle_queued_passes).
int render_faces_sync(bbr_context *c, const std::string &who, float *map, const CasterRequest &q, const DeviceDraws &draws) {
  ShadowOwned &sh = c->shadow;
  HIP_TRY(c, sh.d_sink.ensure((size_t)c->shadow_map * (size_t)c->shadow_map));
  HIP_TRY(c, sh.d_ctr.ensure(kMaxShadowFaces, true));
  return run_pass_sync(c, sh.pass, draws.n_prims, [&] { return shadow_pass_params(c); }, sh.d_ctr.ptr, q.faces, who,
                       [&](const FrameParams &fp, hipStream_t st) { launch_shadow_faces(c, st, fp, draws, q, sh.d_ctr.ptr, map); });
}

// A queued pass that overflowed is the frame's overflow (k_shadow_pass_retire), and the frame's repair -- growing, rendering the
// frame again -- reaches the pass only while that frame is still the recorded one.  This settles the rest.  The context is
// drained.  If the frame in any slot carried a pass and reported an overflow in its pinned words, the capacities grow by what
// those frames asked for, and every pass carried by a frame submitted since the first of them is rendered again, synchronously,
// oldest first, from that frame's own draws -- they are still in its slot's device staging, which only the slot's next frame
// overwrites, and a slot's words are looked at before that (submit_frame_into) -- into the generation the caster slot has now,
// unless a later request has replaced the slot's (CarriedPass::stamp).  The passes BEHIND the overflowed one are included because
// they ran on the pass slot's residue.  The frames shaded with the incomplete maps in between keep their pixels, as frames do
// that were queued behind an overflowed frame; `repaired` says that the last frame is among them.
int settle_queued_passes(bbr_context *c, bool *repaired) {
  *repaired = false;
  uint64_t first = ~0ull;
  uint32_t overflow = 0, bin_need = 0, broad_need = 0, clip_need = 0;
  for (const FrameSlot &o : c->slots) {
    const uint32_t *f = o.h_flags.ptr;
    if (!o.had_pass || !f || !f[kFlagOverflow]) continue;
    first = std::min(first, o.serial);
    overflow |= f[kFlagOverflow];
    bin_need = std::max(bin_need, f[kFlagBinNeed]);
    broad_need = std::max({broad_need, f[kFlagBroadNeed], f[kFlagPassBroadNeed]});
    clip_need = std::max({clip_need, f[kFlagClipNeed], f[kFlagPassClipNeed]});
  }
  if (!overflow || c->shadow_map <= 0) return BBR_OK;
  int rc = apply_growth(c, overflow, bin_need, broad_need, clip_need);  // (clears every slot's words)
  if (rc) return rc;
  *repaired = true;
  FrameSlot *order[bbr_context::kMaxSlots];
  int n = 0;
  for (FrameSlot &o : c->slots)
    if (o.had_pass && o.serial >= first) order[n++] = &o;
  std::sort(order, order + n, [](const FrameSlot *a, const FrameSlot *b) { return a->serial < b->serial; });
  for (int i = 0; i < n; ++i) {
    FrameSlot &o = *order[i];
    for (const CarriedPass &cp : o.carried) {
      ShadowSlot &cs = c->shadow.slot[cp.caster];
      if (!cs.valid || cs.stamp != cp.stamp || !o.d_staging.ptr || !o.draws.d) continue;  // (replaced or dropped since; no staging)
      rc = render_faces_sync(c, "queued shadow pass", cs.generation(cs.cur).ptr, cp.q, o.draws);
      if (rc) return rc;
    }
  }
  return BBR_OK;
}

int submit_frame_body(bbr_context *c, int slot_index) {
  if (!c->have_frame) return fail(c, BBR_ERR_NOT_IN_FRAME, "no recorded frame");
  int rc = upload_material_table(c);
  if (rc) return rc;
  FrameSlot &s = c->slots[slot_index];
  // the slot's previous frame (two frames ago) must have left the GPU before its buffers are reused
  if (s.in_flight) {
    if (!s.idle()) {  // still on the GPU: the host waits, and says so
      const auto b0 = std::chrono::steady_clock::now();
      HIP_TRY(c, s.wait_idle());
      c->host_blocked_ns += (uint64_t)std::chrono::duration_cast<std::chrono::nanoseconds>(std::chrono::steady_clock::now() - b0).count();
      ++c->host_blocked_frames;
    }
    s.in_flight = false;
  }
  // Self-healing for hosts that only stream frames: the frame that last used this slot reported an overflow.  Its
  // pixels (and those of the frames queued since) are incomplete and already handed out; from this frame on the
  // capacities fit.  (Synchronising calls do better: they re-render the overflowed frame, sync_and_fix.)
  if (const uint32_t *f = s.h_flags.ptr; f && f[kFlagOverflow]) {
    rc = drain(c);
    if (rc) return rc;
    // the frame carried a queued shadow pass: its overflow bits are in the frame's.  The capacities grow and the pass, and those
    // behind it, are rendered again before this frame's staging replaces its draws (settle_queued_passes, which clears the words)
    if (s.had_pass) ++c->shadow_queue_drains;
    bool repaired = false;
    rc = settle_queued_passes(c, &repaired);
    if (rc) return rc;
    if (f[kFlagOverflow]) {  // (a frame without a pass)
      rc = apply_growth(c, f[kFlagOverflow], f[kFlagBinNeed], f[kFlagBroadNeed], f[kFlagClipNeed]);
      if (rc) return rc;
    }
  }
  // bbr_queue_shadow_caster: the frame's queued casters are the context's from here on, this frame's mode included
  int n_queued = 0;
  rc = apply_queued_casters(c, s, &n_queued);
  if (rc) return rc;
  const FrameMode mode = frame_mode(c);  // decided once for the frame: the buffers, the launches, what the slot remembers
  rc = ensure_slot_buffers(c, s, mode);
  if (rc) return rc;
  if (!n_queued) s.h_flags.ptr[kFlagPassBroadNeed] = s.h_flags.ptr[kFlagPassClipNeed] = 0u;  // (k_shadow_pass_retire's words)

  // the staging: [lights (100 * 64 B)] [draw descriptors] [instances] [item head] [caster table] (StagingLayout)
  const bool carries_table = mode.shadow_casters && c->shadow.table_stale;
  const StagingLayout lay(c->draws.size(), c->host_instances.size(), true, carries_table);
  if (lay.total > s.h_staging.cap) {
    HIP_TRY(c, s.h_staging.ensure(std::max<size_t>(lay.total * 2, 1 << 16)));
    HIP_TRY(c, s.d_staging.ensure(s.h_staging.cap));
    s.forget_visibility();  // (the item head of a short frame lived in the old one)
    s.draws.d = nullptr;    // (... and the descriptors of the slot's last frame)
  }
  uint8_t *const h_staging = s.h_staging.ptr, *const d_staging = s.d_staging.ptr;
  const int n_lights = std::min(std::max(c->frame_u.num_lights, 0), kMaxNumLights);
  // option "view_keep": the slot's light table was cooked from the lights its last frame brought, which are still in the staging
  const bool lights_cooked = s.vis.valid && n_lights <= std::min(std::max(s.frame_u.num_lights, 0), kMaxNumLights) &&
                             std::memcmp(lay.lights(h_staging), c->frame_u.lights, sizeof(Light) * (size_t)n_lights) == 0;
  std::memcpy(lay.lights(h_staging), c->frame_u.lights, sizeof(Light) * kMaxNumLights);
  // draw descriptors point into the device copy of the instance data made by the same transfer
  const DeviceDraws draws = fill_draw_descs(c, lay, h_staging, d_staging);
  // (while the staging still holds the instance blocks of the slot's previous frame: a repeated descriptor has left them in place)
  std::vector<uint32_t> fills;  // draws k_record_static runs for in front of this frame's k_geometry
  plan_static_records(c, s, lay, draws.n, fills);
  if (lay.inst_bytes) std::memcpy(lay.instances(h_staging), c->host_instances.data(), lay.inst_bytes);
  std::memset(lay.item_head(h_staging), 0, 16);
  if (carries_table) fill_caster_table(c->shadow, *lay.caster_table(h_staging));

  const FrameStreams st = c->frame_streams(slot_index);
  for (hipEvent_t e : c->pending_waits) HIP_TRY(c, hipStreamWaitEvent(st.geom, e, 0));  // bbr_wait_event
  c->pending_waits.clear();
  const Event *ev = nullptr;  // this frame's timing events, if it carries any
  if (c->timing && (c->timing_tick++ % (uint64_t)c->timing_stride) == 0) {
    rc = ensure_timing_ring(c, mode.resolve);
    if (rc) return rc;
    ev = &c->ring[bbr_context::kRingEvents * (c->ring_frames % bbr_context::kRingCap)];
    if (c->timing == 1) HIP_TRY(c, hipEventRecord(ev[0], st.geom));
  }
  s.ctr_index = slot_index;
  FrameInputs in = frame_shape(c, s, mode, make_params(c));
  // forward: gl_Position = (P*V) * posWorld; deferred: P * (V * posWorld) -- the kernel gets P and V separately
  in.pv = c->deferred ? c->view_u.proj : proj_view(c->view_u);
  in.view = c->view_u.view, in.draws = draws, in.item_head = lay.item_head(d_staging);
  ShadeInputs sh;
  std::memcpy(sh.sp.view_pos, c->view_u.view_pos, sizeof sh.sp.view_pos);
  sh.sp.enable_normal_map = c->view_u.enable_normal_map;
  sh.sp.tone_enable = c->frame_u.enable_tone_mapping, sh.sp.exposure = c->frame_u.exposure;
  sh.sp.num_lights = n_lights, sh.lights = lay.lights(d_staging);
  float4 *const out = sh.final_out = !mode.frame32() ? nullptr : (c->ext_out ? static_cast<float4 *>(c->ext_out) : s.d_frame.ptr);
  sh.out = mode.resolve ? s.d_fine.ptr : out;
  sh.out8 = mode.shade_presents() ? s.d_present.ptr : nullptr, sh.tables = mode.shade_presents() ? c->d_srgb_tables.ptr : nullptr;
  sh.table = carries_table ? lay.caster_table(d_staging) : nullptr;

  // Option "view_keep": is this frame's visibility what the slot's buffers hold?  `in`: what the kernels make it from beside the draws'
  // contents; `buffers`: where they put it.  The contents are plan_static_records' business: every draw found its key repeated and its
  // static part written, so descriptors, places, instance blocks and resources are the last frame's.  The frame before must have been complete, and one
  // that a frame may be kept behind (`keepable`); the five-event breakdown (option "timing" 1) asks for every stage.  Nothing here looks at the device.
  const decltype(s.vis.buffers) buffers = {d_staging, s.d_tris.ptr, s.d_attrs.ptr, s.d_clip.ptr, s.d_broad.ptr, s.d_tile_count.ptr, s.d_bins.ptr,
                                 s.d_frags.ptr, s.d_frag_count.ptr, s.d_items.ptr, s.d_cooked.ptr, s.d_heavy.ptr, s.d_item_groups.ptr,
                                 s.d_block_stats.ptr, out};
  const bool keepable = keeps_own_image(c, s, mode, out) && !n_queued && !c->dump_records;
  bool all_light = c->static_records && fills.empty();
  for (uint32_t k = 0; all_light && k < draws.n; ++k) all_light = lay.descs(h_staging)[k].flags == kDrawStaticPresent;
  const bool kept = sh.kept = c->view_keep && keepable && all_light && c->timing != 1 && s.vis.valid && same_inputs(s.vis.in, in) &&
                              buffers == s.vis.buffers && !s.h_flags.ptr[kFlagOverflow];
  sh.cook = kept && !lights_cooked && n_lights > 0;
  if (kept) {
    ++c->view_kept_frames;
    s.vis.kept_last = true;
  } else {
    ++c->view_full_frames;
    s.vis = {keepable, false, in, buffers};
  }
  // Option "surface_keep": is this kept frame shaded from the slot's surface?  It could be if it takes the plain k_shade on the
  // long route (a kept frame is forward, of the whole image, into the slot's own fp32 frame, without a resolve: keeps_own_image)
  // and the slot's pinned word holds the item count its last full frame left.  Such a frame under the normal-map switch of the
  // slot's last frame is one more of the run: lit if the surface is valid, the storing frame if it is the n-th.  A full frame, a
  // kept frame that could not be lit and one under another switch start the run again, and the surface is stale.
  {
    SurfaceKeep &k = s.surf;
    const uint32_t n_items = s.h_flags.ptr[kFlagItemCount];
    const bool could = kept && c->surface_keep > 0 && !in.short_frame && !mode.shadow && c->mip_levels == 1 && c->max_anisotropy == 1 &&
                       !c->dump_surface && n_items > 0 && n_items <= in.max_items;
    if (!could || k.normal_map != sh.sp.enable_normal_map || k.all_packed != c->all_packed) {
      k.forget();
    } else if (k.valid && k.buffer == s.d_surface_keep.ptr && k.items == n_items) {
      sh.lit = true;
    } else if (++k.run >= (uint32_t)c->surface_keep) {
      // (the slot's frames have left the GPU: growing frees nothing that is in use)
      HIP_TRY(c, s.d_surface_keep.ensure(surface_keep_entries((n_items + kShadeWaves - 1) / kShadeWaves * kShadeWaves)));
      k.valid = true, k.buffer = s.d_surface_keep.ptr, k.items = n_items;
      sh.lit = sh.store = true;
      ++c->surface_stored_frames;
    }
    k.normal_map = sh.sp.enable_normal_map, k.all_packed = c->all_packed;
    if (sh.lit) {
      // the capacity the kernels index the planes by: what the buffer was sized for
      sh.surface = s.d_surface_keep.ptr, sh.surface_items = (n_items + kShadeWaves - 1) / kShadeWaves * kShadeWaves;
      ++c->surface_lit_frames;
    }
  }

  // (a kept frame: up to the item head, which a short frame's shading counts its items by and the full frame's k_raster left)
  HIP_TRY(c, hipMemcpyAsync(d_staging, h_staging, kept ? lay.head_offset : lay.total, hipMemcpyHostToDevice, st.geom));
  if (kept && carries_table)
    HIP_TRY(c, hipMemcpyAsync(lay.caster_table(d_staging), lay.caster_table(h_staging), sizeof(ShadowCasterTable), hipMemcpyHostToDevice, st.geom));
  if (n_queued) {
    rc = launch_queued_passes(c, s, st.geom, draws, c->d_counters.ptr + s.ctr_index);
    if (rc) return rc;
  }
  with_tile(in.tile_mode, [&](auto tile) {
    constexpr int T = decltype(tile)::value;
    launch_frame<T, T>(c, s, mode, st, ev, in, sh, lay.descs(h_staging), fills);
  });
  HIP_TRY(c, hipGetLastError());
  s.in_flight = true;
  for (int k = 0; k < kMaxShadowCasters; ++k) s.shadow_gen[k] = (mode.shadow && c->shadow.slot[k].valid) ? (int8_t)c->shadow.slot[k].cur : (int8_t)-1;
  s.had_pass = n_queued != 0;
  s.carried.clear();
  for (int k = 0; n_queued && k < kMaxShadowCasters; ++k)
    if (c->shadow.queued[k].on) s.carried.push_back({k, c->shadow.slot[k].stamp, c->shadow.queued[k]});
  s.draws = draws;
  s.serial = ++c->frame_serial;
  s.mode = mode;
  s.present.active = mode.fused;  // fused presentation: the frame IS the presented image
  s.present.out = mode.fused ? s.d_present.ptr : nullptr;
  s.present.enable = c->frame_u.enable_tone_mapping;
  s.present.exposure = c->frame_u.exposure;
  s.present.hdr16 = 1;
  s.present.copy_to = nullptr;
  s.present.auto_e = s.present.metered = false;
  s.frame_u = c->frame_u;
  s.view_u = c->view_u;
  s.out_used = out;
  c->last_slot = slot_index;
  return BBR_OK;
}

// Queue the recorded frame into slot `slot_index`.  Asynchronous.  A submission that fails leaves the caster slots, and the
// recorded frame's queued entries, as they were: the queued casters become the context's in front of steps that can fail
// (apply_queued_casters), and a caster whose maps were never rendered must not stay in use.
int submit_frame_into(bbr_context *c, int slot_index) {
  struct {
    CasterPublished slot;
    bool queued;
  } kept[kMaxShadowCasters];
  ShadowOwned &sh = c->shadow;
  const bool table_stale = sh.table_stale;
  for (int k = 0; k < kMaxShadowCasters; ++k) kept[k] = {sh.slot[k].published(), sh.queued[k].on};
  const int rc = submit_frame_body(c, slot_index);
  if (rc != BBR_OK) {
    for (int k = 0; k < kMaxShadowCasters; ++k) sh.slot[k].published() = kept[k].slot, sh.queued[k].on = kept[k].queued;
    sh.table_stale = table_stale;
  }
  return rc;
}

int ensure_srgb_tables(bbr_context *c) {
  if (!c->d_srgb_tables.ptr) {
    // t_k = float(decode((k - 0.5) / 255)) (the same table the CPU oracle builds), then the table keyed by the
    // float's top bits: thresholds <= lower edge of each cell; a cell may contain at most one threshold
    auto hp = std::make_unique<SrgbTables>();  // 4.3 KB: not on the stack, not shared between contexts
    SrgbTables &h = *hp;
    for (int k = 1; k <= 255; ++k) {
      const double b = ((double)k - 0.5) / 255.0;
      h.thr[k - 1] = (float)(b <= 0.04045 ? b / 12.92 : std::pow((b + 0.055) / 1.055, 2.4));
    }
    h.thr[255] = std::numeric_limits<float>::infinity();
    for (uint32_t cell = 0; cell < kSrgbLutCells; ++cell) {
      auto edge = [](uint32_t cl) {
        uint32_t bits = ((kSrgbLutFirstExp << 8) + cl) << 15;
        float f;
        std::memcpy(&f, &bits, 4);
        return f;
      };
      const float lo = edge(cell), hi = edge(cell + 1);
      uint32_t below = 0, inside = 0;
      for (int k = 0; k < 255; ++k) {
        below += h.thr[k] <= lo;
        inside += h.thr[k] > lo && h.thr[k] < hi;
      }
      if (inside > 1) return fail(c, BBR_ERR_HIP, "sRGB table: two thresholds in one cell");
      h.lut[cell] = (uint8_t)below;
    }
    HIP_TRY(c, c->d_srgb_tables.ensure(1));
    HIP_TRY(c, upload_sync(c->d_srgb_tables.ptr, &h, sizeof h));
  }
  return BBR_OK;
}

// Option "bloom": the sizes of a pyramid over a W x H frame (w_k = (w_{k-1} + 1) >> 1, never below 1) and where each level
// starts in its allocation, in texels; levels 1 .. L (index 0 is the frame's own extent)
struct BloomShape {
  int levels = 0;
  int32_t w[kMaxBloomLevels + 1] = {}, h[kMaxBloomLevels + 1] = {};
  size_t at[kMaxBloomLevels + 1] = {}, texels = 0;
  BloomShape(int32_t width, int32_t height, int l) : levels(l) {
    w[0] = width, h[0] = height;
    for (int k = 1; k <= l; ++k) {
      w[k] = (w[k - 1] + 1) >> 1, h[k] = (h[k - 1] + 1) >> 1;
      at[k] = texels;
      texels += (size_t)w[k] * (size_t)h[k];
    }
  }
};
// Option "auto_exposure", the two launches in front of a presentation's conversion, on its stream `ps`.  A unit is a frame
// slot's index or ExposureOwned::kBufferUnit.
// k_luminance: the n pixels of `frame` into the unit's histogram (zero on entry).  luminance_ring holds its interval.
int queue_luminance(bbr_context *c, hipStream_t ps, int unit, const float4 *frame, size_t n) {
  if (c->timing) {
    HIP_TRY(c, c->luminance_ring.ensure());
    HIP_TRY(c, c->luminance_ring.begin(ps));
  }
  const size_t per_block = (size_t)kLumaThreads * kLumaPerThread;
  hipLaunchKernelGGL(k_luminance, dim3((unsigned)((n + per_block - 1) / per_block)), dim3(kLumaThreads), 0, ps, frame, n, c->exposure.hist(unit));
  HIP_TRY(c, hipGetLastError());
  if (c->timing) HIP_TRY(c, c->luminance_ring.end(ps));
  return BBR_OK;
}
// k_exposure: the unit's histogram into its record and into the history of `source`.  Source 0's presentations run on the
// streams of their slots: each adapt step waits on the device for the one before it (the host never does).  Source 1's calls
// are ordered as a whole (bbr_present_buffer_auto).  `fallback`: the exposure of a frame with nothing to count and no history.
int queue_exposure(bbr_context *c, hipStream_t ps, int unit, int source, float fallback) {
  bbr_context::ExposureOwned &x = c->exposure;
  if (source == 0) {
    HIP_TRY(c, x.ev_adapted.ensure(hipEventDisableTiming));
    if (x.adapted) HIP_TRY(c, hipStreamWaitEvent(ps, x.ev_adapted, 0));
  }
  hipLaunchKernelGGL(k_exposure, dim3(1), dim3(kExposureThreads), 0, ps, x.hist(unit), x.record(unit), x.d_history.ptr + source,
                     c->exposure_params, fallback);
  HIP_TRY(c, hipGetLastError());
  if (source == 0) {
    HIP_TRY(c, hipEventRecord(x.ev_adapted, ps));
    x.adapted = true;
  }
  return BBR_OK;
}
// A presentation failed between its k_luminance and its k_exposure: the unit's histogram goes back to zero behind whatever
// was queued, so the unit's next presentation counts its own pixels only (best effort: the failure is what gets reported)
void abandon_metering(bbr_context *c, hipStream_t ps, int unit) {
  (void)hipMemsetAsync(c->exposure.hist(unit), 0, kLumaWords * sizeof(uint32_t), ps);
}
// k_present (k_present_auto with `d_exposure`) over n pixels on `ps`; `adapt` as in queue_bloom_present
template <class Adapt>
int queue_plain_present(bbr_context *c, hipStream_t ps, const float4 *frame, uint32_t *out, size_t n, int enable, float exposure, int hdr16,
                        const float *d_exposure, Adapt &&adapt) {
  if (c->timing) {
    HIP_TRY(c, c->present_ring.ensure());
    HIP_TRY(c, c->present_ring.begin(ps));
  }
  if (int rc = adapt()) return rc;
  const dim3 grid((unsigned)((n + (size_t)kPresentThreads * kPresentPerThread - 1) / ((size_t)kPresentThreads * kPresentPerThread)));
  if (d_exposure)
    hipLaunchKernelGGL(k_present_auto, grid, dim3(kPresentThreads), 0, ps, frame, out, n, c->d_srgb_tables.ptr, enable, d_exposure, hdr16);
  else
    hipLaunchKernelGGL(k_present, grid, dim3(kPresentThreads), 0, ps, frame, out, n, c->d_srgb_tables.ptr, enable, exposure, hdr16);
  HIP_TRY(c, hipGetLastError());
  if (c->timing) HIP_TRY(c, c->present_ring.end(ps));
  return BBR_OK;
}

// The chain over `frame` into `levels` (afterwards U_1 .. U_L), then k_present_bloom into `out`: everything on `ps`.
// bloom_ring holds the chain's interval, present_ring k_present_bloom's, as it holds k_present's.
// `d_exposure` (option "auto_exposure"): the exposure is read there by k_present_bloom_auto, and k_exposure is queued between
// the chain and that kernel (`meter`), inside present_ring's interval.
template <class Meter>
int queue_bloom_present(bbr_context *c, hipStream_t ps, const float4 *frame, uint32_t *out, const BloomShape &sh, float4 *levels,
                        int enable, float exposure, int hdr16, const float *d_exposure, Meter &&adapt) {
  auto grid = [](int32_t w, int32_t h) { return dim3((unsigned)((w + kBloomThreads - 1) / kBloomThreads), (unsigned)h); };
  auto level = [&](int k) { return levels + sh.at[k]; };
  if (c->timing) {
    HIP_TRY(c, c->bloom_ring.ensure());
    HIP_TRY(c, c->present_ring.ensure());
    HIP_TRY(c, c->bloom_ring.begin(ps));
  }
  hipLaunchKernelGGL(k_bloom_first, grid(sh.w[1], sh.h[1]), dim3(kBloomThreads), 0, ps, frame, sh.w[0], sh.h[0], level(1), sh.w[1],
                     c->bloom_threshold);
  for (int k = 1; k < sh.levels; ++k)
    hipLaunchKernelGGL(k_bloom_down, grid(sh.w[k + 1], sh.h[k + 1]), dim3(kBloomThreads), 0, ps, (const float4 *)level(k), sh.w[k], sh.h[k],
                       level(k + 1), sh.w[k + 1]);
  for (int k = sh.levels - 1; k >= 1; --k)
    hipLaunchKernelGGL(k_bloom_up, grid(sh.w[k], sh.h[k]), dim3(kBloomThreads), 0, ps, (const float4 *)level(k + 1), sh.w[k + 1], sh.h[k + 1],
                       level(k), sh.w[k]);
  HIP_TRY(c, hipGetLastError());
  if (c->timing) {
    HIP_TRY(c, c->bloom_ring.end(ps));
    HIP_TRY(c, c->present_ring.begin(ps));
  }
  if (int rc = adapt()) return rc;
  if (d_exposure)
    hipLaunchKernelGGL(k_present_bloom_auto, grid(sh.w[0], sh.h[0]), dim3(kBloomThreads), 0, ps, frame, (const float4 *)level(1), sh.w[1],
                       sh.h[1], out, sh.w[0], c->d_srgb_tables.ptr, enable, d_exposure, hdr16, c->bloom_intensity);
  else
    hipLaunchKernelGGL(k_present_bloom, grid(sh.w[0], sh.h[0]), dim3(kBloomThreads), 0, ps, frame, (const float4 *)level(1), sh.w[1], sh.h[1],
                       out, sh.w[0], c->d_srgb_tables.ptr, enable, exposure, hdr16, c->bloom_intensity);
  HIP_TRY(c, hipGetLastError());
  if (c->timing) HIP_TRY(c, c->present_ring.end(ps));
  return BBR_OK;
}

// k_present for the frame in slot `s`, on the shade stream (ordered after the frame's k_shade); option "bloom" >= 1: the
// chain on the slot's own pyramid and k_present_bloom in its place (no partition then: the shard is the W x H frame).
// Option "auto_exposure": a presentation queued under it converts with the exposure in the slot's record; the first one of
// the frame in the slot meters it in front (k_luminance, then the chain, then k_exposure: the chain does not need the
// exposure and runs while the adapt step of the presentation before may still be awaited).
int queue_present(bbr_context *c, FrameSlot &s) {
  int rc_tables = ensure_srgb_tables(c);
  if (rc_tables) return rc_tables;
  const size_t n = c->shard_pixels();
  const hipStream_t ps = c->slot_present_stream(s);
  const int unit = (int)(&s - c->slots);
  const bool meter = s.present.auto_e && !s.present.metered;
  const float *d_exposure = s.present.auto_e ? &c->exposure.record(unit)->applied : nullptr;
  if (c->bloom) HIP_TRY(c, s.d_bloom.ensure(BloomShape(c->width, c->height, c->bloom).texels));  // (grows only behind a drain: at the slot's first bloomed present)
  if (ps != s.stream_used) HIP_TRY(c, s.follow(ps));  // behind the frame's k_shade
  bool adapted = false;  // k_exposure is queued: it leaves the histogram zeroed
  auto adapt = [&]() -> int {
    const int rc = meter ? queue_exposure(c, ps, unit, 0, s.present.exposure) : (int)BBR_OK;
    adapted = rc == BBR_OK;
    return rc;
  };
  int rc = meter ? queue_luminance(c, ps, unit, s.out_used, n) : (int)BBR_OK;
  if (rc == BBR_OK && c->bloom) {
    const BloomShape sh(c->width, c->height, c->bloom);
    rc = queue_bloom_present(c, ps, s.out_used, s.present.out, sh, s.d_bloom.ptr, s.present.enable, s.present.exposure, s.present.hdr16, d_exposure, adapt);
    if (rc == BBR_OK) s.bloom_ran = sh.levels;
  } else if (rc == BBR_OK) {
    rc = queue_plain_present(c, ps, s.out_used, s.present.out, n, s.present.enable, s.present.exposure, s.present.hdr16, d_exposure, adapt);
  }
  if (rc != BBR_OK) {
    if (meter && !adapted) abandon_metering(c, ps, unit);
    return rc;
  }
  if (meter) {
    s.present.metered = true;
    c->exposure.last_slot = unit;
  }
  HIP_TRY(c, s.busy_until(ps));  // ... until the presented image exists
  return BBR_OK;
}

// The checks the buffer calls with an extent share
int check_present_buffer(bbr_context *c, const char *who, const void *rgba32f_device, const void *rgba8_device, int32_t width, int32_t height) {
  if (!rgba32f_device || !rgba8_device) return fail(c, BBR_ERR_INVALID_ARGUMENT, std::string(who) + ": NULL");
  if ((uintptr_t)rgba32f_device % 16 || (uintptr_t)rgba8_device % 4)
    return fail(c, BBR_ERR_INVALID_ARGUMENT, std::string(who) + ": the source must be 16-byte aligned, the output 4-byte aligned");
  if (width < 1 || height < 1 || width > kMaxExtent || height > kMaxExtent)
    return fail(c, BBR_ERR_INVALID_ARGUMENT, std::string(who) + ": width/height out of range (1 .. 32768)");
  return BBR_OK;
}
// The chain and the bloomed conversion of a caller's frame on the context's one pyramid (option "bloom" >= 1); `d_exposure`
// and `adapt` as in queue_bloom_present
template <class Adapt>
int queue_buffer_bloom(bbr_context *c, hipStream_t ps, const void *rgba32f_device, void *rgba8_device, int32_t width, int32_t height,
                              int32_t enable, float exposure, int32_t hdr16, const float *d_exposure, Adapt &&adapt) {
  bbr_context::BloomBuffer &b = c->bloom_buffer;
  const BloomShape sh(width, height, c->bloom);
  HIP_TRY(c, b.ev_used.ensure(hipEventDisableTiming));
  // the one pyramid is never used twice at once: this call's stream waits for the call before it; a pyramid that has to grow
  // is freed only once that call has left the GPU
  if (b.used && sh.texels > b.d_levels.cap) HIP_TRY(c, hipEventSynchronize(b.ev_used));
  HIP_TRY(c, b.d_levels.ensure(sh.texels));
  if (b.used) HIP_TRY(c, hipStreamWaitEvent(ps, b.ev_used, 0));
  b.ran = 0;
  if (int rc = queue_bloom_present(c, ps, (const float4 *)rgba32f_device, (uint32_t *)rgba8_device, sh, b.d_levels.ptr, enable, exposure, hdr16 != 0,
                                   d_exposure, adapt))
    return rc;
  HIP_TRY(c, hipEventRecord(b.ev_used, ps));
  b.used = true;
  b.w = width, b.h = height, b.ran = sh.levels;
  return BBR_OK;
}

// Fused presentation: the slot's image (the frame itself) copied to the caller's buffer
int copy_presented(bbr_context *c, FrameSlot &s, void *dst) {
  const hipStream_t ps = c->present_stream();
  HIP_TRY(c, s.follow(ps));
  HIP_TRY(c, hipMemcpyAsync(dst, s.d_present.ptr, c->shard_pixels() * 4, hipMemcpyDeviceToDevice, ps));
  HIP_TRY(c, s.busy_until(ps));
  return BBR_OK;
}

int submit_frame(bbr_context *c) {
  const auto t0 = std::chrono::steady_clock::now();
  int slot = (int)(c->frame_counter % (uint64_t)c->n_slots());
  int rc = submit_frame_into(c, slot);
  if (rc == BBR_OK) ++c->frame_counter;
  c->host_submit_ns += (uint64_t)std::chrono::duration_cast<std::chrono::nanoseconds>(std::chrono::steady_clock::now() - t0).count();
  ++c->host_frames;
  return rc;
}

// Synchronise and, if a capacity overflowed in the most recent frame, grow it and render that frame again.
// Render the recorded frame once more into the slot it was last rendered in (after a capacity growth, or for a diagnostic
// dump) and put the slot's presentation state back: the presented image is made again from the new frame, a caller's
// copy of it is refreshed, and bbr_read_presented / bbr_draw_overlays keep working afterwards.
int resubmit_last_frame(bbr_context *c) {
  FrameSlot &s = c->slots[c->last_slot];
  const auto present = s.present;
  int rc = submit_frame_into(c, c->last_slot);
  if (rc) return rc;
  if (present.active && !s.mode.fused) {
    s.present = present;
    rc = queue_present(c, s);
    if (rc) return rc;
  } else if (s.mode.fused && present.copy_to) {  // fused: the re-rendered frame is the image; redo the caller's copy
    s.present.copy_to = present.copy_to;
    return copy_presented(c, s, present.copy_to);
  }
  return BBR_OK;
}

int sync_and_fix(bbr_context *c, Counters *out_counters) {
  for (int attempt = 0; attempt < 8; ++attempt) {
    int rc = drain(c);
    if (rc) return rc;
    // queued shadow passes that overflowed, in whichever frame: grown and rendered again; the last frame was shaded with their
    // incomplete maps (or is itself one of those frames) and is rendered again, too -- its counters are read after that
    bool repaired = false;
    rc = settle_queued_passes(c, &repaired);
    if (rc) return rc;
    if (repaired) {
      if (out_counters) *out_counters = Counters{};
      if (!c->have_frame || c->last_slot < 0) return BBR_OK;
      rc = resubmit_last_frame(c);
      if (rc) return rc;
      continue;
    }
    Counters h = {};
    if (c->have_frame && c->last_slot >= 0 && c->d_counters.ptr)
      HIP_TRY(c, hipMemcpy(&h, c->d_counters_done.ptr + c->slots[c->last_slot].ctr_index, sizeof h, hipMemcpyDeviceToHost));
    if (out_counters) *out_counters = h;
    if (!h.overflow) return BBR_OK;
    // (a queued shadow pass overflows as part of its frame: k_shadow_pass_retire; the frame is rendered again with its pass)
    rc = apply_growth(c, h.overflow, h.bin_need, std::max(h.n_broad, h.pass_broad), std::max(h.n_clip_slots, h.pass_clip));
    if (rc) return rc;
    rc = resubmit_last_frame(c);
    if (rc) return rc;
  }
  return fail(c, BBR_ERR_CAPACITY, std::string("bin ") + kStillExceeded);
}

// Render the last frame again with a dump switched on (bbr_context::dump_vis / dump_gbuffer / dump_surface): nothing of
// what the read-backs hand out lives in memory after a frame.  The dump's buffer is filled when this returns BBR_OK.
int rerender_with(bbr_context *c, bool bbr_context::*dump) {
  int rc = sync_and_fix(c, nullptr);
  if (rc) return rc;
  forget_image(c);  // (a diagnostic frame: rendered in full)
  c->*dump = true;
  rc = resubmit_last_frame(c);
  if (rc == BBR_OK) rc = sync_and_fix(c, nullptr);
  c->*dump = false;
  return rc;
}

const void *last_output(const bbr_context *c) {
  return c->last_slot >= 0 ? (const void *)c->slots[c->last_slot].out_used : nullptr;
}

}  // namespace

// ================================================================================================
// overlay subpass: light markers + corner gizmo over the presented image
// ================================================================================================
namespace {

int upload_internal_mesh(bbr_context *c, Mesh &m, const std::vector<Vertex> &v, const std::vector<uint32_t> &idx) {
  m = Mesh();
  HIP_TRY(c, m.d_vertices.ensure(v.size()));
  HIP_TRY(c, upload_sync(m.d_vertices.ptr, v.data(), v.size() * sizeof(Vertex)));
  HIP_TRY(c, m.d_indices.ensure(idx.size()));
  HIP_TRY(c, upload_sync(m.d_indices.ptr, idx.data(), idx.size() * sizeof(uint32_t)));
  m.n_vertices = (uint32_t)v.size();
  m.n_indices = (uint32_t)idx.size();
  m.alive = true;
  return BBR_OK;
}

// generateUVSphereMesh(0.1f, 16, 16) as the light markers use it: positions only (src/main.cpp:953-957,
// src/render.cpp:1774-1833; sphericalToCartesian src/vector_math.cpp:284-292; pi32 = 3.141592f)
int ensure_marker_mesh(bbr_context *c) {
  if (c->marker_mesh.alive) return BBR_OK;
  constexpr float pi32 = 3.141592f, half_pi32 = pi32 * 0.5f, two_pi32 = pi32 * 2.f, radius = 0.1f;
  constexpr int hdiv = 16, vdiv = 16;
  std::vector<Vertex> v;
  std::vector<uint32_t> idx;
  for (int iv = 0; iv <= vdiv; ++iv) {
    const float theta = -half_pi32 + pi32 * ((float)iv / (float)vdiv);
    for (int ih = 0; ih <= hdiv; ++ih) {
      const float phi = two_pi32 * ((float)ih / (float)hdiv);
      const float cos_theta = cosf(theta);
      Vertex vx = {};
      vx.pos[0] = radius * cos_theta * cosf(phi);
      vx.pos[1] = radius * sinf(theta);
      vx.pos[2] = radius * cos_theta * sinf(phi);
      v.push_back(vx);
    }
  }
  for (int iv = 0; iv < vdiv; ++iv)
    for (int ih = 0; ih < hdiv; ++ih) {
      const uint32_t base = (uint32_t)((hdiv + 1) * iv + ih);
      if (iv < vdiv - 1) { idx.push_back(base); idx.push_back(base + hdiv + 1); idx.push_back(base + hdiv + 2); }
      if (iv > 0) { idx.push_back(base + hdiv + 2); idx.push_back(base + 1); idx.push_back(base); }
    }
  return upload_internal_mesh(c, c->marker_mesh, v, idx);
}

inline float dot3_fma(const float *a, const float *b) { return std::fmaf(a[2], b[2], std::fmaf(a[1], b[1], a[0] * b[0])); }

// column-major M * v with the vertex stage's fma chain
inline void mat_vec(const Mat4 &m, const float *v, float *out) {
  for (int i = 0; i < 4; ++i)
    out[i] = std::fmaf(m.M[3][i], v[3], std::fmaf(m.M[2][i], v[2], std::fmaf(m.M[1][i], v[1], m.M[0][i] * v[0])));
}

// TBN line overlay (option "tbn"): the last frame's draws through k_tbn_segments (clipped, snapped segment records,
// binned to 32 x 32 tiles), then k_tbn_raster over the presented image.  Synchronous, like the rest of the overlay pass.
int tbn_launch_params(bbr_context *c, int32_t w, int32_t h, TbnParams &tp) {
  tp.width = w;
  tp.height = h;
  tp.tiles_x = (w + kTbnTile - 1) / kTbnTile;
  tp.tiles_y = (h + kTbnTile - 1) / kTbnTile;
  tp.bin_cap = c->tbn_pass.bin_cap;
  tp.half_w = 0.5f * (float)w;
  tp.half_h = 0.5f * (float)h;
  auto &t = c->tbn_pass;
  HIP_TRY(c, t.d_tile_count.ensure((size_t)tp.tiles_x * tp.tiles_y));
  HIP_TRY(c, t.d_bins.ensure((size_t)tp.tiles_x * tp.tiles_y * tp.bin_cap));
  HIP_TRY(c, t.d_ctr.ensure(2));
  HIP_TRY(c, zero_fill_sync(t.d_tile_count.ptr, (size_t)tp.tiles_x * tp.tiles_y * sizeof(uint32_t)));
  HIP_TRY(c, zero_fill_sync(t.d_ctr.ptr, 2 * sizeof(uint32_t)));
  return BBR_OK;
}

// after a binning launch: 0 = the bins held everything, 1 = grown (redo the pass), < 0 = error
int tbn_check_bins(bbr_context *c, hipStream_t st) {
  HIP_TRY(c, hipGetLastError());
  HIP_TRY(c, hipStreamSynchronize(st));
  uint32_t h[2] = {0, 0};
  HIP_TRY(c, hipMemcpy(h, c->tbn_pass.d_ctr.ptr, sizeof h, hipMemcpyDeviceToHost));
  if (!h[0]) return 0;
  uint32_t cap = c->tbn_pass.bin_cap;
  while (cap < h[1]) cap *= 2;
  c->tbn_pass.bin_cap = cap;
  c->retries++;
  return 1;
}

int draw_tbn(bbr_context *c, FrameSlot &fs) {
  auto &t = c->tbn_pass;
  t.valid = false;
  const uint32_t n_prims = c->n_prims;
  DeviceDraws up;
  if (int rc = upload_recorded_draws(c, t.d_staging, up)) return rc;
  HIP_TRY(c, t.d_segs.ensure(std::max<size_t>((size_t)n_prims * 8, 1)));
  t.n_slots = n_prims * 8;
  const Mat4 pv = proj_view(fs.view_u);  // vCombined = uProjMat * uViewMat (tbn.vert:21), both render passes
  hipStream_t st = c->shade_stream();
  for (int attempt = 0; attempt < 8; ++attempt) {
    TbnParams tp;
    int rc = tbn_launch_params(c, c->width, c->height, tp);
    if (rc) return rc;
    if (n_prims)
      hipLaunchKernelGGL(k_tbn_segments, dim3((n_prims + 255) / 256), dim3(256), 0, st, up.d, up.n, n_prims, pv,
                         fs.view_u.enable_normal_map, c->d_materials.ptr, tp, t.d_segs.ptr, t.d_tile_count.ptr, t.d_bins.ptr,
                         t.d_ctr.ptr);
    rc = tbn_check_bins(c, st);
    if (rc < 0) return rc;
    if (rc == 1) continue;  // a bin overflowed: nothing was drawn yet, redo the pass with the grown bins
    const size_t px = (size_t)c->width * c->height;
    HIP_TRY(c, t.d_keys.ensure(px));
    HIP_TRY(c, hipMemsetAsync(t.d_keys.ptr, 0, px * sizeof(uint32_t), st));
    hipLaunchKernelGGL(k_tbn_raster, dim3(tp.tiles_x, tp.tiles_y, kTbnSplit), dim3(kTbnThreads), 0, st, t.d_segs.ptr,
                       t.d_tile_count.ptr, t.d_bins.ptr, tp, fs.d_depth.ptr, t.d_keys.ptr);
    hipLaunchKernelGGL(k_tbn_colour, dim3((unsigned)((px + 255) / 256)), dim3(256), 0, st, t.d_keys.ptr, fs.present.out, px);
    HIP_TRY(c, hipGetLastError());
    HIP_TRY(c, hipStreamSynchronize(st));
    t.valid = true;
    return BBR_OK;
  }
  return fail(c, BBR_ERR_CAPACITY, "draw_overlays: TBN bins still overflow after 8 growth steps");
}

}  // namespace

extern "C" int bbr_upload_gizmo(bbr_context *c, const void *gizmo_vertices, uint32_t n_vertices, const uint32_t *indices,
                                uint32_t n_indices) {
  if (!c) return BBR_ERR_INVALID_ARGUMENT;
  BBR_ON_DEVICE(c);
  if (!gizmo_vertices || !n_vertices) return fail(c, BBR_ERR_INVALID_ARGUMENT, "upload_gizmo: null/empty input");
  int rc = drain(c);
  if (rc) return rc;
  // bb::GizmoVertex {Pos, Color, Normal} (src/render.h:122-126) -> Vertex {pos, uv, normal, tangent := colour}
  const float *g = static_cast<const float *>(gizmo_vertices);
  std::vector<Vertex> v(n_vertices);
  for (uint32_t i = 0; i < n_vertices; ++i) {
    Vertex vx = {};
    for (int k = 0; k < 3; ++k) {
      vx.pos[k] = g[9 * i + k];
      vx.tangent[k] = g[9 * i + 3 + k];
      vx.normal[k] = g[9 * i + 6 + k];
    }
    v[i] = vx;
  }
  std::vector<uint32_t> idx;
  if (indices) {
    for (uint32_t i = 0; i < n_indices; ++i)
      if (indices[i] >= n_vertices) return fail(c, BBR_ERR_INVALID_ARGUMENT, "upload_gizmo: index out of range");
    idx.assign(indices, indices + n_indices / 3 * 3);
  } else {
    for (uint32_t i = 0; i < n_vertices / 3 * 3; ++i) idx.push_back(i);
  }
  return upload_internal_mesh(c, c->gizmo_mesh, v, idx);
}

extern "C" int bbr_draw_overlays(bbr_context *c, int32_t gizmo_extent) {
  if (!c) return BBR_ERR_INVALID_ARGUMENT;
  BBR_ON_DEVICE(c);
  if (!c->have_frame || c->last_slot < 0) return fail(c, BBR_ERR_NOT_IN_FRAME, "draw_overlays: nothing rendered");
  if (c->world > 1) return fail(c, BBR_ERR_INVALID_ARGUMENT, "draw_overlays: not available with a partition");
  if (int rc = refuse_without_depth_rule(c, "draw_overlays", "no depth resolve rule: option depth_resolve is 0")) return rc;
  int rc = sync_and_fix(c, nullptr);  // the overlay pass is synchronous: it is a debugging aid, not part of the hot path
  if (rc) return rc;
  forget_image(c);
  FrameSlot &fs = c->slots[c->last_slot];
  if (!fs.mode.depth) return fail(c, BBR_ERR_INVALID_ARGUMENT, "draw_overlays: the frame was rendered without option \"overlays\"");
  if (!fs.present.active) return fail(c, BBR_ERR_NOT_IN_FRAME, "draw_overlays: call bbr_present first (overlays go into the presented image)");
  if (c->tbn) {  // the TBN lines first, then the markers and the gizmo over them (src/main.cpp:132-136)
    rc = draw_tbn(c, fs);
    if (rc) return rc;
  }
  rc = ensure_marker_mesh(c);
  if (rc) return rc;
  rc = ensure_srgb_tables(c);
  if (rc) return rc;

  // ---- the pass's draw list: instanced markers, then the gizmo (src/main.cpp:138-171) ----
  const int n_lights = std::max(0, std::min(fs.frame_u.num_lights, kMaxNumLights));
  const bool gizmo = gizmo_extent > 0 && c->gizmo_mesh.alive;
  const Mat4 pv = proj_view(fs.view_u);  // uProjMat * uViewMat
  std::vector<InstanceBlock> inst((size_t)n_lights + (gizmo ? 1 : 0));
  for (int i = 0; i < n_lights; ++i) {
    const Light &l = fs.frame_u.lights[i];
    InstanceBlock ib = {};
    ib.model = pv;  // (P*V) * modelMat, modelMat = identity with column 3 = (pos, 1): light.vert:11-14
    const float p[4] = {l.pos[0], l.pos[1], l.pos[2], 1.0f};
    mat_vec(pv, p, ib.model.M[3]);
    ib.inv_model.M[0][0] = l.color[0]; ib.inv_model.M[0][1] = l.color[1]; ib.inv_model.M[0][2] = l.color[2];
    inst[i] = ib;
  }
  if (gizmo) {  // gizmo.vert:13-24
    const Mat4 &uv = fs.view_u.view;
    const float right[3] = {uv.M[0][0], uv.M[1][0], uv.M[2][0]}, up[3] = {uv.M[0][1], uv.M[1][1], uv.M[2][1]};
    const float look[3] = {uv.M[0][2], uv.M[1][2], uv.M[2][2]};
    const float view_pos[3] = {look[0] * -27.0f, look[1] * -27.0f, look[2] * -27.0f};
    ViewUniformBlock gv = fs.view_u;
    gv.view.M[3][0] = -dot3_fma(view_pos, right);
    gv.view.M[3][1] = -dot3_fma(view_pos, up);
    gv.view.M[3][2] = -dot3_fma(view_pos, look);
    const float d = 1.0f / tanf(0.261799f);
    gv.proj.M[0][0] = d;
    gv.proj.M[1][1] = -d;
    InstanceBlock ib = {};
    ib.model = proj_view(gv);
    ib.inv_model = gv.view;
    inst[(size_t)n_lights] = ib;
  }
  const uint32_t marker_tris = c->marker_mesh.n_indices / 3, gizmo_tris = gizmo ? c->gizmo_mesh.n_indices / 3 : 0;
  const uint32_t n_prims = marker_tris * (uint32_t)n_lights + gizmo_tris;
  if (!n_prims) return BBR_OK;
  std::vector<DrawDesc> draws;
  FrameSlot &s = c->ov;
  const StagingLayout lay(2, inst.size());  // (as a synchronous pass keeps the recorded draws)
  HIP_TRY(c, s.d_staging.ensure(lay.total));
  const InstanceBlock *d_inst = lay.instances(s.d_staging.ptr);
  if (n_lights) {
    DrawDesc d = {};
    d.vertices = c->marker_mesh.d_vertices.ptr; d.indices = c->marker_mesh.d_indices.ptr; d.instances = d_inst;
    d.n_instances = (uint32_t)n_lights; d.tris_per_instance = marker_tris; d.first_prim = 0; d.material = 1u;  // program: marker
    draws.push_back(d);
  }
  if (gizmo) {
    DrawDesc d = {};
    d.vertices = c->gizmo_mesh.d_vertices.ptr; d.indices = c->gizmo_mesh.d_indices.ptr; d.instances = d_inst + n_lights;
    d.n_instances = 1; d.tris_per_instance = gizmo_tris; d.first_prim = marker_tris * (uint32_t)n_lights; d.material = 2u;  // program: gizmo
    draws.push_back(d);
  }
  HIP_TRY(c, upload_sync(lay.descs(s.d_staging.ptr), draws.data(), draws.size() * sizeof(DrawDesc)));
  HIP_TRY(c, upload_sync(lay.instances(s.d_staging.ptr), inst.data(), lay.inst_bytes));
  DeviceDraws ov = {lay.descs(s.d_staging.ptr), (uint32_t)draws.size(), {{0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu}}, n_prims};
  for (size_t q = 1; q < draws.size() && q <= (size_t)kInlineFirstPrims; ++q) ov.first_prims.v[q - 1] = draws[q].first_prim;

  auto params = [&] {
    FrameParams fp = make_output_params(c);
    fp.deferred = 0;
    fp.gbuffer_view = -1;
    fp.ov_first_gizmo_prim = gizmo ? marker_tris * (uint32_t)n_lights : 0xFFFFFFFFu;
    const int x0 = c->width - gizmo_extent;
    fp.ov_half = 0.5f * (float)gizmo_extent;
    fp.ov_cx = (float)x0 + fp.ov_half;
    fp.ov_cy = fp.ov_half;
    fp.ov_x0 = std::max(x0, 0); fp.ov_y0 = 0; fp.ov_x1 = c->width; fp.ov_y1 = std::min(gizmo_extent, c->height);
    return fp;
  };
  Counters *ctr = c->d_counters.ptr + bbr_context::kMaxSlots;  // (the overlay pass's block: the frame rendered has made them)
  // When an overlay triangle did not fit, the presented pixels the attempt already wrote are a subset of the right ones (same
  // colours), so growing and drawing again on top is correct
  return run_pass_sync(c, s, n_prims, params, ctr, 1, "draw_overlays", [&](const FrameParams &fp, hipStream_t st) {
    const Mat4 ident = {};
    RasterIO io;  // tested against the frame's depth; the colour is k_shade_overlay's
    io.rows = fp.tiles_y, io.depth_io = fs.d_depth.ptr;
    with_tile(c->tile_mode, [&](auto tile) {
      constexpr int T = decltype(tile)::value;
      launch_geometry<T, T, true>(c, s, st, ctr, fp, ov, ident, ident);
      launch_raster<T, T, true>(s, st, ctr, fp, io);
      constexpr int kChunks = T * T / kShadeThreads;
      hipLaunchKernelGGL((k_shade_overlay<T, T>), dim3(fp.tiles_x * kChunks, fp.tiles_y), dim3(kShadeThreads), 0, st, fp,
                         s.d_attrs.ptr, s.d_clip.ptr, s.d_frags.ptr, s.d_frag_count.ptr, c->d_srgb_tables.ptr, fs.present.out);
    });
  });
}

// ================================================================================================
// shadow map pass (option "shadow_map"): the recorded draws once more, from the light's view, depth only
// ================================================================================================

// Synchronous, like the overlay pass, and built like it: the context is drained, the pass has a slot of its own
// (bbr_context::shadow.pass) and counter blocks of its own (cleared before it returns), and a capacity that overflows is
// grown and the pass run again.  The kernels are the frame's own k_geometry and k_raster, untouched:
// k_raster keeps its depth through the pointer the option "overlays" uses (so every tile takes the general path and every
// texel is stored, the clear value where nothing is drawn), and its colour stores -- the background of uncovered texels --
// go as presented words into d_sink, which nothing reads; it makes no items.  The map ignores the partition.
//
// One call renders F = 1 .. 6 faces (bbr_render_shadow_faces; bbr_render_shadow_map is F = 1).  The draws and instances are
// uploaded once.  The faces run back to back on the stream through the one pass slot: k_raster leaves every tile's bin
// counts at zero behind it (the general path's clear), the triangle records, bins, clip arena and every-tile list of face f
// are dead when its k_raster has finished, and the stream orders face f + 1's k_geometry behind that.  Only the counters
// must not be shared -- the every-tile and clip allocators start at zero for every face -- so each face has a block of its
// own in ShadowOwned::d_ctr.  One wait, one read of the F blocks, one clear.  If any face overflowed, the capacities grow by
// the largest need among the faces and ALL faces are rendered again: the faces of a cube see the same draws, so one that
// overflows is rarely alone, and which texels of the others were complete is not worth tracking.
//
// A call renders ONE caster slot (bbr_render_shadow_caster; bbr_render_shadow_map and _faces are slot 0).  The pass slot, the sink and the
// counter blocks are shared by the slots; the maps are the slot's own.  Every argument is judged before anything is
// invalidated: a refused call leaves every slot as it was.

// The table k_shade_shadow_casters reads, rebuilt from the slots.  The caller has drained the context.  It is made at the
// first use of a slot other than 0: a context that only ever uses slot 0 owns what it owned before there were slots.
static int upload_caster_table(bbr_context *c) {
  ShadowOwned &sh = c->shadow;
  if (!sh.d_table.ptr && !sh.beyond_first()) return BBR_OK;
  HIP_TRY(c, sh.d_table.ensure(1));
  std::vector<ShadowCasterTable> host(1);  // (3.6 KB)
  ShadowCasterTable &t = host[0];
  fill_caster_table(sh, t);
  HIP_TRY(c, upload_sync(sh.d_table.ptr, &t, sizeof t));
  sh.table_stale = false;  // (frames read this table again, not a copy of their own)
  return BBR_OK;
}

// A call's arguments judged, for the synchronous calls and (`queued`) for bbr_queue_shadow_caster.  The order of the checks
// decides which refusal a call with two faults gets.  The queued form differs in two places: a light is also taken by a slot the
// recorded frame has queued, and the call has to stand inside the frame.
static int check_caster_request(bbr_context *c, const std::string &who, int32_t caster, int32_t light_index, int32_t n_faces,
                                const void *light_view_blocks, float bias, bool queued) {
  if (c->shadow_map <= 0) return fail(c, BBR_ERR_INVALID_ARGUMENT, who + ": option shadow_map is 0");
  if (caster < 0 || caster >= kMaxShadowCasters) return fail(c, BBR_ERR_INVALID_ARGUMENT, who + ": caster outside 0 .. 7");
  if (n_faces < 1 || n_faces > kMaxShadowFaces) return fail(c, BBR_ERR_INVALID_ARGUMENT, who + ": n_faces outside 1 .. 6");
  if (light_index < 0 || light_index >= kMaxNumLights) return fail(c, BBR_ERR_INVALID_ARGUMENT, who + ": light_index outside 0 .. 99");
  if (!light_view_blocks) return fail(c, BBR_ERR_INVALID_ARGUMENT, who + ": NULL view block");
  if (bias != bias) return fail(c, BBR_ERR_INVALID_ARGUMENT, who + ": bias is NaN");
  const ShadowOwned &sh = c->shadow;
  for (int s = 0; s < kMaxShadowCasters; ++s)
    if (s != caster && ((sh.slot[s].valid && sh.slot[s].args.light == light_index) || (queued && sh.queued[s].on && sh.queued[s].light == light_index)))
      return fail(c, BBR_ERR_INVALID_ARGUMENT, who + (queued ? ": another caster slot, in use or queued in this frame, holds this light_index (one slot per light)"
                                                              : ": another caster slot in use holds this light_index (one slot per light)"));
  if (queued && !c->in_frame) return fail(c, BBR_ERR_NOT_IN_FRAME, who + ": outside begin_frame/end_frame");
  if (!c->in_frame && !c->have_frame) return fail(c, BBR_ERR_NOT_IN_FRAME, who + ": no recorded draws (call it after bbr_draw or after bbr_end_frame)");
  for (const RecordedDraw &rd : c->draws)
    if (!c->meshes[rd.mesh].alive || !c->materials[rd.material].alive)
      return fail(c, BBR_ERR_BAD_HANDLE, who + ": a recorded draw's mesh or material was freed");
  return BBR_OK;
}
// ... and made into the request (the view blocks are copied)
static CasterRequest caster_request(int32_t light_index, int32_t n_faces, const void *light_view_blocks, float bias, bool queued) {
  CasterRequest q = {};
  q.on = queued;
  q.light = light_index, q.faces = n_faces, q.bias = bias;
  std::memcpy(q.view, light_view_blocks, sizeof(ViewUniformBlock) * (size_t)n_faces);
  return q;
}

static int render_shadow_faces(bbr_context *c, const std::string &who, int32_t caster, int32_t light_index, int32_t n_faces,
                               const void *light_view_blocks, float bias) {
  if (!c) return BBR_ERR_INVALID_ARGUMENT;
  BBR_ON_DEVICE(c);
  if (int rc = check_caster_request(c, who, caster, light_index, n_faces, light_view_blocks, bias, false)) return rc;
  const CasterRequest q = caster_request(light_index, n_faces, light_view_blocks, bias, false);
  int rc = sync_and_fix(c, nullptr);  // the frames in flight leave the GPU (and the last one is complete)
  if (rc) return rc;
  rc = upload_material_table(c);
  if (rc) return rc;

  ShadowOwned &sh = c->shadow;
  ShadowSlot &cs = sh.slot[caster];
  // (outside a frame the recorded frame's queued pass for this slot is replaced too: a replay shows this call's maps.  Inside
  //  one it is not: the queued pass stands in front of bbr_end_frame, behind this call)
  if (!c->in_frame) sh.queued[caster].on = false;
  if (cs.valid) {  // (the slot's maps are about to be overwritten: until they are whole again no frame may use them)
    cs.valid = false;
    rc = upload_caster_table(c);
    if (rc) return rc;
  }
  HIP_TRY(c, cs.d_map.ensure((size_t)c->shadow_map * (size_t)c->shadow_map * (size_t)n_faces));
  DeviceDraws draws;
  rc = upload_recorded_draws(c, sh.pass.d_staging, draws);
  if (rc) return rc;
  rc = render_faces_sync(c, who, cs.d_map.ptr, q, draws);
  if (rc) return rc;
  for (DeviceBuffer<float> &g : cs.d_more) g.release();  // (nothing is in flight: the generations of earlier queued passes go)
  publish(c, cs, 0, q);  // (the synchronous pass writes generation 0)
  rc = upload_caster_table(c);
  if (rc) cs.valid = false;  // (the table still says so)
  return rc;
}

extern "C" int bbr_render_shadow_map(bbr_context *c, int32_t light_index, const void *light_view_block, float bias) {
  return render_shadow_faces(c, "render_shadow_map", 0, light_index, 1, light_view_block, bias);
}

extern "C" int bbr_render_shadow_faces(bbr_context *c, int32_t light_index, int32_t n_faces, const void *light_view_blocks, float bias) {
  return render_shadow_faces(c, "render_shadow_faces", 0, light_index, n_faces, light_view_blocks, bias);
}

extern "C" int bbr_render_shadow_caster(bbr_context *c, int32_t caster, int32_t light_index, int32_t n_faces, const void *light_view_blocks,
                                        float bias) {
  return render_shadow_faces(c, "render_shadow_caster", caster, light_index, n_faces, light_view_blocks, bias);
}

// The queued form of bbr_render_shadow_caster: judged like it, recorded with the frame, rendered when the frame is submitted
// (apply_queued_casters, launch_queued_passes).  Copies the view blocks; launches nothing, waits for nothing.
extern "C" int bbr_queue_shadow_caster(bbr_context *c, int32_t caster, int32_t light_index, int32_t n_faces, const void *light_view_blocks,
                                       float bias) {
  if (!c) return BBR_ERR_INVALID_ARGUMENT;
  if (int rc = check_caster_request(c, "queue_shadow_caster", caster, light_index, n_faces, light_view_blocks, bias, true)) return rc;
  // (a second call for the slot in one frame: the last one stands)
  c->shadow.queued[caster] = caster_request(light_index, n_faces, light_view_blocks, bias, true);
  return BBR_OK;
}

extern "C" int bbr_shadow_queue_counts(const bbr_context *c, uint64_t *out_queued_passes, uint64_t *out_drains) {
  if (!c) return BBR_ERR_INVALID_ARGUMENT;
  if (out_queued_passes) *out_queued_passes = c->shadow_queue_passes;
  if (out_drains) *out_drains = c->shadow_queue_drains;
  return BBR_OK;
}

extern "C" int bbr_drop_shadow_caster(bbr_context *c, int32_t caster) {
  if (!c) return BBR_ERR_INVALID_ARGUMENT;
  BBR_ON_DEVICE(c);
  if (caster < 0 || caster >= kMaxShadowCasters) return fail(c, BBR_ERR_INVALID_ARGUMENT, "drop_shadow_caster: caster outside 0 .. 7");
  ShadowSlot &cs = c->shadow.slot[caster];
  if (!cs.valid) return BBR_OK;
  int rc = sync_and_fix(c, nullptr);  // the frames in flight read the table and the maps
  if (rc) return rc;
  cs.valid = false;
  if (!c->in_frame) c->shadow.queued[caster].on = false;  // (as in render_shadow_faces)
  rc = upload_caster_table(c);
  cs = ShadowSlot();
  return rc;
}

extern "C" int bbr_get_shadow_casters(bbr_context *c, int32_t *out_light_index, int32_t *out_faces) {
  if (!c) return BBR_ERR_INVALID_ARGUMENT;
  if (!out_light_index || !out_faces) return fail(c, BBR_ERR_INVALID_ARGUMENT, "get_shadow_casters: NULL");
  for (int s = 0; s < kMaxShadowCasters; ++s) {
    const ShadowSlot &cs = c->shadow.slot[s];
    const bool used = c->shadow_map > 0 && cs.valid;
    out_light_index[s] = used ? cs.args.light : -1;
    out_faces[s] = used ? cs.args.faces : 0;
  }
  return BBR_OK;
}

// `unused`: what a slot not in use is answered with (the calls of slot 0 from before there were slots: BBR_ERR_NOT_IN_FRAME)
static int read_shadow_caster_face(bbr_context *c, int32_t caster, int32_t face, float *host, int unused) {
  if (!c) return BBR_ERR_INVALID_ARGUMENT;
  BBR_ON_DEVICE(c);
  if (!host) return fail(c, BBR_ERR_INVALID_ARGUMENT, "read_shadow_map: NULL");
  if (c->shadow_map <= 0) return fail(c, BBR_ERR_INVALID_ARGUMENT, "read_shadow_map: option shadow_map is 0");
  if (caster < 0 || caster >= kMaxShadowCasters) return fail(c, BBR_ERR_INVALID_ARGUMENT, "read_shadow_caster_face: caster outside 0 .. 7");
  const ShadowSlot &cs = c->shadow.slot[caster];
  if (!cs.valid) return fail(c, unused, "read_shadow_map: no map rendered (bbr_render_shadow_map, bbr_render_shadow_caster)");
  if (face < 0 || face >= cs.args.faces) return fail(c, BBR_ERR_INVALID_ARGUMENT, "read_shadow_face: face outside 0 .. F - 1");
  const size_t texels = (size_t)c->shadow_map * c->shadow_map;
  // (a queued pass may still be on the GPU, or have overflowed with its frame: the read-back drains, like the others)
  if (c->shadow.pass_queued)
    if (int rc = sync_and_fix(c, nullptr)) return rc;
  HIP_TRY(c, hipMemcpy(host, c->shadow.slot[caster].args.map + (size_t)face * texels, texels * sizeof(float), hipMemcpyDeviceToHost));
  return BBR_OK;
}

extern "C" int bbr_read_shadow_face(bbr_context *c, int32_t face, float *host) {
  return read_shadow_caster_face(c, 0, face, host, BBR_ERR_NOT_IN_FRAME);
}
extern "C" int bbr_read_shadow_caster_face(bbr_context *c, int32_t caster, int32_t face, float *host) {
  return read_shadow_caster_face(c, caster, face, host, BBR_ERR_INVALID_ARGUMENT);
}

extern "C" int bbr_read_shadow_map(bbr_context *c, float *host) { return bbr_read_shadow_face(c, 0, host); }

// The class (and, F >= 2, the deciding face) of every pixel of the last frame: the DUMP form of k_shade_shadow /
// k_shade_shadow_faces (with it the surface dump, which is dropped).  With one face the face index follows from the class.
enum class ShadowDump { kMask, kFace, kTaps };
// One re-render dumps one caster slot.  With a slot other than 0 in use the kernel is k_shade_shadow_casters, whose DUMP form
// writes all three outputs itself, whatever F and R.
static int read_shadow_classes(bbr_context *c, const std::string &who, uint8_t *host, ShadowDump want, int32_t caster = 0) {
  const bool want_face = want == ShadowDump::kFace;
  if (!c) return BBR_ERR_INVALID_ARGUMENT;
  BBR_ON_DEVICE(c);
  if (!host) return fail(c, BBR_ERR_INVALID_ARGUMENT, who + ": NULL");
  if (caster < 0 || caster >= kMaxShadowCasters) return fail(c, BBR_ERR_INVALID_ARGUMENT, who + ": caster outside 0 .. 7");
  if (int rc = refuse_supersampled(c, who.c_str())) return rc;
  FrameMode mode = frame_mode(c);
  if (!mode.shadow || !c->shadow.slot[caster].valid)
    return fail(c, BBR_ERR_INVALID_ARGUMENT, who + ": no shadow map in use (option shadow_map, bbr_render_shadow_map, bbr_render_shadow_caster)");
  if (!c->have_frame || c->last_slot < 0) return fail(c, BBR_ERR_NOT_IN_FRAME, who + ": nothing rendered");
  if (c->world > 1) return fail(c, BBR_ERR_INVALID_ARGUMENT, who + ": not available on a partitioned context");
  const size_t pixels = (size_t)c->width * c->height;
  int rc = BBR_OK;
  if (mode.shadow_casters) mode.shadow_faces = true;  // (below: the kernel writes the face index and k itself)
  const bool want_taps = want == ShadowDump::kTaps && (mode.shadow_filter || mode.shadow_casters);  // (R = 0: K = 1, k follows from the class)
  c->dump_shadow_slot = caster;
  for (DeviceBuffer<uint8_t> *b : {mode.shadow_faces ? &c->d_shadow_face : nullptr, (want_taps || mode.shadow_casters) ? &c->d_shadow_taps : nullptr}) {
    if (!b || rc != BBR_OK) continue;  // (an uncovered pixel keeps the fill: face 255, k 255)
    hipError_t e = b->ensure(pixels);
    if (e == hipSuccess) e = hipMemset(b->ptr, 0xFF, pixels);
    if (e == hipSuccess) e = hipStreamSynchronize(nullptr);
    if (e != hipSuccess) rc = fail(c, BBR_ERR_HIP, who + ": " + hipGetErrorString(e));
  }
  if (rc == BBR_OK) {
    c->dump_surface = true;
    rc = rerender_with(c, &bbr_context::dump_shadow_mask);
    c->dump_surface = false;
  }
  if (rc == BBR_OK) {
    const uint8_t *src = (want_face && mode.shadow_faces) ? c->d_shadow_face.ptr : (want_taps ? c->d_shadow_taps.ptr : c->d_shadow_mask.ptr);
    hipError_t e = hipMemcpy(host, src, pixels, hipMemcpyDeviceToHost);
    if (e != hipSuccess) rc = fail(c, BBR_ERR_HIP, who + ": " + hipGetErrorString(e));
    else if (want_face && !mode.shadow_faces)
      for (size_t i = 0; i < pixels; ++i) host[i] = (host[i] == kShadowLit || host[i] == kShadowShadowed || host[i] == kShadowPartial) ? 0 : 255;
    else if (want == ShadowDump::kTaps && !want_taps)
      for (size_t i = 0; i < pixels; ++i) host[i] = host[i] == kShadowLit ? 1 : (host[i] == kShadowShadowed ? 0 : 255);
  }
  c->d_shadow_mask.release();  // (uncovered pixels are the zeros of a fresh buffer)
  c->d_shadow_face.release();
  c->d_shadow_taps.release();
  c->d_surface.release();
  c->dump_shadow_slot = 0;
  return rc;
}

extern "C" int bbr_read_shadow_mask(bbr_context *c, uint8_t *host) {
  return read_shadow_classes(c, "read_shadow_mask", host, ShadowDump::kMask);
}
extern "C" int bbr_read_shadow_face_index(bbr_context *c, uint8_t *host) {
  return read_shadow_classes(c, "read_shadow_face_index", host, ShadowDump::kFace);
}
// k, the number of lit taps, of every pixel of the last frame (option "shadow_filter"; 255 where the class is 0 or OUTSIDE)
extern "C" int bbr_read_shadow_taps(bbr_context *c, uint8_t *host) {
  return read_shadow_classes(c, "read_shadow_taps", host, ShadowDump::kTaps);
}
// ... and of one caster slot each
extern "C" int bbr_read_shadow_caster_mask(bbr_context *c, int32_t caster, uint8_t *host) {
  return read_shadow_classes(c, "read_shadow_caster_mask", host, ShadowDump::kMask, caster);
}
extern "C" int bbr_read_shadow_caster_face_index(bbr_context *c, int32_t caster, uint8_t *host) {
  return read_shadow_classes(c, "read_shadow_caster_face_index", host, ShadowDump::kFace, caster);
}
extern "C" int bbr_read_shadow_caster_taps(bbr_context *c, int32_t caster, uint8_t *host) {
  return read_shadow_classes(c, "read_shadow_caster_taps", host, ShadowDump::kTaps, caster);
}

// ================================================================================================
// GUI pass (src/main.cpp:172): the back end's draw lists blended into the presented image
// ================================================================================================

extern "C" int bbr_ui_validate(const bbr_ui_draw *draw, int32_t fb_width, int32_t fb_height, int32_t *out_box) {
  return ui_validate(draw, fb_width, fb_height, out_box);
}

extern "C" int bbr_upload_ui_texture(bbr_context *c, const uint8_t *rgba8, int32_t w, int32_t h, int32_t *out_texture) {
  if (!c) return BBR_ERR_INVALID_ARGUMENT;
  BBR_ON_DEVICE(c);
  if (!rgba8 || !out_texture || w <= 0 || h <= 0 || w > 16384 || h > 16384)
    return fail(c, BBR_ERR_INVALID_ARGUMENT, "upload_ui_texture: null input or size outside 1..16384");
  bbr_context::UiTexture t;
  const size_t bytes = (size_t)w * h * 4;
  HIP_TRY(c, t.d_texels.ensure((size_t)w * h));
  const hipError_t e = upload_sync(t.d_texels.ptr, rgba8, bytes);
  if (e != hipSuccess) return fail(c, BBR_ERR_HIP, std::string("upload_ui_texture: ") + hipGetErrorString(e));
  t.w = w;
  t.h = h;
  // handles start at 1: 0 is the GUI's null ImTextureID.  The lowest freed handle is handed out again, so a host that
  // rebuilds its atlas again and again does not grow the table.
  size_t at = 0;
  while (at < c->ui_textures.size() && c->ui_textures[at].d_texels.ptr) ++at;
  if (at == c->ui_textures.size()) c->ui_textures.push_back(std::move(t));
  else c->ui_textures[at] = std::move(t);
  *out_texture = (int32_t)at + 1;
  return BBR_OK;
}

extern "C" int bbr_free_ui_texture(bbr_context *c, int32_t texture) {
  if (!c) return BBR_ERR_INVALID_ARGUMENT;
  if (!is_live(c)) return BBR_ERR_BAD_HANDLE;
  BBR_ON_DEVICE(c);
  if (texture < 1 || texture > (int32_t)c->ui_textures.size() || !c->ui_textures[texture - 1].d_texels.ptr)
    return fail(c, BBR_ERR_BAD_HANDLE, "free_ui_texture: bad handle");
  int rc = drain(c);  // a queued GUI pass may still sample it
  if (rc) return rc;
  c->ui_textures[texture - 1] = bbr_context::UiTexture();
  return BBR_OK;
}

extern "C" int bbr_draw_ui(bbr_context *c, const bbr_ui_draw *draw) {
  if (!c) return BBR_ERR_INVALID_ARGUMENT;
  BBR_ON_DEVICE(c);
  if (!draw) return fail(c, BBR_ERR_INVALID_ARGUMENT, "draw_ui: NULL");
  if (!c->have_frame || c->last_slot < 0) return fail(c, BBR_ERR_NOT_IN_FRAME, "draw_ui: nothing rendered");
  if (c->world > 1) return fail(c, BBR_ERR_INVALID_ARGUMENT, "draw_ui: not available with a partition");
  FrameSlot &s = c->slots[c->last_slot];
  if (!s.present.active || !s.present.out)
    return fail(c, BBR_ERR_NOT_IN_FRAME, "draw_ui: call bbr_present first (the GUI goes into the presented image)");
  forget_image(c);
  // int fb_width = (int)(DisplaySize.x * FramebufferScale.x), as the back end computes it
  for (int k = 0; k < 2; ++k) {
    const float f = draw->display_size[k] * draw->framebuffer_scale[k];
    if (!(draw->display_size[k] > 0.0f) || !(f >= 0.0f && f < 65536.0f) || (int32_t)f != (k == 0 ? c->width : c->height))
      return fail(c, BBR_ERR_INVALID_ARGUMENT, "draw_ui: (int)(display_size * framebuffer_scale) is not the context's extent");
  }
  int32_t box[4];
  if (ui_validate(draw, c->width, c->height, box) != BBR_OK)
    return fail(c, BBR_ERR_INVALID_ARGUMENT, "draw_ui: malformed draw data (see bbr_ui_validate)");
  for (uint32_t i = 0; i < draw->n_cmds; ++i) {
    const int32_t t = draw->cmds[i].texture;
    if (draw->cmds[i].elem_count && (t < 1 || t > (int32_t)c->ui_textures.size() || !c->ui_textures[t - 1].d_texels.ptr))
      return fail(c, BBR_ERR_INVALID_ARGUMENT, "draw_ui: a command names a texture that is not alive");
  }
  if (box[2] <= box[0] || box[3] <= box[1]) return BBR_OK;  // nothing can pass a scissor

  // ---- staging: [commands | vertices | indices]; a command whose scissor admits nothing has no triangles ----
  std::vector<UiCmd> cmds;
  cmds.reserve(draw->n_cmds);
  uint64_t n_tris64 = 0;
  for (uint32_t i = 0; i < draw->n_cmds; ++i) {
    const bbr_ui_cmd &in = draw->cmds[i];
    int32_t sc[4];
    if (!in.elem_count || !ui_scissor(in.clip_rect, *draw, c->width, c->height, sc)) continue;
    const bbr_context::UiTexture &t = c->ui_textures[in.texture - 1];
    UiCmd u = {};
    u.texels = t.d_texels.ptr; u.tw = t.w; u.th = t.h;
    u.vtx_offset = in.vtx_offset; u.idx_offset = in.idx_offset;
    u.first_tri = (uint32_t)n_tris64;
    u.sx0 = sc[0]; u.sy0 = sc[1]; u.sx1 = sc[2]; u.sy1 = sc[3];
    cmds.push_back(u);
    n_tris64 += in.elem_count / 3u;
  }
  if (!n_tris64 || n_tris64 > 0x7FFFFFFFull) return n_tris64 ? fail(c, BBR_ERR_TOO_MANY_PRIMITIVES, "draw_ui: too many triangles") : (int)BBR_OK;
  const uint32_t n_tris = (uint32_t)n_tris64;
  const size_t cmds_bytes = cmds.size() * sizeof(UiCmd);
  const size_t vtx_at = (cmds_bytes + 15) & ~(size_t)15, vtx_bytes = (size_t)draw->n_vertices * kUiVertexBytes;
  const size_t idx_at = (vtx_at + vtx_bytes + 15) & ~(size_t)15, idx_bytes = (size_t)draw->n_indices * sizeof(uint16_t);
  const size_t total = idx_at + idx_bytes;

  int rc = ensure_srgb_tables(c);
  if (rc) return rc;
  if (!c->d_ui_dec.ptr) {
    float dec[256];
    ui_dec_table(dec);
    HIP_TRY(c, c->d_ui_dec.ensure(256));
    HIP_TRY(c, upload_sync(c->d_ui_dec.ptr, dec, sizeof dec));
  }
  auto &ui = s.ui;
  HIP_TRY(c, ui.ev_copied.ensure(hipEventDisableTiming));
  // Each buffer is tested against its own capacity, so that a call after a failed allocation grows what is still missing.
  if (total > ui.h_staging.cap || total > ui.d_staging.cap || n_tris > ui.d_tris.cap || n_tris > ui.d_boxes.cap) {
    // growing: everything queued for this slot (an earlier GUI pass included) must have left the buffers first
    HIP_TRY(c, s.wait_idle());
    ui.copy_pending = false;
    if (total > ui.h_staging.cap) HIP_TRY(c, ui.h_staging.ensure(std::max<size_t>(total * 2, 1 << 16)));
    if (total > ui.d_staging.cap) HIP_TRY(c, ui.d_staging.ensure(ui.h_staging.cap));  // (the device block has a capacity of its own)
    const size_t tri_cap = std::max<size_t>((size_t)n_tris * 2, 4096);
    if (n_tris > ui.d_tris.cap) HIP_TRY(c, ui.d_tris.ensure(tri_cap));
    if (n_tris > ui.d_boxes.cap) HIP_TRY(c, ui.d_boxes.ensure(tri_cap));
  }
  if (ui.copy_pending) {  // an earlier call for this slot: its copy must have read the staging before it is overwritten
    HIP_TRY(c, hipEventSynchronize(ui.ev_copied));
    ui.copy_pending = false;
  }
  uint8_t *h = ui.h_staging.ptr;
  std::memcpy(h, cmds.data(), cmds_bytes);
  std::memcpy(h + vtx_at, draw->vertices, vtx_bytes);
  std::memcpy(h + idx_at, draw->indices, idx_bytes);

  // behind the presentation (and whatever was queued on the image since), on the stream the presentation used
  const hipStream_t ps = c->slot_present_stream(s);
  HIP_TRY(c, s.follow(ps));
  HIP_TRY(c, hipMemcpyAsync(ui.d_staging.ptr, h, total, hipMemcpyHostToDevice, ps));
  HIP_TRY(c, hipEventRecord(ui.ev_copied, ps));
  ui.copy_pending = true;
  const UiTransform t = ui_transform(*draw, c->width, c->height);
  UiParams p = {};
  for (int k = 0; k < 2; ++k) {
    p.scale[k] = t.scale[k];
    p.translate[k] = t.translate[k];
    p.half[k] = t.half[k];
  }
  p.width = c->width;
  p.height = c->height;
  hipLaunchKernelGGL(k_ui_setup, dim3((n_tris + 255u) / 256u), dim3(256), 0, ps, p,
                     reinterpret_cast<const UiCmd *>(ui.d_staging.ptr), (uint32_t)cmds.size(),
                     reinterpret_cast<const uint32_t *>(ui.d_staging.ptr + vtx_at),
                     reinterpret_cast<const uint16_t *>(ui.d_staging.ptr + idx_at), n_tris, ui.d_tris.ptr, ui.d_boxes.ptr);
  // only the tiles of the union of the scissors
  const int32_t tx0 = box[0] / kUiTile, ty0 = box[1] / kUiTile;
  const int32_t tx1 = (box[2] + kUiTile - 1) / kUiTile, ty1 = (box[3] + kUiTile - 1) / kUiTile;
  hipLaunchKernelGGL(k_ui_tiles, dim3((unsigned)(tx1 - tx0), (unsigned)(ty1 - ty0)), dim3(kUiThreads), 0, ps, ui.d_tris.ptr,
                     ui.d_boxes.ptr, n_tris, tx0, ty0, c->width, c->height, c->d_ui_dec.ptr, c->d_srgb_tables.ptr,
                     s.present.out);
  HIP_TRY(c, hipGetLastError());
  if (s.mode.fused && s.present.copy_to) {
    // fused presentation into a caller's buffer: bbr_present copied the slot's image there before the GUI was in it, so the
    // rows the pass may have touched (those of the union box, whole and contiguous) are copied again behind it
    const size_t first = (size_t)box[1] * c->width, count = (size_t)(box[3] - box[1]) * c->width;
    HIP_TRY(c, hipMemcpyAsync(static_cast<uint32_t *>(s.present.copy_to) + first, s.present.out + first, count * 4,
                              hipMemcpyDeviceToDevice, ps));
  }
  HIP_TRY(c, s.busy_until(ps));  // ... until the GUI is in the image
  return BBR_OK;
}

// ================================================================================================
// C ABI
// ================================================================================================

extern "C" {

int bbr_device_count(void) {
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess) return 0;
  return n;
}

const char *bbr_last_error(const bbr_context *ctx) { return ctx ? ctx->last_error.c_str() : g_create_error.c_str(); }

// Everything a context owns, whatever state its construction reached (bbr_destroy, and bbr_create when a step fails): the
// context's members own themselves, and nothing is freed before the drain.
static void release_context(bbr_context *c) {
  (void)hipSetDevice(c->device);
  (void)drain(c);
  if (c->comm) (void)g_rccl.comm_destroy(c->comm);
  delete c;
}

int bbr_create(int32_t width, int32_t height, int32_t device, bbr_context **out_ctx) {
  if (!out_ctx) return fail(nullptr, BBR_ERR_INVALID_ARGUMENT, "out_ctx is NULL");
  *out_ctx = nullptr;
  if (width <= 0 || height <= 0 || width > kMaxExtent || height > kMaxExtent)
    return fail(nullptr, BBR_ERR_INVALID_ARGUMENT, "width/height out of range");
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess || n <= 0)
    return fail(nullptr, BBR_ERR_NO_DEVICE, "no HIP device: this library has no CPU fallback");
  if (device < 0 || device >= n) return fail(nullptr, BBR_ERR_INVALID_ARGUMENT, "device index out of range");
  bbr_context *c = new bbr_context();
  c->device = device;
  c->width = width;
  c->height = height;
#define CREATE_TRY(expr)                                                                       \
  do {                                                                                         \
    hipError_t _e = (expr);                                                                    \
    if (_e != hipSuccess) {                                                                    \
      g_create_error = std::string(#expr) + ": " + hipGetErrorString(_e);                      \
      release_context(c);                                                                      \
      return _e == hipErrorOutOfMemory ? BBR_ERR_OUT_OF_MEMORY : BBR_ERR_HIP;                  \
    }                                                                                          \
  } while (0)
  CREATE_TRY(hipSetDevice(device));
  {
    int cus = 0;
    CREATE_TRY(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, device));
    if (cus > 0) c->n_cus = cus;
  }
  {
    // geometry + raster are latency-bound and short: give them the high-priority queue so that their workgroups
    // slot in between the (ALU-bound, GPU-filling) shade kernel of the previous frame
    int prio_low = 0, prio_high = 0;
    CREATE_TRY(hipDeviceGetStreamPriorityRange(&prio_low, &prio_high));
    // (measured on C3/C5: swapping or equalising the two priorities changes the pipelined frame time by < 2 %)
    CREATE_TRY(c->s_geom.create(hipStreamNonBlocking, prio_high));
    // (created here, next to s_geom: a stream made later, once the others are busy, was measured to serialise with them)
    CREATE_TRY(c->s_raster.create(hipStreamNonBlocking, prio_high));
    CREATE_TRY(c->s_shade.create(hipStreamNonBlocking, prio_low));
    CREATE_TRY(c->s_present.create(hipStreamNonBlocking, prio_low));
  }
  // `default` material maps (resources/pbr/default/*.png are uniform images): 1x1 RGBA8 each -- the table a packed material
  // broadcasts from (bb_pack.h)
  CREATE_TRY(c->d_default_texels.ensure(sizeof kDefaultTexel));
  CREATE_TRY(upload_sync(c->d_default_texels.ptr, kDefaultTexel, sizeof kDefaultTexel));
#undef CREATE_TRY
  {
    std::lock_guard<std::mutex> lock(g_live_mutex);
    g_live.insert(c);
  }
  *out_ctx = c;
  return BBR_OK;
}

int bbr_destroy(bbr_context *c) {
  if (!c) return BBR_ERR_INVALID_ARGUMENT;
  {
    std::lock_guard<std::mutex> lock(g_live_mutex);
    if (!g_live.erase(c)) return BBR_ERR_BAD_HANDLE;  // never created, or destroyed already
  }
  release_context(c);
  return BBR_OK;
}

int bbr_upload_mesh(bbr_context *c, const void *vertices, uint32_t n_vertices, const uint32_t *indices,
                    uint32_t n_indices, int32_t *out_mesh) {
  if (!c) return BBR_ERR_INVALID_ARGUMENT;
  BBR_ON_DEVICE(c);
  if (!vertices || !n_vertices || !out_mesh) return fail(c, BBR_ERR_INVALID_ARGUMENT, "upload_mesh: null/empty input");
  if (indices) {
    for (uint32_t i = 0; i < n_indices; ++i)
      if (indices[i] >= n_vertices) return fail(c, BBR_ERR_INVALID_ARGUMENT, "upload_mesh: index out of range");
  } else if (n_indices) {
    return fail(c, BBR_ERR_INVALID_ARGUMENT, "upload_mesh: n_indices without indices");
  }
  Mesh m;
  m.n_vertices = n_vertices;
  m.n_indices = indices ? n_indices : 0;
  // (a failure half way gives back what the mesh already owns: the handle never comes to exist, so nobody else could)
  HIP_TRY(c, m.d_vertices.ensure(n_vertices));
  HIP_TRY(c, upload_sync(m.d_vertices.ptr, vertices, (size_t)n_vertices * sizeof(Vertex)));
  if (m.n_indices) {
    HIP_TRY(c, m.d_indices.ensure(n_indices));
    HIP_TRY(c, upload_sync(m.d_indices.ptr, indices, (size_t)n_indices * sizeof(uint32_t)));
  }
  m.alive = true;
  ++c->resource_epoch;
  c->meshes.push_back(std::move(m));
  *out_mesh = (int32_t)c->meshes.size() - 1;
  return BBR_OK;
}

int bbr_free_mesh(bbr_context *c, int32_t mesh) {
  if (!c) return BBR_ERR_INVALID_ARGUMENT;
  if (!is_live(c)) return BBR_ERR_BAD_HANDLE;  // the context is gone and took the mesh with it (checked before c is touched)
  BBR_ON_DEVICE(c);
  if (mesh < 0 || mesh >= (int32_t)c->meshes.size() || !c->meshes[mesh].alive)
    return fail(c, BBR_ERR_BAD_HANDLE, "free_mesh: bad handle");
  int rc = drain(c);
  if (rc) return rc;
  bool repaired = false;  // (a queued shadow pass that overflowed is rendered again while its frame's draws can still be read)
  if ((rc = settle_queued_passes(c, &repaired)) != BBR_OK) return rc;
  c->meshes[mesh] = Mesh();
  ++c->resource_epoch;
  c->have_frame = false;
  return BBR_OK;
}

int bbr_upload_material(bbr_context *c, const bbr_image maps[BBR_MAP_COUNT], int32_t *out_material) {
  if (!c) return BBR_ERR_INVALID_ARGUMENT;
  BBR_ON_DEVICE(c);
  if (!maps || !out_material) return fail(c, BBR_ERR_INVALID_ARGUMENT, "upload_material: null input");
  Material m;  // (a failed upload gives back what it had already allocated)
  for (int i = 0; i < kMapCount; ++i) {
    const bbr_image &im = maps[i];
    if (im.rgba && im.width > 0 && im.height > 0) {
      if (im.width > 16384 || im.height > 16384) return fail(c, BBR_ERR_INVALID_ARGUMENT, "upload_material: map too large");
      size_t bytes = (size_t)im.width * im.height * 4;
      HIP_TRY(c, m.d_texels[i].ensure(bytes));
      HIP_TRY(c, upload_sync(m.d_texels[i].ptr, im.rgba, bytes));
      m.desc.maps[i] = TexDesc{m.d_texels[i].ptr, im.width, im.height};
    } else {
      // missing map => the `default` material's map (src/render.cpp:1328-1336)
      m.desc.maps[i] = TexDesc{c->d_default_texels.ptr + 4 * i, 1, 1};
    }
  }
  // Interleave the five shaded maps when the supplied ones agree on one size (bb_pack.h; missing maps are uniform, so they
  // broadcast): a bilinear tap then costs one 12-byte load of a 9-byte record instead of five 4-byte loads from five arrays.
  {
    const PackPlan plan = pack_plan(maps);
    if (plan.packable) {
      std::vector<uint8_t> host(plan.bytes);
      pack_fill(maps, plan, host.data());
      HIP_TRY(c, m.d_packed.ensure(host.size()));
      HIP_TRY(c, upload_sync(m.d_packed.ptr, host.data(), host.size()));
      m.desc.packed = m.d_packed.ptr;
      m.desc.pw = plan.pw;
      m.desc.ph = plan.ph;
    }
  }
  if (c->mip_levels > 1) {
    const int rc = build_chain(c, m);
    if (rc) return rc;
  }
  m.alive = true;
  c->materials.push_back(std::move(m));
  c->materials_dirty = true;
  ++c->resource_epoch;
  *out_material = (int32_t)c->materials.size() - 1;
  return BBR_OK;
}

int bbr_free_material(bbr_context *c, int32_t material) {
  if (!c) return BBR_ERR_INVALID_ARGUMENT;
  if (!is_live(c)) return BBR_ERR_BAD_HANDLE;  // the context is gone and took the material with it (checked before c is touched)
  BBR_ON_DEVICE(c);
  if (material < 0 || material >= (int32_t)c->materials.size() || !c->materials[material].alive)
    return fail(c, BBR_ERR_BAD_HANDLE, "free_material: bad handle");
  int rc = drain(c);
  if (rc) return rc;
  bool repaired = false;  // (as in bbr_free_mesh)
  if ((rc = settle_queued_passes(c, &repaired)) != BBR_OK) return rc;
  c->materials[material] = Material();
  c->materials_dirty = true;
  ++c->resource_epoch;
  c->have_frame = false;
  return BBR_OK;
}

int bbr_pack_material(const bbr_image maps[BBR_MAP_COUNT], int32_t *out_packable, int32_t *out_width, int32_t *out_height,
                      uint64_t *out_bytes, uint8_t *out_or_null, uint64_t capacity) {
  if (!maps || !out_packable || !out_width || !out_height || !out_bytes) return BBR_ERR_INVALID_ARGUMENT;
  for (int i = 0; i < kMapCount; ++i)
    if (map_supplied(maps[i]) && (maps[i].width > 16384 || maps[i].height > 16384)) return BBR_ERR_INVALID_ARGUMENT;
  const PackPlan plan = pack_plan(maps);
  *out_packable = plan.packable ? 1 : 0;
  *out_width = plan.packable ? plan.pw : 0;
  *out_height = plan.packable ? plan.ph : 0;
  *out_bytes = plan.bytes;
  if (out_or_null && plan.packable) {
    if (capacity < plan.bytes) return BBR_ERR_CAPACITY;
    pack_fill(maps, plan, out_or_null);
  }
  return BBR_OK;
}

int bbr_set_frame_uniforms(bbr_context *c, const void *block) {
  if (!c) return BBR_ERR_INVALID_ARGUMENT;
  BBR_ON_DEVICE(c);
  if (!block) return fail(c, BBR_ERR_INVALID_ARGUMENT, "set_frame_uniforms: NULL");
  // the reference asserts NumLights < MAX_NUM_LIGHTS (src/main.cpp:1289-1290); a refused block leaves the context's own as it was
  int32_t num_lights;
  std::memcpy(&num_lights, static_cast<const char *>(block) + offsetof(FrameUniformBlock, num_lights), sizeof num_lights);
  if (num_lights < 0 || num_lights >= kMaxNumLights)
    return fail(c, BBR_ERR_INVALID_ARGUMENT, "set_frame_uniforms: NumLights must be in [0, 100)");
  std::memcpy(&c->frame_u, block, sizeof(FrameUniformBlock));
  return BBR_OK;
}

int bbr_set_view_uniforms(bbr_context *c, const void *block) {
  if (!c) return BBR_ERR_INVALID_ARGUMENT;
  BBR_ON_DEVICE(c);
  if (!block) return fail(c, BBR_ERR_INVALID_ARGUMENT, "set_view_uniforms: NULL");
  std::memcpy(&c->view_u, block, sizeof(ViewUniformBlock));
  return BBR_OK;
}

int bbr_begin_frame(bbr_context *c) {
  if (!c) return BBR_ERR_INVALID_ARGUMENT;
  BBR_ON_DEVICE(c);
  c->draws.clear();
  c->host_instances.clear();
  c->n_prims = 0;
  c->in_frame = true;
  c->have_frame = false;
  for (CasterRequest &q : c->shadow.queued) q.on = false;  // (bbr_queue_shadow_caster: they belonged to the frame before)
  return BBR_OK;
}

int bbr_draw(bbr_context *c, int32_t mesh, int32_t material, const void *instance_blocks, uint32_t n_instances) {
  if (!c) return BBR_ERR_INVALID_ARGUMENT;
  BBR_ON_DEVICE(c);
  if (!c->in_frame) return fail(c, BBR_ERR_NOT_IN_FRAME, "draw outside begin_frame/end_frame");
  if (mesh < 0 || mesh >= (int32_t)c->meshes.size() || !c->meshes[mesh].alive)
    return fail(c, BBR_ERR_BAD_HANDLE, "draw: bad mesh handle");
  if (material < 0 || material >= (int32_t)c->materials.size() || !c->materials[material].alive)
    return fail(c, BBR_ERR_BAD_HANDLE, "draw: bad material handle");
  if (n_instances && !instance_blocks) return fail(c, BBR_ERR_INVALID_ARGUMENT, "draw: NULL instance data");
  const Mesh &m = c->meshes[mesh];
  uint32_t tris = (m.d_indices.ptr ? m.n_indices : m.n_vertices) / 3;
  uint64_t total = (uint64_t)c->n_prims + (uint64_t)tris * n_instances;
  if (total >= kMaxPrims) return fail(c, BBR_ERR_TOO_MANY_PRIMITIVES, "draw: more than 2^29 primitives in one frame");
  RecordedDraw rd;
  rd.mesh = mesh;
  rd.material = material;
  rd.n_instances = n_instances;
  rd.first_instance = (uint32_t)c->host_instances.size();
  rd.first_prim = c->n_prims;
  rd.tris_per_instance = tris;
  const InstanceBlock *ib = static_cast<const InstanceBlock *>(instance_blocks);
  c->host_instances.insert(c->host_instances.end(), ib, ib + n_instances);
  c->draws.push_back(rd);
  c->n_prims = (uint32_t)total;
  return BBR_OK;
}

int bbr_end_frame(bbr_context *c) {
  if (!c) return BBR_ERR_INVALID_ARGUMENT;
  BBR_ON_DEVICE(c);
  if (!c->in_frame) return fail(c, BBR_ERR_NOT_IN_FRAME, "end_frame without begin_frame");
  c->in_frame = false;
  c->have_frame = true;
  return submit_frame(c);
}

int bbr_replay_frame(bbr_context *c) {
  if (!c) return BBR_ERR_INVALID_ARGUMENT;
  BBR_ON_DEVICE(c);
  if (!c->have_frame) return fail(c, BBR_ERR_NOT_IN_FRAME, "replay_frame: no recorded frame");
  return submit_frame(c);
}

int bbr_synchronize(bbr_context *c) {
  if (!c) return BBR_ERR_INVALID_ARGUMENT;
  BBR_ON_DEVICE(c);
  return sync_and_fix(c, nullptr);
}

int bbr_read_framebuffer(bbr_context *c, float *host) {
  if (!c) return BBR_ERR_INVALID_ARGUMENT;
  BBR_ON_DEVICE(c);
  if (!host) return fail(c, BBR_ERR_INVALID_ARGUMENT, "read_framebuffer: NULL");
  if (c->world > 1) return fail(c, BBR_ERR_INVALID_ARGUMENT, "read_framebuffer on a partitioned context: use bbr_read_shard");
  if (!c->have_frame) return fail(c, BBR_ERR_NOT_IN_FRAME, "read_framebuffer: nothing rendered");
  if (c->last_slot >= 0 && c->slots[c->last_slot].mode.fused)
    return fail(c, BBR_ERR_INVALID_ARGUMENT, "read_framebuffer: the frame was rendered with option present_fused (no fp32 frame); use bbr_read_presented");
  int rc = sync_and_fix(c, nullptr);
  if (rc) return rc;
  HIP_TRY(c, hipMemcpy(host, last_output(c), (size_t)c->width * c->height * 16, hipMemcpyDeviceToHost));
  return BBR_OK;
}

int bbr_read_shard(bbr_context *c, float *host) {
  if (!c) return BBR_ERR_INVALID_ARGUMENT;
  BBR_ON_DEVICE(c);
  if (!host) return fail(c, BBR_ERR_INVALID_ARGUMENT, "read_shard: NULL");
  if (!c->have_frame) return fail(c, BBR_ERR_NOT_IN_FRAME, "read_shard: nothing rendered");
  if (c->last_slot >= 0 && c->slots[c->last_slot].mode.fused)
    return fail(c, BBR_ERR_INVALID_ARGUMENT, "read_shard: the frame was rendered with option present_fused (no fp32 frame); use bbr_read_presented");
  int rc = sync_and_fix(c, nullptr);
  if (rc) return rc;
  HIP_TRY(c, hipMemcpy(host, last_output(c), c->shard_pixels() * 16, hipMemcpyDeviceToHost));
  return BBR_OK;
}

// rep(s) of every fine pixel of the last frame, row-major, as an index 0 .. n^2 - 1 of its block (the identity without a
// map).  The frame has completed; whole-frame contexts only.
static int read_sample_map_synced(bbr_context *c, uint8_t *host) {
  const FrameSlot &s = c->slots[c->last_slot];
  const int n = s.mode.n;
  const size_t fw = (size_t)c->render_width(), fh = (size_t)c->render_height();
  if (!s.mode.merged) {
    for (size_t y = 0; y < fh; ++y)
      for (size_t x = 0; x < fw; ++x) host[y * fw + x] = (uint8_t)((y % n) * n + (x % n));
    return BBR_OK;
  }
  const size_t pixels = (size_t)c->width * c->height;
  std::vector<unsigned long long> words(s.mode.map_words);
  HIP_TRY(c, hipMemcpy(words.data(), s.d_sample_map.ptr, pixels * sample_map_word_bytes(n), hipMemcpyDeviceToHost));
  const uint16_t *w2 = reinterpret_cast<const uint16_t *>(words.data());
  for (size_t y = 0; y < fh; ++y)
    for (size_t x = 0; x < fw; ++x) {
      const size_t o = (y / n) * (size_t)c->width + x / n;
      const unsigned long long w = n == 2 ? (unsigned long long)w2[o] : words[o];
      host[y * fw + x] = (uint8_t)((w >> (4 * ((y % n) * n + (x % n)))) & (unsigned long long)(n * n - 1));
    }
  return BBR_OK;
}

int bbr_read_samples(bbr_context *c, float *host) {
  if (!c) return BBR_ERR_INVALID_ARGUMENT;
  BBR_ON_DEVICE(c);
  if (!host) return fail(c, BBR_ERR_INVALID_ARGUMENT, "read_samples: NULL");
  if (c->world > 1) return fail(c, BBR_ERR_INVALID_ARGUMENT, "read_samples: not available on a partitioned context");
  if (!c->have_frame || c->last_slot < 0) return fail(c, BBR_ERR_NOT_IN_FRAME, "read_samples: nothing rendered");
  const FrameSlot &s = c->slots[c->last_slot];
  if (!s.mode.resolve) return bbr_read_framebuffer(c, host);  // one sample per pixel: the frame itself
  int rc = sync_and_fix(c, nullptr);
  if (rc) return rc;
  HIP_TRY(c, hipMemcpy(host, s.d_fine.ptr, (size_t)c->render_width() * c->render_height() * 16, hipMemcpyDeviceToHost));
  if (s.mode.merged) {
    // option "sample_shading" 0: g, every sample the value of its representative (a diagnostic: replicated here, on the host;
    // the fine frame holds nothing defined at a sample that is not one).  A representative precedes what it stands for.
    std::vector<uint8_t> rep((size_t)c->render_width() * c->render_height());
    rc = read_sample_map_synced(c, rep.data());
    if (rc) return rc;
    const int n = s.mode.n;
    const size_t fw = (size_t)c->render_width();
    for (size_t y = 0; y < (size_t)c->render_height(); ++y)
      for (size_t x = 0; x < fw; ++x) {
        const int r = rep[y * fw + x];
        const size_t src = ((y / n) * n + (size_t)(r / n)) * fw + (x / n) * n + (size_t)(r % n);
        if (src != y * fw + x) memcpy(host + 4 * (y * fw + x), host + 4 * src, 16);
      }
  }
  return BBR_OK;
}

int bbr_read_sample_map(bbr_context *c, uint8_t *host) {
  if (!c) return BBR_ERR_INVALID_ARGUMENT;
  BBR_ON_DEVICE(c);
  if (!host) return fail(c, BBR_ERR_INVALID_ARGUMENT, "read_sample_map: NULL");
  if (c->world > 1) return fail(c, BBR_ERR_INVALID_ARGUMENT, "read_sample_map: not available on a partitioned context");
  if (!c->have_frame || c->last_slot < 0) return fail(c, BBR_ERR_NOT_IN_FRAME, "read_sample_map: nothing rendered");
  int rc = sync_and_fix(c, nullptr);
  if (rc) return rc;
  return read_sample_map_synced(c, host);
}

int bbr_framebuffer_device_ptr(bbr_context *c, void **out_ptr, uint64_t *out_bytes) {
  if (!c) return BBR_ERR_INVALID_ARGUMENT;
  BBR_ON_DEVICE(c);
  if (!out_ptr) return fail(c, BBR_ERR_INVALID_ARGUMENT, "framebuffer_device_ptr: NULL");
  if (!c->have_frame || c->last_slot < 0) return fail(c, BBR_ERR_NOT_IN_FRAME, "framebuffer_device_ptr: nothing rendered");
  forget_image(c);  // (the caller may write through the pointer before the next frame)
  *out_ptr = (void *)c->slots[c->last_slot].out_used;
  if (out_bytes)
    *out_bytes = c->ext_out ? c->ext_out_bytes : (uint64_t)c->width * std::max(c->height, c->shard_rows()) * 16;
  return BBR_OK;
}

int bbr_set_output_device_ptr(bbr_context *c, void *device_ptr, uint64_t bytes) {
  if (!c) return BBR_ERR_INVALID_ARGUMENT;
  BBR_ON_DEVICE(c);
  if (device_ptr) {
    uint64_t need = (uint64_t)c->shard_pixels() * 16;
    if (bytes < need) return fail(c, BBR_ERR_INVALID_ARGUMENT, "set_output_device_ptr: buffer too small");
    if ((uintptr_t)device_ptr & 15u) return fail(c, BBR_ERR_INVALID_ARGUMENT, "set_output_device_ptr: need 16-byte alignment");
  }
  c->ext_out = device_ptr;
  c->ext_out_bytes = device_ptr ? bytes : 0;
  forget_image(c);
  return BBR_OK;
}

int bbr_set_stream(bbr_context *c, void *stream) {
  if (!c) return BBR_ERR_INVALID_ARGUMENT;
  BBR_ON_DEVICE(c);
  int rc = drain(c);
  if (rc) return rc;
  c->user_stream = (hipStream_t)stream;
  c->frame_counter = 0;
  return BBR_OK;
}

int bbr_wait_event(bbr_context *c, void *hip_event) {
  if (!c) return BBR_ERR_INVALID_ARGUMENT;
  BBR_ON_DEVICE(c);
  if (!hip_event) return fail(c, BBR_ERR_INVALID_ARGUMENT, "wait_event: NULL");
  c->pending_waits.push_back((hipEvent_t)hip_event);  // the next frame's first stream waits for it (which stream that is
                                                      // depends on the stream layout)
  return BBR_OK;
}

int bbr_stream_wait_frame(bbr_context *c, void *stream) {
  if (!c) return BBR_ERR_INVALID_ARGUMENT;
  BBR_ON_DEVICE(c);
  if (!c->have_frame || c->last_slot < 0) return fail(c, BBR_ERR_NOT_IN_FRAME, "stream_wait_frame: nothing rendered");
  HIP_TRY(c, c->slots[c->last_slot].follow((hipStream_t)stream));
  return BBR_OK;
}

int bbr_tile_height(const bbr_context *c, int32_t *out) {
  if (!c || !out) return BBR_ERR_INVALID_ARGUMENT;
  *out = c->tile_h();
  return BBR_OK;
}

int bbr_set_partition(bbr_context *c, int32_t rank, int32_t world, int32_t band_rows) {
  if (!c) return BBR_ERR_INVALID_ARGUMENT;
  BBR_ON_DEVICE(c);
  if (world < 1 || rank < 0 || rank >= world) return fail(c, BBR_ERR_INVALID_ARGUMENT, "set_partition: bad rank/world");
  if (band_rows <= 0) band_rows = c->tile_h();
  if (band_rows % c->tile_h()) return fail(c, BBR_ERR_INVALID_ARGUMENT, "set_partition: band_rows must be a multiple of the tile height");
  if (refused_bloom_partition(c->bloom, world))
    return fail(c, BBR_ERR_INVALID_ARGUMENT, "set_partition: world > 1 is not available with option bloom >= 1 (the chain needs its neighbours' rows)");
  if (refused_auto_partition(c->auto_exposure, world))
    return fail(c, BBR_ERR_INVALID_ARGUMENT, "set_partition: world > 1 is not available with option auto_exposure 1 (metering needs the whole frame: bbr_present_buffer_auto on the gathered one)");
  int rc = drain(c);
  if (rc) return rc;
  c->rank = rank;
  c->world = world;
  c->band_rows = band_rows;
  forget_image(c);
  for (FrameSlot &s : c->slots) {  // (a fine shard's padding rows, and their map words, are the zeros of a fresh buffer)
    s.d_fine.release();
    s.d_fine_depth.release();
    s.d_sample_map.release();
  }
  c->exchange_slot = -1;  // (block sizes change with the partition)
  c->exchange_whole = nullptr;
  if (c->ext_out) {
    uint64_t need = (uint64_t)c->shard_pixels() * 16;
    if (c->ext_out_bytes < need) {
      c->ext_out = nullptr;
      c->ext_out_bytes = 0;
    }
  }
  return BBR_OK;
}

// The render or the output extent changed (bbr_resize, option "supersample"): everything sized by either goes, the flag words
// are forgotten and there is no current frame.  The context is drained.
static void drop_extent_buffers(bbr_context *c) {
  auto drop_slot = [](FrameSlot &s) {
    drop<TileSized>(s);
    drop<ExtentSized>(s);
    s.mode = FrameMode{};
    s.present.active = false;
    s.present.out = nullptr;
    s.present.copy_to = nullptr;
    s.present.auto_e = s.present.metered = false;
    s.bloom_ran = 0;
    s.out_used = nullptr;
    s.in_flight = false;
    s.forget_extent();
    s.forget_image();
  };
  for (FrameSlot &s : c->slots) drop_slot(s);
  drop_slot(c->ov);
  drop<bbr_context::TbnRecords>(c->tbn_pass);
  drop<ExtentDumps>(*c);
  c->bloom_buffer = bbr_context::BloomBuffer();
  c->exposure.last_slot = -1;  // (the histories are no extent's: they stay)
  forget_current_frame(c);  // (the whole frame of the last exchange had the old extent, too)
}

// onWindowResize (src/main.cpp:1042-1061): wait for the device, drop everything whose size follows the swap-chain
// extent, keep meshes, materials and options.  Buffers come back lazily with the next frame.
int bbr_resize(bbr_context *c, int32_t width, int32_t height) {
  if (!c) return BBR_ERR_INVALID_ARGUMENT;
  BBR_ON_DEVICE(c);
  if (width <= 0 || height <= 0 || width > kMaxExtent || height > kMaxExtent)
    return fail(c, BBR_ERR_INVALID_ARGUMENT, "resize: width/height out of range");
  if (int rc = check_render_extent(c, "resize", c->supersample, width, height)) return rc;
  if (c->in_frame) return fail(c, BBR_ERR_INVALID_ARGUMENT, "resize: between begin_frame and end_frame");
  int rc = drain(c);
  if (rc) return rc;
  forget_image(c);
  c->exposure.last_slot = -1;
  if (width == c->width && height == c->height) return BBR_OK;
  c->width = width;
  c->height = height;
  drop_extent_buffers(c);
  // a caller-owned output buffer was sized for the old extent: the caller sets it again (bbr_set_output_device_ptr)
  c->ext_out = nullptr;
  c->ext_out_bytes = 0;
  return BBR_OK;
}

int bbr_stream_layout_state(const bbr_context *c, int32_t *out_layout, int32_t *out_decided, float *out_ms) {
  if (!c) return BBR_ERR_INVALID_ARGUMENT;
  if (out_layout) *out_layout = c->pipelined() ? c->layout_mode : 0;
  if (out_decided) *out_decided = 1;  // (the layout is a plain option: nothing is timed or decided at run time)
  if (out_ms)
    for (int l = 0; l < bbr_context::kLayouts; ++l) out_ms[l] = 0.f;
  return BBR_OK;
}

int bbr_shard_rows(const bbr_context *c, int32_t *out_rows) {
  if (!c || !out_rows) return BBR_ERR_INVALID_ARGUMENT;
  *out_rows = c->shard_rows();
  return BBR_OK;
}

int bbr_get_stats(bbr_context *c, bbr_stats *out) {
  if (!c) return BBR_ERR_INVALID_ARGUMENT;
  BBR_ON_DEVICE(c);
  if (!out) return fail(c, BBR_ERR_INVALID_ARGUMENT, "get_stats: NULL");
  if (!c->have_frame) return fail(c, BBR_ERR_NOT_IN_FRAME, "get_stats: nothing rendered");
  Counters h;
  int rc = sync_and_fix(c, &h);
  if (rc) return rc;
  const FrameSlot &s = c->slots[c->last_slot];
  std::memset(out, 0, sizeof *out);
  out->n_prims = c->n_prims;
  {
    size_t nb = ((c->n_prims + 255) / 256) * 4;  // (one record per wave of k_geometry)
    std::vector<BlockStats> bs(nb);
    if (nb) HIP_TRY(c, hipMemcpy(bs.data(), s.d_block_stats.ptr, nb * sizeof(BlockStats), hipMemcpyDeviceToHost));
    for (const BlockStats &b : bs) {
      out->n_raster_tris += b.raster_tris;
      out->n_clipped_prims += b.clipped_prims;
      out->n_bin_refs += b.bin_refs;
    }
  }
  {
    // N_shaded = sum of the per-tile fragment counts of the tiles this rank owns
    size_t tiles = (size_t)c->tiles_x() * c->tiles_y();
    std::vector<uint32_t> fc(tiles);
    HIP_TRY(c, hipMemcpy(fc.data(), s.d_frag_count.ptr, tiles * sizeof(uint32_t), hipMemcpyDeviceToHost));
    int band_tiles = c->band_tiles();
    for (int ty = 0; ty < c->tiles_y(); ++ty) {
      if (c->world > 1 && ((ty / band_tiles) % c->world) != c->rank) continue;
      for (int tx = 0; tx < c->tiles_x(); ++tx) out->n_shaded += fc[(size_t)ty * c->tiles_x() + tx] & ~kFullTile;
    }
  }
  out->n_broad_tris = h.n_broad;
  out->bin_overflow = (uint32_t)c->retries;
  out->tile_w = (uint32_t)c->tile_w();
  out->tile_h = (uint32_t)c->tile_h();
  out->n_tiles = (uint32_t)(c->tiles_x() * c->tiles_y());
  return BBR_OK;
}

int bbr_read_visibility(bbr_context *c, uint32_t *prim_host, float *depth_host) {
  if (!c) return BBR_ERR_INVALID_ARGUMENT;
  BBR_ON_DEVICE(c);
  if (int rc = refuse_without_depth_rule(c, "read_visibility", "its buffers have the output extent and option depth_resolve is 0")) return rc;
  if (!c->have_frame) return fail(c, BBR_ERR_NOT_IN_FRAME, "read_visibility: nothing rendered");
  if (c->world > 1) return fail(c, BBR_ERR_INVALID_ARGUMENT, "read_visibility: not available on a partitioned context");
  int rc = rerender_with(c, &bbr_context::dump_vis);  // (n >= 2: k_resolve_depth's PRIM form fills the two buffers)
  if (rc) return rc;
  size_t n = (size_t)c->width * c->height;
  if (prim_host) HIP_TRY(c, hipMemcpy(prim_host, c->d_vis_prim.ptr, n * 4, hipMemcpyDeviceToHost));
  if (depth_host) HIP_TRY(c, hipMemcpy(depth_host, c->d_vis_depth.ptr, n * 4, hipMemcpyDeviceToHost));
  return BBR_OK;
}

// the winners and depths of the render extent, as k_raster dumps them: no rule is involved
int bbr_read_sample_visibility(bbr_context *c, uint32_t *prim_host, float *depth_host) {
  if (!c) return BBR_ERR_INVALID_ARGUMENT;
  BBR_ON_DEVICE(c);
  if (c->world > 1) return fail(c, BBR_ERR_INVALID_ARGUMENT, "read_sample_visibility: not available on a partitioned context");
  if (!c->have_frame || c->last_slot < 0) return fail(c, BBR_ERR_NOT_IN_FRAME, "read_sample_visibility: nothing rendered");
  if (!frame_mode(c).resolve) return bbr_read_visibility(c, prim_host, depth_host);  // one sample per pixel
  int rc = rerender_with(c, &bbr_context::dump_vis);
  if (rc) return rc;
  const size_t n = (size_t)c->render_width() * c->render_height();
  if (prim_host) HIP_TRY(c, hipMemcpy(prim_host, c->d_vis_fine_prim.ptr, n * 4, hipMemcpyDeviceToHost));
  if (depth_host) HIP_TRY(c, hipMemcpy(depth_host, c->d_vis_fine_depth.ptr, n * 4, hipMemcpyDeviceToHost));
  return BBR_OK;
}

// the depth the last frame kept for the overlay pass (n >= 2: k_resolve_depth's plain form wrote it)
int bbr_read_depth(bbr_context *c, float *depth_host) {
  if (!c) return BBR_ERR_INVALID_ARGUMENT;
  BBR_ON_DEVICE(c);
  if (!depth_host) return fail(c, BBR_ERR_INVALID_ARGUMENT, "read_depth: NULL");
  if (c->world > 1) return fail(c, BBR_ERR_INVALID_ARGUMENT, "read_depth: not available on a partitioned context");
  if (int rc = refuse_without_depth_rule(c, "read_depth", "no depth resolve rule: option depth_resolve is 0")) return rc;
  if (!c->have_frame || c->last_slot < 0) return fail(c, BBR_ERR_NOT_IN_FRAME, "read_depth: nothing rendered");
  int rc = sync_and_fix(c, nullptr);
  if (rc) return rc;
  const FrameSlot &s = c->slots[c->last_slot];
  if (!s.mode.depth) return fail(c, BBR_ERR_INVALID_ARGUMENT, "read_depth: the frame was rendered without option \"overlays\"");
  HIP_TRY(c, hipMemcpy(depth_host, s.d_depth.ptr, (size_t)c->width * c->height * 4, hipMemcpyDeviceToHost));
  return BBR_OK;
}

int bbr_read_gbuffer(bbr_context *c, float *host) {
  if (!c) return BBR_ERR_INVALID_ARGUMENT;
  BBR_ON_DEVICE(c);
  if (!host) return fail(c, BBR_ERR_INVALID_ARGUMENT, "read_gbuffer: NULL");
  if (int rc = refuse_supersampled(c, "read_gbuffer")) return rc;
  if (!c->have_frame || c->last_slot < 0) return fail(c, BBR_ERR_NOT_IN_FRAME, "read_gbuffer: nothing rendered");
  if (!c->deferred) return fail(c, BBR_ERR_INVALID_ARGUMENT, "read_gbuffer: option render_pass is not 1 (deferred)");
  if (c->world > 1) return fail(c, BBR_ERR_INVALID_ARGUMENT, "read_gbuffer: not available with a partition");
  int rc = rerender_with(c, &bbr_context::dump_gbuffer);  // (the fused deferred kernel keeps the G-buffer in registers)
  if (rc) return rc;
  const size_t n = (size_t)c->width * c->height * 16;
  std::vector<_Float16> h(n);
  HIP_TRY(c, hipMemcpy(h.data(), c->d_gbuffer.ptr, n * 2, hipMemcpyDeviceToHost));
  for (size_t i = 0; i < n; ++i) host[i] = (float)h[i];
  c->d_gbuffer.release();
  return BBR_OK;
}

int bbr_read_surface(bbr_context *c, float *host) {
  if (!c) return BBR_ERR_INVALID_ARGUMENT;
  BBR_ON_DEVICE(c);
  if (!host) return fail(c, BBR_ERR_INVALID_ARGUMENT, "read_surface: NULL");
  if (int rc = refuse_supersampled(c, "read_surface")) return rc;
  if (!c->have_frame || c->last_slot < 0) return fail(c, BBR_ERR_NOT_IN_FRAME, "read_surface: nothing rendered");
  if (c->world > 1) return fail(c, BBR_ERR_INVALID_ARGUMENT, "read_surface: not available on a partitioned context");
  int rc = rerender_with(c, &bbr_context::dump_surface);  // (the dumping instantiation of k_shade_aniso)
  if (rc == BBR_OK) {
    const size_t n = (size_t)c->width * c->height * kSurfaceFloats;
    hipError_t e = hipMemcpy(host, c->d_surface.ptr, n * sizeof(float), hipMemcpyDeviceToHost);
    if (e != hipSuccess) rc = fail(c, BBR_ERR_HIP, std::string("read_surface: ") + hipGetErrorString(e));
  }
  c->d_surface.release();  // (uncovered pixels are the zeros of a fresh buffer)
  return rc;
}

// a copy of the set of a live material that has level `level`, for the chain read-backs (nothing of the context changes)
static int chain_set(bbr_context *c, int32_t material, int set, int32_t level, const char *who, MipSet *out) {
  if (material < 0 || material >= (int32_t)c->materials.size() || !c->materials[material].alive)
    return fail(c, BBR_ERR_BAD_HANDLE, std::string(who) + ": bad material handle");
  const Material &m = c->materials[material];
  if (c->mip_levels > 1) *out = m.mip.set[set];
  else *out = MipSet{1, 0, {set < kMapCount ? m.desc.maps[set].texels : m.desc.packed}};  // no chain: level 0 alone
  if (level < 0 || level >= out->levels) return fail(c, BBR_ERR_INVALID_ARGUMENT, std::string(who) + ": the chain has no such level");
  return BBR_OK;
}

int bbr_read_material_level(bbr_context *c, int32_t material, int32_t map, int32_t level, uint8_t *out_rgba8, uint64_t cap,
                            int32_t *out_width, int32_t *out_height) {
  if (!c) return BBR_ERR_INVALID_ARGUMENT;
  BBR_ON_DEVICE(c);
  if (map < 0 || map >= kMapCount || !out_width || !out_height) return fail(c, BBR_ERR_INVALID_ARGUMENT, "read_material_level: bad map or NULL size");
  int rc = drain(c);
  if (rc) return rc;
  MipSet ms;
  if ((rc = chain_set(c, material, map, level, "read_material_level", &ms)) != BBR_OK) return rc;
  const TexDesc &td = c->materials[material].desc.maps[map];
  *out_width = mip_extent(td.w, level);
  *out_height = mip_extent(td.h, level);
  const uint64_t bytes = (uint64_t)*out_width * (uint64_t)*out_height * 4;
  if (out_rgba8) {
    if (cap < bytes) return fail(c, BBR_ERR_CAPACITY, "read_material_level: capacity below width * height * 4");
    HIP_TRY(c, hipMemcpy(out_rgba8, ms.level[level], bytes, hipMemcpyDeviceToHost));
  }
  return BBR_OK;
}

int bbr_read_packed_level(bbr_context *c, int32_t material, int32_t level, uint8_t *out, uint64_t cap, uint64_t *out_bytes) {
  if (!c) return BBR_ERR_INVALID_ARGUMENT;
  BBR_ON_DEVICE(c);
  if (!out_bytes) return fail(c, BBR_ERR_INVALID_ARGUMENT, "read_packed_level: NULL size");
  int rc = drain(c);
  if (rc) return rc;
  *out_bytes = 0;
  MipSet ms;
  if ((rc = chain_set(c, material, kMapCount, level, "read_packed_level", &ms)) != BBR_OK) return rc;
  const MaterialDesc &md = c->materials[material].desc;
  if (!md.packed) return BBR_OK;  // not packed: nothing to read
  *out_bytes = packed_level_bytes(mip_extent(md.pw, level), mip_extent(md.ph, level));
  if (out) {
    if (cap < *out_bytes) return fail(c, BBR_ERR_CAPACITY, "read_packed_level: capacity below the level's bytes");
    HIP_TRY(c, hipMemcpy(out, ms.level[level], *out_bytes, hipMemcpyDeviceToHost));
  }
  return BBR_OK;
}

int bbr_read_records(bbr_context *c, void *records, void *triangles, uint32_t cap, uint32_t *out_count) {
  if (!c) return BBR_ERR_INVALID_ARGUMENT;
  BBR_ON_DEVICE(c);
  if (!out_count) return fail(c, BBR_ERR_INVALID_ARGUMENT, "read_records: NULL count");
  if (int rc = refuse_supersampled(c, "read_records")) return rc;
  if (!c->have_frame || c->last_slot < 0) return fail(c, BBR_ERR_NOT_IN_FRAME, "read_records: nothing rendered");
  if (c->world > 1) return fail(c, BBR_ERR_INVALID_ARGUMENT, "read_records: not available on a partitioned context");
  int rc = sync_and_fix(c, nullptr);
  if (rc) return rc;
  // k_geometry writes neither a record nor a triangle for a primitive it culls, and the slot's buffers have held other
  // frames: fill both, so that "not written" is readable, and have the frame's own k_geometry write them again.
  const size_t n = c->n_prims;
  {
    FrameSlot &s = c->slots[c->last_slot];
    if (n > s.d_attrs.cap || n > s.d_tris.cap) return fail(c, BBR_ERR_NOT_IN_FRAME, "read_records: the last frame's buffers are gone");
    if (n) {
      HIP_TRY(c, hipMemset(s.d_attrs.ptr, 0xFF, n * sizeof(ShadeRec)));
      HIP_TRY(c, hipMemset(s.d_tris.ptr, 0xFF, n * sizeof(RasterTri)));
      HIP_TRY(c, hipStreamSynchronize(nullptr));  // (the context's streams do not order themselves after the NULL stream)
    }
  }
  // (the full path, whatever option "static_records" says: a culled primitive keeps the fill.  The slot's static parts are gone
  //  with the fill, and the resubmission forgets them: plan_static_records)
  c->dump_records = true;
  rc = resubmit_last_frame(c);
  if (rc == BBR_OK) rc = sync_and_fix(c, nullptr);
  c->dump_records = false;
  if (rc) return rc;
  const FrameSlot &s = c->slots[c->last_slot];
  const size_t m = std::min<size_t>(cap, n);
  if (records && m) HIP_TRY(c, hipMemcpy(records, s.d_attrs.ptr, m * sizeof(ShadeRec), hipMemcpyDeviceToHost));
  if (triangles && m) HIP_TRY(c, hipMemcpy(triangles, s.d_tris.ptr, m * sizeof(RasterTri), hipMemcpyDeviceToHost));
  *out_count = (uint32_t)n;
  return BBR_OK;
}

int bbr_last_frame_time_ms(bbr_context *c, float *out_frame_ms, float *out_shade_ms) {
  if (!c) return BBR_ERR_INVALID_ARGUMENT;
  BBR_ON_DEVICE(c);
  if (!c->timing) return fail(c, BBR_ERR_INVALID_ARGUMENT, "last_frame_time_ms: enable option \"timing\" first");
  if (!c->ring_frames) return fail(c, BBR_ERR_NOT_IN_FRAME, "last_frame_time_ms: no timed frame yet");
  int rc = drain(c);
  if (rc) return rc;
  const Event *e = &c->ring[bbr_context::kRingEvents * ((c->ring_frames - 1) % bbr_context::kRingCap)];
  float a = 0.f, b = 0.f;
  if (c->timing == 1) HIP_TRY(c, hipEventElapsedTime(&a, e[0], frame_end_event(c, c->ring_frames - 1)));
  HIP_TRY(c, hipEventElapsedTime(&b, e[3], e[4]));
  if (out_frame_ms) *out_frame_ms = a;
  if (out_shade_ms) *out_shade_ms = b;
  return BBR_OK;
}

int bbr_host_timing(const bbr_context *c, uint64_t *out_frames, uint64_t *out_submit_ns, uint64_t *out_blocked_ns,
                    uint64_t *out_blocked_frames) {
  if (!c) return BBR_ERR_INVALID_ARGUMENT;
  if (out_frames) *out_frames = c->host_frames;
  if (out_submit_ns) *out_submit_ns = c->host_submit_ns;
  if (out_blocked_ns) *out_blocked_ns = c->host_blocked_ns;
  if (out_blocked_frames) *out_blocked_frames = c->host_blocked_frames;
  return BBR_OK;
}

int bbr_host_timing_reset(bbr_context *c) {
  if (!c) return BBR_ERR_INVALID_ARGUMENT;
  c->host_frames = c->host_submit_ns = c->host_blocked_ns = c->host_blocked_frames = 0;
  return BBR_OK;
}

int bbr_capacity_growths(const bbr_context *c, uint32_t *out_count) {
  if (!c || !out_count) return BBR_ERR_INVALID_ARGUMENT;
  *out_count = (uint32_t)c->retries;
  return BBR_OK;
}

int bbr_static_record_counts(const bbr_context *c, uint64_t *out_fills, uint64_t *out_light_draws) {
  if (!c) return BBR_ERR_INVALID_ARGUMENT;
  if (out_fills) *out_fills = c->static_fills;
  if (out_light_draws) *out_light_draws = c->static_light_draws;
  return BBR_OK;
}

int bbr_view_keep_counts(const bbr_context *c, uint64_t *out_kept, uint64_t *out_full) {
  if (!c) return BBR_ERR_INVALID_ARGUMENT;
  if (out_kept) *out_kept = c->view_kept_frames;
  if (out_full) *out_full = c->view_full_frames;
  return BBR_OK;
}

int bbr_surface_keep_counts(const bbr_context *c, uint64_t *out_stored, uint64_t *out_lit) {
  if (!c) return BBR_ERR_INVALID_ARGUMENT;
  if (out_stored) *out_stored = c->surface_stored_frames;
  if (out_lit) *out_lit = c->surface_lit_frames;
  return BBR_OK;
}

int bbr_read_surface_keep(bbr_context *c, int32_t slot, float *out_values, uint32_t *out_index, uint64_t capacity, uint32_t *out_items) {
  if (!c) return BBR_ERR_INVALID_ARGUMENT;
  BBR_ON_DEVICE(c);
  if (slot < 0 || slot >= c->n_slots()) return fail(c, BBR_ERR_INVALID_ARGUMENT, "read_surface_keep: no such frame slot");
  int rc = drain(c);
  if (rc) return rc;
  const FrameSlot &s = c->slots[slot];
  const SurfaceKeep &k = s.surf;
  if (!s.vis.valid || !k.valid || !k.buffer || k.buffer != s.d_surface_keep.ptr)
    return fail(c, BBR_ERR_NOT_IN_FRAME, "read_surface_keep: the slot holds no valid surface");
  if (out_items) *out_items = k.items;
  if (!out_values && !out_index) return BBR_OK;
  const size_t n = (size_t)k.items * 64;
  if (capacity < n) return fail(c, BBR_ERR_INVALID_ARGUMENT, "read_surface_keep: capacity is smaller than 64 x the item count");
  const size_t plane = (size_t)((k.items + kShadeWaves - 1) / kShadeWaves * kShadeWaves) * 64;  // (the capacity the planes are indexed by)
  if (out_values) {
    std::vector<float4> planes(n);
    for (int p = 0; p < kSurfacePlanes; ++p) {
      HIP_TRY(c, hipMemcpy(planes.data(), s.d_surface_keep.ptr + p * plane, n * sizeof(float4), hipMemcpyDeviceToHost));
      for (size_t e = 0; e < n; ++e) std::memcpy(out_values + e * 4 * kSurfacePlanes + 4 * p, &planes[e], sizeof(float4));
    }
  }
  if (out_index) HIP_TRY(c, hipMemcpy(out_index, s.d_surface_keep.ptr + kSurfacePlanes * plane, n * sizeof(uint32_t), hipMemcpyDeviceToHost));
  return BBR_OK;
}

int bbr_read_sky_tiles(bbr_context *c, uint8_t *out, uint32_t cap, uint32_t *out_count) {
  if (!c) return BBR_ERR_INVALID_ARGUMENT;
  BBR_ON_DEVICE(c);
  if (!c->have_frame || c->last_slot < 0) return fail(c, BBR_ERR_NOT_IN_FRAME, "read_sky_tiles: nothing rendered");
  int rc = sync_and_fix(c, nullptr);
  if (rc) return rc;
  const FrameSlot &s = c->slots[c->last_slot];
  const uint32_t tiles = (uint32_t)c->tiles_x() * (uint32_t)c->tiles_y();
  if (out_count) *out_count = tiles;
  if (!out) return BBR_OK;
  if (cap < tiles) return fail(c, BBR_ERR_INVALID_ARGUMENT, "read_sky_tiles: cap is smaller than the tile count");
  std::fill(out, out + tiles, (uint8_t)BBR_SKY_TILE_NONE);
  const uint32_t stamp = s.sky.used;  // (the frame, or its re-render after a capacity growth, ran under it)
  const uint32_t *state = sky_words(s, tiles);
  if (!stamp || !state || state != s.sky.state) return BBR_OK;
  std::vector<uint32_t> words(tiles);
  HIP_TRY(c, hipMemcpy(words.data(), state, tiles * sizeof(uint32_t), hipMemcpyDeviceToHost));
  // (a kept frame, option "view_keep": k_raster did not run, the words are the previous frame's, and nothing was stored into
  //  any tile they call background)
  for (uint32_t t = 0; t < tiles; ++t)
    if ((words[t] & ~kSkyKept) == stamp) out[t] = ((words[t] & kSkyKept) || s.vis.kept_last) ? BBR_SKY_TILE_KEPT : BBR_SKY_TILE_FILLED;
  return BBR_OK;
}

int bbr_debug_live_resources(uint64_t out[5]) {
  if (!out) return BBR_ERR_INVALID_ARGUMENT;
  const LiveCounts &n = g_live_counts;
  for (const std::atomic<uint64_t> *v : {&n.device_allocs, &n.device_bytes, &n.pinned_blocks, &n.events, &n.streams}) *out++ = v->load();
  return BBR_OK;
}

int bbr_timing_reset(bbr_context *c) {
  if (!c) return BBR_ERR_INVALID_ARGUMENT;
  BBR_ON_DEVICE(c);
  int rc = drain(c);
  if (rc) return rc;
  // (the three places that reset timing state reset different sets, and stay apart: this one the ring, present and resolve;
  //  option "timing" those and the stride's tick; option "supersample" the ring, resolve and the tick, not present)
  c->ring_frames = 0;
  c->present_ring.reset();
  c->bloom_ring.reset();
  c->luminance_ring.reset();
  c->resolve_ring.reset();
  return BBR_OK;
}

int bbr_timing_summary(bbr_context *c, uint32_t *out_frames, float *out_avg_frame_ms, float *out_avg_geometry_ms,
                       float *out_avg_raster_ms, float *out_avg_shade_ms) {
  if (!c) return BBR_ERR_INVALID_ARGUMENT;
  BBR_ON_DEVICE(c);
  if (!c->timing) return fail(c, BBR_ERR_INVALID_ARGUMENT, "timing_summary: enable option \"timing\" first");
  int rc = drain(c);
  if (rc) return rc;
  uint32_t n = std::min(c->ring_frames, bbr_context::kRingCap);
  double f = 0, g = 0, r = 0, t = 0;
  for (uint32_t i = 0; i < n; ++i) {
    const Event *e = &c->ring[bbr_context::kRingEvents * i];
    float a = 0.f, b = 0.f, d = 0.f, h = 0.f;
    if (c->timing == 1) {
      HIP_TRY(c, hipEventElapsedTime(&a, e[0], frame_end_event(c, i)));
      HIP_TRY(c, hipEventElapsedTime(&b, e[0], e[1]));
      HIP_TRY(c, hipEventElapsedTime(&d, e[1], e[2]));
    }
    HIP_TRY(c, hipEventElapsedTime(&h, e[3], e[4]));
    f += a; g += b; r += d; t += h;
  }
  if (out_frames) *out_frames = n;
  if (out_avg_frame_ms) *out_avg_frame_ms = n ? (float)(f / n) : 0.f;
  if (out_avg_geometry_ms) *out_avg_geometry_ms = n ? (float)(g / n) : 0.f;
  if (out_avg_raster_ms) *out_avg_raster_ms = n ? (float)(r / n) : 0.f;
  if (out_avg_shade_ms) *out_avg_shade_ms = n ? (float)(t / n) : 0.f;
  return BBR_OK;
}

// bbr_present_timing / bbr_resolve_timing: launches and average milliseconds of one ring of pairs
static int pair_ring_timing(bbr_context *c, PairRing bbr_context::*which, const char *who, uint32_t *out_launches, float *out_avg_ms) {
  if (!c) return BBR_ERR_INVALID_ARGUMENT;
  BBR_ON_DEVICE(c);
  if (!c->timing) return fail(c, BBR_ERR_INVALID_ARGUMENT, std::string(who) + ": enable option \"timing\" first");
  int rc = drain(c);
  if (rc) return rc;
  const PairRing &ring = c->*which;
  uint32_t n = std::min(ring.launches, kRingCap);
  double t = 0;
  for (uint32_t i = 0; i < n; ++i) {
    float ms = 0.f;
    HIP_TRY(c, hipEventElapsedTime(&ms, ring.start(i), ring.stop(i)));
    t += ms;
  }
  if (out_launches) *out_launches = n;
  if (out_avg_ms) *out_avg_ms = n ? (float)(t / n) : 0.f;
  return BBR_OK;
}

int bbr_present_timing(bbr_context *c, uint32_t *out_launches, float *out_avg_ms) {
  return pair_ring_timing(c, &bbr_context::present_ring, "present_timing", out_launches, out_avg_ms);
}

int bbr_resolve_timing(bbr_context *c, uint32_t *out_launches, float *out_avg_ms) {
  return pair_ring_timing(c, &bbr_context::resolve_ring, "resolve_timing", out_launches, out_avg_ms);
}

}  // extern "C" (the option rows name their members through templates)

// ---- bbr_set_option: one row per name (kOptions), which states everything the call does with it ----
namespace {
// A plain option: the checked value goes into a member
template <auto MEMBER> int store(bbr_context *c, int64_t value) {
  c->*MEMBER = static_cast<std::decay_t<decltype(c->*MEMBER)>>(value);
  return BBR_OK;
}
int set_timing(bbr_context *c, int64_t value) {
  c->timing = (int)value;
  if (int rc = value ? ensure_timing_ring(c, frame_mode(c).resolve) : BBR_OK) return rc;
  c->ring_frames = 0;  // (see bbr_timing_reset on what each of the three reset sites resets)
  c->present_ring.reset();
  c->bloom_ring.reset();
  c->luminance_ring.reset();
  c->resolve_ring.reset();
  c->timing_tick = 0;
  return BBR_OK;
}
int set_tile_mode(bbr_context *c, int64_t value) {
  if (c->world > 1 && c->band_rows % (value == 0 ? 64 : 32))
    return fail(c, BBR_ERR_INVALID_ARGUMENT, "tile_mode: band_rows not a multiple of the new tile height");
  c->tile_mode = (int)value;
  for (FrameSlot &s : c->slots) drop<TileSized>(s);
  drop<TileSized>(c->ov);
  drop<TileSized>(c->shadow.pass);  // (the map itself has no tiles: it stays)
  return BBR_OK;
}
// a capacity and the buffer it sizes, which goes: of every frame slot and (`OVERLAY_TOO`) of the overlay pass
template <auto CAP, auto BUFFER, bool OVERLAY_TOO> int set_capacity(bbr_context *c, int64_t value) {
  c->*CAP = (uint32_t)value;
  for (FrameSlot &s : c->slots) (s.*BUFFER).release();
  if (OVERLAY_TOO) (c->ov.*BUFFER).release();
  return BBR_OK;
}
int set_mip_levels(bbr_context *c, int64_t value) {
  if (refused_shadow_pair(value, c->shadow_map))
    return fail(c, BBR_ERR_INVALID_ARGUMENT, "mip_levels: >= 2 is not available with option shadow_map > 0 (k_shade_shadow has no trilinear form)");
  // every chain is built for the option's value: drop them all, then build the new ones of every live material
  for (Material &m : c->materials) free_chain(m);
  c->mip_levels = (int)value;
  c->materials_dirty = true;
  ++c->resource_epoch;
  if (value == 1) c->d_mip_tables.release();
  for (Material &m : c->materials)
    if (int rc = (m.alive && value > 1) ? build_chain(c, m) : BBR_OK) {
      for (Material &q : c->materials) free_chain(q);
      c->mip_levels = 1;
      return rc;
    }
  return BBR_OK;
}
// like a resize of the render extent; the output extent, and with it a caller's output buffer, stay
int set_supersample(bbr_context *c, int64_t value) {
  if (int rc = check_render_extent(c, "supersample", value, c->width, c->height)) return rc;
  if (c->in_frame) return fail(c, BBR_ERR_INVALID_ARGUMENT, "supersample: between begin_frame and end_frame");
  if (refused_pair(value, c->sample_shading))
    return fail(c, BBR_ERR_INVALID_ARGUMENT, "supersample: 3 is not available with option sample_shading 0 (a 3 x 3 block straddles the tiles)");
  if ((int)value == c->supersample) return BBR_OK;
  // (the one step that can fail comes first: a refused call leaves the context as it was)
  if (int rc = c->timing ? ensure_timing_ring(c, value > 1) : BBR_OK) return rc;
  c->supersample = (int)value;
  drop_extent_buffers(c);
  c->ring_frames = 0;  // (a frame's interval ends behind its k_resolve: the ring holds frames of one kind)
  c->resolve_ring.reset();
  c->timing_tick = 0;
  return BBR_OK;
}
// no extent changes: only the sample maps go, and there is no current frame (its samples were of the other kind)
int set_sample_shading(bbr_context *c, int64_t value) {
  if (c->in_frame) return fail(c, BBR_ERR_INVALID_ARGUMENT, "sample_shading: between begin_frame and end_frame");
  if (refused_pair(c->supersample, value))
    return fail(c, BBR_ERR_INVALID_ARGUMENT, "sample_shading: 0 is not available with option supersample 3 (a 3 x 3 block straddles the tiles)");
  if ((int)value == c->sample_shading) return BBR_OK;
  for (FrameSlot &s : c->slots) s.d_sample_map.release();
  forget_current_frame(c);
  return store<&bbr_context::sample_shading>(c, value);
}
// VkResolveModeFlagBits; AVERAGE (2) has no winner.  At n = 1 the value is only stored; with n >= 2 the current frame was
// rendered under the other rule (or kept no depth at all): there is none any more, and the fine depth goes
int set_depth_resolve(bbr_context *c, int64_t value) {
  if (c->in_frame) return fail(c, BBR_ERR_INVALID_ARGUMENT, "depth_resolve: between begin_frame and end_frame");
  if ((int)value != c->depth_resolve && c->supersample > 1) {
    for (FrameSlot &s : c->slots) s.d_fine_depth.release();
    forget_current_frame(c);
  }
  return store<&bbr_context::depth_resolve>(c, value);
}
// the side of the map; a change drops the map and its pass buffers (the context is drained): frames are unshadowed again
// until bbr_render_shadow_map has rendered the new one
int set_shadow_map(bbr_context *c, int64_t value) {
  if (refused_shadow_pair(c->mip_levels, value))
    return fail(c, BBR_ERR_INVALID_ARGUMENT, "shadow_map: > 0 is not available with option mip_levels >= 2 (k_shade_shadow has no trilinear form)");
  if ((int)value != c->shadow_map) c->shadow = ShadowOwned();
  return store<&bbr_context::shadow_map>(c, value);
}
// the levels of the pyramid.  The frames and the images already presented stay; the pyramids hold the levels of the other
// value (bbr_read_bloom_level: none until the next present), and at 0 nothing of the option exists
int set_bloom(bbr_context *c, int64_t value) {
  if (refused_bloom_partition(value, c->world))
    return fail(c, BBR_ERR_INVALID_ARGUMENT, "bloom: >= 1 is not available on a partition of world > 1 (the chain needs its neighbours' rows)");
  if (refused_bloom_fused(value, c->present_fused))
    return fail(c, BBR_ERR_INVALID_ARGUMENT, "bloom: >= 1 is not available with option present_fused (there is no fp32 frame)");
  if ((int)value != c->bloom) {
    for (FrameSlot &s : c->slots) s.bloom_ran = 0;
    c->bloom_buffer.ran = 0;
  }
  if (value == 0) {
    for (FrameSlot &s : c->slots) s.d_bloom.release();
    c->bloom_buffer = bbr_context::BloomBuffer();
    c->bloom_ring = PairRing();
  }
  return store<&bbr_context::bloom>(c, value);
}
// the slots keep their visibility and forget their surfaces: the run starts again under the new n; at 0 nothing of the option exists
int set_surface_keep(bbr_context *c, int64_t value) {
  for (FrameSlot &s : c->slots) {
    s.surf.forget();
    if (value == 0) s.d_surface_keep.release();
  }
  return store<&bbr_context::surface_keep>(c, value);
}
// 1: the device buffers of the option come (zeroed: no history, empty histograms).  0: nothing of it stays -- a slot whose
// image was made under it keeps the exposure it was made with as a plain number, so whatever presents its frame again makes
// the same image.  The context is drained.
int set_auto_exposure(bbr_context *c, int64_t value) {
  if (refused_auto_partition(value, c->world))
    return fail(c, BBR_ERR_INVALID_ARGUMENT, "auto_exposure: not available on a partition of world > 1 (metering needs the whole frame: bbr_present_buffer_auto on the gathered one)");
  if (refused_auto_fused(value, c->present_fused))
    return fail(c, BBR_ERR_INVALID_ARGUMENT, "auto_exposure: not available with option present_fused (the exposure would be needed before the frame exists)");
  using X = bbr_context::ExposureOwned;
  X &x = c->exposure;
  if (value && !c->auto_exposure) {
    X fresh;
    HIP_TRY(c, fresh.d_hist.ensure((size_t)X::kUnits * kLumaWords, true));
    HIP_TRY(c, fresh.d_records.ensure(X::kUnits, true));
    HIP_TRY(c, fresh.d_history.ensure(2, true));
    x = std::move(fresh);
  } else if (!value && c->auto_exposure) {
    for (int k = 0; k < bbr_context::kMaxSlots; ++k) {
      FrameSlot &s = c->slots[k];
      if (s.present.auto_e && s.present.metered)
        HIP_TRY(c, hipMemcpy(&s.present.exposure, &x.record(k)->applied, sizeof(float), hipMemcpyDeviceToHost));
      s.present.auto_e = s.present.metered = false;
    }
    x = X();
    c->luminance_ring = PairRing();
  }
  return store<&bbr_context::auto_exposure>(c, value);
}
int set_present_fused(bbr_context *c, int64_t value) {
  if (refused_auto_fused(c->auto_exposure, value))
    return fail(c, BBR_ERR_INVALID_ARGUMENT, "present_fused: not available with option auto_exposure 1 (the exposure would be needed before the frame exists)");
  if (refused_bloom_fused(c->bloom, value))
    return fail(c, BBR_ERR_INVALID_ARGUMENT, "present_fused: not available with option bloom >= 1 (there is no fp32 frame)");
  return store<&bbr_context::present_fused>(c, value);
}
// the radius of the box of compares; stored at any "shadow_map", and the map stays.  The current frame was shaded under the
// other rule: there is none any more
int set_shadow_filter(bbr_context *c, int64_t value) {
  if ((int)value != c->shadow_filter) forget_current_frame(c);
  return store<&bbr_context::shadow_filter>(c, value);
}

// What bbr_set_option does with a name.  Its checks in order: NULL name; a row that does not wait is checked and applied at once; every
// other call (an unknown name too) waits for the GPU and makes the slots forget; then the row's range; then `apply`, which holds the refusals that
// depend on another option or on the recorded frame.  (So a value refused behind the wait has made the slots forget: one full frame, no pixel.)
struct OptionRow {
  const char *name;
  int64_t lo, hi;       // the accepted values ...
  uint32_t only;        // ... non-zero: of lo .. hi only those whose bit is set (lo = 0)
  const char *accepts;  // what the refusal says behind the name
  bool waits;           // the call drains the context (the others take effect with the next submitted frame)
  // "view_keep": the call leaves the slots' visibility alone ("sky_keep" forgets whatever the option is: options are not set
  // between the frames of a steady run).  Such change shading alone, or what a submission decides by itself: the GUI of the
  // application restated here sets them between frames of one view.  Every other one may change the parameters, the mode or a buffer.
  bool leaves_visibility;
  int (*apply)(bbr_context *, int64_t);
};
constexpr int64_t kAny = std::numeric_limits<int64_t>::max();
constexpr bool kWaits = true, kLeaves = true, kForgets = false;  // (OptionRow::waits, ::leaves_visibility)
using Ctx = bbr_context;
const OptionRow kOptions[] = {
    {"gbuffer_view", -1, 3, 0, ": -1 (the lit scene) or 0..3 (position, normal, albedo, MRAH)", !kWaits, kLeaves, store<&Ctx::gbuffer_view>},
    {"render_pass", 0, 1, 0, ": 0 (forward) or 1 (deferred)", !kWaits, kLeaves, store<&Ctx::deferred>},
    {"timing", 0, 2, 0, ": 0, 1 or 2", kWaits, kLeaves, set_timing},
    {"timing_stride", 1, 1024, 0, ": 1 .. 1024", kWaits, kLeaves, [](Ctx *c, int64_t v) { return c->timing_tick = 0, store<&Ctx::timing_stride>(c, v); }},
    {"frames_in_flight", 1, Ctx::kMaxSlots, 0, ": 1 .. 4", kWaits, kForgets, [](Ctx *c, int64_t v) { return c->frame_counter = 0, store<&Ctx::frames_in_flight>(c, v); }},
    {"tile_mode", 0, 1, 0, ": 0 (64x64) or 1 (32x32)", kWaits, kForgets, set_tile_mode},
    {"bin_cap", 1, 1 << 20, 0, " out of range", kWaits, kForgets, set_capacity<&Ctx::bin_cap, &FrameSlot::d_bins, false>},
    {"ablate", kAblateBuild ? -kAny - 1 : 0, kAblateBuild ? kAny : 0, 0, ": diagnostic builds only (make EXTRA=-DBB_ABLATE)", kWaits, kForgets, store<&Ctx::ablate>},
    {"max_anisotropy", 1, kMaxAnisotropy, 0, ": 1 (bilinear) .. 16", kWaits, kLeaves, store<&Ctx::max_anisotropy>},
    {"mip_levels", 1, kMaxMipLevels, 0, ": 1 (no chain) .. 15", kWaits, kLeaves, set_mip_levels},
    {"supersample", 1, 4, 0, ": 1 (off) .. 4", kWaits, kForgets, set_supersample},
    {"sample_shading", 0, 1, 0, ": 1 (every sample) or 0 (one fragment per primitive and pixel)", kWaits, kForgets, set_sample_shading},
    {"depth_resolve", 0, kDepthMax, 1u | 1u << kDepthZero | 1u << kDepthMin | 1u << kDepthMax, ": 0 (none), 1 (SAMPLE_ZERO), 4 (MIN) or 8 (MAX)", kWaits, kForgets, set_depth_resolve},
    {"shadow_map", 0, kMaxShadowMap, 0, ": 0 (off) or the side of the map, 1 .. 8192", kWaits, kLeaves, set_shadow_map},
    {"shadow_filter", 0, 2, 0, ": 0 (the hard compare), 1 (3 x 3 taps) or 2 (5 x 5 taps)", kWaits, kLeaves, set_shadow_filter},
    {"static_records", 0, 1, 0, ": 1 (write a static draw's record part once) or 0 (every frame)", kWaits, kLeaves, store<&Ctx::static_records>},
    {"sky_keep", 0, 1, 0, ": 1 (a tile that stays background is filled once per frame slot) or 0 (every frame)", kWaits, kLeaves, store<&Ctx::sky_keep>},
    {"view_keep", 0, 1, 0, ": 1 (a frame whose view and draws repeat in its frame slot launches its shading only) or 0 (every frame runs every stage)", kWaits, kLeaves, store<&Ctx::view_keep>},
    {"surface_keep", 0, 1 << 20, 0, ": 0 (off) or n >= 1 (a slot's n-th kept frame in a row stores its shaded surface; it and those behind it are lit from it)", kWaits, kLeaves, set_surface_keep},
    {"present_fused", -kAny - 1, kAny, 0, "", kWaits, kForgets, set_present_fused},  // (any value: non-zero is on)
    {"bloom", 0, kMaxBloomLevels, 0, ": 0 (off) or the levels of the pyramid, 1 .. 8", kWaits, kLeaves, set_bloom},
    {"auto_exposure", 0, 1, 0, ": 0 (the frame's own Exposure) or 1 (metered on the device)", kWaits, kLeaves, set_auto_exposure},
    {"overlays", -kAny - 1, kAny, 0, "", kWaits, kForgets, store<&Ctx::overlays>},
    {"tbn", -kAny - 1, kAny, 0, "", kWaits, kForgets, store<&Ctx::tbn>},
    {"stream_layout", 0, Ctx::kLayouts - 1, 0, ": 0, 1 or 2", kWaits, kForgets, store<&Ctx::layout_mode>},
    {"push_mode", 0, 1, 0, ": 0 (copies) or 1 (one kernel, all peers)", kWaits, kLeaves, store<&Ctx::push_mode>},
    {"no_tail_items", 0, kAny, 0, " must be >= 0", kWaits, kForgets, store<&Ctx::no_tail_items>},
    {"heavy_tiles", -1, 1 << 24, 0, ": -1 (automatic), 0 (off) or a reference count", kWaits, kForgets, store<&Ctx::heavy_tiles>},
    // starting capacity of the every-tile list / the clip arena (entries); both double when a frame overflows them
    {"broad_cap", 1, 1 << 24, 0, " out of range (1 .. 2^24)", kWaits, kForgets, set_capacity<&Ctx::broad_cap, &FrameSlot::d_broad, true>},
    {"clip_cap", 1, 1 << 24, 0, " out of range (1 .. 2^24)", kWaits, kForgets, set_capacity<&Ctx::clip_cap, &FrameSlot::d_clip, true>},
    {"broad_threshold", 1, kAny, 0, " must be >= 1", kWaits, kForgets, store<&Ctx::broad_threshold>},
};
}  // namespace

extern "C" {
int bbr_set_option(bbr_context *c, const char *name, int64_t value) {
  if (!c) return BBR_ERR_INVALID_ARGUMENT;
  BBR_ON_DEVICE(c);
  if (!name) return fail(c, BBR_ERR_INVALID_ARGUMENT, "set_option: NULL name");
  const OptionRow *row = std::find_if(std::begin(kOptions), std::end(kOptions), [&](const OptionRow &r) { return std::strcmp(r.name, name) == 0; });
  if (row == std::end(kOptions)) row = nullptr;  // (an unknown name)
  if (!row || row->waits) {
    if (int rc = drain(c)) return rc;
    for (FrameSlot &s : c->slots) (row && row->leaves_visibility) ? s.forget_sky() : s.forget_image();
  }
  if (!row) return fail(c, BBR_ERR_INVALID_ARGUMENT, std::string("unknown option: ") + name);
  if (value < row->lo || value > row->hi || (row->only && !(row->only >> value & 1u)))
    return fail(c, BBR_ERR_INVALID_ARGUMENT, std::string(row->name) + row->accepts);
  return row->apply(c, value);
}

#ifdef BB_STAMPS
int bbr_debug_raster_stamps(bbr_context *c, unsigned long long *out) {
  if (!c || c->last_slot < 0) return BBR_ERR_INVALID_ARGUMENT;
  int rc = drain(c);
  if (rc) return rc;
  size_t tiles = (size_t)c->tiles_x() * c->tiles_y();
  HIP_TRY(c, hipMemcpy(out, c->slots[c->last_slot].d_frag_count.ptr + tiles, tiles * 64, hipMemcpyDeviceToHost));
  return BBR_OK;
}
// diagnostic build only: copy out the k_geometry time stamps of the last frame (8 x u64 per workgroup)
int bbr_debug_stamps(bbr_context *c, unsigned long long *out, uint32_t n_blocks) {
  if (!c || c->last_slot < 0) return BBR_ERR_INVALID_ARGUMENT;
  int rc = drain(c);
  if (rc) return rc;
  HIP_TRY(c, hipMemcpy(out, c->slots[c->last_slot].d_clip.ptr + c->clip_cap, (size_t)n_blocks * 64, hipMemcpyDeviceToHost));
  return BBR_OK;
}
#endif

int bbr_present(bbr_context *c, void *rgba8_device, int32_t hdr16) {
  if (!c) return BBR_ERR_INVALID_ARGUMENT;
  BBR_ON_DEVICE(c);
  if (!c->have_frame || c->last_slot < 0) return fail(c, BBR_ERR_NOT_IN_FRAME, "present: nothing rendered");
  FrameSlot &s = c->slots[c->last_slot];
  if (c->present_fused && s.present.active && s.present.out == s.d_present.ptr) {
    // the frame was rendered as presented pixels already (binary16 stage included); a caller buffer gets a copy
    if (!hdr16) return fail(c, BBR_ERR_INVALID_ARGUMENT, "present: option present_fused always applies the binary16 stage");
    s.present.copy_to = rgba8_device;
    return rgba8_device ? copy_presented(c, s, rgba8_device) : (int)BBR_OK;
  }
  if (!rgba8_device) HIP_TRY(c, s.d_present.ensure(c->shard_pixels()));
  s.present.active = true;
  s.present.out = rgba8_device ? (uint32_t *)rgba8_device : s.d_present.ptr;
  s.present.enable = s.frame_u.enable_tone_mapping;  // of the frame in the slot, not the uniforms set since
  s.present.exposure = s.frame_u.exposure;
  s.present.hdr16 = hdr16 != 0;
  s.present.auto_e = c->auto_exposure != 0;  // every call of the host is one presentation: it meters and adapts
  s.present.metered = false;
  return queue_present(c, s);
}

int bbr_present_buffer(bbr_context *c, const void *rgba32f_device, void *rgba8_device, uint64_t n_pixels, int32_t enable,
                       float exposure, int32_t hdr16, void *stream) {
  if (!c) return BBR_ERR_INVALID_ARGUMENT;
  BBR_ON_DEVICE(c);
  if (!rgba32f_device || !rgba8_device) return fail(c, BBR_ERR_INVALID_ARGUMENT, "present_buffer: NULL");
  if (!n_pixels) return BBR_OK;
  int rc = ensure_srgb_tables(c);
  if (rc) return rc;
  const size_t per_block = (size_t)kPresentThreads * kPresentPerThread;
  hipLaunchKernelGGL(k_present, dim3((unsigned)((n_pixels + per_block - 1) / per_block)), dim3(kPresentThreads), 0,
                     stream ? (hipStream_t)stream : c->shade_stream(), (const float4 *)rgba32f_device,
                     (uint32_t *)rgba8_device, (size_t)n_pixels, c->d_srgb_tables.ptr, enable, exposure, hdr16 != 0);
  HIP_TRY(c, hipGetLastError());
  return BBR_OK;
}

int bbr_set_bloom(bbr_context *c, float threshold, float intensity) {
  if (!c) return BBR_ERR_INVALID_ARGUMENT;
  BBR_ON_DEVICE(c);
  if (!std::isfinite(threshold) || !std::isfinite(intensity) || threshold < 0.f || intensity < 0.f)
    return fail(c, BBR_ERR_INVALID_ARGUMENT, "set_bloom: threshold and intensity must be finite and >= 0");
  if (int rc = drain(c)) return rc;  // like option "bloom": the slots keep their visibility
  for (FrameSlot &s : c->slots) s.forget_sky();
  c->bloom_threshold = threshold;
  c->bloom_intensity = intensity;
  return BBR_OK;
}

int bbr_get_bloom(bbr_context *c, int32_t *out_levels, float *out_threshold, float *out_intensity) {
  if (!c) return BBR_ERR_INVALID_ARGUMENT;
  if (out_levels) *out_levels = c->bloom;
  if (out_threshold) *out_threshold = c->bloom_threshold;
  if (out_intensity) *out_intensity = c->bloom_intensity;
  return BBR_OK;
}

int bbr_present_buffer_bloom(bbr_context *c, const void *rgba32f_device, void *rgba8_device, int32_t width, int32_t height,
                             int32_t enable, float exposure, int32_t hdr16, void *stream) {
  if (!c) return BBR_ERR_INVALID_ARGUMENT;
  BBR_ON_DEVICE(c);
  if (int rc = check_present_buffer(c, "present_buffer_bloom", rgba32f_device, rgba8_device, width, height)) return rc;
  if (!c->bloom)
    return bbr_present_buffer(c, rgba32f_device, rgba8_device, (uint64_t)width * (uint64_t)height, enable, exposure, hdr16, stream);
  if (int rc = ensure_srgb_tables(c)) return rc;
  const hipStream_t ps = stream ? (hipStream_t)stream : c->shade_stream();
  return queue_buffer_bloom(c, ps, rgba32f_device, rgba8_device, width, height, enable, exposure, hdr16, nullptr, [] { return (int)BBR_OK; });
}

int bbr_read_bloom_level(bbr_context *c, int32_t source, int32_t level, float *out_rgb, uint64_t capacity, int32_t *out_w, int32_t *out_h) {
  if (!c) return BBR_ERR_INVALID_ARGUMENT;
  BBR_ON_DEVICE(c);
  if (source != 0 && source != 1) return fail(c, BBR_ERR_INVALID_ARGUMENT, "read_bloom_level: source is 0 (the last frame's slot) or 1 (the buffer call)");
  if (level < 1 || level > c->bloom) return fail(c, BBR_ERR_INVALID_ARGUMENT, "read_bloom_level: option bloom has no such level");
  const float4 *levels = nullptr;
  int32_t w0 = 0, h0 = 0;
  if (source == 0) {
    if (!c->have_frame || c->last_slot < 0 || !c->slots[c->last_slot].present.active || c->slots[c->last_slot].bloom_ran != c->bloom)
      return fail(c, BBR_ERR_NOT_IN_FRAME, "read_bloom_level: bbr_present with option bloom >= 1 was not called for the last frame");
    if (int rc = sync_and_fix(c, nullptr)) return rc;  // (a frame rendered again has its chain run again: resubmit_last_frame)
    levels = c->slots[c->last_slot].d_bloom.ptr, w0 = c->width, h0 = c->height;
  } else {
    const bbr_context::BloomBuffer &b = c->bloom_buffer;
    if (b.ran != c->bloom || !b.used) return fail(c, BBR_ERR_NOT_IN_FRAME, "read_bloom_level: bbr_present_buffer_bloom has not run with option bloom >= 1");
    HIP_TRY(c, hipEventSynchronize(b.ev_used));
    levels = b.d_levels.ptr, w0 = b.w, h0 = b.h;
  }
  const BloomShape sh(w0, h0, c->bloom);
  const size_t texels = (size_t)sh.w[level] * (size_t)sh.h[level];
  if (out_w) *out_w = sh.w[level];
  if (out_h) *out_h = sh.h[level];
  if (!out_rgb) return BBR_OK;
  if (capacity < (uint64_t)texels * 3 * sizeof(float)) return fail(c, BBR_ERR_CAPACITY, "read_bloom_level: capacity (bytes) too small for w * h * 3 floats");
  std::vector<float4> host(texels);
  HIP_TRY(c, hipMemcpy(host.data(), levels + sh.at[level], texels * sizeof(float4), hipMemcpyDeviceToHost));
  for (size_t i = 0; i < texels; ++i) out_rgb[3 * i] = host[i].x, out_rgb[3 * i + 1] = host[i].y, out_rgb[3 * i + 2] = host[i].z;
  return BBR_OK;
}

int bbr_bloom_timing(bbr_context *c, uint32_t *out_launches, float *out_avg_ms) {
  return pair_ring_timing(c, &bbr_context::bloom_ring, "bloom_timing", out_launches, out_avg_ms);
}

int bbr_set_auto_exposure(bbr_context *c, float key, float e_min, float e_max, float rate, int32_t lo_permille, int32_t hi_permille) {
  if (!c) return BBR_ERR_INVALID_ARGUMENT;
  BBR_ON_DEVICE(c);
  if (!std::isfinite(key) || !std::isfinite(e_min) || !std::isfinite(e_max) || !std::isfinite(rate) || !(key > 0.f) || !(e_min > 0.f) ||
      !(e_min <= e_max) || !(rate >= 0.f && rate <= 1.f))
    return fail(c, BBR_ERR_INVALID_ARGUMENT, "set_auto_exposure: every float finite, key > 0, 0 < e_min <= e_max, 0 <= rate <= 1");
  if (lo_permille < 0 || lo_permille >= hi_permille || hi_permille > 1000)
    return fail(c, BBR_ERR_INVALID_ARGUMENT, "set_auto_exposure: 0 <= lo_permille < hi_permille <= 1000");
  // No wait: k_exposure takes the parameters by value at its launch, so the presentations already queued keep theirs and the
  // next one has these (a host sets `rate` from its clock every frame)
  c->exposure_params = ExposureParams{key, e_min, e_max, rate, lo_permille, hi_permille};
  return BBR_OK;
}

int bbr_get_auto_exposure(bbr_context *c, float *out_key, float *out_e_min, float *out_e_max, float *out_rate,
                          int32_t *out_lo_permille, int32_t *out_hi_permille) {
  if (!c) return BBR_ERR_INVALID_ARGUMENT;
  const ExposureParams &p = c->exposure_params;
  if (out_key) *out_key = p.key;
  if (out_e_min) *out_e_min = p.e_min;
  if (out_e_max) *out_e_max = p.e_max;
  if (out_rate) *out_rate = p.rate;
  if (out_lo_permille) *out_lo_permille = p.lo;
  if (out_hi_permille) *out_hi_permille = p.hi;
  return BBR_OK;
}

int bbr_reset_exposure(bbr_context *c) {
  if (!c) return BBR_ERR_INVALID_ARGUMENT;
  BBR_ON_DEVICE(c);
  if (int rc = drain(c)) return rc;
  for (FrameSlot &s : c->slots) s.forget_sky();
  if (c->auto_exposure) HIP_TRY(c, zero_fill_sync(c->exposure.d_history.ptr, 2 * sizeof(ExposureHistory)));
  return BBR_OK;
}

int bbr_present_buffer_auto(bbr_context *c, const void *rgba32f_device, void *rgba8_device, int32_t width, int32_t height,
                            int32_t enable, float exposure, int32_t hdr16, void *stream) {
  if (!c) return BBR_ERR_INVALID_ARGUMENT;
  BBR_ON_DEVICE(c);
  if (int rc = check_present_buffer(c, "present_buffer_auto", rgba32f_device, rgba8_device, width, height)) return rc;
  if (!c->auto_exposure) return fail(c, BBR_ERR_INVALID_ARGUMENT, "present_buffer_auto: option auto_exposure is 0");
  if (int rc = ensure_srgb_tables(c)) return rc;
  using X = bbr_context::ExposureOwned;
  X &x = c->exposure;
  const hipStream_t ps = stream ? (hipStream_t)stream : c->shade_stream();
  // the calls share one unit and history 1: each is ordered behind the one before it, whatever their streams
  HIP_TRY(c, x.ev_buffer.ensure(hipEventDisableTiming));
  if (x.buffer_used) HIP_TRY(c, hipStreamWaitEvent(ps, x.ev_buffer, 0));
  const size_t n = (size_t)width * (size_t)height;
  const float *d_exposure = &x.record(X::kBufferUnit)->applied;
  bool adapted = false;  // k_exposure is queued: it leaves the histogram zeroed
  auto adapt = [&] {
    const int rc = queue_exposure(c, ps, X::kBufferUnit, 1, exposure);
    adapted = rc == BBR_OK;
    return rc;
  };
  int rc = queue_luminance(c, ps, X::kBufferUnit, (const float4 *)rgba32f_device, n);
  if (rc == BBR_OK)
    rc = c->bloom ? queue_buffer_bloom(c, ps, rgba32f_device, rgba8_device, width, height, enable, exposure, hdr16, d_exposure, adapt)
                  : queue_plain_present(c, ps, (const float4 *)rgba32f_device, (uint32_t *)rgba8_device, n, enable, exposure, hdr16 != 0,
                                        d_exposure, adapt);
  if (rc != BBR_OK && !adapted) abandon_metering(c, ps, X::kBufferUnit);
  // (recorded after a failure too: the next call is ordered behind whatever this one did queue)
  const hipError_t recorded = hipEventRecord(x.ev_buffer, ps);
  if (recorded == hipSuccess) x.buffer_used = true;
  if (rc != BBR_OK) return rc;
  HIP_TRY(c, recorded);
  return BBR_OK;
}

int bbr_read_exposure(bbr_context *c, int32_t source, bbr_exposure_record *out) {
  if (!c) return BBR_ERR_INVALID_ARGUMENT;
  BBR_ON_DEVICE(c);
  if (source != 0 && source != 1) return fail(c, BBR_ERR_INVALID_ARGUMENT, "read_exposure: source is 0 (bbr_present) or 1 (bbr_present_buffer_auto)");
  if (!c->auto_exposure) return fail(c, BBR_ERR_INVALID_ARGUMENT, "read_exposure: option auto_exposure is 0");
  if (!out) return fail(c, BBR_ERR_INVALID_ARGUMENT, "read_exposure: NULL");
  using X = bbr_context::ExposureOwned;
  const X &x = c->exposure;
  int unit = X::kBufferUnit;
  if (source == 0) {
    if (x.last_slot < 0) return fail(c, BBR_ERR_NOT_IN_FRAME, "read_exposure: bbr_present has not run under option auto_exposure");
    if (int rc = sync_and_fix(c, nullptr)) return rc;  // (a frame rendered again is presented with its record's exposure: the record stays)
    unit = x.last_slot;
  } else {
    if (!x.buffer_used) return fail(c, BBR_ERR_NOT_IN_FRAME, "read_exposure: bbr_present_buffer_auto has not run under option auto_exposure");
    HIP_TRY(c, hipEventSynchronize(x.ev_buffer));
  }
  static_assert(sizeof(bbr_exposure_record) == sizeof(ExposureRecord) && offsetof(bbr_exposure_record, sum) == offsetof(ExposureRecord, sum) &&
                    offsetof(bbr_exposure_record, applied) == offsetof(ExposureRecord, applied) &&
                    offsetof(bbr_exposure_record, flags) == offsetof(ExposureRecord, flags),
                "the record of the header is the record the kernels write");
  HIP_TRY(c, hipMemcpy(out, x.record(unit), sizeof(ExposureRecord), hipMemcpyDeviceToHost));
  return BBR_OK;
}

int bbr_luminance_timing(bbr_context *c, uint32_t *out_launches, float *out_avg_ms) {
  return pair_ring_timing(c, &bbr_context::luminance_ring, "luminance_timing", out_launches, out_avg_ms);
}

int bbr_read_presented(bbr_context *c, uint8_t *host) {
  if (!c) return BBR_ERR_INVALID_ARGUMENT;
  BBR_ON_DEVICE(c);
  if (!host) return fail(c, BBR_ERR_INVALID_ARGUMENT, "read_presented: NULL");
  if (!c->have_frame || c->last_slot < 0 || !c->slots[c->last_slot].present.active)
    return fail(c, BBR_ERR_NOT_IN_FRAME, "read_presented: bbr_present was not called for the last frame");
  int rc = sync_and_fix(c, nullptr);
  if (rc) return rc;
  const size_t n = c->shard_pixels();
  HIP_TRY(c, hipMemcpy(host, c->slots[c->last_slot].present.out, n * 4, hipMemcpyDeviceToHost));
  return BBR_OK;
}

int bbr_presented_device_ptr(bbr_context *c, void **out_ptr, uint64_t *out_bytes) {
  if (!c) return BBR_ERR_INVALID_ARGUMENT;
  BBR_ON_DEVICE(c);
  if (!out_ptr) return fail(c, BBR_ERR_INVALID_ARGUMENT, "presented_device_ptr: NULL");
  if (!c->have_frame || c->last_slot < 0 || !c->slots[c->last_slot].present.active)
    return fail(c, BBR_ERR_NOT_IN_FRAME, "presented_device_ptr: bbr_present was not called for the last frame");
  *out_ptr = c->slots[c->last_slot].present.out;
  if (out_bytes) *out_bytes = (uint64_t)c->shard_pixels() * 4;
  return BBR_OK;
}

}  // extern "C" (the exchange's internals are templates over the wire forms)

// ================================================================================================
// native exchange (BASELINE config #4): the step in which every rank gets the whole frame
//   collective form: RCCL all-gather of the ranks' blocks (ring over xGMI), one process per GPU
//   peer form:       every rank puts its block into every rank's gather buffer -- ONE kernel that stores to all peers at once
//                    (option push_mode 1, the default: every xGMI link of the mesh busy together), or hipMemcpyPeerAsync
//                    copies one behind the other (push_mode 0, and the fallback when a peer cannot be mapped); for one
//                    process that drives several GPUs, or several processes that exchanged IPC handles
// Both run on the stream of the frame's slot, right behind its k_shade: with stream layout 2 a frame's kernels share a
// stream with nothing else, so the exchange is simply the frame's last step, the next frame of the same slot is ordered
// behind it without an event, and the frames of the other slots render while the links are busy.
// ================================================================================================
namespace {

// ---- the wire forms, host side: one row per BBR_SHARD_* value (the device side: bb_kernels.hip.h, "wire forms") ----
struct WireForm {
  size_t (*block_bytes)(size_t n);  // bytes of one rank's block of n pixels
  size_t whole_pixel_bytes;         // per pixel of the whole frame an exchange of this form leaves behind
  bool presented;                   // made of the presented shard (needs bbr_present), not of the fp32 frame (no present_fused)
  // alignment (include/bibim_hip.h, "Alignment"), each the widest access a kernel makes there: of a block that is written
  // (pack's stores; a plain form is copied, and k_push_block's narrow form stores 4-byte words), of a gather buffer that is
  // un-interleaved (Form::load).  The whole frame is stored a pixel at a time: whole_pixel_bytes.
  size_t block_align, gathered_align;
  void (*pack)(const float4 *shard, void *block, size_t n, hipStream_t st);  // nullptr: the shard already is the block
  void (*unpack)(const bbr_context *c, const void *gathered, void *whole, hipStream_t st);
};
dim3 pixel_grid(size_t n) { return dim3((unsigned)((n + 255) / 256)); }  // every exchange kernel: 256 threads, a pixel each
void pack_packed(const float4 *shard, void *block, size_t n, hipStream_t st) {
  hipLaunchKernelGGL(k_pack_shard, pixel_grid(n), dim3(256), 0, st, shard, (float *)block,
                     (unsigned long long *)((uint8_t *)block + WirePacked::mask_offset(n)), n);
}
void pack_half(const float4 *shard, void *block, size_t n, hipStream_t st) {
  hipLaunchKernelGGL(k_pack_shard_half, pixel_grid(n), dim3(256), 0, st, shard, (uint2 *)block, n);
}
template <class Form>
void unpack(const bbr_context *c, const void *gathered, void *whole, hipStream_t st) {
  hipLaunchKernelGGL(k_unpack_gathered<Form>, pixel_grid((size_t)c->width * c->height), dim3(256), 0, st, (const uint8_t *)gathered,
                     (typename Form::Whole *)whole, c->width, c->height, c->world, c->eff_band_rows(), c->shard_pixels());
}
template <class Form>
constexpr WireForm wire_form(bool presented, decltype(WireForm::pack) pack) {
  return {&Form::block_bytes, sizeof(typename Form::Whole), presented, pack ? (size_t)8 : (size_t)4, Form::kLoadAlign, pack, &unpack<Form>};
}
const WireForm kWireForms[] = {wire_form<WireRgba32f>(false, nullptr), wire_form<WirePacked>(false, pack_packed),
                               wire_form<WireRgba8>(true, nullptr), wire_form<WireRgba16f>(false, pack_half)};
static_assert(BBR_SHARD_RGBA32F == 0 && BBR_SHARD_PACKED == 1 && BBR_SHARD_RGBA8 == 2 && BBR_SHARD_RGBA16F == 3, "kWireForms");

bool valid_form(int form) { return form >= 0 && form < (int)(sizeof(kWireForms) / sizeof(kWireForms[0])); }
bool aligned(const void *p, size_t a) { return ((uintptr_t)p % a) == 0; }
// nothing is launched on a pointer a kernel would access misaligned
int check_unpack_pointers(bbr_context *c, int form, const void *gathered, const void *whole, const char *who) {
  const WireForm &f = kWireForms[form];
  if (!aligned(gathered, f.gathered_align) || !aligned(whole, f.whole_pixel_bytes))
    return fail(c, BBR_ERR_INVALID_ARGUMENT, std::string(who) + ": gather buffer or whole frame not aligned for this form (include/bibim_hip.h, Alignment)");
  return BBR_OK;
}
size_t exchange_block_bytes(const bbr_context *c, int form) { return kWireForms[form].block_bytes(c->shard_pixels()); }
size_t whole_frame_bytes(const bbr_context *c, int form) { return (size_t)c->width * c->height * kWireForms[form].whole_pixel_bytes; }

int open_rccl(bbr_context *c) {
  std::lock_guard<std::mutex> lock(g_rccl_mutex);
  if (g_rccl.lib) return BBR_OK;
  void *lib = nullptr;
  for (const char *name : {"librccl.so.1", "librccl.so"}) {
    lib = dlopen(name, RTLD_NOW | RTLD_LOCAL);
    if (lib) break;
  }
  if (!lib) return fail(c, BBR_ERR_HIP, std::string("RCCL not found (librccl.so.1): ") + dlerror());
  Rccl r;
  r.get_unique_id = (decltype(r.get_unique_id))dlsym(lib, "ncclGetUniqueId");
  r.comm_init_rank = (decltype(r.comm_init_rank))dlsym(lib, "ncclCommInitRank");
  r.all_gather = (decltype(r.all_gather))dlsym(lib, "ncclAllGather");
  r.comm_destroy = (decltype(r.comm_destroy))dlsym(lib, "ncclCommDestroy");
  r.comm_count = (decltype(r.comm_count))dlsym(lib, "ncclCommCount");
  r.error_string = (decltype(r.error_string))dlsym(lib, "ncclGetErrorString");
  if (!r.get_unique_id || !r.comm_init_rank || !r.all_gather || !r.comm_destroy || !r.comm_count || !r.error_string)
    return fail(c, BBR_ERR_HIP, "librccl lacks an entry point");
  r.lib = lib;
  g_rccl = r;
  return BBR_OK;
}

#define RCCL_TRY(ctx, expr)                                                                                    \
  do {                                                                                                         \
    ncclResult_t _r = (expr);                                                                                  \
    if (_r != ncclSuccess) return fail(ctx, BBR_ERR_HIP, std::string(#expr) + ": " + g_rccl.error_string(_r)); \
  } while (0)

// Put this rank's block of the last frame where the exchange reads it: `dst` (the rank's slot of a gather buffer, or a
// peer's).  rgba32f / rgba8 blocks that already live there (the frame was rendered into the slot) cost nothing.
int stage_block(bbr_context *c, FrameSlot &s, int form, void *dst, hipStream_t st) {
  const WireForm &f = kWireForms[form];
  const void *shard = f.presented ? (const void *)s.present.out : (const void *)s.out_used;
  if (f.pack) {
    f.pack((const float4 *)shard, dst, c->shard_pixels(), st);
    HIP_TRY(c, hipGetLastError());
  } else if (shard != dst) {
    HIP_TRY(c, hipMemcpyAsync(dst, shard, exchange_block_bytes(c, form), hipMemcpyDeviceToDevice, st));
  }
  return BBR_OK;
}

int check_exchange(bbr_context *c, int form, const char *who) {
  if (!valid_form(form))
    return fail(c, BBR_ERR_INVALID_ARGUMENT, std::string(who) + ": form must be BBR_SHARD_RGBA32F, _PACKED, _RGBA8 or _RGBA16F");
  if (!c->have_frame || c->last_slot < 0) return fail(c, BBR_ERR_NOT_IN_FRAME, std::string(who) + ": nothing rendered");
  const FrameSlot &s = c->slots[c->last_slot];
  if (form == BBR_SHARD_PACKED && c->supersample > 1)  // (the form keeps one alpha BIT: a resolved alpha is a covered fraction)
    return fail(c, BBR_ERR_INVALID_ARGUMENT, std::string(who) + ": BBR_SHARD_PACKED is not lossless with option supersample >= 2");
  if (kWireForms[form].presented) {
    if (!s.present.active || !s.present.out) return fail(c, BBR_ERR_NOT_IN_FRAME, std::string(who) + ": BBR_SHARD_RGBA8 needs bbr_present first");
  } else if (s.mode.fused) {
    return fail(c, BBR_ERR_INVALID_ARGUMENT, std::string(who) + ": no fp32 frame with option present_fused (use BBR_SHARD_RGBA8)");
  }
  return BBR_OK;
}

int unpack_whole(bbr_context *c, int form, const void *gathered, void *whole, hipStream_t st) {
  forget_image(c);  // (`whole` may be a slot's frame: the caller's pointer)
  kWireForms[form].unpack(c, gathered, whole, st);
  HIP_TRY(c, hipGetLastError());
  return BBR_OK;
}

// the per-form bbr_unpack_gathered* calls: bbr_unpack_whole without its bookkeeping -- no rendered frame needed, the
// caller's `frame`, the context's shading stream by default, no trace in what bbr_read_whole_frame reads
int unpack_gathered(bbr_context *c, int form, const void *gathered, void *frame, void *stream) {
  if (!c) return BBR_ERR_INVALID_ARGUMENT;
  BBR_ON_DEVICE(c);
  if (!gathered || !frame) return fail(c, BBR_ERR_INVALID_ARGUMENT, "unpack_gathered: NULL");
  if (int rc = check_unpack_pointers(c, form, gathered, frame, "unpack_gathered")) return rc;
  return unpack_whole(c, form, gathered, frame, stream ? (hipStream_t)stream : c->shade_stream());
}

}  // namespace

extern "C" {

int bbr_comm_unique_id(bbr_context *c, uint8_t *out_id) {
  if (!c) return BBR_ERR_INVALID_ARGUMENT;
  BBR_ON_DEVICE(c);
  if (!out_id) return fail(c, BBR_ERR_INVALID_ARGUMENT, "comm_unique_id: NULL");
  int rc = open_rccl(c);
  if (rc) return rc;
  static_assert(BBR_COMM_ID_BYTES == NCCL_UNIQUE_ID_BYTES, "BBR_COMM_ID_BYTES");
  ncclUniqueId id;
  RCCL_TRY(c, g_rccl.get_unique_id(&id));
  memcpy(out_id, id.internal, BBR_COMM_ID_BYTES);
  return BBR_OK;
}

int bbr_comm_init(bbr_context *c, int32_t rank, int32_t world, const uint8_t *unique_id) {
  if (!c) return BBR_ERR_INVALID_ARGUMENT;
  BBR_ON_DEVICE(c);
  if (!unique_id || world < 1 || rank < 0 || rank >= world) return fail(c, BBR_ERR_INVALID_ARGUMENT, "comm_init: bad rank / world / id");
  if (c->comm) return fail(c, BBR_ERR_INVALID_ARGUMENT, "comm_init: the context already has a communicator (bbr_comm_destroy first)");
  int rc = open_rccl(c);
  if (rc) return rc;
  ncclUniqueId id;
  memcpy(id.internal, unique_id, BBR_COMM_ID_BYTES);
  RCCL_TRY(c, g_rccl.comm_init_rank(&c->comm, world, id, rank));  // collective: returns once every rank has called it
  c->comm_rank = rank;
  c->comm_world = world;
  return BBR_OK;
}

int bbr_comm_probe(bbr_context *c) {
  if (!c) return BBR_ERR_INVALID_ARGUMENT;
  BBR_ON_DEVICE(c);
  return open_rccl(c);  // dlopen + dlsym only: nothing collective, safe to call on one rank alone
}

int bbr_comm_count(bbr_context *c, int32_t *out_ranks) {
  if (!c) return BBR_ERR_INVALID_ARGUMENT;
  if (!out_ranks) return fail(c, BBR_ERR_INVALID_ARGUMENT, "comm_count: NULL");
  if (!c->comm) return fail(c, BBR_ERR_NOT_IN_FRAME, "comm_count: no communicator (bbr_comm_init)");
  int n = 0;
  RCCL_TRY(c, g_rccl.comm_count(c->comm, &n));
  *out_ranks = n;
  return BBR_OK;
}

int bbr_stage_shard(bbr_context *c, int32_t form, void *block_device, void *stream) {
  if (!c) return BBR_ERR_INVALID_ARGUMENT;
  BBR_ON_DEVICE(c);
  int rc = check_exchange(c, form, "stage_shard");
  if (rc) return rc;
  if (!block_device) return fail(c, BBR_ERR_INVALID_ARGUMENT, "stage_shard: NULL");
  if (!aligned(block_device, kWireForms[form].block_align))
    return fail(c, BBR_ERR_INVALID_ARGUMENT, "stage_shard: block not aligned for this form (include/bibim_hip.h, Alignment)");
  FrameSlot &s = c->slots[c->last_slot];
  hipStream_t st = stream ? (hipStream_t)stream : s.stream_used;  // a caller's stream must already wait for the frame
  return stage_block(c, s, form, block_device, st);
}

int bbr_comm_destroy(bbr_context *c) {
  if (!c) return BBR_ERR_INVALID_ARGUMENT;
  BBR_ON_DEVICE(c);
  if (!c->comm) return BBR_OK;
  int rc = drain(c);
  if (rc) return rc;
  ncclComm_t comm = c->comm;
  c->comm = nullptr;
  c->comm_rank = -1;
  c->comm_world = 0;
  RCCL_TRY(c, g_rccl.comm_destroy(comm));
  return BBR_OK;
}

int bbr_exchange_block_bytes(const bbr_context *c, int32_t form, uint64_t *out_bytes) {
  if (!c || !out_bytes || !valid_form(form)) return BBR_ERR_INVALID_ARGUMENT;
  *out_bytes = exchange_block_bytes(c, form);
  return BBR_OK;
}

int bbr_allgather_frame(bbr_context *c, int32_t form, void *gathered, void *whole, void *stream) {
  if (!c) return BBR_ERR_INVALID_ARGUMENT;
  BBR_ON_DEVICE(c);
  int rc = check_exchange(c, form, "allgather_frame");
  if (rc) return rc;
  if (!c->comm) return fail(c, BBR_ERR_NOT_IN_FRAME, "allgather_frame: no communicator (bbr_comm_init)");
  if (c->comm_rank != c->rank || c->comm_world != c->world)
    return fail(c, BBR_ERR_INVALID_ARGUMENT, "allgather_frame: the communicator's rank / world differ from the partition's (bbr_set_partition)");
  if (!aligned(gathered, kWireForms[form].block_align))  // (NULL passes every check: the slot's own buffers are hipMalloc'ed)
    return fail(c, BBR_ERR_INVALID_ARGUMENT, "allgather_frame: gather buffer not aligned for this form (include/bibim_hip.h, Alignment)");
  rc = check_unpack_pointers(c, form, gathered, whole, "allgather_frame");
  if (rc) return rc;
  FrameSlot &s = c->slots[c->last_slot];
  const size_t block = exchange_block_bytes(c, form);
  if (!gathered) {
    HIP_TRY(c, s.d_gathered.ensure(block * (size_t)c->world));
    gathered = s.d_gathered.ptr;
  }
  if (!whole) {
    HIP_TRY(c, s.d_whole.ensure(whole_frame_bytes(c, form)));
    whole = s.d_whole.ptr;
  }
  hipStream_t st = stream ? (hipStream_t)stream : s.stream_used;
  HIP_TRY(c, s.follow(st));
  uint8_t *mine = (uint8_t *)gathered + block * (size_t)c->rank;
  rc = stage_block(c, s, form, mine, st);
  if (rc) return rc;
  // in place: the send buffer is this rank's slot of the receive buffer
  RCCL_TRY(c, g_rccl.all_gather(mine, gathered, block, ncclUint8, c->comm, st));
  rc = unpack_whole(c, form, gathered, whole, st);
  if (rc) return rc;
  if (!stream) HIP_TRY(c, s.busy_until(st));  // ... until its exchange is through
  c->exchange_slot = c->last_slot;
  c->exchange_form = form;
  c->exchange_whole = whole;
  return BBR_OK;
}

int bbr_push_shard(bbr_context *c, int32_t form, void *const *peer_gathered, const int32_t *peer_devices, void *stream) {
  if (!c) return BBR_ERR_INVALID_ARGUMENT;
  BBR_ON_DEVICE(c);
  int rc = check_exchange(c, form, "push_shard");
  if (rc) return rc;
  if (!peer_gathered || !peer_devices) return fail(c, BBR_ERR_INVALID_ARGUMENT, "push_shard: NULL");
  FrameSlot &s = c->slots[c->last_slot];
  const size_t block = exchange_block_bytes(c, form);
  hipStream_t st = stream ? (hipStream_t)stream : s.stream_used;
  HIP_TRY(c, s.follow(st));
  for (int p = 0; p < c->world; ++p)
    if (!peer_gathered[p]) return fail(c, BBR_ERR_INVALID_ARGUMENT, "push_shard: a peer's gather buffer is NULL");
  for (int p = 0; p < c->world; ++p)
    if (!aligned(peer_gathered[p], kWireForms[form].block_align))
      return fail(c, BBR_ERR_INVALID_ARGUMENT, "push_shard: a peer's gather buffer is not aligned for this form (include/bibim_hip.h, Alignment)");
  // the block is made once, in this rank's own gather buffer, and goes from there to the peers
  uint8_t *mine = (uint8_t *)peer_gathered[c->rank] + block * (size_t)c->rank;
  rc = stage_block(c, s, form, mine, st);
  if (rc) return rc;
  // push_mode 1 (default): ONE kernel stores the block into every peer's buffer, all links busy at once.  It needs the
  // peers' memory mapped into this device's address space: the same device, an opened IPC handle, or peer access, which
  // is switched on here the first time a device shows up.  A peer that cannot be mapped: the copies below instead.
  bool direct = c->push_mode == 1 && c->world > 1;
  for (int p = 0; direct && p < c->world; ++p) {
    const int dev = peer_devices[p];
    if (dev == c->device || c->peer_mapped.count(dev)) continue;
    int can = 0;
    hipError_t e = hipDeviceCanAccessPeer(&can, c->device, dev);
    if (e == hipSuccess && can) e = hipDeviceEnablePeerAccess(dev, 0);
    (void)hipGetLastError();  // (neither outcome may linger as the runtime's "last error": the copies below are a full substitute)
    if (!can || (e != hipSuccess && e != hipErrorPeerAccessAlreadyEnabled)) { direct = false; break; }
    c->peer_mapped.insert(dev);
  }
  if (direct) {
    bool wide = block % 16 == 0;   // 16-byte accesses when every address involved allows them, 4-byte ones otherwise
    for (int p = 0; p < c->world; ++p) wide = wide && ((uintptr_t)peer_gathered[p] % 16) == 0;
    const size_t n = wide ? block / 16 : block / 4;   // (every block form is a whole number of 4-byte words)
    // a grid of one workgroup per CU: the copy is bound by the links (world - 1 x ~60 GB/s), not by the CUs it occupies
    const unsigned grid = (unsigned)std::max<size_t>(1, std::min<size_t>((size_t)c->n_cus, (n + kPushThreads - 1) / kPushThreads));
    for (int k0 = 1; k0 < c->world; k0 += kMaxPushPeers) {
      PushTargets t = {};
      int nt = 0;
      for (int k = k0; k < c->world && nt < kMaxPushPeers; ++k)
        t.dst[nt++] = (uint8_t *)peer_gathered[(c->rank + k) % c->world] + block * (size_t)c->rank;
      if (wide) hipLaunchKernelGGL(k_push_block<uint4>, dim3(grid), dim3(kPushThreads), 0, st, (const uint4 *)mine, t, nt, n);
      else hipLaunchKernelGGL(k_push_block<uint32_t>, dim3(grid), dim3(kPushThreads), 0, st, (const uint32_t *)mine, t, nt, n);
    }
    HIP_TRY(c, hipGetLastError());
  } else {
    // push_mode 0: copies queued one behind the other on the one stream, nearest rank first (rank + 1, rank + 2, ...): at any
    // moment this rank drives ONE of its links -- ring timing on a full mesh
    for (int k = 1; k < c->world; ++k) {
      const int p = (c->rank + k) % c->world;
      HIP_TRY(c, hipMemcpyPeerAsync((uint8_t *)peer_gathered[p] + block * (size_t)c->rank, peer_devices[p], mine, c->device, block, st));
    }
  }
  c->last_push_direct = direct;
  if (!stream) HIP_TRY(c, s.busy_until(st));
  return BBR_OK;
}

int bbr_push_state(const bbr_context *c, int32_t *out_direct) {
  if (!c || !out_direct) return BBR_ERR_INVALID_ARGUMENT;
  *out_direct = c->last_push_direct ? 1 : 0;
  return BBR_OK;
}

int bbr_unpack_whole(bbr_context *c, int32_t form, const void *gathered, void *whole, void *stream) {
  if (!c) return BBR_ERR_INVALID_ARGUMENT;
  BBR_ON_DEVICE(c);
  if (!valid_form(form) || !gathered) return fail(c, BBR_ERR_INVALID_ARGUMENT, "unpack_whole: bad form / NULL");
  if (c->last_slot < 0) return fail(c, BBR_ERR_NOT_IN_FRAME, "unpack_whole: nothing rendered");
  if (int rc = check_unpack_pointers(c, form, gathered, whole, "unpack_whole")) return rc;
  FrameSlot &s = c->slots[c->last_slot];
  if (!whole) {
    HIP_TRY(c, s.d_whole.ensure(whole_frame_bytes(c, form)));
    whole = s.d_whole.ptr;
  }
  int rc = unpack_whole(c, form, gathered, whole, stream ? (hipStream_t)stream : s.stream_used);
  if (rc) return rc;
  c->exchange_slot = c->last_slot;
  c->exchange_form = form;
  c->exchange_whole = whole;
  return BBR_OK;
}

// ---- the per-form calls that came before the general ones: each is one form of bbr_stage_shard / bbr_unpack_whole ----
int bbr_unpack_gathered(bbr_context *c, const void *g, void *frame, void *st) { return unpack_gathered(c, BBR_SHARD_RGBA32F, g, frame, st); }
int bbr_unpack_gathered_packed(bbr_context *c, const void *g, void *frame, void *st) { return unpack_gathered(c, BBR_SHARD_PACKED, g, frame, st); }
int bbr_unpack_gathered_rgba8(bbr_context *c, const void *g, void *frame, void *st) { return unpack_gathered(c, BBR_SHARD_RGBA8, g, frame, st); }
int bbr_packed_shard_bytes(const bbr_context *c, uint64_t *out_bytes) { return bbr_exchange_block_bytes(c, BBR_SHARD_PACKED, out_bytes); }
int bbr_pack_shard(bbr_context *c, void *packed, void *stream) {
  if (c && !packed) return fail(c, BBR_ERR_INVALID_ARGUMENT, "pack_shard: NULL");  // (reported ahead of the frame's state)
  return bbr_stage_shard(c, BBR_SHARD_PACKED, packed, stream);
}

int bbr_whole_frame_device_ptr(bbr_context *c, void **out_ptr, uint64_t *out_bytes) {
  if (!c) return BBR_ERR_INVALID_ARGUMENT;
  if (!out_ptr) return fail(c, BBR_ERR_INVALID_ARGUMENT, "whole_frame_device_ptr: NULL");
  if (c->exchange_slot < 0 || !c->exchange_whole) return fail(c, BBR_ERR_NOT_IN_FRAME, "whole_frame_device_ptr: no exchange yet");
  *out_ptr = c->exchange_whole;
  if (out_bytes) *out_bytes = whole_frame_bytes(c, c->exchange_form);
  return BBR_OK;
}

int bbr_read_whole_frame(bbr_context *c, void *host) {
  if (!c) return BBR_ERR_INVALID_ARGUMENT;
  BBR_ON_DEVICE(c);
  if (!host) return fail(c, BBR_ERR_INVALID_ARGUMENT, "read_whole_frame: NULL");
  if (c->exchange_slot < 0 || !c->exchange_whole) return fail(c, BBR_ERR_NOT_IN_FRAME, "read_whole_frame: no exchange yet");
  int rc = drain(c);  // (not sync_and_fix: a re-render on one rank alone would leave the collective unmatched)
  if (rc) return rc;
  HIP_TRY(c, hipMemcpy(host, c->exchange_whole, whole_frame_bytes(c, c->exchange_form), hipMemcpyDeviceToHost));
  return BBR_OK;
}

int bbr_device_alloc(bbr_context *c, uint64_t bytes, void **out_ptr) {
  if (!c) return BBR_ERR_INVALID_ARGUMENT;
  BBR_ON_DEVICE(c);
  if (!out_ptr || !bytes) return fail(c, BBR_ERR_INVALID_ARGUMENT, "device_alloc: NULL / zero bytes");
  *out_ptr = nullptr;
  HIP_TRY(c, hipMalloc(out_ptr, bytes));
  HIP_TRY(c, zero_fill_sync(*out_ptr, bytes));
  return BBR_OK;
}

int bbr_device_free(bbr_context *c, void *ptr) {
  if (!c) return BBR_ERR_INVALID_ARGUMENT;
  BBR_ON_DEVICE(c);
  if (!ptr) return BBR_OK;
  int rc = drain(c);
  if (rc) return rc;
  HIP_TRY(c, hipFree(ptr));
  return BBR_OK;
}

int bbr_copy_to_host(bbr_context *c, void *host, const void *device_ptr, uint64_t bytes) {
  if (!c) return BBR_ERR_INVALID_ARGUMENT;
  BBR_ON_DEVICE(c);
  if (!host || !device_ptr) return fail(c, BBR_ERR_INVALID_ARGUMENT, "copy_to_host: NULL");
  int rc = drain(c);
  if (rc) return rc;
  HIP_TRY(c, hipMemcpy(host, device_ptr, bytes, hipMemcpyDeviceToHost));
  return BBR_OK;
}

int bbr_ipc_export(bbr_context *c, void *device_ptr, uint8_t *out_handle) {
  if (!c) return BBR_ERR_INVALID_ARGUMENT;
  BBR_ON_DEVICE(c);
  if (!device_ptr || !out_handle) return fail(c, BBR_ERR_INVALID_ARGUMENT, "ipc_export: NULL");
  static_assert(BBR_IPC_HANDLE_BYTES == sizeof(hipIpcMemHandle_t), "BBR_IPC_HANDLE_BYTES");
  hipIpcMemHandle_t h;
  HIP_TRY(c, hipIpcGetMemHandle(&h, device_ptr));
  memcpy(out_handle, &h, sizeof h);
  return BBR_OK;
}

int bbr_ipc_open(bbr_context *c, const uint8_t *handle, void **out_ptr) {
  if (!c) return BBR_ERR_INVALID_ARGUMENT;
  BBR_ON_DEVICE(c);
  if (!handle || !out_ptr) return fail(c, BBR_ERR_INVALID_ARGUMENT, "ipc_open: NULL");
  hipIpcMemHandle_t h;
  memcpy(&h, handle, sizeof h);
  HIP_TRY(c, hipIpcOpenMemHandle(out_ptr, h, hipIpcMemLazyEnablePeerAccess));
  return BBR_OK;
}

int bbr_ipc_close(bbr_context *c, void *ptr) {
  if (!c) return BBR_ERR_INVALID_ARGUMENT;
  BBR_ON_DEVICE(c);
  if (!ptr) return fail(c, BBR_ERR_INVALID_ARGUMENT, "ipc_close: NULL");
  HIP_TRY(c, hipIpcCloseMemHandle(ptr));
  return BBR_OK;
}

int bbr_selftest_rcp(bbr_context *c, uint32_t lo_bits, uint32_t hi_bits, uint64_t *out_mismatches) {
  if (!c) return BBR_ERR_INVALID_ARGUMENT;
  BBR_ON_DEVICE(c);
  if (!out_mismatches || hi_bits < lo_bits) return fail(c, BBR_ERR_INVALID_ARGUMENT, "selftest_rcp: bad arguments");
  int rc = drain(c);
  if (rc) return rc;
  unsigned long long h = 0;
  DeviceBuffer<unsigned long long> d;
  HIP_TRY(c, d.ensure(1, true));
  hipLaunchKernelGGL(k_selftest_rcp, dim3(4096), dim3(256), 0, c->geom_stream(), d.ptr, lo_bits, hi_bits);
  HIP_TRY(c, hipMemcpy(&h, d.ptr, sizeof h, hipMemcpyDeviceToHost));
  *out_mismatches = h;
  return BBR_OK;
}

static_assert(sizeof(bbr_tbn_segment) == sizeof(TbnSeg) && offsetof(bbr_tbn_segment, za) == offsetof(TbnSeg, za) &&
                  offsetof(bbr_tbn_segment, key) == offsetof(TbnSeg, key), "bbr_tbn_segment");

int bbr_read_tbn_segments(bbr_context *c, bbr_tbn_segment *out, uint32_t cap, uint32_t *out_count) {
  if (!c) return BBR_ERR_INVALID_ARGUMENT;
  BBR_ON_DEVICE(c);
  if (!out_count) return fail(c, BBR_ERR_INVALID_ARGUMENT, "read_tbn_segments: NULL count");
  if (!c->tbn_pass.valid) return fail(c, BBR_ERR_NOT_IN_FRAME, "read_tbn_segments: no TBN draw since the context was created or resized");
  int rc = drain(c);
  if (rc) return rc;
  std::vector<TbnSeg> all(c->tbn_pass.n_slots);
  if (!all.empty()) HIP_TRY(c, hipMemcpy(all.data(), c->tbn_pass.d_segs.ptr, all.size() * sizeof(TbnSeg), hipMemcpyDeviceToHost));
  uint32_t n = 0;
  for (const TbnSeg &s : all) {
    if (s.key == kTbnNoSeg) continue;
    if (out && n < cap) std::memcpy(out + n, &s, sizeof s);
    ++n;
  }
  *out_count = n;
  return BBR_OK;
}

int bbr_selftest_lines(bbr_context *c, const bbr_tbn_segment *segs, uint32_t n, int32_t width, int32_t height,
                       const float *depth, uint32_t *out_keys) {
  if (!c) return BBR_ERR_INVALID_ARGUMENT;
  BBR_ON_DEVICE(c);
  if ((n && !segs) || !depth || !out_keys || width <= 0 || height <= 0 || width > 32768 || height > 32768)
    return fail(c, BBR_ERR_INVALID_ARGUMENT, "selftest_lines: bad arguments");
  std::vector<TbnSeg> h(n);
  if (n) std::memcpy(h.data(), segs, (size_t)n * sizeof(TbnSeg));
  for (const TbnSeg &s : h) {
    const int32_t lim = 1 << 25;  // (what the guard band guarantees for the pass's own segments)
    if (s.key == kTbnNoSeg || std::abs(s.X0) > lim || std::abs(s.Y0) > lim || std::abs(s.X1) > lim || std::abs(s.Y1) > lim)
      return fail(c, BBR_ERR_INVALID_ARGUMENT, "selftest_lines: key 0xFFFFFFFF or a coordinate beyond 2^25");
  }
  int rc = drain(c);
  if (rc) return rc;
  const size_t px = (size_t)width * height;
  DeviceBuffer<TbnSeg> segs_buf;
  DeviceBuffer<float> depth_buf;
  DeviceBuffer<uint32_t> keys_buf;
  hipError_t e = segs_buf.ensure(std::max<size_t>(n, 1));
  if (e == hipSuccess) e = depth_buf.ensure(px);
  if (e == hipSuccess) e = keys_buf.ensure(px);
  TbnSeg *const d_segs = segs_buf.ptr;
  float *const d_depth = depth_buf.ptr;
  uint32_t *const d_keys = keys_buf.ptr;
  if (e == hipSuccess && n) e = upload_sync(d_segs, h.data(), (size_t)n * sizeof(TbnSeg));
  if (e == hipSuccess) e = upload_sync(d_depth, depth, px * sizeof(float));
  HIP_TRY(c, e);
  hipStream_t st = c->geom_stream();
  rc = BBR_ERR_CAPACITY;
  for (int attempt = 0; attempt < 8 && rc == BBR_ERR_CAPACITY; ++attempt) {
    TbnParams tp;
    int r = tbn_launch_params(c, width, height, tp);
    if (r) return r;
    if (n) hipLaunchKernelGGL(k_tbn_bin, dim3((n + 255) / 256), dim3(256), 0, st, d_segs, n, tp, c->tbn_pass.d_tile_count.ptr,
                              c->tbn_pass.d_bins.ptr, c->tbn_pass.d_ctr.ptr);
    r = tbn_check_bins(c, st);
    if (r < 0) return r;
    if (r == 1) continue;
    e = hipMemsetAsync(d_keys, 0, px * sizeof(uint32_t), st);
    if (e == hipSuccess)
      hipLaunchKernelGGL(k_tbn_raster, dim3(tp.tiles_x, tp.tiles_y, kTbnSplit), dim3(kTbnThreads), 0, st, d_segs,
                         c->tbn_pass.d_tile_count.ptr, c->tbn_pass.d_bins.ptr, tp, d_depth, d_keys);
    if (e == hipSuccess) e = hipGetLastError();
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    if (e == hipSuccess) e = hipMemcpy(out_keys, d_keys, px * sizeof(uint32_t), hipMemcpyDeviceToHost);
    rc = BBR_OK;
  }
  HIP_TRY(c, e);
  if (rc) return fail(c, rc, "selftest_lines: bins still overflow after 8 growth steps");
  return BBR_OK;
}

int bbr_tone_map(bbr_context *c, int32_t enable, float exposure) {
  if (!c) return BBR_ERR_INVALID_ARGUMENT;
  BBR_ON_DEVICE(c);
  if (!c->have_frame || c->last_slot < 0) return fail(c, BBR_ERR_NOT_IN_FRAME, "tone_map: nothing rendered");
  if (c->slots[c->last_slot].mode.fused) return fail(c, BBR_ERR_INVALID_ARGUMENT, "tone_map: no fp32 frame with option present_fused");
  float4 *frame = c->slots[c->last_slot].out_used;
  size_t n = c->shard_pixels();
  forget_image(c);  // (in place)
  // same stream as the frame's shade kernel: ordered after it
  hipLaunchKernelGGL(k_tone_map, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, c->slots[c->last_slot].stream_used, frame, n, enable, exposure);
  HIP_TRY(c, hipGetLastError());
  return BBR_OK;
}

}  // extern "C"

#ifdef BB_STAMPS
// diagnostic build only: per-wave phase cycles of the last k_shade launch (8 x u64 per wave, 4096 waves)
extern "C" int bbr_debug_shade_stamps(bbr_context *c, unsigned long long *out) {
  if (!c || !out) return BBR_ERR_INVALID_ARGUMENT;
  int rc = drain(c);
  if (rc) return rc;
  HIP_TRY(c, hipMemcpyFromSymbol(out, HIP_SYMBOL(bbr::g_shade_stamps), sizeof(unsigned long long) * 4096 * 8));
  return BBR_OK;
}
#endif
