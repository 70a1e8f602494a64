// bb_ui.h -- the GUI pass's host side: what bbr_ui_validate checks, and the few binary32 expressions the host and the
// kernels must agree on bit for bit (vertex snap, scissor, decode table).  No HIP is needed: any C++17 compiler with <cmath>
// takes it; under hipcc ui_snap is also device code, and k_ui_setup calls this very function, so that the bound checked
// here is the bound of the coordinates the kernels see.
//
// The draw data is the GUI back end's (external/imgui/imgui_impl_vulkan.cpp:301-306, 406-425): nothing in it is trusted.
// ui_validate is the only door to the kernels (bb_ui_kernels.hip.h), which bound every loop and every address by the counts
// that passed here and check nothing again.
#pragma once
#include <cstddef>
#include <cstdint>
#include <cstring>
#include <cmath>
#include <math.h>  // ::fmaf, ::fabsf, ::rintf: the names host and device code share

#include "bibim_hip.h"

#if defined(__HIPCC__)
#define BB_UI_HD __host__ __device__ inline
#else
#define BB_UI_HD inline
#endif

namespace bbr {

constexpr int kUiVertexBytes = 20;            // ImDrawVert: pos f32x2 @0, uv f32x2 @8, col RGBA8 @16
constexpr int32_t kUiSnapLimit = 1 << 23;     // |snapped coordinate| in 1/256 pixel: edge functions stay far inside int64

// scale / translate of the vertex stage (external/imgui/imgui_impl_vulkan.cpp:301-306) and the viewport's half extents
struct UiTransform {
  float scale[2], translate[2], half[2];
};

inline UiTransform ui_transform(const bbr_ui_draw &d, int32_t fb_w, int32_t fb_h) {
  UiTransform t;
  for (int k = 0; k < 2; ++k) {
    t.scale[k] = 2.0f / d.display_size[k];
    const float ps = d.display_pos[k] * t.scale[k];
    t.translate[k] = -1.0f - ps;
  }
  t.half[0] = 0.5f * (float)fb_w;
  t.half[1] = 0.5f * (float)fb_h;
  return t;
}

// One coordinate: ndc = pos * scale + translate (a multiply, then an add: external/imgui/imgui_impl_vulkan.cpp:126), then
// the viewport transform and snap of project_vertex (bb_kernels.hip.h) with w = 1, restated: fmaf(ndc, half, centre) with the
// centre at half, the same range test, rintf of 256 xs.  False: not finite or outside +-kUiSnapLimit.  The validator and
// k_ui_setup both call this function; nothing else snaps a GUI vertex.
BB_UI_HD bool ui_snap(float pos, float scale, float translate, float half, int32_t &X) {
  const float m = pos * scale;
  const float ndc = m + translate;
  const float xs = fmaf(ndc, half, half);
  if (!(fabsf(xs) <= 4194304.0f)) return false;
  X = (int32_t)rintf(xs * 256.0f);
  return X >= -kUiSnapLimit && X <= kUiSnapLimit;
}

// The scissor of one command, external/imgui/imgui_impl_vulkan.cpp:406-425 with its quirks: the command is skipped unless
// x < fb_w && y < fb_h && z >= 0 && w >= 0 (a NaN skips it); negative x / y become 0; offset = (int32)x and extent =
// (uint32)(z - x): the DIFFERENCE is truncated, not the ends.  A negative difference (z < x), which the back end hands to an
// undefined conversion, is an empty scissor here.  Returned as the pixel box offset <= p < offset + extent, cut to the frame;
// false: nothing can pass.
inline bool ui_scissor(const float clip[4], const bbr_ui_draw &d, int32_t fb_w, int32_t fb_h, int32_t box[4]) {
  float r[4];
  for (int k = 0; k < 4; ++k) r[k] = (clip[k] - d.display_pos[k & 1]) * d.framebuffer_scale[k & 1];
  box[0] = box[1] = box[2] = box[3] = 0;
  if (!(r[0] < (float)fb_w && r[1] < (float)fb_h && r[2] >= 0.0f && r[3] >= 0.0f)) return false;
  if (r[0] < 0.0f) r[0] = 0.0f;
  if (r[1] < 0.0f) r[1] = 0.0f;
  const int32_t lim[2] = {fb_w, fb_h};
  for (int k = 0; k < 2; ++k) {
    const int64_t off = (int64_t)(int32_t)r[k];  // 0 <= r[k] < fb extent: the conversion is defined
    const float diff = r[k + 2] - r[k];
    int64_t ext = 0;
    if (diff >= 4294967296.0f) ext = 4294967295ll;
    else if (diff >= 1.0f) ext = (int64_t)diff;
    const int64_t end = off + ext < (int64_t)lim[k] ? off + ext : (int64_t)lim[k];
    box[k] = (int32_t)off;
    box[k + 2] = (int32_t)end;
  }
  return box[2] > box[0] && box[3] > box[1];
}

inline bool ui_finite(float x) { return x - x == 0.0f; }

// Everything bbr_draw_ui requires of the draw data itself (a texture handle needs a context).  out_box: the union of the
// drawing commands' scissors cut to the frame (x0 y0 x1 y1, exclusive ends; all zero when nothing can be drawn).
inline int ui_validate(const bbr_ui_draw *d, int32_t fb_w, int32_t fb_h, int32_t *out_box) {
  if (out_box) out_box[0] = out_box[1] = out_box[2] = out_box[3] = 0;
  if (!d || fb_w <= 0 || fb_h <= 0 || fb_w > 32768 || fb_h > 32768) return BBR_ERR_INVALID_ARGUMENT;
  if ((d->n_vertices && !d->vertices) || (d->n_indices && !d->indices) || (d->n_cmds && !d->cmds)) return BBR_ERR_INVALID_ARGUMENT;
  for (int k = 0; k < 2; ++k) {
    if (!(d->display_size[k] > 0.0f) || !ui_finite(d->display_size[k])) return BBR_ERR_INVALID_ARGUMENT;
    if (!ui_finite(d->display_pos[k]) || !ui_finite(d->framebuffer_scale[k])) return BBR_ERR_INVALID_ARGUMENT;
  }
  const UiTransform t = ui_transform(*d, fb_w, fb_h);
  const uint8_t *vb = static_cast<const uint8_t *>(d->vertices);
  for (uint32_t i = 0; i < d->n_vertices; ++i) {
    float f[4];
    std::memcpy(f, vb + (size_t)i * kUiVertexBytes, sizeof f);  // pos, uv
    if (!ui_finite(f[0]) || !ui_finite(f[1]) || !ui_finite(f[2]) || !ui_finite(f[3])) return BBR_ERR_INVALID_ARGUMENT;
    int32_t X, Y;
    if (!ui_snap(f[0], t.scale[0], t.translate[0], t.half[0], X) || !ui_snap(f[1], t.scale[1], t.translate[1], t.half[1], Y))
      return BBR_ERR_INVALID_ARGUMENT;
  }
  int32_t u[4] = {0, 0, 0, 0};
  bool any = false;
  for (uint32_t ci = 0; ci < d->n_cmds; ++ci) {
    const bbr_ui_cmd &cmd = d->cmds[ci];
    if (cmd.elem_count % 3u) return BBR_ERR_INVALID_ARGUMENT;
    if ((uint64_t)cmd.idx_offset + cmd.elem_count > (uint64_t)d->n_indices) return BBR_ERR_INVALID_ARGUMENT;
    for (uint32_t k = 0; k < cmd.elem_count; ++k)
      if ((uint64_t)cmd.vtx_offset + d->indices[cmd.idx_offset + k] >= (uint64_t)d->n_vertices) return BBR_ERR_INVALID_ARGUMENT;
    int32_t b[4];
    if (!cmd.elem_count || !ui_scissor(cmd.clip_rect, *d, fb_w, fb_h, b)) continue;
    if (!any) {
      std::memcpy(u, b, sizeof u);
      any = true;
    } else {
      u[0] = b[0] < u[0] ? b[0] : u[0];
      u[1] = b[1] < u[1] ? b[1] : u[1];
      u[2] = b[2] > u[2] ? b[2] : u[2];
      u[3] = b[3] > u[3] ? b[3] : u[3];
    }
  }
  if (out_box) std::memcpy(out_box, u, sizeof u);
  return BBR_OK;
}

// dec[b]: the linear value an sRGB byte stands for, (float) of the binary64 EOTF of b / 255.0 -- the destination of a blend
inline void ui_dec_table(float dec[256]) {
  for (int b = 0; b < 256; ++b) {
    const double x = (double)b / 255.0;
    dec[b] = (float)(x <= 0.04045 ? x / 12.92 : std::pow((x + 0.055) / 1.055, 2.4));
  }
}

}  // namespace bbr
