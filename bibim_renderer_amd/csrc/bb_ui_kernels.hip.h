// bb_ui_kernels.hip.h -- the GUI pass (bbr_draw_ui): the back end's draw lists blended into the presented image.
//
// Replaces ImGui_ImplVulkan_RenderDrawData (src/main.cpp:172; external/imgui/imgui_impl_vulkan.cpp:122-126, 181-183,
// 301-306, 406-425, 610-618, 716, 724-732).  The rule is pinned in DESIGN.md section 3 and include/bibim_hip.h; in short:
// vertices snapped like scene triangles, integer edge functions with the top-left rule and no culling, the back end's
// scissor, attributes in the difference form from binary64 planes, colour * one bilinear tap, and a SRC_ALPHA /
// ONE_MINUS_SRC_ALPHA blend on the sRGB bytes that is requantised after EVERY fragment, fragments in command and index order.
//
// Order without atomics: k_ui_setup stores triangle t's records at index t, so the arrays are the order; k_ui_tiles gives
// one workgroup a 32 x 32 tile whose pixels live in registers, scans the box records front to back and keeps the survivors
// in an ordered LDS list.  Nothing here checks the draw data: ui_validate (bb_ui.h) has, before anything is launched.
#pragma once
#include "bb_kernels.hip.h"
#include "bb_ui.h"

namespace bbr {

constexpr int kUiTile = 32;
constexpr int kUiThreads = 256;
constexpr int kUiPixelsPerThread = kUiTile * kUiTile / kUiThreads;  // 4: rows ty, ty + 8, ty + 16, ty + 24 of column tx
constexpr int kUiChunk = 1024;                                      // survivors held in LDS at a time

// one command as the kernels see it (built by bbr_draw_ui from a validated bbr_ui_cmd)
struct UiCmd {
  const uint32_t *texels;  // RGBA8, row-major
  int32_t tw, th;
  uint32_t vtx_offset, idx_offset;
  uint32_t first_tri, pad;  // index of the command's first triangle in pass order
  int32_t sx0, sy0, sx1, sy1;  // scissor cut to the frame, exclusive ends
};
static_assert(sizeof(UiCmd) == 48, "UiCmd");

struct UiParams {
  float scale[2], translate[2], half[2];
  int32_t width, height;
};

// attribute k of a triangle in the difference form: a0, a1 - a0, a2 - a0
struct UiAttr {
  float a0, d1, d2;
};
enum { kUiU = 0, kUiV, kUiR, kUiG, kUiB, kUiA, kUiAttrs };

struct alignas(16) UiTri {
  int32_t X[3], Y[3];              // snapped, vertices 1 and 2 exchanged when the area was negative
  float l1dx, l1dy, l2dx, l2dy;    // binary64 planes rounded once (as setup_tri)
  UiAttr attr[kUiAttrs];
  const uint32_t *texels;
  int32_t tw, th;
  int32_t bx0, by0, bx1, by1;      // = the box record
};
static_assert(sizeof(UiTri) == 144, "UiTri");

// pixel box of the triangle ^ scissor ^ frame, exclusive ends; all zero for a triangle that draws nothing
struct UiBox {
  int32_t x0, y0, x1, y1;
};

__global__ __launch_bounds__(256) void k_ui_setup(UiParams p, const UiCmd *__restrict__ cmds, uint32_t n_cmds,
                                                  const uint32_t *__restrict__ vertices, const uint16_t *__restrict__ indices,
                                                  uint32_t n_tris, UiTri *__restrict__ tris, UiBox *__restrict__ boxes) {
  const uint32_t ti = blockIdx.x * 256u + threadIdx.x;
  if (ti >= n_tris) return;
  // the command holding triangle ti: the last one whose first_tri <= ti (bbr_draw_ui leaves out every command without
  // triangles, so first_tri rises strictly and cmds[0].first_tri is 0)
  uint32_t lo = 0, hi = n_cmds;
  while (hi - lo > 1u) {
    const uint32_t mid = lo + ((hi - lo) >> 1);
    if (cmds[mid].first_tri <= ti) lo = mid;
    else hi = mid;
  }
  const UiCmd cmd = cmds[lo];
  const uint32_t i0 = cmd.idx_offset + 3u * (ti - cmd.first_tri);

  int32_t X[3] = {0, 0, 0}, Y[3] = {0, 0, 0};
  float a[3][kUiAttrs];
  bool ok = true;
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    const uint32_t *v = vertices + (size_t)(cmd.vtx_offset + (uint32_t)indices[i0 + k]) * (kUiVertexBytes / 4);
    // the validator's own function: what passed there is inside +-kUiSnapLimit here, bit for bit
    ok &= ui_snap(__uint_as_float(v[0]), p.scale[0], p.translate[0], p.half[0], X[k]);
    ok &= ui_snap(__uint_as_float(v[1]), p.scale[1], p.translate[1], p.half[1], Y[k]);
    a[k][kUiU] = __uint_as_float(v[2]);
    a[k][kUiV] = __uint_as_float(v[3]);
    const uint32_t col = v[4];
#pragma unroll
    for (int ch = 0; ch < 4; ++ch) a[k][kUiR + ch] = (float)((col >> (8 * ch)) & 0xFFu) * (1.0f / 255.0f);
  }
  long long dx1 = (long long)X[1] - X[0], dy1 = (long long)Y[1] - Y[0];
  long long dx2 = (long long)X[2] - X[0], dy2 = (long long)Y[2] - Y[0];
  long long S = dx1 * dy2 - dx2 * dy1;
  if (S < 0) {  // cullMode NONE: the back face is the same triangle with vertices 1 and 2 exchanged, attributes included
    const int32_t tx = X[1], ty = Y[1];
    X[1] = X[2]; Y[1] = Y[2]; X[2] = tx; Y[2] = ty;
#pragma unroll
    for (int q = 0; q < kUiAttrs; ++q) {
      const float t = a[1][q];
      a[1][q] = a[2][q];
      a[2][q] = t;
    }
    const long long sx = dx1, sy = dy1;
    dx1 = dx2; dy1 = dy2; dx2 = sx; dy2 = sy;
    S = -S;
  }
  UiBox b = {0, 0, 0, 0};
  if (ok && S > 0) {
    const int32_t minX = min(X[0], min(X[1], X[2])), maxX = max(X[0], max(X[1], X[2]));
    const int32_t minY = min(Y[0], min(Y[1], Y[2])), maxY = max(Y[0], max(Y[1], Y[2]));
    // pixels whose centre 256 p + 128 lies in [min, max]
    const int32_t x0 = max((minX + 127) >> 8, cmd.sx0), x1 = min(((maxX - 128) >> 8) + 1, cmd.sx1);
    const int32_t y0 = max((minY + 127) >> 8, cmd.sy0), y1 = min(((maxY - 128) >> 8) + 1, cmd.sy1);
    if (x0 < x1 && y0 < y1) b = UiBox{x0, y0, x1, y1};
  }
  boxes[ti] = b;
  if (b.x1 <= b.x0) return;  // its triangle record is never read
  UiTri t;
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    t.X[k] = X[k];
    t.Y[k] = Y[k];
  }
  const double rS = 1.0 / (double)S;
  t.l1dx = (float)((double)dy2 * rS);
  t.l1dy = (float)(-(double)dx2 * rS);
  t.l2dx = (float)(-(double)dy1 * rS);
  t.l2dy = (float)((double)dx1 * rS);
#pragma unroll
  for (int q = 0; q < kUiAttrs; ++q) t.attr[q] = UiAttr{a[0][q], a[1][q] - a[0][q], a[2][q] - a[0][q]};
  t.texels = cmd.texels;
  t.tw = cmd.tw;
  t.th = cmd.th;
  t.bx0 = b.x0; t.by0 = b.y0; t.bx1 = b.x1; t.by1 = b.y1;
  tris[ti] = t;
}

// One fragment over the pixel's bytes: src = colour * texel, SRC_ALPHA / ONE_MINUS_SRC_ALPHA on the decoded bytes, the
// back end's alpha factors, requantised at once.
BB_DEV uint32_t ui_blend(uint32_t px, const float src[4], const float *dec, const SrgbTables &tables) {
  const float sa = src[3];
  const float ia = 1.0f - sa;
  uint32_t out = 0u;
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    const float d = dec[(px >> (8 * k)) & 0xFFu];
    const float di = d * ia;
    out |= srgb8(fmaf(src[k], sa, di), tables) << (8 * k);
  }
  const float oa = sa * ia;
  out |= (uint32_t)rintf(255.0f * clamp01(oa)) << 24;
  return out;
}

__global__ __launch_bounds__(kUiThreads) void k_ui_tiles(const UiTri *__restrict__ tris, const UiBox *__restrict__ boxes,
                                                         uint32_t n_tris, int32_t tile_x0, int32_t tile_y0, int32_t width,
                                                         int32_t height, const float *__restrict__ dec_g,
                                                         const SrgbTables *__restrict__ tables_g, uint32_t *__restrict__ image) {
  __shared__ float s_dec[256];
  __shared__ SrgbTables s_tables;
  __shared__ uint32_t s_list[kUiChunk];
  __shared__ uint32_t s_count[kUiThreads / 64];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  s_dec[tid] = dec_g[tid];
  {
    static_assert(sizeof(SrgbTables) % 4 == 0, "SrgbTables is copied by dwords");
    const uint32_t *src = reinterpret_cast<const uint32_t *>(tables_g);
    uint32_t *dst = reinterpret_cast<uint32_t *>(&s_tables);
    for (int i = tid; i < (int)(sizeof(SrgbTables) / 4); i += kUiThreads) dst[i] = src[i];
  }
  const int ox = (tile_x0 + (int)blockIdx.x) * kUiTile, oy = (tile_y0 + (int)blockIdx.y) * kUiTile;  // the tile's first pixel
  const int x = ox + (tid & 31), y0 = oy + (tid >> 5);
  uint32_t px[kUiPixelsPerThread];
  uint32_t touched = 0u;
#pragma unroll
  for (int k = 0; k < kUiPixelsPerThread; ++k) {
    const int y = y0 + 8 * k;
    px[k] = (x < width && y < height) ? image[(size_t)y * width + x] : 0u;
  }
  __syncthreads();

  // the survivors of s_list[0 .. n) over this thread's pixels, in list order
  auto flush = [&](uint32_t n) {
    for (uint32_t j = 0; j < n; ++j) {
      const uint32_t ti = __builtin_amdgcn_readfirstlane(s_list[j]);  // the same for every lane: the record comes by scalar loads
      const UiTri &t = tris[ti];
      if (x < t.bx0 || x >= t.bx1) continue;
      const int Xc = x * 256 + 128, Yc = y0 * 256 + 128;
      long long E[3];
      long long step[3];
#pragma unroll
      for (int i = 0; i < 3; ++i) {
        const int n1 = i == 2 ? 0 : i + 1;
        const int dx = t.X[n1] - t.X[i], dy = t.Y[n1] - t.Y[i];  // |coordinates| <= 2^23: differences fit 32 bits
        const long long bias = (dy < 0 || (dy == 0 && dx > 0)) ? 0 : -1;  // top-left rule
        E[i] = (long long)dx * (long long)(Yc - t.Y[i]) - (long long)dy * (long long)(Xc - t.X[i]) + bias;
        step[i] = (long long)dx * 2048;  // eight rows down
      }
      const float dxp = (float)(Xc - t.X[0]);
#pragma unroll
      for (int k = 0; k < kUiPixelsPerThread; ++k) {
        const int y = y0 + 8 * k;
        const bool in = (E[0] | E[1] | E[2]) >= 0 && y >= t.by0 && y < t.by1;
#pragma unroll
        for (int i = 0; i < 3; ++i) E[i] += step[i];
        if (!in) continue;
        const float dyp = (float)(y * 256 + 128 - t.Y[0]);
        const float l1 = fmaf(t.l1dx, dxp, t.l1dy * dyp);
        const float l2 = fmaf(t.l2dx, dxp, t.l2dy * dyp);
        float a[kUiAttrs];
#pragma unroll
        for (int q = 0; q < kUiAttrs; ++q) a[q] = fmaf(l2, t.attr[q].d2, fmaf(l1, t.attr[q].d1, t.attr[q].a0));
        const BilinearTaps tp = bilinear_taps(a[kUiU], a[kUiV], t.tw, t.th);
        const uint32_t t00 = t.texels[tp.o00], t10 = t.texels[tp.o10], t01 = t.texels[tp.o01], t11 = t.texels[tp.o11];
        float src[4];
#pragma unroll
        for (int ch = 0; ch < 4; ++ch) src[ch] = a[kUiR + ch] * filter_channel(t00, t10, t01, t11, 8 * ch, tp.fx, tp.fy);
        px[k] = ui_blend(px[k], src, s_dec, s_tables);
        touched |= 1u << k;
      }
    }
  };

  const int tx1 = ox + kUiTile, ty1 = oy + kUiTile;
  uint32_t list_n = 0;
  for (uint32_t base = 0; base < n_tris; base += kUiThreads) {
    const uint32_t i = base + (uint32_t)tid;
    bool hit = false;
    if (i < n_tris) {
      const UiBox b = boxes[i];
      hit = b.x0 < b.x1 && b.x0 < tx1 && b.x1 > ox && b.y0 < ty1 && b.y1 > oy;
    }
    const unsigned long long m = __ballot(hit);
    if (lane == 0) s_count[wave] = (uint32_t)__popcll(m);
    __syncthreads();
    uint32_t before = 0, total = 0;
#pragma unroll
    for (int w = 0; w < kUiThreads / 64; ++w) {
      const uint32_t c = s_count[w];
      before += w < wave ? c : 0u;
      total += c;
    }
    if (list_n + total > (uint32_t)kUiChunk) {  // (uniform) the chunk is full: blend it before the list is reused
      flush(list_n);
      list_n = 0;
      __syncthreads();
    }
    if (hit) s_list[list_n + before + (uint32_t)__popcll(m & ((1ull << lane) - 1ull))] = i;
    list_n += total;
    __syncthreads();
  }
  if (list_n == 0 && touched == 0u) return;  // no survivor: the image is not touched
  flush(list_n);
#pragma unroll
  for (int k = 0; k < kUiPixelsPerThread; ++k)
    if (touched & (1u << k)) image[(size_t)(y0 + 8 * k) * width + x] = px[k];
}

}  // namespace bbr
