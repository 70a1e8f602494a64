// bb_kernels.hip.h -- HIP kernels of the forward PBR path for gfx950 (MI355X / CDNA4).
//
//   k_geometry   forward_brdf.vert + clip/cull/viewport/snap + triangle setup + tile binning
//                (reference: src/shaders/forward_brdf.vert:24-37; state src/render.cpp:1069-1125)
//   k_raster     per screen tile: LDS-resident 64-bit visibility keys (depth | primitive) filled with
//                ds_max_u64, ballot/popcount compaction of the covered pixels into the tile's fragment list
//   k_shade_items  the frame's shading work list: one item per 64 fragments of a tile's list (scan of the per-tile counts);
//                also cooks the frame's light table
//   k_shade      forward_brdf.frag + brdf.glsl once per visible pixel (src/shaders/forward_brdf.frag:15-76,
//                brdf.glsl:2-36): one wave per item; a TAIL instantiation loops over what the main launch's estimate missed
//   (in front of k_shade, "what the fragment kernels share": barycentrics, item decode, fragment fetch, late clip slot, counter
//                hand-over, normal, one map tap, deferred tail and final store, each stated once for k_shade, k_shade_aniso
//                and k_shade_overlay)
//   k_present, k_tone_map, k_deferred_background, k_shade_overlay, k_pack_shard / k_unpack_*: the rows either side of the path
//   k_tbn_segments, k_tbn_raster, k_tbn_colour: the TBN line overlay (option "tbn"; tbn.vert / tbn.geom)
//   k_resolve    option "supersample": the n x n samples of the fine frame averaged into the output pixel, in a pinned order
//   k_sample_merge, k_resolve_merged    option "sample_shading" 0: the fragment lists thinned to one fragment per primitive and
//                output pixel behind k_raster, and the resolve that knows which sample stands for which
//   k_resolve_depth    option "depth_resolve": the depth (and winner) of one sample of the block for the output pixel
//   k_bloom_first, k_bloom_down, k_bloom_up, k_present_bloom    option "bloom": a pyramid of what passes a threshold, added to
//                the pixel in front of present_pixel (behind k_resolve, whose shape they share)
//   k_luminance, k_exposure, k_present_auto, k_present_bloom_auto    option "auto_exposure": a histogram of the frame's log2
//                luminance, the exposure it asks for adapted against a history, and the two present kernels reading it
//   k_shade_shadow     option "shadow_map": k_shade_aniso's fragment stage with a shadow test in front of one light's iteration
//   k_shade_shadow_faces    ... with 2 .. 6 faces for that light (bbr_render_shadow_faces): cube maps, cascades
//   k_shade_shadow_pcf      option "shadow_filter" 1 .. 2: ... with a 3 x 3 or 5 x 5 box of compares, 1 .. 6 faces
//   k_shade_shadow_casters  bbr_render_shadow_caster: ... with up to eight casters, each in front of its own light's iteration
//
// Arithmetic contract: every floating-point expression below has the same operand order and the same
// explicit fmaf() placement as the CPU oracle; the file is compiled with -ffp-contract=off, IEEE
// division and sqrt (hipcc default), denormals on.  Integer coverage is exact (24.8 fixed point,
// 64-bit edge functions, top-left rule).
#pragma once

#include <hip/hip_runtime.h>

#include "bb_types.h"

namespace bbr {

#define BB_DEV __device__ __forceinline__

// Diagnostic ablations (skip parts of the pipeline to see what they cost) exist only in -DBB_ABLATE builds; in the
// shipped library the tests fold to constants.
#ifdef BB_ABLATE
#define BB_ABLATE(bits) ((fp.ablate & (bits)) != 0u)
#else
#define BB_ABLATE(bits) false
#endif

constexpr float kGuardBand = 32.0f;
constexpr float kPi = 3.14159265358979323846f;
constexpr float kInvPi = 0.31830988618379067154f;

struct f3 {
  float x, y, z;
};
struct f4 {
  float x, y, z, w;
};

BB_DEV f3 mk3(float x, float y, float z) { return f3{x, y, z}; }
BB_DEV f3 ld3(const float *p) { return f3{p[0], p[1], p[2]}; }
BB_DEV float dot3(f3 a, f3 b) { return fmaf(a.z, b.z, fmaf(a.y, b.y, a.x * b.x)); }
BB_DEV f3 add3(f3 a, f3 b) { return f3{a.x + b.x, a.y + b.y, a.z + b.z}; }
BB_DEV f3 sub3(f3 a, f3 b) { return f3{a.x - b.x, a.y - b.y, a.z - b.z}; }
BB_DEV f3 scale3(f3 a, float s) { return f3{a.x * s, a.y * s, a.z * s}; }
BB_DEV f3 neg3(f3 a) { return f3{-a.x, -a.y, -a.z}; }
BB_DEV f3 cross3(f3 a, f3 b) {
  return f3{fmaf(a.y, b.z, -(a.z * b.y)), fmaf(a.z, b.x, -(a.x * b.z)), fmaf(a.x, b.y, -(a.y * b.x))};
}
// GLSL inversesqrt as a fixed sequence (integer seed + three Newton steps, max error 1.1 ulp): the same bits as the
// oracle's bb_rsqrt, at a third of the instruction count of IEEE sqrt + divide.
// The IEEE paths behind the guards are real function calls: taken for zero, denormal, infinite and NaN arguments only,
// they would otherwise be expanded inline (a 12-instruction division, a 25-instruction square root) at each of the
// shader's 25 call sites -- a tenth of k_shade's code.
BB_DEV float bb_rsqrt_slow(float x) { return 1.0f / sqrtf(x); }
BB_DEV float bb_rcp_slow(float x) { return 1.0f / x; }
// The guards are WAVE-level: the fast sequence runs unconditionally and a uniform, almost never taken branch repairs
// the lanes whose argument was not a normal number.  (As a per-lane if/else the compiler wrapped every call site in an
// exec-mask save / restore -- five scalar instructions and a branch around each of the shader's sixteen guards per
// pixel, a tenth of a wave's issue slots.)
BB_DEV float bb_rsqrt(float x) {
  float y = __uint_as_float(0x5F375A86u - (__float_as_uint(x) >> 1));
  const float h = 0.5f * x;
  y = y * fmaf(-(h * y), y, 1.5f);
  y = y * fmaf(-(h * y), y, 1.5f);
  y = y * fmaf(-(h * y), y, 1.5f);
  const bool odd = !__builtin_amdgcn_classf(x, 0x100);  // anything but a positive normal number (one v_cmp_class)
  if (__builtin_expect(__ballot(odd) != 0ull, 0)) {
    if (odd) y = bb_rsqrt_slow(x);
  }
  return y;
}
// Reciprocal: the correctly rounded 1/x, i.e. what the oracle computes with an IEEE division.  v_rcp_f32 (1 ulp) plus
// ONE Newton step lands on the correctly rounded value for every one of the 2 113 929 216 normal inputs whose
// reciprocal is normal (k_selftest_rcp below checks all of them against the IEEE division in 0.3 s; so does
// tools/microbench/exact_rcp.hip) -- the result does not depend on which 1-ulp seed the hardware returns.  The same
// idea does not work for 1/sqrt (13 % of the inputs end up off by an ulp), so bb_rsqrt keeps its integer seed.
BB_DEV float bb_rcp(float x) {
  const float y0 = __builtin_amdgcn_rcpf(x);
  float y = fmaf(y0, fmaf(-x, y0, 1.0f), y0);
  // a seed that is not a normal number (x zero, denormal, huge, infinite or NaN): the IEEE division.  One v_cmp_class
  // on the seed replaces two range compares on x.
  const bool odd = !__builtin_amdgcn_classf(y0, 0x108);
  if (__builtin_expect(__ballot(odd) != 0ull, 0)) {
    if (odd) y = bb_rcp_slow(x);
  }
  return y;
}
// bb_rcp for a call site that can PROVE its argument is a normal number with a normal reciprocal (the guard and its
// branch are a twentieth of k_shade's instruction stream).  Each use states its proof; k_selftest_rcp checks the
// whole range [2^-100, 2^100] against the IEEE division.
BB_DEV float bb_rcp_normal(float x) {
  const float y = __builtin_amdgcn_rcpf(x);
  return fmaf(y, fmaf(-x, y, 1.0f), y);
}
// nearest binary16 value (ties to even), as binary32: v_cvt_f16_f32 / v_cvt_f32_f16 do exactly this on gfx950
// (round-to-nearest-even, binary16 subnormals kept -- the default float mode of HIP kernels; every binary16
// midpoint +-3 ulp is checked against the oracle's integer formulation in tests/test_gpu_parity.py)
// The empty asm pins the binary32 value: without it the compiler folds a producing fma and the conversion into one
// v_fma_mix*_f16, which rounds the exact fma result ONCE to binary16 -- different from rounding the binary32 result
// (what an attachment write does) exactly when that result sits on a binary16 tie.
BB_DEV float bb_half_round(float x) {
  asm("" : "+v"(x));
  return (float)(_Float16)x;
}

BB_DEV float bb_exp(float x) {
  if (!(x >= -104.0f)) return x < -104.0f ? 0.0f : x;
  if (x > 88.7228317f) return __uint_as_float(0x7F800000u);
  const float n = __builtin_rintf(x * 1.44269502f);
  float r = fmaf(n, -0.693145752f, x);
  r = fmaf(n, -1.42860677e-06f, r);
  float p = 1.98412701e-04f;
  p = fmaf(p, r, 1.38888892e-03f);
  p = fmaf(p, r, 8.33333377e-03f);
  p = fmaf(p, r, 4.16666679e-02f);
  p = fmaf(p, r, 1.66666672e-01f);
  p = fmaf(p, r, 0.5f);
  p = fmaf(p, r, 1.0f);
  p = fmaf(p, r, 1.0f);
  const int ni = (int)n, h = ni / 2;
  const float s1 = __uint_as_float((uint32_t)(h + 127) << 23), s2 = __uint_as_float((uint32_t)(ni - h + 127) << 23);
  return (p * s1) * s2;
}

// sRGB byte = number of thresholds t_k <= c (NaN -> 0).  Instead of a binary search (eight dependent LDS probes)
// the byte is read from a table keyed by the top 16 bits of the float: 256 cells per octave over the 13 octaves
// [2^-13, 1) that contain all thresholds.  A cell is narrower than the closest pair of thresholds (0.39 % against
// >= 0.88 %; checked when the table is built), so it holds the count at its lower edge and at most one more
// threshold, which one compare settles: two LDS reads, same bytes as the search for every float.
constexpr uint32_t kSrgbLutFirstExp = 114u;             // 2^-13
constexpr uint32_t kSrgbLutCells = 13u * 256u;          // biased exponents 114..126
struct SrgbTables {                                      // device copy built by the host
  float thr[256];                                        // t_1..t_255, then +inf
  uint8_t lut[kSrgbLutCells];                            // thresholds <= lower edge of the cell
};

BB_DEV uint32_t srgb8(float c, const SrgbTables &t) {
  const uint32_t u = __float_as_uint(c);
  if ((int32_t)u < (int32_t)(kSrgbLutFirstExp << 23)) return 0u;  // below 2^-13, zero, negative, negative NaN
  if (u >= (127u << 23)) return u <= 0x7F800000u ? 255u : 0u;     // >= 1 (and +inf) -> 255, NaN -> 0
  const uint32_t k = t.lut[(u >> 15) - (kSrgbLutFirstExp << 8)];
  return k + (t.thr[k] <= c ? 1u : 0u);
}

// One presented pixel (hdr_tone_mapping.frag:9-18 + the sRGB UNORM8 attachment write): binary16 HDR value, tone map,
// sRGB byte per channel, alpha 255.  Shared by k_present and the fused output of k_shade / k_raster.
BB_DEV uint32_t present_pixel(float r, float g, float b, const SrgbTables &t, int enable, float exposure, int hdr16) {
  float v[3] = {r, g, b};
  uint32_t px = 0xFF000000u;  // outColor.a = 1.0
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    float x = v[k];
    if (hdr16) x = bb_half_round(x);
    if (enable) x = 1.0f - bb_exp(-x * exposure);
    px |= srgb8(x, t) << (8 * k);
  }
  return px;
}

BB_DEV f3 normalize3(f3 a) { return scale3(a, bb_rsqrt(dot3(a, a))); }
// max(a, 0) with the oracle's `a > 0 ? a : 0` semantics: NaN -> +0, -0 -> +0.  v_max_f32 does exactly that (IEEE
// maxNum with -0 < +0; k_selftest_rcp checks every bit pattern), and costs one instruction where the compiler, which
// may not assume the -0 case, emits a compare and a select.
BB_DEV float max0(float a) { return __builtin_fmaxf(a, 0.0f); }
// saturate: clamp to [0, 1], NaN -> +0 (the `clamp` output modifier of the producing instruction under DX10_CLAMP, the
// float mode HIP kernels run in: no instruction of its own, where v_max_f32 is a half-rate one that also breaks the
// 2-cycle issue cadence of the fma / mul stream around it -- profiles/r02_issue_rate.txt)
BB_DEV float sat01(float a) { return __builtin_amdgcn_fmed3f(a, 0.0f, 1.0f); }

// 32-bit integer multiply that stays v_mul_lo_u32.  The 24-bit forms the compiler prefers for small operands (v_mul_u32_u24,
// v_mad_i32_i24, ...) cost ~10 issue cycles each on gfx950 where v_mul_lo_u32 costs 3.5 (profiles/r02_issue_rate.txt, rows
// iso_*): the empty asm hides the operand's known-zero bits from the instruction selector.
BB_DEV int mul32(int a, int b) {
  asm("" : "+v"(a));
  return a * b;
}

// A pixel of the frame is written once and never read again by these kernels: a NON-TEMPORAL store (global_store ... nt).
// 133 MB of pixels per 4K frame otherwise stream through the L2s as ordinary dirty lines and push out what the shading
// does re-read -- texels and primitive records: with nt the pipelined C3 frame went 122.2 -> 110.6 us, C2 26.5 -> 24.9
// (plain / nt / sc1: 122.2 / 110.6 / 120.0 us; sc1 drops the line from the L2 once written back, nt marks it
// first-to-go from the start).
typedef float v4f __attribute__((ext_vector_type(4)));
BB_DEV void store_pixel(float4 *p, float4 v) {
  const v4f q = {v.x, v.y, v.z, v.w};
  __builtin_nontemporal_store(q, reinterpret_cast<v4f *>(p));  // one global_store_dwordx4 ... nt
}
BB_DEV void store_pixel(uint32_t *p, uint32_t v) { __builtin_nontemporal_store(v, p); }
// (The intermediates that are written once and read once -- fragment words, RasterTri records -- stay ordinary accesses:
//  non-temporal they made the frame 2 % slower, 112.1 -> 114.8 / 113.8 us: their one reader does find them in the L2.)

template <typename M4>  // (Mat4 in any address space)
BB_DEV f4 mat4_mul(const M4 &m, f4 v) {
  f4 r;
  r.x = fmaf(m.M[3][0], v.w, fmaf(m.M[2][0], v.z, fmaf(m.M[1][0], v.y, m.M[0][0] * v.x)));
  r.y = fmaf(m.M[3][1], v.w, fmaf(m.M[2][1], v.z, fmaf(m.M[1][1], v.y, m.M[0][1] * v.x)));
  r.z = fmaf(m.M[3][2], v.w, fmaf(m.M[2][2], v.z, fmaf(m.M[1][2], v.y, m.M[0][2] * v.x)));
  r.w = fmaf(m.M[3][3], v.w, fmaf(m.M[2][3], v.z, fmaf(m.M[1][3], v.y, m.M[0][3] * v.x)));
  return r;
}

// The nine words coverage and depth need of a triangle: the first 36 bytes of a RasterTri (bb_types.h) and of an
// every-tile-list entry, a column of k_raster's StagedTri.  Vertices in 24.8 fixed point, the depth plane relative to vertex 0.
struct TriCore {
  int X0, Y0, X1, Y1, X2, Y2;
  float z0, dzdx, dzdy;
};
BB_DEV TriCore tri_core(const RasterTri &t) { return TriCore{t.X0, t.Y0, t.X1, t.Y1, t.X2, t.Y2, t.z0, t.dzdx, t.dzdy}; }
// Pixels [x0, x1] x [y0, y1], both ends included: a tile, the frame, the gizmo's scissor, a triangle's box; and what two share.
struct PixRect {
  int x0, x1, y0, y1;
  BB_DEV bool any() const { return x0 <= x1 && y0 <= y1; }
};
BB_DEV PixRect intersect(const PixRect &a, const PixRect &b) { return PixRect{max(a.x0, b.x0), min(a.x1, b.x1), max(a.y0, b.y0), min(a.y1, b.y1)}; }
// the larger side of a triangle's bounding box, in 1/256 pixel
BB_DEV int tri_span(const TriCore &t) { return max(max(t.X0, max(t.X1, t.X2)) - min(t.X0, min(t.X1, t.X2)), max(t.Y0, max(t.Y1, t.Y2)) - min(t.Y0, min(t.Y1, t.Y2))); }
// The pixels whose CENTRES lie inside a triangle's bounding box and inside rectangles `a` and `b`, clamped in this order.
BB_DEV PixRect pixel_box(const TriCore &t, const PixRect &a, const PixRect &b) {
  const int32_t minX = min(t.X0, min(t.X1, t.X2)), maxX = max(t.X0, max(t.X1, t.X2));
  const int32_t minY = min(t.Y0, min(t.Y1, t.Y2)), maxY = max(t.Y0, max(t.Y1, t.Y2));
  return PixRect{max(max((minX - 128 + 255) >> 8, a.x0), b.x0), min(min((maxX - 128) >> 8, a.x1), b.x1),
                 max(max((minY - 128 + 255) >> 8, a.y0), b.y0), min(min((maxY - 128) >> 8, a.y1), b.y1)};
}
BB_DEV PixRect pixel_box(const TriCore &t, const PixRect &r) { return pixel_box(t, r, r); }

// ------------------------------------------------------------------------------------------------
// geometry: vertex stage, clip, setup, binning
// ------------------------------------------------------------------------------------------------

struct ClipVert {
  float c[4];
  float b[3];
};

BB_DEV float plane_dist(const float *c, int plane) {
  switch (plane) {
    case 0: return c[3] - c[2];  // near (reverse-Z: z <= w)
    case 1: return c[2];         // far
    case 2: return fmaf(kGuardBand, c[3], c[0]);
    case 3: return fmaf(kGuardBand, c[3], -c[0]);
    case 4: return fmaf(kGuardBand, c[3], c[1]);
    default: return fmaf(kGuardBand, c[3], -c[1]);
  }
}

BB_DEV void clip_lerp(const ClipVert &in, float din, const ClipVert &out, float dout, ClipVert &r) {
  float t = din / (din - dout);
  for (int k = 0; k < 4; ++k) r.c[k] = fmaf(t, out.c[k] - in.c[k], in.c[k]);
  for (int k = 0; k < 3; ++k) r.b[k] = fmaf(t, out.b[k] - in.b[k], in.b[k]);
}

constexpr int kMaxClipVerts = 12;

// Per-wave LDS workspace of the polygon clipper.  The clipper indexes its vertex arrays dynamically; in
// registers that would spill to scratch (and a kernel that owns scratch pays for it on every launch), in LDS
// it is a plain ds_read/ds_write.  Clipped primitives are rare; the wave clips them one after the other,
// all lanes working on the same polygon.
struct ClipWork {
  ClipVert poly[2][kMaxClipVerts];  // ping-pong
  int32_t X[kMaxClipVerts], Y[kMaxClipVerts];
  float rw[kMaxClipVerts], z[kMaxClipVerts];
  uint32_t prim, base;  // primitive being clipped, its first clip-arena slot
  int32_t n_slots;      // fan triangles of the clipped polygon (0: nothing survived)
  int32_t n_valid;      // of which front-facing and covering a pixel centre
};

// Wave-parallel Sutherland-Hodgman against near, far and the four guard-band planes: lane i owns edge
// (v_i, v_i+1), emits 0, 1 or 2 vertices, and a ballot/popcount prefix gives every lane its output position -- the
// same vertices in the same order as the serial algorithm, in six steps instead of six loops over the polygon.
// The input polygon (n vertices) is in w.poly[0]; returns the buffer index holding the result and its size.
BB_DEV int clip_polygon_wave(ClipWork &w, int &n) {
  const int lane = threadIdx.x & 63;
  int cur = 0;
  for (int plane = 0; plane < 6; ++plane) {
    bool ina = false, cross = false;
    ClipVert a, b;
    float da = 0.0f, db = 0.0f;
    if (lane < n) {
      a = w.poly[cur][lane];
      b = w.poly[cur][lane + 1 == n ? 0 : lane + 1];
      da = plane_dist(a.c, plane);
      db = plane_dist(b.c, plane);
      ina = da >= 0.0f;
      cross = ina != (db >= 0.0f);
    }
    const unsigned long long ma = __ballot(ina), mx = __ballot(cross);
    const unsigned long long lt = (1ull << lane) - 1ull;
    int pos = (int)__popcll(ma & lt) + (int)__popcll(mx & lt);
    __builtin_amdgcn_wave_barrier();
    if (ina) w.poly[cur ^ 1][pos++] = a;
    if (cross) {
      ClipVert r;
      if (ina) clip_lerp(a, da, b, db, r);
      else clip_lerp(b, db, a, da, r);
      w.poly[cur ^ 1][pos] = r;
    }
    __builtin_amdgcn_wave_barrier();
    n = (int)__popcll(ma) + (int)__popcll(mx);
    cur ^= 1;
    if (n < 3) {
      n = 0;
      break;
    }
  }
  return cur;
}

// viewport transform: half extents and centre in pixels (the main passes cover the whole target: centre = half extent)
struct Viewport {
  float half_w, half_h, cx, cy;
};

BB_DEV bool project_vertex(const float *c, const Viewport &vp, int32_t &X, int32_t &Y, float &rw, float &zndc) {
  float w = c[3];
  if (!(w > 0.0f)) return false;
  float r = 1.0f / w;
  float xs = fmaf(c[0] * r, vp.half_w, vp.cx);
  float ys = fmaf(c[1] * r, vp.half_h, vp.cy);
  if (!(fabsf(xs) <= 4194304.0f) || !(fabsf(ys) <= 4194304.0f)) return false;
  X = (int32_t)rintf(xs * 256.0f);
  Y = (int32_t)rintf(ys * 256.0f);
  rw = r;
  zndc = c[2] * r;
  return true;
}

// cull + plane setup (binary64, rounded once -- same expressions as the oracle's setup_tri)
BB_DEV bool setup_tri(RasterTri &t, float z0, float z1, float z2) {
  long long dx1 = (long long)t.X1 - t.X0, dy1 = (long long)t.Y1 - t.Y0;
  long long dx2 = (long long)t.X2 - t.X0, dy2 = (long long)t.Y2 - t.Y0;
  long long S = dx1 * dy2 - dx2 * dy1;
  if (S <= 0) return false;
  double rS = 1.0 / (double)S;
  t.l1dx = (float)((double)dy2 * rS);
  t.l1dy = (float)(-(double)dx2 * rS);
  t.l2dx = (float)(-(double)dy1 * rS);
  t.l2dy = (float)((double)dx1 * rS);
  double dz1 = (double)z1 - (double)z0, dz2 = (double)z2 - (double)z0;
  t.z0 = z0;
  t.dzdx = (float)((dz1 * (double)dy2 - dz2 * (double)dy1) * rS);
  t.dzdy = (float)((dz2 * (double)dx1 - dz1 * (double)dx2) * rS);
  return true;
}

// ---- tiles and bins ----

struct TileRange {
  int tx0, tx1, ty0, ty1;
};

// The geometry stage's one box: the pixels whose CENTRES lie inside a triangle's bounding box and inside the frame.
// tile_range and raster_class read it, for a survivor and for a fan triangle of the clipper.  (pixel_box with the frame's
// rectangle is the same box; stated through it k_geometry came out one instruction longer: profiles/r11_geometry_stage.txt.)
BB_DEV PixRect frame_box(const RasterTri &t, const FrameParams &fp) {
  const int32_t minX = min(t.X0, min(t.X1, t.X2)), maxX = max(t.X0, max(t.X1, t.X2));
  const int32_t minY = min(t.Y0, min(t.Y1, t.Y2)), maxY = max(t.Y0, max(t.Y1, t.Y2));
  return PixRect{max((minX - 128 + 255) >> 8, 0), min((maxX - 128) >> 8, fp.width - 1), max((minY - 128 + 255) >> 8, 0), min((maxY - 128) >> 8, fp.height - 1)};
}

// box of pixel centres -> tile range; false if the box holds no pixel centre
template <int TILE_W, int TILE_H>
BB_DEV bool tile_range(const PixRect &box, TileRange &r) {
  if (!box.any()) return false;
  r.tx0 = box.x0 / TILE_W; r.tx1 = box.x1 / TILE_W; r.ty0 = box.y0 / TILE_H; r.ty1 = box.y1 / TILE_H;
  return true;
}

// Raster classes: how many lanes of k_raster work on one triangle.  Decided once per triangle from its
// full pixel bounding box, so that every loop of the raster kernel runs over triangles of similar cost.
//   0: tiny  (box <= 64 px, spans <= 32 px)      one triangle per lane, 32-bit stepped edge functions
//   1: small (spans <= 64 px)                    16 lanes per triangle, 4x4 pixel blocks, 24-bit multiply-adds
//   2: large                                     one wave per triangle, 8x8 blocks, trivial accept / reject
// box: the frame-clamped box of pixel centres; span: tri_span, the unclamped extent in 1/256 pixel
constexpr uint32_t kBinClasses = 3;

BB_DEV uint32_t raster_class(const PixRect &box, int span) {
  const int area = (box.x1 - box.x0 + 1) * (box.y1 - box.y0 + 1);
  if (span <= 32 * 256 && area <= 64) return 0u;
  if (span <= 64 * 256) return 1u;
  return 2u;
}

BB_DEV void broad_insert(const RasterTri &t, uint32_t ref, const FrameParams &fp, Counters *ctr, BroadTri *broad_list) {
  uint32_t slot = atomicAdd(&ctr->n_broad, 1u);
  if (slot < fp.broad_cap) {
    BroadTri b;
    b.tri = t;
    b.ref = ref;
    b.pad[0] = b.pad[1] = b.pad[2] = 0;
    broad_list[slot] = b;
  } else {
    atomicOr(&ctr->overflow, 2u);
  }
}

// ---- screen-band partition (fp.world > 1): tile rows in bands of fp.band_tiles, band b belongs to rank b mod world ----
BB_DEV int band_of_row(const FrameParams &fp, int ty) { return ty / fp.band_tiles; }
// tile row ty is this rank's (every row of an unpartitioned frame is)
BB_DEV bool row_owned(const FrameParams &fp, int ty) { return fp.world <= 1 || band_of_row(fp, ty) % fp.world == fp.rank; }
// tile rows [ty0, ty1] hold a row of this rank's: the first owned band at or behind ty0's is not behind ty1's
BB_DEV bool rows_owned(const FrameParams &fp, int ty0, int ty1) {
  if (fp.world <= 1) return true;
  const int b0 = band_of_row(fp, ty0), b1 = band_of_row(fp, ty1);
  const int first = b0 + ((fp.rank - b0 % fp.world) + fp.world) % fp.world;
  return first <= b1;
}
// owned tile row -> row of this rank's launch grid: the inverse of tile_row (k_raster)
BB_DEV uint32_t grid_row(const FrameParams &fp, uint32_t ty) {
  if (fp.world <= 1) return ty;
  const uint32_t band = ty / (uint32_t)fp.band_tiles;
  return (band / (uint32_t)fp.world) * (uint32_t)fp.band_tiles + (ty - band * (uint32_t)fp.band_tiles);
}

// Wave grouping: the lanes with `has` that name the same key form a group (ballot loop, ALU only); every member learns the
// group's lowest lane, its own rank among the members and the group's size.  Must be called by all lanes of the wave.
struct WaveGroup {
  int leader;
  uint32_t rank, size;
};
BB_DEV WaveGroup wave_group(bool has, uint32_t key) {
  const int lane = threadIdx.x & 63;
  unsigned long long pending = __ballot(has);
  WaveGroup g = {lane, 0u, 0u};
  while (pending) {
    int l = __builtin_amdgcn_readfirstlane(__ffsll((long long)pending) - 1);
    uint32_t lk = (uint32_t)__builtin_amdgcn_readlane((int)key, l);
    bool mine = has && key == lk;
    unsigned long long m = __ballot(mine);
    if (mine) {
      g.leader = l;
      g.rank = (uint32_t)__popcll(m & ((1ull << lane) - 1ull));
      g.size = (uint32_t)__popcll(m);
    }
    pending &= ~m;
  }
  return g;
}

// Wave-aggregated bin insertion.  Consecutive primitives of a mesh land in the same few tiles, so the lanes of
// a wave that target one bin segment are grouped (wave_group) and the lowest lane of each group
// reserves all the group's slots with ONE returning atomic; the leaders of all groups issue their atomics in the
// same instruction, so a wave pays one memory round trip however many tiles it touches, and a tile that
// receives thousands of tiny triangles sees tens of atomics instead of thousands.
// Must be called by all lanes of the wave (has = false for lanes with nothing to insert).
// The reservation is split from the write so that a caller with several insertions per lane can issue all their
// atomics before waiting for the first result (one memory round trip for the batch instead of one per insertion).
struct BinTicket {
  uint32_t base;   // valid in the group's leader lane until redeemed
  uint32_t rank;
  uint32_t gsize;  // slots the leader reserved (leader lane only)
  int leader;
};

BB_DEV BinTicket wave_bin_reserve(bool has, uint32_t seg, uint32_t *tile_count) {
  const WaveGroup g = wave_group(has, seg);
  BinTicket t = {0u, g.rank, g.size, g.leader};
  if (has && (int)(threadIdx.x & 63) == g.leader) t.base = atomicAdd(&tile_count[seg], g.size);
  return t;
}
// redeem: this lane's slot in the bin (waits for the leader's atomic)
BB_DEV uint32_t bin_slot(const BinTicket &t) { return (uint32_t)__shfl((int)t.base, t.leader) + t.rank; }

// heavy: the frame's heavy-tile list (fp.heavy_threshold != 0).  The ONE reservation that takes a bin's count across the
// threshold appends the tile -- as the launch slot k_raster's screen order gives it, and the class of the bin -- so a tile
// is listed at most once per class, and which of its entries does the work follows from the final counts (k_raster).
BB_DEV void wave_bin_write(bool has, uint32_t seg, uint32_t ref, const BinTicket &t, const FrameParams &fp, Counters *ctr,
                           uint32_t *bins, uint32_t *heavy) {
  const uint32_t slot = bin_slot(t);
  if (heavy && has && (int)(threadIdx.x & 63) == t.leader && t.base < fp.heavy_threshold && t.base + t.gsize >= fp.heavy_threshold) {
    const uint32_t tile = seg / kBinClasses, c = seg - tile * kBinClasses;
    const uint32_t ty = tile / (uint32_t)fp.tiles_x, tx = tile - ty * (uint32_t)fp.tiles_x;
    const uint32_t k = atomicAdd(&ctr->n_heavy, 1u);
    if (k < kBinClasses * (uint32_t)(fp.tiles_x * fp.tiles_y)) heavy[k] = (grid_row(fp, ty) * (uint32_t)fp.tiles_x + tx) | (c << 30);
  }
  if (has) {
    if (slot < fp.bin_cap) {
      bins[(size_t)seg * fp.bin_cap + slot] = ref;
    } else {
      atomicOr(&ctr->overflow, 1u);
      atomicMax(&ctr->bin_need, slot + 1u);
    }
  }
}

// Rare path: the primitive of lane `owner` crosses a clip plane.  The whole wave works on it: parallel polygon
// clip, lane i projects vertex i and then sets up fan triangle i (binary64 planes), stores its ClipSlot and its
// entry of the every-tile list -- a clipped primitive is typically huge (the ground plane), so its sub-triangles skip
// the bins.  One atomic reserves the arena slots, one the list entries.  Results in w.n_valid / w.base.
BB_DEV void clip_primitive_wave(ClipWork &w, int owner, const float (*clip)[4], uint32_t prim, const FrameParams &fp,
                                const Viewport &vp, ClipSlot *clip_arena, Counters *ctr, BroadTri *broad_list) {
  const int lane = threadIdx.x & 63;
  if (lane == owner) {
    w.prim = prim;
    w.n_slots = 0;
    w.n_valid = 0;
    w.base = kNotClipped;
    for (int i = 0; i < 3; ++i) {
      ClipVert v;
      for (int k = 0; k < 4; ++k) v.c[k] = clip[i][k];
      v.b[0] = i == 0 ? 1.0f : 0.0f;
      v.b[1] = i == 1 ? 1.0f : 0.0f;
      v.b[2] = i == 2 ? 1.0f : 0.0f;
      w.poly[0][i] = v;
    }
  }
  __builtin_amdgcn_wave_barrier();
  int n = 3;
  const int cur = clip_polygon_wave(w, n);
  if (n < 3) return;
  // projection: lane i -> vertex i
  bool bad = false;
  if (lane < n) {
    const ClipVert v = w.poly[cur][lane];
    int32_t X = 0, Y = 0;
    float rw = 0.0f, z = 0.0f;
    bad = !project_vertex(v.c, vp, X, Y, rw, z);
    w.X[lane] = X; w.Y[lane] = Y; w.rw[lane] = rw; w.z[lane] = z;
  }
  if (__ballot(bad) != 0ull) return;
  const int n_slots = min(n - 2, kMaxSubTris);
  __builtin_amdgcn_wave_barrier();
  // fan triangle i = (v0, v_i, v_i+1): lane i - 1.  The setup needs no reservation, so it runs first and BOTH reservations
  // -- arena slots (lane 0) and every-tile entries (lane 1) -- go out together afterwards: one memory round trip per clipped
  // primitive instead of two (the ground plane's two primitives are k_geometry's critical path at 1080p: in-kernel stamps).
  bool ok = false;
  RasterTri tri = {};
  if (lane < n_slots) {
    const int i = lane + 1;
    tri.X0 = w.X[0]; tri.Y0 = w.Y[0];
    tri.X1 = w.X[i]; tri.Y1 = w.Y[i];
    tri.X2 = w.X[i + 1]; tri.Y2 = w.Y[i + 1];
    tri.rw0 = w.rw[0]; tri.rw1 = w.rw[i]; tri.rw2 = w.rw[i + 1];
    ok = setup_tri(tri, w.z[0], w.z[i], w.z[i + 1]);
    ok = ok && frame_box(tri, fp).any();
  }
  const unsigned long long m = __ballot(ok);
  const int n_valid = (int)__popcll(m);
  uint32_t got = 0;
  if (lane == 0) got = atomicAdd(&ctr->n_clip_slots, (uint32_t)n_slots);
  if (lane == 1 && n_valid) got = atomicAdd(&ctr->n_broad, (uint32_t)n_valid);
  const uint32_t base = (uint32_t)__shfl((int)got, 0), slot = (uint32_t)__shfl((int)got, 1);
  const bool arena_fits = base + (uint32_t)n_slots <= fp.clip_cap;
  const bool list_fits = slot + (uint32_t)n_valid <= fp.broad_cap;
  if (!arena_fits && lane == 0) atomicOr(&ctr->overflow, 4u);
  if (n_valid && !list_fits && lane == 0) atomicOr(&ctr->overflow, 2u);
  const bool listed = n_valid != 0 && list_fits;  // (an overflowed list: the frame takes none of its entries, k_raster)
  if (listed && ok) {
    // the run of entries is reserved and fits, so every one of them is written: a real entry, or -- when the arena had
    // no room for the sub-triangles, and the frame is rendered again anyway -- an entry no tile can touch (all zero)
    BroadTri *const entry = broad_list + (slot + (uint32_t)__popcll(m & ((1ull << lane) - 1ull)));
    if (arena_fits) {
      BroadTri b;
      b.tri = tri;
      b.ref = (w.prim << 3) | (uint32_t)lane;  // the OWNER's primitive (prim is per lane)
      b.pad[0] = base + (uint32_t)lane + 1u;     // its clip-arena slot + 1: travels into the fragment word (k_raster)
      b.pad[1] = b.pad[2] = 0;
      *entry = b;
    } else {
      *entry = BroadTri{};
    }
  }
  if (arena_fits && lane < n_slots) {
    // (The slot is put together here -- behind the reservation and behind the list entry, when only the planes of the triangle
    //  are still needed -- from the triangle and the polygon in LDS: built next to the binary64 setup, its twenty values were
    //  this kernel's register peak.)
    const int i = lane + 1;
    ClipSlot s;
    for (int c = 0; c < 3; ++c) {
      s.bary[0][c] = w.poly[cur][0].b[c];
      s.bary[1][c] = w.poly[cur][i].b[c];
      s.bary[2][c] = w.poly[cur][i + 1].b[c];
    }
    s.pad = 0;
    s.valid = ok ? 1u : 0u;
    s.h = PlaneHead{tri.X0, tri.Y0, tri.l1dx, tri.l1dy, tri.l2dx, tri.l2dy, tri.rw0, tri.rw1, tri.rw2};
    clip_arena[base + (uint32_t)lane] = s;
  }
  if (lane == owner && arena_fits) {
    w.base = base;
    w.n_slots = n_slots;
    if (listed) w.n_valid = n_valid;
  }
}

// ---- a primitive's inputs, as k_geometry and k_tbn_segments find them ----
// (global, not flat, loads: through pointers the compiler knows to be global memory)
typedef const Vertex __attribute__((address_space(1))) *GlobalVertex;
typedef const uint32_t __attribute__((address_space(1))) *GlobalIndex;
typedef const InstanceBlock __attribute__((address_space(1))) *GlobalInstance;

// which draw, from the table alone, starting at draw d
BB_DEV uint32_t find_draw(const DrawDesc *__restrict__ draws, uint32_t n_draws, uint32_t prim, uint32_t d = 0) {
  while (d + 1 < n_draws && prim >= draws[d + 1].first_prim) ++d;
  return d;
}
// which draw: the first few draws' first_prim are kernel arguments (no load); more draws than that: the table
BB_DEV uint32_t find_draw(const DrawDesc *__restrict__ draws, uint32_t n_draws, const FirstPrims &first_prims, uint32_t prim) {
  uint32_t d = 0;
#pragma unroll
  for (int q = 0; q < kInlineFirstPrims; ++q) d += prim >= first_prims.v[q] ? 1u : 0u;
  if (n_draws > (uint32_t)kInlineFirstPrims + 1u) d = find_draw(draws, n_draws, prim, d);
  return d;
}

// Where a primitive's three vertices and its instance block are.  (One shape of loads for indexed and non-indexed meshes --
// three 44-byte vertices at three indices: left as an if / else of two copies into the same array the compiler merged them
// into flat dword loads with selected addresses.)
struct PrimSource {
  GlobalVertex v[3];
  GlobalInstance ib;
};

BB_DEV PrimSource prim_source(const DrawDesc &draw, uint32_t prim) {
  const uint32_t local = prim - draw.first_prim;
  const uint32_t inst = local / draw.tris_per_instance;
  const uint32_t tri = local - inst * draw.tris_per_instance;
  uint32_t vi[3] = {3u * tri, 3u * tri + 1u, 3u * tri + 2u};
  if (draw.indices) {
    const GlobalIndex ix = (GlobalIndex)draw.indices + 3u * tri;
    vi[0] = ix[0]; vi[1] = ix[1]; vi[2] = ix[2];
  }
  PrimSource s;
  const GlobalVertex gv = (GlobalVertex)draw.vertices;
#pragma unroll
  for (int k = 0; k < 3; ++k) s.v[k] = gv + vi[k];
  s.ib = (GlobalInstance)draw.instances + inst;
  return s;
}

// The positions phase's loads: the three positions and the instance's model matrix, one batch.  The fence keeps the compiler from
// sinking the loads to their first use (one round trip for the batch, not one per matrix column).
BB_DEV void load_positions(const PrimSource &s, float (*pos)[3], Mat4 &model) {
#pragma unroll
  for (int k = 0; k < 3; ++k)
#pragma unroll
    for (int c = 0; c < 3; ++c) pos[k][c] = s.v[k]->pos[c];
#pragma unroll
  for (int r = 0; r < 4; ++r)
#pragma unroll
    for (int cc = 0; cc < 4; ++cc) model.M[r][cc] = s.ib->model.M[r][cc];
  asm volatile("" :: "v"(pos[0][0]), "v"(pos[1][0]), "v"(pos[2][0]), "v"(model.M[0][0]),
               "v"(model.M[0][1]), "v"(model.M[0][2]), "v"(model.M[0][3]), "v"(model.M[1][0]), "v"(model.M[1][1]), "v"(model.M[1][2]),
               "v"(model.M[1][3]), "v"(model.M[2][0]), "v"(model.M[2][1]), "v"(model.M[2][2]), "v"(model.M[2][3]), "v"(model.M[3][0]),
               "v"(model.M[3][1]), "v"(model.M[3][2]), "v"(model.M[3][3]) : "memory");
}

// ---- the vertex program's expressions (forward_brdf.vert:25,31-35 = tbn.vert:18-25), each stated once: k_geometry and
// k_tbn_segments both call them, so the TBN overlay's N, T, B and posWorld are the forward pass's, bit for bit ----
// posWorld = model * (pos, 1)
template <typename M4>
BB_DEV f4 vertex_world(const M4 &model, const float *pos) { return mat4_mul(model, f4{pos[0], pos[1], pos[2], 1.0f}); }
// a direction (normal, tangent) through normalMat = transpose(mat3(aInvModel)), im = the inverse model matrix's upper 3 x 3:
// normalize(normalMat * v).  B = cross3(N, T).
BB_DEV f3 normal_dir(const float (*im)[3], f3 v) { return normalize3(mk3(dot3(ld3(im[0]), v), dot3(ld3(im[1]), v), dot3(ld3(im[2]), v))); }

// gl_Position of one vertex (and posWorld of the main passes' vertex program).
template <bool OVERLAY>
BB_DEV f4 vertex_clip_pos(const Mat4 &model, const float *pos, const Mat4 &pv, const Mat4 &view, const FrameParams &fp, f3 &world) {
  // OVERLAY: the host folds the matrices: ib.model = (P*V)*modelMat of the light (light.vert:11-14) or the gizmo's own
  // projMat*viewMat (gizmo.vert:13-24)
  const f4 w = vertex_world(model, pos);
  if (OVERLAY) {
    world = mk3(0.0f, 0.0f, 0.0f);
    return w;
  }
  world = mk3(w.x, w.y, w.z);
  // forward_brdf.vert:27 multiplies (P*V) * posWorld (pv = P*V); gbuffer.vert:19-22 P * (V * posWorld) (pv = P)
  return fp.deferred ? mat4_mul(pv, mat4_mul(view, w)) : mat4_mul(pv, w);
}

// The clip-space positions of a primitive: draw -> source -> positions and model matrix -> gl_Position of the three vertices
// (and posWorld).  k_geometry evaluates it for every primitive, and once more for the few that go through the clipper: the
// same expressions on the same operands, hence the same bits.  stamp(i): the caller's timing hooks (1: the draw is known,
// 6: the loads have been asked for).
struct PrimInputs {
  DrawDesc draw;
  PrimSource src;
};
template <bool OVERLAY, class Stamp>
BB_DEV PrimInputs prim_clip_positions(const DrawDesc *__restrict__ draws, uint32_t n_draws, const FirstPrims &first_prims, uint32_t prim,
                                      const Mat4 &pv, const Mat4 &view, const FrameParams &fp, float (*clip)[4], float (*pw)[3],
                                      Stamp stamp) {
  PrimInputs in;
  in.draw = draws[find_draw(draws, n_draws, first_prims, prim)];
  stamp(1);
  in.src = prim_source(in.draw, prim);
  float pos[3][3];
  Mat4 model;
  load_positions(in.src, pos, model);
  stamp(6);
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    f3 w;
    const f4 c = vertex_clip_pos<OVERLAY>(model, pos[k], pv, view, fp, w);
    pw[k][0] = w.x; pw[k][1] = w.y; pw[k][2] = w.z;
    clip[k][0] = c.x; clip[k][1] = c.y; clip[k][2] = c.z; clip[k][3] = c.w;
  }
  return in;
}

// Four dwords of a primitive record.  The record leaves k_geometry in 16-byte pieces as soon as their values exist --
// never as one 56-register struct -- and the pieces are the same fourteen dwordx4 stores the struct assignment was.
// `dword`: kRecPlanes, kRecHeadRest, kRecBody (bb_types.h, next to ShadeRec) plus a multiple of four.
typedef uint32_t rec_u32x4_ __attribute__((ext_vector_type(4)));
typedef rec_u32x4_ rec_u32x4 __attribute__((aligned(8)));  // (a record is 8-byte aligned: it holds a pointer)
BB_DEV void rec_store4(ShadeRec *rec, int dword, uint32_t a, uint32_t b, uint32_t c, uint32_t d) {
  rec_u32x4 v;
  v.x = a; v.y = b; v.z = c; v.w = d;
  *reinterpret_cast<rec_u32x4 *>(reinterpret_cast<uint32_t *>(rec) + dword) = v;
}
BB_DEV void rec_store4(ShadeRec *rec, int dword, float a, float b, float c, float d) {
  rec_store4(rec, dword, __float_as_uint(a), __float_as_uint(b), __float_as_uint(c), __float_as_uint(d));
}
// The rest of the head, three pieces: rw2, the first two varyings of the three vertices (uv; the overlay programs' own),
// packed_dims, packed, material, clip_base.  (A clipped primitive's clip_base is patched in once the clipper has its arena slots.)
BB_DEV void rec_store_head_rest(ShadeRec *rec, float rw2, const float *v0, const float *v1, const float *v2, uint32_t packed_dims,
                                const uint8_t *packed, uint32_t material) {
  const unsigned long long packed_bits = (unsigned long long)reinterpret_cast<uintptr_t>(packed);
  rec_store4(rec, kRecHeadRest, rw2, v0[0], v0[1], v1[0]);
  rec_store4(rec, kRecHeadRest + 4, __float_as_uint(v1[1]), __float_as_uint(v2[0]), __float_as_uint(v2[1]), packed_dims);
  rec_store4(rec, kRecHeadRest + 8, (uint32_t)packed_bits, (uint32_t)(packed_bits >> 32), material, kNotClipped);
}

// One thread per primitive, all draw calls of the frame in one launch (API order = primitive index order).
// OVERLAY = true is the overlay subpass (light markers, corner gizmo): other vertex programs and a
// per-primitive viewport, everything downstream of the vertex stage shared.
// The body's phases, each a marked block that states its inputs and outputs: positions, frustum fate, setup and ownership,
// record, bins, clipper, statistics (which of them can be functions: profiles/r11_geometry_stage.txt).
template <int TILE_W, int TILE_H, bool OVERLAY = false>
__global__ __launch_bounds__(256) void k_geometry(const DrawDesc *__restrict__ draws, uint32_t n_draws, uint32_t n_prims,
                                                  FirstPrims first_prims,
                                                  RasterTri *__restrict__ tris, ShadeRec *__restrict__ recs,
                                                  uint32_t *__restrict__ tile_count, uint32_t *__restrict__ bins,
                                                  Counters *__restrict__ ctr,
                                                  Mat4 pv, Mat4 view, FrameParams fp, ClipSlot *__restrict__ clip_arena,
                                                  BroadTri *__restrict__ broad_list,
                                                  const MaterialDesc *__restrict__ materials,
                                                  BlockStats *__restrict__ block_stats, uint32_t *__restrict__ heavy) {
#ifdef BB_STAMPS
#define BB_STAMP(i) do { if (threadIdx.x == 0) reinterpret_cast<unsigned long long *>(clip_arena + fp.clip_cap)[blockIdx.x * 8 + (i)] = wall_clock64(); } while (0)
  const auto phase1_stamp = [&](int i) {
    if (i == 6) asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");  // (the loads have arrived)
    BB_STAMP(i);
  };
#else
#define BB_STAMP(i) do { } while (0)
  const auto phase1_stamp = [](int) {};
#endif
  // This kernel's waves issue one instruction in ~18 cycles and wait for memory most of their lives; with frames in flight
  // they share their SIMDs with k_shade's, which want to issue all the time.  At the highest issue priority their few
  // instructions go out when they are ready and the wave gives its slot back sooner (k_raster does the same; C3 frame
  // -2 % on two boxes of three, 0 on the third; C5 the same as without).
  __builtin_amdgcn_s_setprio(3);
  BB_STAMP(0);
  __shared__ ClipWork s_clip[4];  // one per wave
  // (No workgroup barrier anywhere in this kernel: the four waves of a workgroup share nothing -- each has its own clip
  //  workspace and leaves its own statistics record -- so a wave retires when ITS primitives are done.)
  const uint32_t prim = blockIdx.x * blockDim.x + threadIdx.x;
  bool needs_clip = false;
  bool survives_out = false;  // this lane's primitive is rasterised unclipped (statistics)
  bool binned = false;  // this lane holds an unclipped, set-up triangle that goes to tile bins
  uint32_t cls = 0;     // raster class of the triangle: bin segment (kBinClasses per tile)
  TileRange tr = {0, -1, 0, -1};
  uint32_t clipped_raster = 0;  // wave-uniform: sub-triangles of this wave's clipped primitives that reached the every-tile list
  Viewport vp = {fp.half_w, fp.half_h, fp.half_w, fp.half_h};
  if (prim < n_prims) {
    // ---- positions.  In: prim.  Out: clip (gl_Position of the three vertices), pw (posWorld, main passes), the draw and
    // where the primitive's inputs are.  Every lane, positions and the model matrix only: gl_Position decides whether the
    // primitive can touch a pixel at all; half of a closed mesh faces away from the camera and is culled below.  Normals,
    // tangents, texture coordinates and the inverse model matrix are asked for behind the cull, by the survivors alone: carried
    // through the cull and the binary64 setup they made this kernel the largest register holder of the pipelined frame ----
    float clip[3][4];
    float pw[3][3];
    const PrimInputs in = prim_clip_positions<OVERLAY>(draws, n_draws, first_prims, prim, pv, view, fp, clip, pw, phase1_stamp);
    const DrawDesc &draw = in.draw;
    const PrimSource &src = in.src;
    ShadeRec *const rec = recs + prim;
    if (OVERLAY && prim >= fp.ov_first_gizmo_prim) vp = Viewport{fp.ov_half, fp.ov_half, fp.ov_cx, fp.ov_cy};
    // ---- frustum fate.  In: clip.  Out: culled (all three vertices outside one plane of the TRUE frustum: cannot change any
    // pixel), all_in (every vertex inside near, far and the guard band: rasterised as it is); neither: crossing, the clipper's ----
    bool o_l = true, o_r = true, o_t = true, o_b = true, o_n = true, o_f = true, all_in = true;
#pragma unroll
    for (int i = 0; i < 3; ++i) {
      const float *c = clip[i];
      o_l &= (c[3] + c[0] < 0.0f); o_r &= (c[3] - c[0] < 0.0f);
      o_t &= (c[3] + c[1] < 0.0f); o_b &= (c[3] - c[1] < 0.0f);
      o_n &= (c[3] - c[2] < 0.0f); o_f &= (c[2] < 0.0f);
#pragma unroll
      for (int p = 0; p < 6; ++p) all_in &= (plane_dist(c, p) >= 0.0f);
    }
    const bool culled = o_l | o_r | o_t | o_b | o_n | o_f;
    // ---- setup and ownership.  In: clip, vp, culled, all_in.  Out: t (set up; zero unless all_in), its tile range tr, survives
    // (unclipped, front-facing, holds a pixel centre of this rank's bands), needs_clip ----
    RasterTri t = {};
    bool survives = false;
    if (!culled) {
      if (all_in) {
        float z0, z1, z2;
        if (project_vertex(clip[0], vp, t.X0, t.Y0, t.rw0, z0) && project_vertex(clip[1], vp, t.X1, t.Y1, t.rw1, z1) &&
            project_vertex(clip[2], vp, t.X2, t.Y2, t.rw2, z2) && setup_tri(t, z0, z1, z2) &&
            tile_range<TILE_W, TILE_H>(frame_box(t, fp), tr)) {
          // screen-band partition: a primitive whose tile rows hold none of this rank's bands is somebody else's: no record,
          // no bin entry.  (Every rank still runs the vertex positions of every primitive -- that is what tells it whose they are.)
          survives = rows_owned(fp, tr.ty0, tr.ty1);
        }
      } else if (!BB_ABLATE(128u)) {
        needs_clip = true;
      }
    }
    BB_STAMP(7);
    if (survives || needs_clip) {
      // ---- record.  In: t, tr, pw, draw, src.  Out: tris[prim], recs[prim]; binned, cls; an every-tile-list entry for a
      // survivor of more than fp.broad_threshold tiles.  Survivors ask for the attributes and the upper 3 x 3 of the instance's
      // inverse model matrix (the normal matrix; the overlay programs' colour / view rows) -- one batch, one more dependent
      // round trip, closed by a fence like the positions' -- and, while they travel, send off everything known already: the
      // triangle, the record's planes and posWorld.  Only two values (rw2, posWorld.z of vertex 2: the first dwords of 16-byte
      // pieces that the attributes complete) and the tile range wait for the loads with the lane. ----
      const bool keep = !BB_ABLATE(64u);
      // The light path: the host says (kDrawStaticPresent) that the camera-independent part of the draw's records -- uv, the
      // material binding, the whole body -- is in `recs` already, bit for bit what this block would store (k_record_static).
      // Such a lane asks for no attributes, computes no N, T, B and stores the planes, rw2 and clip_base only.
      const bool light = !OVERLAY && (draw.flags & kDrawStaticPresent) != 0u;
      if (keep) {
        if (survives) tris[prim] = t;
        // planes of the unclipped triangle; zero for a primitive that goes through the clipper (its sub-triangles have their
        // own): t is written in the unclipped branch only, so there it still holds the zeros it was initialised with
        rec_store4(rec, kRecPlanes, (uint32_t)t.X0, (uint32_t)t.Y0, __float_as_uint(t.l1dx), __float_as_uint(t.l1dy));
        rec_store4(rec, kRecPlanes + 4, t.l2dx, t.l2dy, t.rw0, t.rw1);
        if (!OVERLAY && !light) {
          // body varyings 0..2 (posWorld), varying-major: vary[j][k] = pw[k][j]
          rec_store4(rec, kRecBody, pw[0][0], pw[1][0], pw[2][0], pw[0][1]);
          rec_store4(rec, kRecBody + 4, pw[1][1], pw[2][1], pw[0][2], pw[1][2]);
        }
      }
      const float rw2 = t.rw2, pwz2 = pw[2][2];
      survives_out = survives;
      if (survives) {
        uint32_t ntiles = (uint32_t)(tr.tx1 - tr.tx0 + 1) * (uint32_t)(tr.ty1 - tr.ty0 + 1);
        if (ntiles > fp.broad_threshold) broad_insert(t, prim << 3, fp, ctr, broad_list);
        else binned = true;
        cls = raster_class(frame_box(t, fp), tri_span(tri_core(t)));  // (the box again, not kept from the setup: two registers)
      }
      if (light) {
        // (clip_base every frame: a primitive the clipper took last frame and leaves alone now is reset; the clipper patches
        //  it below exactly as on the full path)
        if (keep) {
          uint32_t *const dw = reinterpret_cast<uint32_t *>(rec);
          dw[kRecHeadRest] = __float_as_uint(rw2);
          dw[kRecHeadRest + 11] = kNotClipped;
        }
      } else {
        float nrm[3][3], tng[3][3], uv[3][2], im_[3][3];
#pragma unroll
        for (int k = 0; k < 3; ++k) {
          uv[k][0] = src.v[k]->uv[0]; uv[k][1] = src.v[k]->uv[1];
#pragma unroll
          for (int c = 0; c < 3; ++c) { nrm[k][c] = src.v[k]->normal[c]; tng[k][c] = src.v[k]->tangent[c]; }
        }
#pragma unroll
        for (int r = 0; r < 3; ++r)
#pragma unroll
          for (int cc = 0; cc < 3; ++cc) im_[r][cc] = src.ib->inv_model.M[r][cc];
        asm volatile("" :: "v"(im_[0][0]), "v"(im_[0][1]), "v"(im_[0][2]), "v"(im_[1][0]), "v"(im_[1][1]), "v"(im_[1][2]), "v"(im_[2][0]),
                     "v"(im_[2][1]), "v"(im_[2][2]), "v"(nrm[0][0]), "v"(nrm[1][0]), "v"(nrm[2][0]), "v"(tng[0][0]), "v"(tng[1][0]),
                     "v"(tng[2][0]), "v"(uv[0][0]), "v"(uv[1][0]), "v"(uv[2][0]) : "memory");
        if (OVERLAY) {
          // ib.inv_model row 0 = the light's colour, or the gizmo's viewMat whose upper 3x3 turns the normals
          // (gizmo.vert:27).  draw.material is the program: 1 marker, 2 gizmo (not an index into the material table).
          // Varyings 0, 1 sit in the head, 2..5 in the body.
          float o[3][6];
#pragma unroll
          for (int k = 0; k < 3; ++k) {
#pragma unroll
            for (int j = 0; j < 6; ++j) o[k][j] = 0.0f;
            if (draw.material == 1u) {
              o[k][0] = im_[0][0]; o[k][1] = im_[0][1]; o[k][2] = im_[0][2];
            } else {
              f3 n = ld3(nrm[k]);
              o[k][0] = tng[k][0]; o[k][1] = tng[k][1]; o[k][2] = tng[k][2];  // the gizmo mesh keeps its colour there
              o[k][3] = fmaf(im_[2][0], n.z, fmaf(im_[1][0], n.y, im_[0][0] * n.x));
              o[k][4] = fmaf(im_[2][1], n.z, fmaf(im_[1][1], n.y, im_[0][1] * n.x));
              o[k][5] = fmaf(im_[2][2], n.z, fmaf(im_[1][2], n.y, im_[0][2] * n.x));
            }
          }
          if (keep) {
            rec_store_head_rest(rec, rw2, o[0], o[1], o[2], 0u, nullptr, draw.material);
            rec_store4(rec, kRecBody, o[0][2], o[1][2], o[2][2], o[0][3]);
            rec_store4(rec, kRecBody + 4, o[1][3], o[2][3], o[0][4], o[1][4]);
            rec_store4(rec, kRecBody + 8, o[2][4], o[0][5], o[1][5], o[2][5]);
#pragma unroll
            for (int q = kRecBody + 12; q < kShadeRecDwords; q += 4) rec_store4(rec, q, 0.0f, 0.0f, 0.0f, 0.0f);
          }
        } else {
          // (the material's packed form travels in the draw descriptor: no load of the material table here)
          if (keep) rec_store_head_rest(rec, rw2, uv[0], uv[1], uv[2], draw.packed ? draw.packed_dims : 0u, draw.packed, draw.material);
          // Body varyings 3..11, varying-major like the rest of the body: N of the three vertices, then T, then B, each
          // 16-byte piece stored when its last value exists (the interleaving holds the kernel at 64 registers).
          f3 N[3], T[3], B[3];
#pragma unroll
          for (int k = 0; k < 3; ++k) N[k] = normal_dir(im_, ld3(nrm[k]));
          if (keep) {
            rec_store4(rec, kRecBody + 8, pwz2, N[0].x, N[1].x, N[2].x);
            rec_store4(rec, kRecBody + 12, N[0].y, N[1].y, N[2].y, N[0].z);
          }
#pragma unroll
          for (int k = 0; k < 3; ++k) T[k] = normal_dir(im_, ld3(tng[k]));
          if (keep) {
            rec_store4(rec, kRecBody + 16, N[1].z, N[2].z, T[0].x, T[1].x);
            rec_store4(rec, kRecBody + 20, T[2].x, T[0].y, T[1].y, T[2].y);
          }
#pragma unroll
          for (int k = 0; k < 3; ++k) B[k] = cross3(N[k], T[k]);
          if (keep) {
            rec_store4(rec, kRecBody + 24, T[0].z, T[1].z, T[2].z, B[0].x);
            rec_store4(rec, kRecBody + 28, B[1].x, B[2].x, B[0].y, B[1].y);
            rec_store4(rec, kRecBody + 32, B[2].y, B[0].z, B[1].z, B[2].z);
          }
        }
      }
    }
  }
  BB_STAMP(2);
  // ---- bins.  In: binned, tr, cls.  Out: bins / tile_count, refs (the references the wave wrote).  The lanes walk their tile
  // ranges in lock-step, aggregating per tile across the wave; four insertions per lane are reserved back to back, so their
  // returning atomics share one memory round trip ----
  uint32_t refs = 0;
  {
    const int tw = binned ? tr.tx1 - tr.tx0 + 1 : 0;
    const int nt = (binned && !BB_ABLATE(32u)) ? tw * (tr.ty1 - tr.ty0 + 1) : 0;
    for (int k0 = 0; __ballot(k0 < nt) != 0ull; k0 += 4) {
      bool has[4];
      uint32_t seg[4];
      BinTicket tk[4];
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int k = k0 + j;
        has[j] = k < nt;
        const int ty = has[j] ? tr.ty0 + k / tw : 0, tx = has[j] ? tr.tx0 + k % tw : 0;
        if (has[j] && !row_owned(fp, ty)) has[j] = false;  // another rank's band
        seg[j] = ((uint32_t)ty * (uint32_t)fp.tiles_x + (uint32_t)tx) * kBinClasses + cls;
        tk[j] = wave_bin_reserve(has[j], seg[j], tile_count);
        refs += (uint32_t)__popcll(__ballot(has[j]));
      }
#pragma unroll
      for (int j = 0; j < 4; ++j) wave_bin_write(has[j], seg[j], prim << 3, tk[j], fp, ctr, bins, (OVERLAY || !fp.heavy_threshold) ? nullptr : heavy);
    }
  }
  BB_STAMP(3);
  // ---- clipper (after the bins, so the other lanes' insertions never wait for it).  In: needs_clip, vp.  Out: the clip arena's
  // slots and the every-tile-list entries of the wave's clipped primitives, recs[prim].clip_base, clipped_raster.  The wave
  // clips its clipped primitives one after the other, all lanes on the same polygon ----
  for (unsigned long long cm = __ballot(needs_clip); cm; cm &= cm - 1ull) {
    const int owner = __builtin_amdgcn_readfirstlane(__ffsll((long long)cm) - 1);
    ClipWork &w = s_clip[threadIdx.x >> 6];
    // The owner's clip-space vertices and primitive index are the wave's input.  The vertices are not kept from the positions
    // phase (twelve registers in every lane, through the bin loop, for a handful of primitives per frame): the lanes that clip
    // evaluate them again here.
    float cv[3][4] = {};
    if (needs_clip) {
      float unused[3][3];
      prim_clip_positions<OVERLAY>(draws, n_draws, first_prims, prim, pv, view, fp, cv, unused, [](int) {});
    }
    Viewport ovp = vp;  // the owner's viewport for the whole wave
    if (OVERLAY) {
      ovp.half_w = __shfl(vp.half_w, owner); ovp.half_h = __shfl(vp.half_h, owner);
      ovp.cx = __shfl(vp.cx, owner); ovp.cy = __shfl(vp.cy, owner);
    }
    clip_primitive_wave(w, owner, cv, prim, fp, ovp, clip_arena, ctr, broad_list);
    __builtin_amdgcn_wave_barrier();
    clipped_raster += (uint32_t)w.n_valid;
    if ((int)(threadIdx.x & 63) == owner && w.n_valid) recs[prim].clip_base = w.base;  // (the record itself was written above, with zero planes)
    __builtin_amdgcn_wave_barrier();
  }
  BB_STAMP(4);
  // ---- statistics.  In: survives_out, needs_clip, clipped_raster, refs.  Out: one BlockStats record per WAVE (summed on the
  // host on demand): a few thousand atomics on ONE counter word would serialise at ~90 per microsecond and dominate this kernel ----
  {
    const uint32_t n_survivors = (uint32_t)__popcll(__ballot(survives_out));
    const uint32_t n_clipped = (uint32_t)__popcll(__ballot(needs_clip));
    if ((threadIdx.x & 63) == 0)
      block_stats[blockIdx.x * (blockDim.x / 64) + (threadIdx.x >> 6)] = BlockStats{n_survivors + clipped_raster, n_clipped, refs};
  }
  BB_STAMP(5);
}

// The camera-independent part of the records of ONE draw of the main pass (draws[d]): uv, the material binding and the body
// -- dwords 9..18 and 20..55 of ShadeRec; the planes, rw0..2 (0..8) and clip_base (19) are k_geometry's, every frame.  One thread
// per primitive, culled ones too (a primitive that faces away now may face the camera in the next frame).  The values come
// from the functions k_geometry's full path calls on the same operands, hence the same bits.  Queued by the host once per
// frame slot when a draw's key has repeated (bibim_hip.hip, static_records); k_geometry then takes its light path for the draw.
constexpr int kRecordStaticThreads = 256;
__global__ __launch_bounds__(kRecordStaticThreads) void k_record_static(const DrawDesc *__restrict__ draws, uint32_t d,
                                                                        ShadeRec *__restrict__ recs) {
  const DrawDesc draw = draws[d];
  const uint32_t local = blockIdx.x * blockDim.x + threadIdx.x;
  if (local >= draw.n_instances * draw.tris_per_instance) return;
  const uint32_t prim = draw.first_prim + local;
  const PrimSource src = prim_source(draw, prim);
  float pos[3][3];
  Mat4 model;
  load_positions(src, pos, model);
  float im_[3][3];
#pragma unroll
  for (int r = 0; r < 3; ++r)
#pragma unroll
    for (int cc = 0; cc < 3; ++cc) im_[r][cc] = src.ib->inv_model.M[r][cc];
  ShadeRec *const rec = recs + prim;
  uint32_t *const dw = reinterpret_cast<uint32_t *>(rec);
  // the head behind rw2: uv of the three vertices, packed_dims, packed, material (rec_store_head_rest without its two ends)
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    dw[kRecHeadRest + 1 + 2 * k] = __float_as_uint(src.v[k]->uv[0]);
    dw[kRecHeadRest + 2 + 2 * k] = __float_as_uint(src.v[k]->uv[1]);
  }
  const unsigned long long packed_bits = (unsigned long long)reinterpret_cast<uintptr_t>(draw.packed);
  dw[kRecHeadRest + 7] = draw.packed ? draw.packed_dims : 0u;
  dw[kRecHeadRest + 8] = (uint32_t)packed_bits;
  dw[kRecHeadRest + 9] = (uint32_t)(packed_bits >> 32);
  dw[kRecHeadRest + 10] = draw.material;
  // the body, varying-major: posWorld, N, T, B of the three vertices
  f3 N[3], T[3], B[3];
  float pw[3][3];
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    const f4 w = vertex_world(model, pos[k]);
    pw[k][0] = w.x; pw[k][1] = w.y; pw[k][2] = w.z;
    float nrm[3], tng[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) { nrm[c] = src.v[k]->normal[c]; tng[c] = src.v[k]->tangent[c]; }
    N[k] = normal_dir(im_, ld3(nrm));
    T[k] = normal_dir(im_, ld3(tng));
    B[k] = cross3(N[k], T[k]);
  }
  rec_store4(rec, kRecBody, pw[0][0], pw[1][0], pw[2][0], pw[0][1]);
  rec_store4(rec, kRecBody + 4, pw[1][1], pw[2][1], pw[0][2], pw[1][2]);
  rec_store4(rec, kRecBody + 8, pw[2][2], N[0].x, N[1].x, N[2].x);
  rec_store4(rec, kRecBody + 12, N[0].y, N[1].y, N[2].y, N[0].z);
  rec_store4(rec, kRecBody + 16, N[1].z, N[2].z, T[0].x, T[1].x);
  rec_store4(rec, kRecBody + 20, T[2].x, T[0].y, T[1].y, T[2].y);
  rec_store4(rec, kRecBody + 24, T[0].z, T[1].z, T[2].z, B[0].x);
  rec_store4(rec, kRecBody + 28, B[1].x, B[2].x, B[0].y, B[1].y);
  rec_store4(rec, kRecBody + 32, B[2].y, B[0].z, B[1].z, B[2].z);
}

// ------------------------------------------------------------------------------------------------
// texture sampling (SMP_LINEAR / REPEAT / one mip; src/render.cpp:1338-1371)
// ------------------------------------------------------------------------------------------------

BB_DEV int wrap_repeat(int i, int n) {
  int m = i % n;
  return m < 0 ? m + n : m;
}

struct BilinearTaps {
  uint32_t o00, o10, o01, o11;  // texel indices
  float fx, fy;
};

template <bool BLOCKED = false>
BB_DEV BilinearTaps bilinear_taps(float u, float v, int w, int h) {
  float x = fmaf(u, (float)w, -0.5f);
  float y = fmaf(v, (float)h, -0.5f);
  if (!(fabsf(x) < 1073741824.0f)) x = 0.0f;
  if (!(fabsf(y) < 1073741824.0f)) y = 0.0f;
  float xf = floorf(x), yf = floorf(y);
  BilinearTaps t;
  t.fx = x - xf;
  t.fy = y - yf;
  int ix = (int)xf, iy = (int)yf;
  int x0, x1, y0, y1;
  if (((w & (w - 1)) | (h & (h - 1))) == 0) {  // power-of-two sizes: wrap is a mask
    x0 = ix & (w - 1); x1 = (ix + 1) & (w - 1);
    y0 = iy & (h - 1); y1 = (iy + 1) & (h - 1);
  } else {
    x0 = wrap_repeat(ix, w); x1 = wrap_repeat(ix + 1, w);
    y0 = wrap_repeat(iy, h); y1 = wrap_repeat(iy + 1, h);
  }
  if (BLOCKED) {
    // the packed material is stored block-linear, 4 x 4 texels per 144-byte block (written by bbr_upload_material):
    // texel (x, y) = record ((y >> 2) * ceil(w / 4) + (x >> 2)) * 16 + (y & 3) * 4 + (x & 3).  A minified tap set touches
    // one or two 128-byte lines instead of always two rows 9 w bytes apart.
    const int w4 = (w + 3) >> 2;
    const uint32_t row0 = ((uint32_t)mul32(y0 >> 2, w4) << 4) + (((uint32_t)y0 & 3u) << 2);
    const uint32_t row1 = ((uint32_t)mul32(y1 >> 2, w4) << 4) + (((uint32_t)y1 & 3u) << 2);
    const uint32_t col0 = (((uint32_t)x0 >> 2) << 4) + ((uint32_t)x0 & 3u), col1 = (((uint32_t)x1 >> 2) << 4) + ((uint32_t)x1 & 3u);
    t.o00 = row0 + col0;
    t.o10 = row0 + col1;
    t.o01 = row1 + col0;
    t.o11 = row1 + col1;
    return t;
  }
  const uint32_t row0 = (uint32_t)mul32(y0, w), row1 = (uint32_t)mul32(y1, w);
  t.o00 = row0 + (uint32_t)x0;
  t.o10 = row0 + (uint32_t)x1;
  t.o01 = row1 + (uint32_t)x0;
  t.o11 = row1 + (uint32_t)x1;
  return t;
}

// byte k of a dword as a float: v_cvt_f32_ubyteN.  Spelled out, so that the compiler keeps the conversion: left to
// itself it rewrites float(b) - float(a) as float(int(b) - int(a)) -- v_sub_u32_sdwa + v_cvt_f32_i32, two of the expensive
// (non-fma-class) instructions where the float subtraction is a cheap one; 18 more of them per pixel.
// byte offset of packed texel i (9-byte records): i * 8 + i as one v_lshl_add_u32, not the v_mad_i32_i24 the compiler picks
BB_DEV uint32_t texel_offset(uint32_t i) {
  static_assert(kPackedTexelBytes == 9, "texel_offset");
  asm("" : "+v"(i));
  return (i << 3) + i;
}
BB_DEV float byte_f32(uint32_t t, int shift) {
  float f;
  if (shift == 0) asm("v_cvt_f32_ubyte0 %0, %1" : "=v"(f) : "v"(t));
  else if (shift == 8) asm("v_cvt_f32_ubyte1 %0, %1" : "=v"(f) : "v"(t));
  else if (shift == 16) asm("v_cvt_f32_ubyte2 %0, %1" : "=v"(f) : "v"(t));
  else asm("v_cvt_f32_ubyte3 %0, %1" : "=v"(f) : "v"(t));
  return f;
}
BB_DEV float filter_channel(uint32_t t00, uint32_t t10, uint32_t t01, uint32_t t11, int shift, float fx, float fy) {
  float a = byte_f32(t00, shift), b = byte_f32(t10, shift);
  float c = byte_f32(t01, shift), d = byte_f32(t11, shift);
  float top = fmaf(fx, b - a, a);
  float bot = fmaf(fx, d - c, c);
  return fmaf(fy, bot - top, top) * (1.0f / 255.0f);
}

// ------------------------------------------------------------------------------------------------
// brdf.glsl
// ------------------------------------------------------------------------------------------------

BB_DEV float distribution_ggx(float NdotH_raw, float roughness) {
  float a = roughness * roughness;
  float a2 = a * a;
  float NdotH = max0(NdotH_raw);
  float NdotH2 = NdotH * NdotH;
  float denom = fmaf(NdotH2, a2 - 1.0f, 1.0f);
  denom = (kPi * denom) * denom;
  return a2 * bb_rcp(denom);
}

// roughness comes out of filter_channel (a bilinear blend of bytes / 255, possibly rounded to binary16): it is in
// [0, 1], so k = (r + 1)^2 / 8 is in [0.125, 0.5]; NdotX = max0(dot of two vectors that are unit length, zero or NaN) is
// in [0, 1 + 2^-20] (max0 removes the NaN).  Hence denom is in [0.125, 1.01]: a normal number, no guard needed.
BB_DEV float geometry_schlick_ggx(float NdotX, float k) {
  float denom = fmaf(NdotX, 1.0f - k, k);
  return NdotX * bb_rcp_normal(denom);
}

BB_DEV float mixf(float a, float b, float t) { return fmaf(b, t, a * (1.0f - t)); }
BB_DEV float clamp01(float x) { return x < 0.0f ? 0.0f : (x > 1.0f ? 1.0f : x); }

// ------------------------------------------------------------------------------------------------
// tile kernel
// ------------------------------------------------------------------------------------------------

struct ShadeParams {
  float view_pos[3];
  int32_t enable_normal_map;
  int32_t num_lights;
  int32_t tone_enable;  // fused presentation only (option "present_fused"): FrameUniformBlock.EnableToneMapping / Exposure
  float exposure;
};

// pixel index inside the tile, 8x8-blocked so that 64 consecutive indices form one 8x8 pixel block
template <int TILE_W>
BB_DEV void tile_pixel(int p, int &x, int &y) {
  int block = p >> 6, within = p & 63;
  constexpr int BX = TILE_W / 8;
  x = (block % BX) * 8 + (within & 7);
  y = (block / BX) * 8 + (within >> 3);
}
template <int TILE_W>
BB_DEV int tile_index(int x, int y) {
  constexpr int BX = TILE_W / 8;
  return (((y >> 3) * BX + (x >> 3)) << 6) | ((y & 7) << 3) | (x & 7);
}

// overlay pass: primitives from fp.ov_first_gizmo_prim on are the gizmo -- scissored to its rectangle (src/main.cpp:767-772)
// and lifted above every other depth (see depth_max); `ref` is a bin reference (primitive << 3 | sub-triangle)
template <bool OVERLAY>
BB_DEV bool gizmo_ref(const FrameParams &fp, uint32_t ref) { return OVERLAY && (ref >> 3) >= fp.ov_first_gizmo_prim; }
// the scissor rectangle of a primitive: the gizmo's own, no scissor (every pixel a frame can have) for everything else
template <bool OVERLAY>
BB_DEV PixRect scissor_rect(const FrameParams &fp, uint32_t ref) {
  return gizmo_ref<OVERLAY>(fp, ref) ? PixRect{fp.ov_x0, fp.ov_x1 - 1, fp.ov_y0, fp.ov_y1 - 1} : PixRect{0, (1 << 30) - 1, 0, (1 << 30) - 1};
}

// A triangle against a rectangle of pixel centres [x0,x1] x [y0,y1]: 0 = no centre covered, 1 = some, 2 = all.
// Edge functions are affine, so their extrema over the rectangle sit at corners picked by the gradient signs.
struct EdgeSetup {
  int dx[3], dy[3], bias[3];
  int X[3], Y[3];
};

BB_DEV EdgeSetup edge_setup(const TriCore &t) {
  EdgeSetup e;
  e.X[0] = t.X0; e.Y[0] = t.Y0; e.X[1] = t.X1; e.Y[1] = t.Y1; e.X[2] = t.X2; e.Y[2] = t.Y2;
  e.dx[0] = t.X1 - t.X0; e.dy[0] = t.Y1 - t.Y0;  // |coordinates| < 2^30 (project_vertex), differences fit 32 bits
  e.dx[1] = t.X2 - t.X1; e.dy[1] = t.Y2 - t.Y1;
  e.dx[2] = t.X0 - t.X2; e.dy[2] = t.Y0 - t.Y2;
#pragma unroll
  for (int i = 0; i < 3; ++i) e.bias[i] = (e.dy[i] < 0 || (e.dy[i] == 0 && e.dx[i] > 0)) ? 0 : -1;  // top-left rule
  return e;
}

// exact: 32x32 -> 64-bit products (v_mad_i64_i32)
BB_DEV long long edge_eval(const EdgeSetup &e, int i, int px, int py) {
  int Xc = px * 256 + 128, Yc = py * 256 + 128;
  return (long long)e.dx[i] * (long long)(Yc - e.Y[i]) - (long long)e.dy[i] * (long long)(Xc - e.X[i]) + (long long)e.bias[i];
}

BB_DEV int classify_rect(const EdgeSetup &e, const PixRect &b) {
  const int x0 = b.x0, x1 = b.x1, y0 = b.y0, y1 = b.y1;
  bool all_in = true;
#pragma unroll
  for (int i = 0; i < 3; ++i) {
    // dE/dx = -dy*256, dE/dy = +dx*256
    int xmax = e.dy[i] <= 0 ? x1 : x0, xmin = e.dy[i] <= 0 ? x0 : x1;
    int ymax = e.dx[i] >= 0 ? y1 : y0, ymin = e.dx[i] >= 0 ? y0 : y1;
    if (edge_eval(e, i, xmax, ymax) < 0) return 0;
    all_in &= edge_eval(e, i, xmin, ymin) >= 0;
  }
  return all_in ? 2 : 1;
}

// zbias (overlay pass only): added to the depth BITS of the key, order-preserving -- 0x40000000 lifts the gizmo's
// fragments above every depth in [0, 1] drawn before (the reference clears the rectangle's depth before the gizmo)
// while they still compete among themselves by depth.
BB_DEV void depth_max(const TriCore &t, int px, int py, uint32_t ref, unsigned long long *keys, int key_index,
                      uint32_t zbias = 0u) {
  int Xc = px * 256 + 128, Yc = py * 256 + 128;
  float dxp = (float)(Xc - t.X0), dyp = (float)(Yc - t.Y0);
  float z = fmaf(t.dzdx, dxp, fmaf(t.dzdy, dyp, t.z0));
  if (!(z >= 0.0f)) z = 0.0f;
  if (z > 1.0f) z = 1.0f;
  unsigned long long key = ((unsigned long long)(__float_as_uint(z) + zbias) << 32) | (unsigned long long)(ref + 1u);
  atomicMax(&keys[key_index], key);
}

// One wave rasterises one (wave-uniform) triangle into the tile's LDS keys: 8x8 pixel blocks of bounding box ^ tile,
// one pixel per lane.  Rectangles fully inside the triangle skip the edge tests.  Triangles spanning <= 64 px use
// 32-bit edge functions stepped with 24-bit multiply-adds (exact: every term < 2^30); larger ones use 64-bit products.
// `clip`: the frame's pixels (the gizmo's: inside its scissor rectangle)
template <int TILE_W, int TILE_H>
BB_DEV void raster_triangle_wave(const TriCore &t, uint32_t ref, const PixRect &clip, int tile_x0, int tile_y0,
                                 unsigned long long *keys, int lane, uint32_t zbias) {
  const PixRect box = pixel_box(t, clip, PixRect{tile_x0, tile_x0 + TILE_W - 1, tile_y0, tile_y0 + TILE_H - 1});
  if (!box.any()) return;
  const int px0 = box.x0, px1 = box.x1, py0 = box.y0, py1 = box.y1;
  const EdgeSetup e = edge_setup(t);
  const int w = px1 - px0 + 1, h = py1 - py0 + 1;
  const int lx = lane & 7, ly = lane >> 3;
  if (tri_span(t) <= (1 << 14)) {
    const int Xc0 = px0 * 256 + 128, Yc0 = py0 * 256 + 128;
    int o[3], sx[3], sy[3];
    bool none = false, all = true;
#pragma unroll
    for (int i = 0; i < 3; ++i) {
      o[i] = e.dx[i] * (Yc0 - e.Y[i]) - e.dy[i] * (Xc0 - e.X[i]) + e.bias[i];
      sx[i] = -e.dy[i] * 256;
      sy[i] = e.dx[i] * 256;
      int hi = o[i] + (sx[i] > 0 ? sx[i] * (w - 1) : 0) + (sy[i] > 0 ? sy[i] * (h - 1) : 0);
      int lo = o[i] + (sx[i] < 0 ? sx[i] * (w - 1) : 0) + (sy[i] < 0 ? sy[i] * (h - 1) : 0);
      none |= hi < 0;
      all &= lo >= 0;
    }
    if (none) return;
    for (int by = 0; by < h; by += 8) {
      for (int bx = 0; bx < w; bx += 8) {
        int x = bx + lx, y = by + ly;
        bool in = x < w && y < h;
        if (in && !all) {
          int e0 = mul32(x, sx[0]) + mul32(y, sy[0]) + o[0];
          int e1 = mul32(x, sx[1]) + mul32(y, sy[1]) + o[1];
          int e2 = mul32(x, sx[2]) + mul32(y, sy[2]) + o[2];
          in = (e0 | e1 | e2) >= 0;
        }
        if (in) depth_max(t, px0 + x, py0 + y, ref, keys, tile_index<TILE_W>(px0 + x - tile_x0, py0 + y - tile_y0), zbias);
      }
    }
    return;
  }
  const int cls = classify_rect(e, box);
  if (cls == 0) return;
  for (int by = 0; by < h; by += 8) {
    for (int bx = 0; bx < w; bx += 8) {
      int px = px0 + bx + lx, py = py0 + by + ly;
      bool in = px <= px1 && py <= py1;
      if (in && cls == 1) in = (edge_eval(e, 0, px, py) | edge_eval(e, 1, px, py) | edge_eval(e, 2, px, py)) >= 0;
      if (in) depth_max(t, px, py, ref, keys, tile_index<TILE_W>(px - tile_x0, py - tile_y0), zbias);
    }
  }
}

constexpr int kItemsThreads = 256;  // launch slots per workgroup of k_shade_items
// words between two of k_raster's chunk counters: a 128-byte cache line each.  Atomics on one LINE serialise like atomics on
// one address (packed 32 to a line they cost k_raster 5 us at C5's 32 640 tiles)
constexpr int kItemGroupStride = 32;
constexpr int kItemGroupSlots = 32, kItemGroups = 2048;  // k_raster's chunk totals: one counter per 32 launch slots (fewer
                                                          // addresses made the atomics cost k_raster 7 us at C3)
constexpr int kItemChunkBits = 6, kItemTxBits = 12;  // item = full << 31 | grid row << 18 | tile column << 6 | chunk of 64 fragments
// A tile that ONE triangle covers completely and nothing else touches has no fragment list: its count word carries this flag
// and the tile's list holds a single word (pixel field 0); fragment p of the tile is that word with p in the pixel field.
// k_shade_items hands the flag on in the item word, so that k_shade knows before it loads anything.
constexpr uint32_t kFullTile = 0x80000000u;
constexpr int kFragPixBits = 12;  // pixel-in-tile field of a fragment's high word (tiles of up to 64x64); the clip slot + 1 sits above it
constexpr int kTileThreads = 256;
constexpr int kTileWaves = kTileThreads / 64;

// ONE ROW of a small triangle (raster classes 0 and 1: spans <= 64 px, so every edge-function term fits 32 bits and a
// step is a plain add) by one lane: the row's pixels of bounding box ^ tile, left to right.  k_raster hands the rows of all
// small triangles of a chunk out as one list (see there), so a lane's work is a row whatever the triangle's size.
// Same values as the 64-bit form (edge_eval) at every pixel centre: E' = E + (top-left ? 0 : -1), covered <=> all E' >= 0.
// The depth is depth_max's expression with its row-constant half hoisted: z = fma(dzdx, dxp, fma(dzdy, dyp, z0)), and
// dxp = float(Xc - X0) is stepped by 256.0f (exact: |Xc - X0| <= 2^14 + 2^8 inside the bounding box).
template <int TILE_W>
BB_DEV void raster_triangle_row(const TriCore &t, uint32_t ref, int px0, int px1, int py, int tile_x0, int tile_y0,
                                unsigned long long *keys, uint32_t zbias) {
  const int X0 = t.X0, Y0 = t.Y0, X1 = t.X1, Y1 = t.Y1, X2 = t.X2, Y2 = t.Y2;
  const float z0 = t.z0, dzdx = t.dzdx, dzdy = t.dzdy;
  const int dx0 = X1 - X0, dy0 = Y1 - Y0;
  const int dx1 = X2 - X1, dy1 = Y2 - Y1;
  const int dx2 = X0 - X2, dy2 = Y0 - Y2;
  const int Xc0 = px0 * 256 + 128, Yc = py * 256 + 128;
  int e0 = mul32(dx0, Yc - Y0) - mul32(dy0, Xc0 - X0) + ((dy0 < 0 || (dy0 == 0 && dx0 > 0)) ? 0 : -1);
  int e1 = mul32(dx1, Yc - Y1) - mul32(dy1, Xc0 - X1) + ((dy1 < 0 || (dy1 == 0 && dx1 > 0)) ? 0 : -1);
  int e2 = mul32(dx2, Yc - Y2) - mul32(dy2, Xc0 - X2) + ((dy2 < 0 || (dy2 == 0 && dx2 > 0)) ? 0 : -1);
  const int sx0 = dy0 * 256, sx1 = dy1 * 256, sx2 = dy2 * 256;  // E(x+1) = E - sx
  const float zrow = fmaf(dzdy, (float)(Yc - Y0), z0);
  float dxp = (float)(Xc0 - X0);
  const int y = py - tile_y0;
  constexpr int BX = TILE_W / 8;
  const int row_index = (((y >> 3) * BX) << 6) | ((y & 7) << 3);  // tile_index<TILE_W>(x, y) = row_index + (x >> 3 << 6 | x & 7)
  const unsigned long long key_lo = (unsigned long long)(ref + 1u);
  // (Two variations of this loop were built, bit-exact, and measured slower in round 5 -- the boxes of small triangles are
  //  4 (class 0) / 10 (class 1) pixels wide and 30 % covered at C3, tools/raster_stats.py: (a) bounding the row's span first,
  //  x <= e_i / sx_i per edge from binary32 quotients widened by 0.001 px, the exact test still deciding: 48 instructions per
  //  row, k_raster's VALU count 12.9 M -> 14.5 M; (b) two passes, a coverage bit per pixel and then the depth code over the set
  //  bits only: 15.2 M, k_raster alone 45.6 -> 47.6 us.)
  for (int x = px0 - tile_x0; x <= px1 - tile_x0; ++x) {
    if ((e0 | e1 | e2) >= 0) {
      float z = fmaf(dzdx, dxp, zrow);
      if (!(z >= 0.0f)) z = 0.0f;
      if (z > 1.0f) z = 1.0f;
      atomicMax(&keys[row_index + (((x >> 3) << 6) | (x & 7))], ((unsigned long long)(__float_as_uint(z) + zbias) << 32) | key_lo);
    }
    e0 -= sx0; e1 -= sx1; e2 -= sx2;
    dxp += 256.0f;
  }
}

// owned tile row (grid y) -> global tile row; false if past the frame
BB_DEV bool tile_row(const FrameParams &fp, int grid_y, int &ty, int &out_tile_row) {
  if (fp.world > 1) {
    int lb = grid_y / fp.band_tiles, r = grid_y - lb * fp.band_tiles;
    ty = (lb * fp.world + fp.rank) * fp.band_tiles + r;
  } else {
    ty = grid_y;
  }
  out_tile_row = grid_y;
  return ty < fp.tiles_y;
}

// ---- The two words k_raster hands to the fragment kernels, each with its encoder next to its decoder ----
// item = full-tile flag (kFullTile, or 0) | grid row << 18 | tile column << 6 | chunk of 64 fragments
BB_DEV uint32_t item_word(uint32_t full, uint32_t grid_row, uint32_t tx, uint32_t chunk) { return full | (grid_row << (kItemChunkBits + kItemTxBits)) | (tx << kItemChunkBits) | chunk; }
// one work item: where its 64 fragments are (all wave-uniform, held in scalar registers)
struct ItemPlace {
  int chunk, tx, ty, out_tile_row;
  uint32_t tile;
};
BB_DEV ItemPlace decode_item(const FrameParams &fp, uint32_t item) {
  ItemPlace p;
  p.chunk = (int)(item & 63u);
  p.tx = (int)((item >> kItemChunkBits) & ((1u << kItemTxBits) - 1u));
  tile_row(fp, (int)((item & ~kFullTile) >> (kItemChunkBits + kItemTxBits)), p.ty, p.out_tile_row);
  p.tile = (uint32_t)p.ty * (uint32_t)fp.tiles_x + (uint32_t)p.tx;
  return p;
}

// fragment = ((clip slot + 1) << kFragPixBits | pixel in tile) << 32 | reference
BB_DEV unsigned long long fragment_word(uint32_t clip_slot1, uint32_t pixel, uint32_t ref) {
  return ((((unsigned long long)clip_slot1 << kFragPixBits) | (unsigned long long)pixel) << 32) | (unsigned long long)ref;
}
template <int TILE_PIXELS>
BB_DEV int fragment_pixel(unsigned long long frag) { return (int)(frag >> 32) & (TILE_PIXELS - 1); }
// (the clip slot + 1 is read in place, `frag >> (32 + kFragPixBits)`: k_shade compiled to other code with a helper here)

// this lane's fragment word of an item, and whether the lane has one.  A tile one triangle covers completely has no list and
// no count: one word, the pixel is the lane's own (and the wave is uniform).  CONST_WORD: that word comes through the scalar
// cache (constant address space).
template <int TILE_PIXELS, bool CONST_WORD>
BB_DEV unsigned long long fetch_fragment(uint32_t item, const ItemPlace &p, int lane, const unsigned long long *__restrict__ frags,
                                         const uint32_t *__restrict__ frag_count, bool &valid) {
  typedef const unsigned long long __attribute__((address_space(4))) *ConstFrags;
  unsigned long long frag;
  if (item & kFullTile) {
    frag = (CONST_WORD ? ((ConstFrags)frags)[(size_t)p.tile * TILE_PIXELS] : frags[(size_t)p.tile * TILE_PIXELS]) +
           ((unsigned long long)((uint32_t)p.chunk * 64u + (uint32_t)lane) << 32);
    valid = true;
  } else {
    const uint32_t n_frag = frag_count[p.tile];
    valid = (uint32_t)p.chunk * 64u + (uint32_t)lane < n_frag;
    frag = frags[(size_t)p.tile * TILE_PIXELS + (uint32_t)p.chunk * 64u + (uint32_t)lane];
  }
  return frag;
}

// ------------------------------------------------------------------------------------------------
// k_raster: one workgroup per screen tile.  LDS-resident 64-bit keys (depth bits << 32 | primitive) filled with
// ds_max_u64 -- depth op GREATER_OR_EQUAL with "later primitive wins ties" falls out of the key order -- then
// ballot/popcount compaction of the covered pixels into the tile's fragment list.  Background pixels get the
// clear colour here; covered pixels are coloured by k_shade.
//
// The kernel is latency-bound (bin -> triangle record -> LDS atomics), so the triangle data of up to 256 bin
// entries is staged through LDS by all threads at once: two memory round trips per chunk however the entries
// split over the raster classes, instead of two per loop iteration.  The every-tile list rides along as extra
// "large" entries after a per-tile accept/reject test.
// ------------------------------------------------------------------------------------------------
constexpr int kStage = kTileThreads;  // staged entries per chunk (one per thread)
constexpr uint32_t kBroadSpec = 16;    // every-tile-list entries a light tile fetches before it knows the count
constexpr uint32_t kSkyKept = 1u;      // option "sky_keep": bit 0 of a tile's word = the tile's fill was skipped (stamps are even)

struct StagedTri {  // struct-of-arrays in LDS: thread j owns column j when filling
  int X0[kStage], Y0[kStage], X1[kStage], Y1[kStage], X2[kStage], Y2[kStage];
  float z0[kStage], dzdx[kStage], dzdy[kStage];
  uint32_t ref[kStage];
  uint32_t box[kStage];  // px0 | px1 << 8 | py0 << 16 | py1 << 24 relative to the tile; 0xFFFFFFFF = skip
  BB_DEV void store(int j, const TriCore &t) {
    X0[j] = t.X0; Y0[j] = t.Y0; X1[j] = t.X1; Y1[j] = t.Y1; X2[j] = t.X2; Y2[j] = t.Y2; z0[j] = t.z0; dzdx[j] = t.dzdx; dzdy[j] = t.dzdy;
  }
  BB_DEV TriCore load(int j) const { return TriCore{X0[j], Y0[j], X1[j], Y1[j], X2[j], Y2[j], z0[j], dzdx[j], dzdy[j]}; }
};

// One light as the loop consumes it: 48 bytes, written once per frame by cook_light.
struct CookedLight {
  float px, py, pz;
  int32_t type;
  float cr, cg, cb;  // color * intensity
  float outer;
  float dx, dy, dz;  // type 1: normalize(-dir); type 2: -normalize(dir)
  float inv_eps;     // type 1: 1 / (inner - outer)
};
struct ShadeShared {
  CookedLight lights[kMaxNumLights];
};

BB_DEV CookedLight cook_light(const Light &l) {
  CookedLight c;
  c.px = l.pos[0]; c.py = l.pos[1]; c.pz = l.pos[2];
  c.type = l.type;
  c.cr = l.color[0] * l.intensity; c.cg = l.color[1] * l.intensity; c.cb = l.color[2] * l.intensity;
  c.outer = l.outer_cutoff;
  c.dx = c.dy = c.dz = 0.0f;
  c.inv_eps = 0.0f;
  if (l.type == 1) {
    const f3 d = normalize3(neg3(ld3(l.dir)));
    c.dx = d.x; c.dy = d.y; c.dz = d.z;
    c.inv_eps = bb_rcp(l.inner_cutoff - l.outer_cutoff);
  } else if (l.type == 2) {
    const f3 d = neg3(normalize3(ld3(l.dir)));
    c.dx = d.x; c.dy = d.y; c.dz = d.z;
  }
  return c;
}

// the frame's (or a workgroup's) light table: every thread of the workgroup calls this
template <int THREADS>
BB_DEV void cook_lights(const Light *lights, int n, CookedLight *cooked) {
  for (int li = (int)threadIdx.x; li < n; li += THREADS) cooked[li] = cook_light(lights[li]);
}

// ---- k_raster's phases that are functions (forced inline); why the others are blocks of its body: profiles/r10_raster_phases.txt ----
// SHORT FRAMES: a tile's items go to the frame's list.  In: its chunks of 64 fragments, the full-tile flag.  Out: items[].
// (called by the first wave of the workgroup, all of its lanes; short frames have no heavy rows: blockIdx is the tile's launch slot)
BB_DEV void append_items(uint32_t *item_head, uint32_t *items, int lane, uint32_t chunks, uint32_t flag) {
  uint32_t at = 0u;
  if (lane == 0) at = atomicAdd(item_head, chunks);
  at = (uint32_t)__shfl((int)at, 0);
  if ((uint32_t)lane < chunks) items[1u + at + (uint32_t)lane] = item_word(flag, blockIdx.y, blockIdx.x, (uint32_t)lane);
}
// overlay pass: the gizmo's fragments are lifted above every other depth (see depth_max); 0 everywhere else
template <bool OVERLAY>
BB_DEV uint32_t zbias_of(const FrameParams &fp, uint32_t ref) { return gizmo_ref<OVERLAY>(fp, ref) ? 0x40000000u : 0u; }

// The tile a workgroup of k_raster rasterises.
struct RasterTile {
  int tx, ty;
  uint32_t tile;  // ty * fp.tiles_x + tx
  int x0, y0;     // its first pixel in the frame
  int out_y0;     // the row of that pixel in this rank's output
  PixRect rect;   // its pixels inside the frame
};

// CLEAR.  Out: keys = 0; overlay pass: the depth the scene left behind, low word 0 = "no overlay primitive here".
template <int TILE_W, int TILE_H, bool OVERLAY>
BB_DEV void clear_keys(unsigned long long *keys, const RasterTile &tg, const FrameParams &fp, const float *depth_io, int tid) {
  for (int p = tid; p < TILE_W * TILE_H; p += kTileThreads) {
    unsigned long long k0 = 0ull;
    if (OVERLAY) {  // depth test against what the scene left behind; low word 0 = "no overlay primitive here"
      int x, y;
      tile_pixel<TILE_W>(p, x, y);
      const int gx = tg.x0 + x, gy = tg.y0 + y;
      if (gx < fp.width && gy < fp.height)
        k0 = (unsigned long long)__float_as_uint(depth_io[(size_t)gy * (size_t)fp.width + (size_t)gx]) << 32;
    }
    keys[p] = k0;
  }
}

// LARGE TRIANGLES (class 2 and the every-tile list): one wave per triangle.  In: entries [lo, hi) of the staged chunk that
// begins at entry `base`.  Out: keys.
template <int TILE_W, int TILE_H, bool OVERLAY>
BB_DEV void raster_large(const StagedTri &st, uint32_t lo, uint32_t hi, uint32_t base, const RasterTile &tg, const FrameParams &fp,
                         unsigned long long *keys, int lane, int wave) {
  for (uint32_t e = lo + (uint32_t)wave; e < hi; e += kTileWaves) {
    const int j = __builtin_amdgcn_readfirstlane((int)(e - base));
    if (st.box[j] == 0xFFFFFFFFu) continue;
    const TriCore t = st.load(j);
    const uint32_t ref = st.ref[j];
    // (frame and scissor first, the whole tile second: the order the clamps always had here)
    raster_triangle_wave<TILE_W, TILE_H>(t, ref, intersect(PixRect{0, fp.width - 1, 0, fp.height - 1}, scissor_rect<OVERLAY>(fp, ref)), tg.x0,
                                         tg.y0, keys, lane, zbias_of<OVERLAY>(fp, ref));
  }
}

// A tile's entries in the order they are rasterised: class 0 | class 1 | class 2 | every-tile list.
struct TileEntries {
  uint32_t e1, e2, e3, e_end;  // where class 1, class 2, the every-tile list and the end begin
  const uint32_t *bin0;        // the tile's three bins, bin_cap references each
  uint32_t bin_cap;
  BB_DEV uint32_t fetch_ref(uint32_t e) const {  // bin reference of entry e (0 for the every-tile list and past the end)
    if (e >= e3) return 0u;
    const uint32_t c = e < e1 ? 0u : (e < e2 ? 1u : 2u);
    const uint32_t i = e - (c == 0u ? 0u : (c == 1u ? e1 : e2));
    return bin0[(size_t)c * bin_cap + i];
  }
};
struct Fetched {  // what the staging keeps of an entry
  TriCore core;
  uint32_t ref, clip_slot1;
};
BB_DEV Fetched fetch_tri(const TileEntries &en, uint32_t e, uint32_t ref, const RasterTri *tris, const BroadTri *broad_list) {
  Fetched f = {};
  if (e >= en.e_end) return f;
  const RasterTri *t = e < en.e3 ? &tris[ref >> 3] : &broad_list[e - en.e3].tri;  // binned triangles are never clipped
  f.core = tri_core(*t);
  f.ref = ref;
  if (e >= en.e3) {
    f.ref = broad_list[e - en.e3].ref;
    f.clip_slot1 = broad_list[e - en.e3].pad[0];
  }
  return f;
}

// OVERLAY = true (overlay subpass): the keys start from the scene's resolved depth (`depth_io`, read) instead of 0,
// gizmo primitives are scissored to their rectangle and biased above everything else, pixels no overlay primitive
// wins are left alone (no background fill).  OVERLAY = false with depth_io != nullptr stores the resolved depth.
#ifndef BB_RASTER_WAVES
#define BB_RASTER_WAVES 8  // waves per SIMD the 32 x 32 instantiation is compiled for (64 registers; 20.3 KB of LDS allow eight
                           // workgroups per CU).  64 x 64 tiles hold 32 KB of keys: three.
#endif
template <int TILE_W, int TILE_H, bool OVERLAY = false>
__global__ __launch_bounds__(kTileThreads) __attribute__((amdgpu_waves_per_eu(TILE_W > 32 ? 3 : (OVERLAY ? 7 : BB_RASTER_WAVES)))) void k_raster(
    // (first: what a tile needs before its first load -- these arrive in scalar registers with the wave, "kernarg preload";
    //  the Makefile asks for it.  Everything behind them comes with one scalar load from the kernel-argument segment.)
    uint32_t *__restrict__ tile_count, Counters *__restrict__ ctr, const BroadTri *__restrict__ broad_list,
    uint32_t *__restrict__ frag_count, unsigned long long *__restrict__ frags, float4 *__restrict__ out,
    FrameParams fp, const RasterTri *__restrict__ tris, const ClipSlot *__restrict__ clip_arena,
    const uint32_t *__restrict__ bins,
    uint32_t *__restrict__ vis_prim, float *__restrict__ vis_depth,
    const float4 *__restrict__ background, float *__restrict__ depth_io, uint32_t *__restrict__ host_flags,
    uint32_t *__restrict__ out8, uint32_t *__restrict__ item_groups, uint32_t *__restrict__ item_head,
    uint32_t *__restrict__ items, const Light *__restrict__ lights, int num_lights, CookedLight *__restrict__ cooked,
    const uint32_t *__restrict__ heavy,
    // option "sky_keep" (the light-tile path): the slot's word per tile and this frame's stamp, or nullptr / 0: never keep
    uint32_t *__restrict__ sky_state, uint32_t sky_stamp) {
  constexpr int TILE_PIXELS = TILE_W * TILE_H;
  // ---- the workgroup's LDS ----
  __shared__ unsigned long long keys[TILE_PIXELS];  // depth bits << 32 | reference + 1; 0: nothing drawn
  __shared__ StagedTri st;                          // the chunk being rasterised
  __shared__ uint32_t s_count;                      // the tile's fragments
  // the row list of the chunk's small triangles (see the chunk loop)
  __shared__ uint16_t s_row0[kStage];          // first row of staged entry j in its wave's list
  __shared__ uint32_t s_wave_rows[kTileWaves];  // rows in each wave's list (compaction: covered pixels of each wave)
  // Clipped sub-triangles that touch this tile: (reference, clip-arena slot + 1).  The slot goes into the fragment word,
  // so that k_shade can fetch the sub-triangle's planes together with the primitive record instead of after it.
  // More than kClipRefs of them: the field stays 0 and k_shade finds the slot through the record (one more round trip).
  constexpr uint32_t kClipRefs = 32;
  __shared__ uint32_t s_clip_ref[kClipRefs], s_clip_slot[kClipRefs], s_n_clip_refs;
  __shared__ unsigned long long s_pad_frag;  // the fragment list's first word

  __builtin_amdgcn_s_setprio(3);  // (as k_geometry: a latency-bound wave's instruction goes out when it is ready)
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  // ---- pinned flag words.  In: the frame's counters.  Out: host_flags[] ----
  // This frame's pinned flag words (HostFlagWord, bb_types.h) straight into pinned host memory (final since k_geometry
  // ended): the host looks at them when it reuses the frame's slot -- a few stores instead of a copy kernel on the stream.
  // (kFlagItemCount, the frame's shade item count, is stored by k_shade_items.)
  if (host_flags && blockIdx.x == 0 && blockIdx.y == 0 && tid == 0) {
    host_flags[kFlagOverflow] = ctr->overflow;
    host_flags[kFlagBinNeed] = ctr->bin_need;
    host_flags[kFlagBroadNeed] = ctr->n_broad;
    host_flags[kFlagClipNeed] = ctr->n_clip_slots;
    host_flags[kFlagHeavyTiles] = ctr->n_heavy;   // sizes the heavy rows of this slot's next frame
  }
  // ---- short frames: the light table.  In: lights[].  Out: cooked[] ----
  // SHORT FRAMES (item_head != nullptr; the host decides by the frame's tile count): there is no k_shade_items launch.  The
  // tiles append their items to the frame's list themselves -- one returning atomic per tile on the list's head word, which
  // the frame's staging copy has zeroed -- and this kernel's first workgroup cooks the light table.  A 1080p frame is a
  // chain of dependent kernels whose length over the frames in flight IS its rate; the scan kernel and its boundary were
  // 9 of its 90 us.  The list is then in tile COMPLETION order, not screen order: at 4K that cost 13 % more texel traffic
  // than it saved (round 2), which is why long frames keep k_shade_items.
  if (item_head && cooked && blockIdx.x == 0 && blockIdx.y == 0)
    cook_lights<kTileThreads>(lights, num_lights, cooked);
  static_assert(TILE_PIXELS / 64 <= 64, "a tile's items are written by one wave");
  // ---- launch slot -> tile.  In: blockIdx, the heavy list.  Out: slot, heavy_slot / heavy_class, tg; or the workgroup leaves ----
  // plain row order ...
  uint32_t slot = blockIdx.y * gridDim.x + blockIdx.x;
  // ... behind fp.heavy_rows rows of HEAVY SLOTS (long frames only).  A tile's life is 1.6 us when nothing is binned to it and
  // 14-39 us when a ball is; in plain screen order the last heavy tile starts when the kernel's work is half done and the
  // launch ends in a tail as long as that tile.  k_geometry lists the tiles whose bins reach fp.heavy_threshold references
  // (launch slot | class << 30, at most one entry per class and tile); the workgroups of the first rows take one entry each
  // and rasterise THAT tile, and the tile's own workgroup, which sees the same final counts, leaves at once.  Which entry
  // of a tile listed twice does the work follows from the counts too (the highest class at the threshold), so nobody has to
  // claim anything.  The rows are sized by the host from the list length of the slot's previous frame; a list longer than
  // the rows is not used at all -- every decision is all-or-nothing on values that are final since k_geometry ended.
  const uint32_t heavy_slots = (uint32_t)fp.heavy_rows * gridDim.x;
  bool heavy_slot = false;
  uint32_t heavy_class = 0u;
  if (!OVERLAY && fp.heavy_rows) {
    if (blockIdx.y < (uint32_t)fp.heavy_rows) {
      const uint32_t n_heavy = ctr->n_heavy;
      if (slot >= n_heavy || n_heavy > heavy_slots) return;
      const uint32_t e = heavy[slot];
      heavy_class = e >> 30;
      slot = e & 0x3FFFFFFFu;
      heavy_slot = true;
    } else {
      slot -= heavy_slots;
    }
  }
  const int grid_row = (int)(slot / gridDim.x);
  const int tx = (int)(slot - (uint32_t)grid_row * gridDim.x);
  int ty, out_tile_row;
  const bool live = tile_row(fp, grid_row, ty, out_tile_row);
  if (!live) return;
  const int tile_x0 = tx * TILE_W, tile_y0 = ty * TILE_H;
  const RasterTile tg = {tx, ty, (uint32_t)ty * (uint32_t)fp.tiles_x + (uint32_t)tx, tile_x0, tile_y0, out_tile_row * TILE_H,
                         PixRect{tile_x0, min(tile_x0 + TILE_W, fp.width) - 1, tile_y0, min(tile_y0 + TILE_H, fp.height) - 1}};
#ifdef BB_STAMPS
#define BB_RSTAMP(i) do { if (tid == 0) reinterpret_cast<unsigned long long *>(frag_count + fp.tiles_x * fp.tiles_y)[tg.tile * 8 + (i)] = wall_clock64(); } while (0)
#else
#define BB_RSTAMP(i) do { } while (0)
#endif
  BB_RSTAMP(0);

  // ---- the tile's counts.  In: tile_count[], ctr.  Out: n_cls[], n_broad; or the workgroup leaves (a heavy slot does the tile) ----
  // The tile's bin counts: every thread reads them itself (uniform address: one line), decides with them, and only AFTER
  // the workgroup's first barrier are they cleared for the slot's next frame -- a wave arrives at that barrier with its
  // loads returned, so no wave, however late it started, can see the cleared value.  (Cleared right after the read, a
  // late wave disagreed with its workgroup about the loop bounds: ~100 wrong pixels in one frame of a few hundred
  // whenever other processes shared the GPU.)
  uint32_t n_cls[kBinClasses];
  bool at_threshold[kBinClasses];
#pragma unroll
  for (uint32_t c = 0; c < kBinClasses; ++c) {
    const uint32_t raw = tile_count[tg.tile * kBinClasses + c];
    at_threshold[c] = raw >= fp.heavy_threshold;
    n_cls[c] = BB_ABLATE(1u | (256u << c)) ? 0u : min(raw, fp.bin_cap);
  }
  // A frame whose every-tile list overflowed (bit 1 of ctr->overflow, final since k_geometry ended) is rendered again after
  // the host has grown the list: the clip path reserves a run of entries and writes none of them when the run does not
  // fit, so a prefix of the list may hold entries never written this frame -- the overflowed frame takes none of it.
  // (Both counter words are read unconditionally and combined without a branch -- ONE round trip, together with the bin
  //  counts above, in front of the tile's first decision.  As `overflow & 2 ? 0 : n_broad` the compiler made the second
  //  load wait for the first.)
  const uint32_t ctr_overflow = ctr->overflow, ctr_n_broad = ctr->n_broad, ctr_n_heavy = ctr->n_heavy;
  // SKY KEEP (option "sky_keep"; main passes into the slot's own fp32 frame only, the host decides: bibim_hip.hip, sky_stamp_for).
  // One word per tile, the slot's: sky_stamp (+ kSkyKept) says that every in-frame pixel of the tile, in the buffer this slot's
  // frames go to, holds the clear colour -- the light path below left it so in an earlier frame under the same stamp, and
  // nothing has written the buffer since (whatever does makes the host hand out a fresh stamp: no word can equal it).  Such
  // a tile's 16 KB of background stores are not issued again.  Every other way a tile is finished leaves 0, which no stamp
  // is.  The word travels with the counts above (the same round trip); it is stored by one thread, and only where it changes.
  uint32_t sky = 0u;
  const bool sky_on = !OVERLAY && sky_state != nullptr && sky_stamp != 0u;
  if (sky_on) sky = sky_state[tg.tile];
  auto sky_word = [&](uint32_t want) {  // (thread 0)
    if (sky_on && sky != want) sky_state[tg.tile] = want;
  };
  const uint32_t n_broad = BB_ABLATE(5u) ? 0u : (min(ctr_n_broad, fp.broad_cap) & (((ctr_overflow >> 1) & 1u) - 1u));
  if (!OVERLAY && fp.heavy_rows) {
    if (heavy_slot) {   // (the list is in use, or this workgroup had left above)
      const uint32_t top = at_threshold[2] ? 2u : (at_threshold[1] ? 1u : 0u);
      if (heavy_class != top) return;                          // the tile's other entry does it
    } else if ((at_threshold[0] || at_threshold[1] || at_threshold[2]) && ctr_n_heavy <= heavy_slots) {
      return;                                                  // a heavy slot does it (or has done it)
    }
  }

  // the pixel's colour when no geometry covers it.  forward: the clear colour (src/main.cpp:84); deferred: brdf.frag on the
  // cleared G-buffer texel (k_deferred_background); fused presentation: the same colours as presented pixels (the clear
  // colour presents as (0, 0, 0, 255))
  // (read ONCE, with the tile's first loads: inside store_background it was a scalar load and a wait per pixel pass)
  float4 bg = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
  uint32_t bg8 = 0xFF000000u;
  if (background) {
    bg = background[0];
    bg8 = __float_as_uint(background[1].x);
    // (uniform values: kept in scalar registers -- five vector registers that would otherwise live through the whole chunk loop)
    bg.x = __uint_as_float((uint32_t)__builtin_amdgcn_readfirstlane((int)__float_as_uint(bg.x)));
    bg.y = __uint_as_float((uint32_t)__builtin_amdgcn_readfirstlane((int)__float_as_uint(bg.y)));
    bg.z = __uint_as_float((uint32_t)__builtin_amdgcn_readfirstlane((int)__float_as_uint(bg.z)));
    bg.w = __uint_as_float((uint32_t)__builtin_amdgcn_readfirstlane((int)__float_as_uint(bg.w)));
    bg8 = (uint32_t)__builtin_amdgcn_readfirstlane((int)bg8);
  }
  auto store_background = [&](int x, int y) {
    const size_t o = (size_t)(tg.out_y0 + y) * (size_t)fp.width + (size_t)(tg.x0 + x);
    if (out8) store_pixel(&out8[o], bg8);
    else store_pixel(&out[o], bg);
  };

  // ---- light tiles: no LDS, no barrier.  In: the counts, <= 64 every-tile entries.  Out: background or ONE fragment word ----
  // Most tiles of a frame hold no binned triangle at all: sky, or ground that ONE huge (every-tile-list) triangle covers
  // completely -- 6595 of C3's 8160.  Each of the four waves settles that by itself from the same uniform data (the bin
  // counts above and a classification of the <= 64 list entries, one per lane), so the workgroup agrees without talking:
  //   nothing touches the tile       -> its pixels get the background colour, its fragment count is 0
  //   one triangle covers all of it  -> every pixel's winner is known without a depth atomic: the fragment list is ONE
  //                                     word and the count carries kFullTile (k_shade makes the 64 fragment words of an
  //                                     item from the lane index)
  // and the workgroup is gone after two memory round trips.  Through the general path below these tiles lived 4.8 us each
  // (8 KB of keys cleared, a barrier, one staged entry, another barrier: in-kernel stamps) and held 28 % of the frame's
  // wave-slot time between them.  Anything else falls through.
  // (The first kBroadSpec entries of the every-tile list are fetched BEFORE the counts have arrived -- the list always has
  //  that many entries allocated, and zero-filled ones can touch no tile -- so that a light tile is ONE memory round trip:
  //  counts and entries come back together.  A frame with more entries fetches the rest behind the count.)
  BroadTri spec;
  if (!OVERLAY && (uint32_t)lane < kBroadSpec) spec = broad_list[lane];
  if (!OVERLAY && !vis_prim && !depth_io && (n_cls[0] | n_cls[1] | n_cls[2]) == 0u && n_broad <= 64u) {
    bool ok = false, full = false;
    uint32_t ref = 0u, clip_slot1 = 0u;
    if ((uint32_t)lane < n_broad) {
      BroadTri b;
      if ((uint32_t)lane < kBroadSpec) b = spec;
      else b = broad_list[lane];
      const TriCore t = tri_core(b.tri);
      ref = b.ref;
      clip_slot1 = b.pad[0];
      const PixRect box = pixel_box(t, tg.rect);
      const int w = box.x1 - box.x0 + 1, h = box.y1 - box.y0 + 1;  // (in front of the test on purpose)
      if (box.any()) {
        const int cls_rect = classify_rect(edge_setup(t), box);
        ok = cls_rect != 0;
        full = cls_rect == 2 && w == TILE_W && h == TILE_H;
      }
    }
    const unsigned long long m_ok = __ballot(ok);
    if (m_ok == 0ull) {
      const bool keep = sky_on && (sky & ~kSkyKept) == sky_stamp;
      if (tid == 0) {
        frag_count[tg.tile] = 0u;
        sky_word(keep ? sky_stamp | kSkyKept : sky_stamp);
      }
      if (keep) return;   // (diagnostic build: no stamps for a kept tile)
      // the same pixels in the same order as `for (p = tid; p < TILE_PIXELS; p += kTileThreads) tile_pixel(p)` would visit them,
      // without that function's arithmetic per pixel: pass k of thread tid is pixel (x, y + k * STEP) of the tile
      // (kTileThreads = 256 pixels = 4 blocks of 8 x 8 = a strip TILE_W wide or, for 64-pixel tiles, half of one)
      constexpr int BX = TILE_W / 8;                      // 8 x 8 blocks per row of blocks
      constexpr int PASSES = TILE_PIXELS / kTileThreads;
      static_assert((kTileThreads / 64) % BX == 0 || BX % (kTileThreads / 64) == 0, "fill pattern");
#pragma unroll
      for (int k = 0; k < PASSES; ++k) {
        const int block = (tid >> 6) + k * (kTileThreads / 64);
        const int x = (block % BX) * 8 + (tid & 7), y = (block / BX) * 8 + ((tid >> 3) & 7);
        if (tg.x0 + x < fp.width && tg.y0 + y < fp.height) store_background(x, y);
      }
      BB_RSTAMP(1); BB_RSTAMP(2); BB_RSTAMP(3); BB_RSTAMP(4);   // (diagnostic build: a light tile's phases all end here)
      return;
    }
    if (__popcll(m_ok) == 1 && __ballot(full) == m_ok) {
      if (tid == 0) {
        const int src = __ffsll((long long)m_ok) - 1;
        // the whole list: 8 bytes instead of 8 KB (pixel field 0: fetch_fragment adds the lane's own)
        frags[(size_t)tg.tile * TILE_PIXELS] = fragment_word((uint32_t)__builtin_amdgcn_readlane((int)clip_slot1, src), 0u,
                                                          (uint32_t)__builtin_amdgcn_readlane((int)ref, src));
        frag_count[tg.tile] = (uint32_t)TILE_PIXELS | kFullTile;
        sky_word(0u);
        if (item_groups) atomicAdd(&item_groups[(slot / kItemGroupSlots) * kItemGroupStride], (uint32_t)(TILE_PIXELS / 64));
      }
      if (item_head && wave == 0) append_items(item_head, items, lane, (uint32_t)(TILE_PIXELS / 64), kFullTile);
      BB_RSTAMP(1); BB_RSTAMP(2); BB_RSTAMP(3); BB_RSTAMP(4);   // (diagnostic build: a light tile's phases all end here)
      return;
    }
  }

  // ---- clear.  Out: keys, s_count, s_n_clip_refs; behind the barrier the tile's bin counts ----
  clear_keys<TILE_W, TILE_H, OVERLAY>(keys, tg, fp, depth_io, tid);
  if (tid == 0) {
    sky_word(0u);  // (the general path, a heavy slot's tile included: its pixels are no longer all background)
    s_count = 0;
    s_n_clip_refs = 0;
  }
  __syncthreads();  // keys cleared; every wave has its copy of the counts
  // (a tile rasterised from a heavy slot keeps its counts: its own workgroup may not have looked at them yet.  k_shade_items
  //  clears them.)
  if (!heavy_slot && tid < (int)kBinClasses && (tid == 0 ? n_cls[0] : (tid == 1 ? n_cls[1] : n_cls[2])))
    tile_count[tg.tile * kBinClasses + tid] = 0;  // ready for the slot's next frame

  // entry order: class 0 | class 1 | class 2 | every-tile list
  const uint32_t e1 = n_cls[0], e2 = e1 + n_cls[1], e3 = e2 + n_cls[2], e_end = e3 + n_broad;
  const uint32_t *bin0 = bins + (size_t)(tg.tile * kBinClasses) * fp.bin_cap;

  BB_RSTAMP(1);
  // ---- the chunk loop: up to kStage entries at a time ----
  // An entry is fetched in two dependent trips (bin reference -> triangle record; an every-tile entry in one).  Both run
  // AHEAD of the chunk they belong to: the references of chunk k + 2 and the triangles of chunk k + 1 are asked for before
  // chunk k is rasterised, so a tile with several chunks (a far ball puts 2500 tiny triangles into one tile: ten chunks)
  // pays the two trips once, not once per chunk -- they had been the critical path of the frame's heaviest tiles.
  const TileEntries en = {e1, e2, e3, e_end, bin0, fp.bin_cap};
  uint32_t ref_next = en.fetch_ref((uint32_t)tid + (uint32_t)kStage);
  Fetched cur = fetch_tri(en, (uint32_t)tid, en.fetch_ref((uint32_t)tid), tris, broad_list);
  for (uint32_t base = 0; base < e_end; base += kStage) {
    if (base) __syncthreads();  // previous chunk consumed
    // ---- stage: every thread files one entry; the rows of the small triangles (classes 0 and 1) are counted ----
    // In: cur.  Out: column tid of st (box 0xFFFFFFFF: nothing to draw), the clip references, s_row0[tid], s_wave_rows[wave]
    {
      const uint32_t e = base + (uint32_t)tid;
      uint32_t box = 0xFFFFFFFFu;
      int rows = 0;
      if (e < e_end) {
        const Fetched &t = cur;
        // (only the gizmo is intersected with its scissor: the main passes keep their two clamps per bound)
        const PixRect b = pixel_box(t.core, gizmo_ref<OVERLAY>(fp, t.ref) ? intersect(tg.rect, scissor_rect<OVERLAY>(fp, t.ref)) : tg.rect);
        const int px0 = b.x0, px1 = b.x1, py0 = b.y0, py1 = b.y1;
        bool ok = b.any();
        if (ok && e >= e3) ok = classify_rect(edge_setup(t.core), b) != 0;  // every-tile list: accept / reject
        if (ok) {
          if (t.clip_slot1) {
            const uint32_t k = atomicAdd(&s_n_clip_refs, 1u);
            if (k < kClipRefs) {
              s_clip_ref[k] = t.ref;
              s_clip_slot[k] = t.clip_slot1;
            }
          }
          box = (uint32_t)(px0 - tg.x0) | ((uint32_t)(px1 - tg.x0) << 8) | ((uint32_t)(py0 - tg.y0) << 16) |
                ((uint32_t)(py1 - tg.y0) << 24);
          st.store(tid, t.core);
          st.ref[tid] = t.ref;
          if (e < e2) rows = py1 - py0 + 1;
        }
      }
      st.box[tid] = box;
      // The rows of the wave's small triangles, as one list per wave: lane l's rows are items [first, first + rows) of it.
      // (exclusive prefix sum over the wave, bit-sliced: rows <= TILE_H needs seven ballots and mbcnt pairs -- no LDS traffic, no
      //  shuffle addresses to keep in registers)
      int first = 0;
      uint32_t wave_rows = 0u;
#pragma unroll
      for (int b = 0; (1 << b) <= TILE_H; ++b) {
        const unsigned long long m = __ballot(((rows >> b) & 1) != 0);
        first += (int)(__builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0u)) << b);
        wave_rows += (uint32_t)__popcll(m) << b;
      }
      s_row0[tid] = (uint16_t)first;
      if (lane == 0) s_wave_rows[wave] = wave_rows;
    }
    __syncthreads();
    if (base == 0) BB_RSTAMP(2);
    const uint32_t hi = min(base + (uint32_t)kStage, e_end);
    raster_large<TILE_W, TILE_H, OVERLAY>(st, max(base, e2), hi, base, tg, fp, keys, lane, wave);
    // (behind the wave-per-triangle loop, whose 64-bit edge functions need the registers)
    // the next chunk's triangles and the references of the one after it: in flight while this chunk is rasterised
    const uint32_t e_next = base + (uint32_t)kStage + (uint32_t)tid;
    cur = fetch_tri(en, e_next, ref_next, tris, broad_list);
    ref_next = en.fetch_ref(e_next + (uint32_t)kStage);
    // ---- the row list, classes 0 and 1 (small triangles): one ROW of one triangle per lane.  In: st, s_row0, s_wave_rows.  Out: keys ----
    // Round 4 gave a tiny triangle one lane (its whole bounding box, pixel by pixel: 16 % of the lanes busy) and a small one
    // sixteen lanes (4 x 4 pixel blocks over its box, a 70-instruction edge setup repeated in each of them: 56 % busy); a tile's
    // life was the life of its unluckiest lane group.  Now the rows of all of them are one list and the 256 threads take rows
    // from it in turn: every lane has work of the same kind whatever the triangle's size, consecutive lanes hold consecutive
    // rows of one triangle (the triangle's words are LDS broadcasts, the rows about equally long), and a row's setup is
    // paid once per row, not per 4 x 4 block.  Same pixels, same keys: the edge functions and the depth expression are
    // the ones of the 64-bit form.
    {
      const uint32_t r0 = s_wave_rows[0], r1 = r0 + s_wave_rows[1], r2 = r1 + s_wave_rows[2], r3 = r2 + s_wave_rows[3];
      static_assert(kTileWaves == 4, "row list: four wave regions");
      for (uint32_t i = (uint32_t)tid; i < r3; i += kTileThreads) {
        const uint32_t w = (i >= r0 ? 1u : 0u) + (i >= r1 ? 1u : 0u) + (i >= r2 ? 1u : 0u);
        const uint32_t local = i - (w == 0u ? 0u : (w == 1u ? r0 : (w == 2u ? r1 : r2)));
        // whose row: the last entry of wave w's 64 whose first row is <= local (entries without rows share their successor's
        // first row, so the last one is the one that has it)
        int j = (int)(w * 64u);
#pragma unroll
        for (int step = 32; step; step >>= 1)
          if ((uint32_t)s_row0[j + step] <= local) j += step;
        const uint32_t box = st.box[j];
        const int py = tg.y0 + (int)((box >> 16) & 255u) + (int)(local - (uint32_t)s_row0[j]);
        const uint32_t ref = st.ref[j];
        raster_triangle_row<TILE_W>(st.load(j), ref, tg.x0 + (int)(box & 255u), tg.x0 + (int)((box >> 8) & 255u), py, tg.x0, tg.y0,
                                    keys, zbias_of<OVERLAY>(fp, ref));
      }
    }
  }
  __syncthreads();
  BB_RSTAMP(3);

  // ---- compaction: covered pixels -> fragment list (ballot + popcount prefix); background written here ----
  // In: keys, the clip references.  Out: my_frags[] padded to a multiple of 64, s_count, background / visibility / depth pixels
  unsigned long long *my_frags = frags + (size_t)tg.tile * TILE_PIXELS;
  const uint32_t n_clip_refs = s_n_clip_refs <= kClipRefs ? s_n_clip_refs : 0u;  // too many: k_shade looks the slots up
  // (The wave counts the covered pixels of ALL its passes first and gets the place of its run from a prefix over the four
  //  waves' totals -- no atomic at all; round 4 reserved per pass, four dependent returning LDS atomics per wave of every ball tile.)
  constexpr int PASSES = TILE_PIXELS / kTileThreads;
  unsigned long long pass_mask[PASSES];
  uint32_t wave_total = 0u;
  // Which 8 x 8 block of the tile a wave takes in pass k: CONSECUTIVE blocks (for 32-pixel tiles a row of four, a 32 x 8 strip).
  // The wave's covered pixels go into the fragment list as one run, 64 consecutive fragments are an item of k_shade and
  // four consecutive items a workgroup (one CU; the next workgroup is on the next XCD): with the runs in wave order (below)
  // workgroup j of a tile shades strip j, in every tile and every frame.  Measured with the runs in wave order, k_shade's
  // fetch traffic per launch (FETCH_SIZE, KiB, C3): strips 53.8 k -- what round 4's one-atomic-per-pass compaction had --, a
  // quarter of the tile per wave 62.2 k, a column of blocks per wave 67.1 k (gpurun_out/r5/t12_*).
  auto pass_pixel = [&](int k) -> int { return (wave * PASSES + k) * 64 + lane; };
#pragma unroll
  for (int k = 0; k < PASSES; ++k) {
    const int p = pass_pixel(k);
    int x, y;
    tile_pixel<TILE_W>(p, x, y);
    const bool in_frame = tg.x0 + x < fp.width && tg.y0 + y < fp.height;
    const unsigned long long key = keys[p];
    pass_mask[k] = __ballot(in_frame && (OVERLAY ? (uint32_t)key != 0u : key != 0ull));
    wave_total += (uint32_t)__popcll(pass_mask[k]);
  }
  // The four runs stand in the list in WAVE order -- an exclusive prefix over the waves' totals through LDS, one more barrier
  // -- not in the order in which four atomics happen to arrive: the fragment list of a tile is then the same from frame to
  // frame, and so is which of k_shade's workgroups (which XCD, which L2) shades which part of the tile.  With a returning
  // atomic per wave the runs came in any order and k_shade's fetch traffic rose by a fifth (the same L1 misses, more of them
  // L2 misses: neighbouring tiles no longer sent their shared texel lines to the same L2s).
  if (lane == 0) s_wave_rows[wave] = wave_total;   // (the row list's totals are done with: behind the chunk loop's last barrier)
  __syncthreads();
  uint32_t wave_base = 0u;
#pragma unroll
  for (int w = 0; w < kTileWaves; ++w) wave_base += w < wave ? s_wave_rows[w] : 0u;
  if (tid == 0) s_count = s_wave_rows[0] + s_wave_rows[1] + s_wave_rows[2] + s_wave_rows[3];
#pragma unroll
  for (int k = 0; k < PASSES; ++k) {
    int p = pass_pixel(k);
    int x, y;
    tile_pixel<TILE_W>(p, x, y);
    int gx = tg.x0 + x, gy = tg.y0 + y;
    bool in_frame = gx < fp.width && gy < fp.height;
    unsigned long long key = keys[p];
    // main passes: any key; overlay pass: only pixels an overlay primitive won (low word = reference + 1)
    const unsigned long long mask = pass_mask[k];
    const bool covered = ((mask >> lane) & 1ull) != 0ull;
    if (covered) {
      uint32_t rank_in_wave = (uint32_t)__popcll(mask & ((1ull << lane) - 1ull));
      const uint32_t ref = (uint32_t)key - 1u;
      uint32_t clip_slot1 = 0u;
      for (uint32_t k = 0; k < n_clip_refs; ++k)  // (uniform trip count: a handful of clipped sub-triangles per tile at most)
        if (s_clip_ref[k] == ref) clip_slot1 = s_clip_slot[k];
      const unsigned long long fw = fragment_word(clip_slot1, (uint32_t)p, ref);
      my_frags[wave_base + rank_in_wave] = fw;
      if (wave_base + rank_in_wave == 0u) s_pad_frag = fw;  // the list's first fragment doubles as its padding (below)
    } else if (in_frame && !OVERLAY) {
      store_background(x, y);
    }
    wave_base += (uint32_t)__popcll(mask);
    if (vis_prim && in_frame) {
      size_t o = (size_t)gy * (size_t)fp.width + (size_t)gx;
      vis_prim[o] = key ? (((uint32_t)key - 1u) >> 3) : 0xFFFFFFFFu;
      vis_depth[o] = __uint_as_float((uint32_t)(key >> 32));
    }
    // the resolved depth, kept for the overlay subpass (option "overlays")
    if (!OVERLAY && depth_io && in_frame) depth_io[(size_t)gy * (size_t)fp.width + (size_t)gx] = __uint_as_float((uint32_t)(key >> 32));
  }
  __syncthreads();
  // k_shade works in units of 64 fragments and loads them before it knows the count: the list is padded to a multiple of
  // 64 with copies of its first fragment (the copies are shaded again and not stored).
  {
    const uint32_t n = s_count;
    if (n != 0u && (n & 63u) != 0u && tid < (int)(64u - (n & 63u))) my_frags[n + (uint32_t)tid] = s_pad_frag;
  }
  if (tid == 0) {
    frag_count[tg.tile] = s_count;  // (N_shaded = sum of these, taken on the host on demand)
    // 64-fragment chunks per group of 256 launch slots: what k_shade_items needs to place this group's items
    if (item_groups && s_count) atomicAdd(&item_groups[(slot / kItemGroupSlots) * kItemGroupStride], (s_count + 63u) >> 6);
  }
  if (item_head && wave == 0 && s_count) append_items(item_head, items, lane, (s_count + 63u) >> 6, 0u);
  BB_RSTAMP(4);
  if (tid == 0) {
    BB_RSTAMP(5);
#ifdef BB_STAMPS
    reinterpret_cast<unsigned long long *>(frag_count + fp.tiles_x * fp.tiles_y)[tg.tile * 8 + 6] =
        ((unsigned long long)e_end << 32) | s_count;
    reinterpret_cast<unsigned long long *>(frag_count + fp.tiles_x * fp.tiles_y)[tg.tile * 8 + 7] =
        (unsigned long long)n_cls[0] | ((unsigned long long)n_cls[1] << 16) | ((unsigned long long)n_cls[2] << 32) |
        ((unsigned long long)n_broad << 48);
#endif
  }
}

// The light loop and the ambient term: forward_brdf.frag:27-75 == brdf.frag:26-72 (same statements), on a surface
// point given by position, (unnormalised) normal, albedo, metallic, roughness, ao.
//
// Evaluation order = the CPU checker's "contract" form of the light loop, bit for bit.  Everything that feeds the
// one ill-conditioned quantity of the shader, the GGX denominator q = NdotH^2 (a^2 - 1) + 1, follows the GLSL statement
// by statement (V, N, L, att, H, NdotH); the well-conditioned products behind it are re-associated:
//   D G / max(4 NdotV NdotL, .001) = (a2 NdotV NdotL) / ((q q) (PI dV dL) sden)   one reciprocal instead of four
//   kD albedo / PI                 = (1 - F) ((1 - metallic) albedo / PI)         hoisted out of the loop
//   radiance NdotL                 = (color intensity) (att NdotL)                color * intensity once per light
//   max(N.V, 0), max(N.L, 0), max(H.V, 0) = saturate(...)   the three cosines that do not feed q: differs only where
//                                                           rounding puts a cosine of unit vectors above 1 (<= 2 ulp)
// Why the shape matters on gfx950 (tools/microbench/issue_rate.hip, profiles/r02_issue_rate.txt): with two or more waves on
// a SIMD, v_fma/mul/add_f32 issue every 2.05-2.4 cycles -- also with one scalar-register operand (row iso_fma_sgpr_operand:
// 2.7) -- while v_max / v_cmp / conversions cost ~4, a transcendental 13 and a packed, DPP or 24-bit-multiply instruction in
// a stream of plain ones 9-10.  Per-light constants are cooked once per FRAME (k_shade_items) and reach k_shade's loop through
// the scalar cache (ConstLights below: s_load into scalar registers, the light's type already a scalar); only
// k_deferred_background still stages them in LDS (LdsLights).
// ------------------------------------------------------------------------------------------------

// Where the light loop finds its cooked lights.
//  * LdsLights: a table staged by the workgroup itself (cook_lights + barrier): k_deferred_background.
//  * ConstLights: the frame's table in global memory, cooked once per frame by k_shade_items and read through the SCALAR
//    cache (constant address space -> s_load into scalar registers): k_shade.  No LDS, no staging code, and above all no
//    workgroup barrier in front of the light loop -- the four waves of a workgroup never wait for each other, and a light's
//    type is already a scalar (no v_readfirstlane, 9 issue cycles each).  The price: a VALU instruction that reads one of
//    the light's fields takes it as its one scalar operand.
struct LdsLights {
  const ShadeShared &sh;
  BB_DEV CookedLight get(int li) const { return sh.lights[li]; }
  BB_DEV static int type_of(const CookedLight &c) { return __builtin_amdgcn_readfirstlane(c.type); }
};
typedef const CookedLight __attribute__((address_space(4))) *ConstCooked;
struct ConstLights {
  ConstCooked table;
  BB_DEV CookedLight get(int li) const {
    ConstCooked c = table + li;
    CookedLight o;
    o.px = c->px; o.py = c->py; o.pz = c->pz; o.type = c->type;
    o.cr = c->cr; o.cg = c->cg; o.cb = c->cb; o.outer = c->outer;
    o.dx = c->dx; o.dy = c->dy; o.dz = c->dz; o.inv_eps = c->inv_eps;
    return o;
  }
  BB_DEV static int type_of(const CookedLight &c) { return c.type; }
};

// `skip(li)`: this fragment takes nothing from light li (option "shadow_map": the caster's iteration of a shadowed fragment).
// `skip.colour(li, cr, cg, cb)`: the cooked colour iteration li runs with (option "shadow_filter": the caster's, scaled, for a
// fragment whose taps are partly lit).  The default skips nothing, changes nothing and leaves no trace in the code.
struct NoSkip {
  BB_DEV bool operator()(int) const { return false; }
  BB_DEV void colour(int, float &, float &, float &) const {}
};
template <typename Lights, class Skip = NoSkip>
BB_DEV float4 light_surface(const ShadeParams &sp, const Lights lights, f3 P, f3 normal, f3 albedo, float metallic,
                            float roughness, float ao, const Skip skip = Skip{}) {
  // per-pixel invariants
  const f3 V = normalize3(sub3(mk3(sp.view_pos[0], sp.view_pos[1], sp.view_pos[2]), P));
  const f3 N = normalize3(normal);
  const float NdotV = sat01(dot3(V, N));
  const float rr = roughness + 1.0f;
  const float kk = (rr * rr) * 0.125f, omk = 1.0f - kk;
  const float pidV = kPi * fmaf(NdotV, omk, kk);
  const float a = roughness * roughness, a2 = a * a, a2m1 = a2 - 1.0f;
  const float a2nv = a2 * NdotV, c4 = 4.0f * NdotV;
  const f3 F0 = mk3(mixf(0.04f, albedo.x, metallic), mixf(0.04f, albedo.y, metallic), mixf(0.04f, albedo.z, metallic));
  const f3 omF0 = mk3(1.0f - F0.x, 1.0f - F0.y, 1.0f - F0.z);
  const float om = 1.0f - metallic;
  const f3 kda = mk3((om * albedo.x) * kInvPi, (om * albedo.y) * kInvPi, (om * albedo.z) * kInvPi);

  f3 Lo = mk3(0.0f, 0.0f, 0.0f);
  // The next light is fetched one iteration ahead (LDS broadcasts / scalar loads), so the loop never waits for it.
  CookedLight nxt = {};
  if (sp.num_lights > 0) nxt = lights.get(0);
  for (int li = 0; li < sp.num_lights; ++li) {
    const CookedLight cl = nxt;
    const float px = cl.px, py = cl.py, pz = cl.pz;
    float cr = cl.cr, cg = cl.cg, cb = cl.cb;
    const int type = Lights::type_of(cl);
    nxt = lights.get(li + 1 < sp.num_lights ? li + 1 : li);
    if (skip(li)) continue;  // (as an unknown type, below: nothing)
    skip.colour(li, cr, cg, cb);
    f3 L;
    float att;
    if (type == 0 || type == 1) {
      const f3 Lv = sub3(mk3(px, py, pz), P);
      const float inv_d = bb_rsqrt(dot3(Lv, Lv));
      att = inv_d * inv_d;
      L = scale3(Lv, inv_d);
      if (type == 1) att *= clamp01((dot3(L, mk3(cl.dx, cl.dy, cl.dz)) - cl.outer) * cl.inv_eps);
    } else if (type == 2) {
      L = mk3(cl.dx, cl.dy, cl.dz);
      att = 1.0f;
    } else {
      continue;  // upstream leaves L / att uninitialised; the contract contributes nothing
    }
    const f3 H = normalize3(add3(L, V));
    const float NdotH = max0(dot3(N, H));
    const float q = fmaf(NdotH * NdotH, a2m1, 1.0f);
    const float x = 1.0f - sat01(dot3(H, V));
    const float x2 = x * x;
    const float p5 = (x2 * x2) * x;
    const float NdotL = sat01(dot3(N, L));
    const float dL = fmaf(NdotL, omk, kk);
    const float sden = __builtin_fmaxf(c4 * NdotL, 0.001f);  // NaN -> 0.001
    const float den = ((q * q) * (pidV * dL)) * sden;
    const float S = (a2nv * NdotL) * bb_rcp(den);
    const f3 F = mk3(fmaf(omF0.x, p5, F0.x), fmaf(omF0.y, p5, F0.y), fmaf(omF0.z, p5, F0.z));
    const float rl = att * NdotL;
    Lo.x = fmaf(fmaf(1.0f - F.x, kda.x, F.x * S), cr * rl, Lo.x);
    Lo.y = fmaf(fmaf(1.0f - F.y, kda.y, F.y * S), cg * rl, Lo.y);
    Lo.z = fmaf(fmaf(1.0f - F.z, kda.z, F.z * S), cb * rl, Lo.z);
  }
  float4 color;
  color.x = fmaf(0.03f * albedo.x, ao, Lo.x);
  color.y = fmaf(0.03f * albedo.y, ao, Lo.y);
  color.z = fmaf(0.03f * albedo.z, ao, Lo.z);
  color.w = 1.0f;
  return color;
}

// Deferred path: brdf.frag runs on every pixel of its full-screen triangle (src/main.cpp:101-104), also where the
// G-buffer still holds its clear value 0; that colour is the same for all such pixels (it depends on the lights and
// the camera only -- and is not always 0: a light at the world origin makes it NaN), so it is evaluated once.
constexpr int kBackgroundThreads = 64;
__global__ __launch_bounds__(kBackgroundThreads) void k_deferred_background(ShadeParams sp, const Light *__restrict__ lights,
                                                                            float4 *__restrict__ out,
                                                                            const SrgbTables *__restrict__ tables, int gbuffer_view) {
  __shared__ ShadeShared sh;
  cook_lights<kBackgroundThreads>(lights, sp.num_lights, sh.lights);
  __syncthreads();
  if (threadIdx.x == 0 && blockIdx.x == 0) {
    // (buffer_visualize.frag on a cleared texel: rgb 0, alpha 1)
    const float4 c = gbuffer_view >= 0 ? make_float4(0.f, 0.f, 0.f, 1.f)
                                       : light_surface(sp, LdsLights{sh}, mk3(0.f, 0.f, 0.f), mk3(0.f, 0.f, 0.f), mk3(0.f, 0.f, 0.f), 0.f, 0.f, 0.f);
    out[0] = c;
    // out[1].x: the same colour as a presented pixel (fused presentation)
    if (tables) out[1] = make_float4(__uint_as_float(present_pixel(c.x, c.y, c.z, *tables, sp.tone_enable, sp.exposure, 1)), 0.f, 0.f, 0.f);
  }
}

// ------------------------------------------------------------------------------------------------
// k_shade_items: the work list of k_shade.  One item = 64 consecutive fragments of one tile's list; k_shade runs one
// wave per item (no wave for an empty part of a tile, none half empty).  items[0] = number of items, items[1 + j] =
// full-tile flag << 31 | grid row << 18 | tile column << 6 | chunk of 64 fragments (a tile of 64x64 pixels has 64 chunks: the
// chunk field is 6 bits), in launch-slot (= screen) order: neighbouring waves shade neighbouring pixels.
// ------------------------------------------------------------------------------------------------

// chunks of 64 fragments in the list of launch slot `slot` (0 past the frame)
BB_DEV uint32_t slot_chunks(const FrameParams &fp, const uint32_t *__restrict__ frag_count, uint32_t slot, uint32_t n_slots, int grid_x) {
  if (slot >= n_slots) return 0u;
  const int gy = (int)(slot / (uint32_t)grid_x), tx = (int)(slot - (uint32_t)gy * (uint32_t)grid_x);
  int ty, out_tile_row;
  if (!tile_row(fp, gy, ty, out_tile_row)) return 0u;
  const uint32_t n = frag_count[(uint32_t)ty * (uint32_t)fp.tiles_x + (uint32_t)tx];
  return (((n & ~kFullTile) + 63u) >> 6) | (n & kFullTile);  // (chunks, with the full-tile flag kept on top)
}

// One workgroup per 256 launch slots, no communication between workgroups: the items in front of a workgroup's slots are
// the sum of k_raster's per-group totals (eight independent loads per thread), its own 256 slots get a scan, then their items are
// written.  (A single workgroup doing all of it took 25 us at C3 -- 70 000 scattered 4-byte stores through ONE compute
// unit's address unit; every workgroup summing the raw counts in front of it took 13 us of dependent loads.)
template <int TILE_W, int TILE_H>
__global__ __launch_bounds__(kItemsThreads) void k_shade_items(FrameParams fp, const uint32_t *__restrict__ frag_count,
                                                               const uint32_t *__restrict__ item_groups,
                                                               uint32_t *__restrict__ items, int grid_x, int grid_y,
                                                               uint32_t *__restrict__ host_count,
                                                               const Light *__restrict__ lights, int num_lights,
                                                               CookedLight *__restrict__ cooked,
                                                               uint32_t *__restrict__ tile_count, const Counters *__restrict__ ctr,
                                                               const uint32_t *__restrict__ heavy) {
  __shared__ uint32_t s_wave[2][kItemsThreads / 64];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  // tiles that k_raster rasterised from a heavy slot still have their bin counts (their own workgroups had to see them):
  // cleared here for the slot's next frame
  if (fp.heavy_rows) {
    const uint32_t n_heavy = ctr->n_heavy;
    if (n_heavy <= (uint32_t)fp.heavy_rows * (uint32_t)grid_x)
      for (uint32_t i = blockIdx.x * (uint32_t)kItemsThreads + (uint32_t)tid; i < n_heavy; i += gridDim.x * (uint32_t)kItemsThreads) {
        const uint32_t hs = heavy[i] & 0x3FFFFFFFu;
        const int gy = (int)(hs / (uint32_t)grid_x), tx = (int)(hs - (uint32_t)gy * (uint32_t)grid_x);
        int ty, out_tile_row;
        if (tile_row(fp, gy, ty, out_tile_row)) {
          const uint32_t tile = (uint32_t)ty * (uint32_t)fp.tiles_x + (uint32_t)tx;
#pragma unroll
          for (uint32_t c = 0; c < kBinClasses; ++c) tile_count[tile * kBinClasses + c] = 0u;
        }
      }
  }
  // the frame's cooked light table (k_shade reads it through the scalar cache): once per frame, by the last workgroup
  // (the one with the fewest slots to scan)
  if (blockIdx.x == gridDim.x - 1)
    cook_lights<kItemsThreads>(lights, num_lights, cooked);
  const uint32_t n_slots = (uint32_t)grid_x * (uint32_t)grid_y;
  const uint32_t first = blockIdx.x * (uint32_t)kItemsThreads;
  uint32_t before = 0u;  // (independent loads: one round trip)
#pragma unroll
  for (int q = 0; q < kItemGroups / kItemsThreads; ++q) {
    const uint32_t g = (uint32_t)q * kItemsThreads + (uint32_t)tid;
    before += g < first / kItemGroupSlots ? item_groups[g * kItemGroupStride] : 0u;
  }
  const uint32_t chunks_flag = slot_chunks(fp, frag_count, first + (uint32_t)tid, n_slots, grid_x);
  const uint32_t chunks = chunks_flag & ~kFullTile;
  uint32_t incl = chunks;  // inclusive scan of this workgroup's slots, wave level
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const uint32_t up = (uint32_t)__shfl_up((int)incl, d);
    if (lane >= d) incl += up;
    before += (uint32_t)__shfl_xor((int)before, d);  // (butterfly sum: every lane ends with the wave's total)
  }
  if (lane == 63) s_wave[0][wave] = incl;
  if (lane == 0) s_wave[1][wave] = before;
  __syncthreads();
  uint32_t at = 1u + incl - chunks;
#pragma unroll
  for (int w = 0; w < kItemsThreads / 64; ++w) {
    at += s_wave[1][w];
    if (w < wave) at += s_wave[0][w];
  }
  const uint32_t slot = first + (uint32_t)tid;
  if (chunks != 0u) {
    const uint32_t gy = slot / (uint32_t)grid_x, tx = slot - gy * (uint32_t)grid_x;
    for (uint32_t c = 0; c < chunks; ++c) items[at + c] = item_word(chunks_flag & kFullTile, gy, tx, c);
  }
  // the workgroup of the last slot knows the total
  if (first + (uint32_t)kItemsThreads >= n_slots && tid == kItemsThreads - 1) {
    items[0] = at + chunks - 1u;
    if (host_count) *host_count = at + chunks - 1u;  // the slot's pinned kFlagItemCount word: sizes the launch of its next frame
  }
}

// The frame's cooked light table alone, one workgroup: a kept frame (option "view_keep") runs neither of the kernels that
// cook it on the way (k_raster's first workgroup, k_shade_items' last), and its lights may be new.
__global__ __launch_bounds__(kItemsThreads) void k_cook_lights(const Light *__restrict__ lights, int num_lights,
                                                               CookedLight *__restrict__ cooked) {
  cook_lights<kItemsThreads>(lights, num_lights, cooked);
}

// ------------------------------------------------------------------------------------------------
// k_shade: forward_brdf.frag + brdf.glsl once per visible pixel.
//
// What bounded the first version of this kernel (one workgroup per 256 fragments of a tile) was not arithmetic but the
// chain of dependent memory round trips in front of it -- kernel arguments -> fragment count -> fragment -> primitive
// record -> clip slot -> texels, ~0.8 us each under load -- against ~0.9 us of issue time per 64 fragments: its
// duration followed T = 66 us + 264 us / (waves per SIMD) at C3 (measured by padding LDS: 2, 3, 4, 7 waves -> 198,
// 151, 132, 109 us), and a body that only loaded the fragment and stored a constant still took 52 us.  Hence:
//  * ONE WAVE = ONE ITEM of 64 fragments from the list of k_shade_items (item = grid row, tile column, chunk of the
//    tile's fragment list): no wave is launched for an empty part of a tile, every launched wave is full (k_raster pads
//    each list to a multiple of 64 with copies of its first fragment), and no count has to be read before the fragments.
//    The main launch is sized on the host from the item count the same frame slot produced one frame earlier (pinned
//    word written by k_shade_items) plus 3 % + 64; a second, 32-workgroup instantiation (TAIL) walks whatever lies beyond
//    that estimate in a loop, so a frame that suddenly has more fragments is still complete.  (A SHORT frame -- 1080p --
//    has neither: its raster tiles append their items themselves, k_raster above, the count is read through `item_count`,
//    and it is launched at full coverage.)
//  * the chain is cut to three round trips per item (item word -> fragment words -> record + texels): the fragment
//    word carries the clip-arena slot of a clipped sub-triangle, so its planes are fetched together with the primitive
//    record instead of after it; a wave whose 64 fragments share one primitive fetches the record through the scalar
//    cache (constant address space), and so does every wave the frame's cooked light table: no LDS, no barrier.
//  * many waves per SIMD (64 VGPRs -> the hardware's eight) rather than a persistent, software-pipelined loop: a gfx950 wave issues at
//    most one instruction of ANY kind every ~4 cycles (profiles/r02_issue_rate.txt), so the vector ALU (one instruction
//    every 2 cycles) only fills up with several waves that are all busy issuing.  The persistent forms were built and
//    measured in round 2 ("dead ends"): loop-carried state costs 36 VGPRs, and every forced
//    occupancy spilled.
// ------------------------------------------------------------------------------------------------
#ifndef BB_SHADE_THREADS
#define BB_SHADE_THREADS 256
#endif
#ifndef BB_SHADE_WAVES
#define BB_SHADE_WAVES 8  // waves per SIMD the main forward instantiation is compiled for (64 registers)
#endif
constexpr int kShadeThreads = BB_SHADE_THREADS;
constexpr int kFrontPriorityLights = 6;  // k_shade: from this many lights on, a wave's load phases run at a raised issue priority
#ifdef BB_STAMPS
__device__ unsigned long long g_shade_stamps[4096 * 8];  // diagnostic build: per-wave phase cycles of k_shade
#endif
constexpr int kShadeWaves = kShadeThreads / 64;
typedef const uint8_t __attribute__((address_space(1))) *GlobalBytes;  // a pointer known to point to global memory
typedef uint32_t u32x3 __attribute__((ext_vector_type(3)));
typedef u32x3 __attribute__((aligned(1))) u32x3_any;  // 12 bytes at any byte address: one global_load_dwordx3
typedef const u32x3_any __attribute__((address_space(1))) *GlobalTap;

// ------------------------------------------------------------------------------------------------
// What the fragment kernels share: the rules of the fragment stage that k_shade, k_shade_aniso and k_shade_overlay all
// follow, each stated once.  Everything here is forced inline: the kernels compile to the code they had with the
// statements written out in place.
// ------------------------------------------------------------------------------------------------

// a varying at barycentrics (b0, b1, b2) from its values at the three vertices
BB_DEV float interp3(float b0, float b1, float b2, float v0, float v1, float v2) { return fmaf(b2, v2, fmaf(b1, v1, b0 * v0)); }

// perspective-correct barycentrics of the centre of pixel (px, py) from the screen-space planes of a (sub-)triangle; for a
// clipped sub-triangle then taken through its clip slot's 3 x 3 to those of the unclipped primitive
BB_DEV void plane_bary(const PlaneHead &h, bool clipped, const float (&cb)[3][3], int px, int py, float &b0, float &b1, float &b2) {
  const int Xc = px * 256 + 128, Yc = py * 256 + 128;
  const float dxp = (float)(Xc - h.X0), dyp = (float)(Yc - h.Y0);
  const float l1 = fmaf(h.l1dx, dxp, h.l1dy * dyp);
  const float l2 = fmaf(h.l2dx, dxp, h.l2dy * dyp);
  const float l0 = (1.0f - l1) - l2;
  const float u0 = l0 * h.rw0, u1 = l1 * h.rw1, u2 = l2 * h.rw2;
  const float r = bb_rcp((u0 + u1) + u2);
  b0 = u0 * r; b1 = u1 * r; b2 = u2 * r;
  if (clipped) {
    const float c0 = interp3(b0, b1, b2, cb[0][0], cb[1][0], cb[2][0]);
    const float c1 = interp3(b0, b1, b2, cb[0][1], cb[1][1], cb[2][1]);
    const float c2 = interp3(b0, b1, b2, cb[0][2], cb[1][2], cb[2][2]);
    b0 = c0; b1 = c1; b2 = c2;
  }
}

// The "late" clip slot.  k_raster names a clipped sub-triangle's slot in the fragment word for the first kClipRefs of a
// tile only; a fragment of any further one carries 0 there, although its record says the primitive was clipped.  Its slot
// is then found through the record, one round trip later: sub-triangle (ref & 7) of the primitive's run.
BB_DEV bool late_clip_slot(bool clipped, uint32_t clip_base) { return !clipped && clip_base != kNotClipped; }
BB_DEV uint32_t record_clip_slot(uint32_t clip_base, uint32_t ref) { return clip_base + (ref & 7u); }

// The frame's counter block has done its job (k_geometry filled it, k_raster read it): keep a copy for the host's
// statistics / overflow check and clear the block for the next frame of this slot, and the chunk totals k_shade_items is
// done with.  Frames of different slots share nothing, so their kernels may overlap freely.
BB_DEV void retire_counters(Counters *__restrict__ ctr, Counters *__restrict__ ctr_done, uint32_t *__restrict__ item_groups) {
  if (blockIdx.x == 0 && threadIdx.x < sizeof(Counters) / 4) {
    reinterpret_cast<uint32_t *>(ctr_done)[threadIdx.x] = reinterpret_cast<uint32_t *>(ctr)[threadIdx.x];
    reinterpret_cast<uint32_t *>(ctr)[threadIdx.x] = 0u;
  }
  if (blockIdx.x == 0 && item_groups)
    for (uint32_t g = threadIdx.x; g < (uint32_t)kItemGroups; g += kShadeThreads) item_groups[g * kItemGroupStride] = 0u;
}

// the shading normal from the interpolated varyings a[]: vTBN * nt with vTBN = mat3(T, B, N) and nt the normal map's
// vector (map_vector(): sampled only when the map is on), or without the map the interpolated normal, normalised
// (forward_brdf.frag:24) or as it is (gbuffer.frag:29)
template <bool DEFERRED, class MapVector>
BB_DEV f3 surface_normal(const float (&a)[kNumVary], int enable_normal_map, MapVector map_vector) {
  if (enable_normal_map != 0) {
    const f3 nt = map_vector();
    return mk3(interp3(nt.x, nt.y, nt.z, a[8], a[11], a[5]), interp3(nt.x, nt.y, nt.z, a[9], a[12], a[6]),
               interp3(nt.x, nt.y, nt.z, a[10], a[13], a[7]));
  }
  return DEFERRED ? mk3(a[5], a[6], a[7]) : normalize3(mk3(a[5], a[6], a[7]));
}
BB_DEV float normal_map_axis(float texel) { return fmaf(texel, 2.0f, -1.0f); }  // UNORM channel -> [-1, 1]

// one bilinear tap of one RGBA8 map of the material table: the four texels of the footprint at (u, v), and channel k of them
struct MapTap {
  uint32_t t00, t10, t01, t11;
  float fx, fy;
};
BB_DEV MapTap load_map_tap(const TexDesc &td, float u, float v) {
  const BilinearTaps tp = bilinear_taps(u, v, td.w, td.h);
  const uint32_t *texels = reinterpret_cast<const uint32_t *>(td.texels);
  MapTap r;
  r.t00 = texels[tp.o00]; r.t10 = texels[tp.o10]; r.t01 = texels[tp.o01]; r.t11 = texels[tp.o11];
  r.fx = tp.fx; r.fy = tp.fy;
  return r;
}
BB_DEV float map_channel(const MapTap &r, int k) { return filter_channel(r.t00, r.t10, r.t01, r.t11, 8 * k, r.fx, r.fy); }
BB_DEV float sample_map_r(const TexDesc &td, float u, float v) { return map_channel(load_map_tap(td, u, v), 0); }
BB_DEV f3 sample_map_rgb(const TexDesc &td, float u, float v) {
  const MapTap r = load_map_tap(td, u, v);
  return mk3(map_channel(r, 0), map_channel(r, 1), map_channel(r, 2));
}

// ------------------------------------------------------------------------------------------------
// Shadow mapping (option "shadow_map" = S > 0, bbr_render_shadow_map; k_shade_shadow).  The rule, in binary32 and in this
// operand order (restated independently in tests/shadow_reference.py):
//   map     texel (i, j) = the depth k_raster keeps for pixel (i, j) of an S x S frame of the recorded draws under
//           gl_Position = (L.proj * L.view) * posWorld (the forward order, proj_view(L), whatever "render_pass" is), with the
//           frame's own clipper, cull, snap, fill rule, depth test and clamp; an uncovered texel holds the clear value
//   test    on the P the light loop receives (deferred: after bb_half_round).  M = proj_view(L); c = mat4_mul(M, (P, 1));
//           !(c.w > 0) -> OUTSIDE.  r = bb_rcp(c.w), h = 0.5f * S; xs = fmaf(c.x * r, h, h), ys = fmaf(c.y * r, h, h);
//           !(xs >= 0 && xs < S && ys >= 0 && ys < S) -> OUTSIDE (NaN lands here).  i = (int)xs, j = (int)ys;
//           t = c.z * r + bias; SHADOWED iff map[j][i] > t (a NaN t is not shadowed), otherwise LIT
//   classes 0 not covered, 1 LIT, 2 SHADOWED, 3 OUTSIDE (bbr_read_shadow_mask)
//   loop    the iteration of light `light` of a SHADOWED fragment contributes nothing: the `continue` of an unknown light
//           type.  Every other operation, and the operand order, is light_surface's
// Deviations: a hard compare (option "shadow_filter": a box of them, ShadowPcfTest below), one caster per light (up to eight lights: ShadowCastersTest below), and the deferred background colour (k_deferred_background) is evaluated without the
// test.  A point light gets up to six frusta (ShadowFacesTest, below): a fragment on a seam of exactly-90-degree faces is
// outside all of them and lit, and where frusta overlap the earlier one decides.
// M and the scalars are kernel arguments (scalar registers); the map costs one 4-byte gather per fragment, and only lanes
// inside the map address it: i and j lie in [0, S - 1].
// ------------------------------------------------------------------------------------------------
enum ShadowClass : int { kShadowNone = 0, kShadowLit = 1, kShadowShadowed = 2, kShadowOutside = 3, kShadowPartial = 4 /* "shadow_filter" */ };
struct ShadowArgs {
  Mat4 m;            // proj_view(L)
  const float *map;  // S x S depths, row-major
  uint8_t *mask;     // the DUMP form's second output (bbr_read_shadow_mask): a class per pixel, or nullptr
  int32_t side;      // S
  int32_t light;     // the caster's index in the frame's light list
  float half;        // 0.5f * S
  float bias;
};
struct ShadowSkip {
  int light;
  bool shadowed;
  BB_DEV bool operator()(int li) const { return shadowed && li == light; }
  BB_DEV void colour(int, float &, float &, float &) const {}
};
// What surface_colour asks of its `shadow`: on() classifies the fragment and says which iteration the light loop skips.
struct NoShadow {
  BB_DEV NoSkip on(const FrameParams &, f3, bool, int, int) const { return NoSkip{}; }
};
// The rule's `test` for one face up to the map read, stated once for the four kernels: where P lands in the map of M and the
// depth t it is compared at.  i = (int)xs and j = (int)ys (0 .. S - 1) are formed at the use, behind `inside`.
struct ShadowTexel {
  bool inside;
  float xs, ys, t;
};
template <typename M4>  // (Mat4 in any address space)
BB_DEV ShadowTexel shadow_texel(const M4 &m, f3 P, float side, float half, float bias) {
  const f4 c = mat4_mul(m, f4{P.x, P.y, P.z, 1.0f});
  const float r = bb_rcp(c.w);  // (of a w <= 0 too: not used then)
  const float xs = fmaf(c.x * r, half, half), ys = fmaf(c.y * r, half, half);
  return ShadowTexel{c.w > 0.0f && xs >= 0.0f && xs < side && ys >= 0.0f && ys < side, xs, ys, c.z * r + bias};
}

// Up to six faces for the one caster (bbr_render_shadow_faces with 2 .. 6 view blocks; k_shade_shadow_faces): six 90-degree-class
// frusta at a point light are a cube map, nested orthographic ones are cascades.  The rule (restated
// independently in tests/shadow_faces_reference.py):
//   maps    map_f = the map above for L_f, at map + f * S * S
//   test    for f = 0 .. F - 1 in this order: cls_f = the rule above with M_f = proj_view(L_f) and map_f; the first
//           cls_f != OUTSIDE is the fragment's class and f its face; none: OUTSIDE, face 255
// Where frusta overlap the earlier face wins and the later map is not read; a fragment outside every face is lit (with faces
// of exactly 90 degrees: on the seam planes).  The walk itself: shadow_verdict, below.
constexpr int kMaxShadowFaces = 6;
struct ShadowFacesArgs {
  Mat4 m[kMaxShadowFaces];  // proj_view(L_f)
  const float *map;         // F maps of S x S depths, face f at map + f * S * S
  uint8_t *mask;            // the DUMP form's outputs (bbr_read_shadow_mask, bbr_read_shadow_face_index): a class and ...
  uint8_t *face;            // ... the deciding face per pixel, or nullptr
  int32_t side;             // S
  int32_t light;            // the caster's index in the frame's light list
  int32_t faces;            // F
  float half;               // 0.5f * S
  float bias;
};

// Percentage-closer filtering (option "shadow_filter" = R in 1 .. 2; k_shade_shadow_pcf): a (2R+1) x (2R+1) box of the hard
// rule's compares, K = 9 or 25 taps.  The rule (restated independently in tests/shadow_filter_reference.py):
//   face, i, j, t   the rules above, unchanged: the deciding face f is the first the fragment is not OUTSIDE of, and OUTSIDE
//           and "not covered" are decided before any tap is read
//   taps    for dj = -R .. R, di = -R .. R: texel = map_f[clamp(j + dj, 0, S - 1)][clamp(i + di, 0, S - 1)]; the tap is lit
//           iff !(texel > t) (a NaN t: every tap is lit).  k = the number of lit taps, an integer: the order has no meaning
//   classes 1 LIT (k = K), 2 SHADOWED (k = 0), 4 PARTIAL (0 < k < K); 0 and 3 as above
//   loop    k = K: untouched.  k = 0: the caster's iteration contributes nothing.  Otherwise it runs with the cooked colour
//           color[c] * (intensity * v), v = (float)k * RK, RK[9], RK[25] = the binary32 nearest 1/9, 1/25: the caster's
//           intensity replaced by the binary32 product intensity * v, everything else light_surface's
// Deviations: a box, not bilinear weights; one t for all taps (no receiver-plane bias); taps never leave the deciding face's
// map (on a cube they clamp at the face's edge); the deferred background stays untested.
// R is a kernel argument, a scalar: one kernel serves both radii.  A tap is one 4-byte gather; a window's rows are walked one
// after the other and a row's 2R + 1 gathers are issued together (lit_taps; the plain double loop paid K dependent round
// trips: profiles/shadow_filter.txt).  Only lanes inside face f address its map, and a clamped address lies in [0, S - 1] by
// construction.  The caster's raw colour and intensity are read from the
// frame's light block through the scalar cache (wave-uniform), guarded by light < num_lights.
struct ShadowPcfArgs {
  ShadowFacesArgs f;    // F = 1 .. 6 faces; `mask`, `face`: the DUMP form's outputs, as above
  const Light *lights;  // the frame's light block
  uint8_t *taps;        // the DUMP form's third output (bbr_read_shadow_taps): k per pixel, 255 where OUTSIDE, or nullptr
  int32_t num_lights;
  int32_t radius;       // R
};
typedef const Light __attribute__((address_space(4))) *ConstLight;
struct ShadowScale {
  int light;
  bool shadowed, partial;
  float iv;          // intensity * v
  float r, g, b;     // the caster's raw colour (scalars)
  BB_DEV bool operator()(int li) const { return shadowed && li == light; }
  BB_DEV void colour(int li, float &cr, float &cg, float &cb) const {
    if (partial && li == light) { cr = r * iv; cg = g * iv; cb = b * iv; }
  }
};
// k of the window round texel (i, j) of one face's S x S map: the rows one after the other, a row's 2R + 1 gathers issued together
template <int RADIUS>
BB_DEV int lit_taps(const float *face_map, int side, int i, int j, float t) {
  const int last = side - 1;
  int n = 0;
#pragma unroll 1
  for (int dj = -RADIUS; dj <= RADIUS; ++dj) {
    const float *row = face_map + (size_t)min(max(j + dj, 0), last) * (size_t)side;
    float texel[2 * RADIUS + 1];
#pragma unroll
    for (int di = -RADIUS; di <= RADIUS; ++di) texel[di + RADIUS] = row[min(max(i + di, 0), last)];
#pragma unroll
    for (int q = 0; q <= 2 * RADIUS; ++q) n += texel[q] > t ? 0 : 1;
  }
  return n;
}
// k for R = 0 .. 2: the hard compare is the window of one tap
BB_DEV int lit_count(const float *face_map, int side, int R, int i, int j, float t) {
  if (R == 0) return face_map[(size_t)j * (size_t)side + (size_t)i] > t ? 0 : 1;
  return R == 1 ? lit_taps<1>(face_map, side, i, j, t) : lit_taps<2>(face_map, side, i, j, t);
}
BB_DEV int shadow_taps(int R) { return (2 * R + 1) * (2 * R + 1); }                                   // K
BB_DEV float shadow_rk(int R) { return R == 0 ? 1.0f : (R == 1 ? 1.0f / 9.0f : 1.0f / 25.0f); }  // RK
BB_DEV int shadow_class(int k, int K) { return k == K ? kShadowLit : (k == 0 ? kShadowShadowed : kShadowPartial); }
// the caster's intensity under a PARTIAL verdict: intensity * v
BB_DEV float partial_intensity(float intensity, int k, float rk) { return intensity * ((float)k * rk); }

// What the test says of a fragment under one caster; the DUMP forms store it per pixel (bbr_read_shadow_mask,
// bbr_read_shadow_face_index, bbr_read_shadow_taps), each output only where its pointer is set.
struct ShadowVerdict {
  int cls, face, k;  // OUTSIDE: face 255, k 255
  BB_DEV void dump(const FrameParams &fp, int gx, int gy, uint8_t *mask, uint8_t *face_out, uint8_t *taps) const {
    const size_t o = (size_t)gy * (size_t)fp.width + (size_t)gx;
    if (mask) mask[o] = (uint8_t)cls;
    if (face_out) face_out[o] = (uint8_t)face;
    if (taps) taps[o] = (uint8_t)k;
  }
};
// of a fragment inside face f, at texel ((int)x.xs, (int)x.ys) of its map
BB_DEV ShadowVerdict face_verdict(const ShadowTexel &x, const float *face_map, int side, int R, int f) {
  const int k = lit_count(face_map, side, R, (int)x.xs, (int)x.ys, x.t);
  return ShadowVerdict{shadow_class(k, shadow_taps(R)), f, k};
}
// The face walk of the faces rule, with M_f = matrix_of(f): kernel arguments (faces_verdict) or the caster table
// (ShadowCastersTest).  The loop is uniform over the wave: f is a scalar, so M_f arrives through scalar loads and every lane
// runs the same face; a lane that has its class only carries it.  The loop ends when no lane of the wave is undecided (a
// ballot): most waves of a cube-lit frame see one or two faces.  Only lanes inside face f address its map, with i, j in
// [0, S - 1] by the comparisons (and the clamps of lit_taps) and f < F by the loop bound.
template <class MatrixOf>
BB_DEV ShadowVerdict shadow_verdict(MatrixOf matrix_of, const float *map, int faces, int side, float half, float bias, int R, f3 P) {
  const size_t texels = (size_t)side * (size_t)side;
  ShadowVerdict v{kShadowOutside, 255, 255};
  for (int f = 0; f < faces; ++f) {
    const bool undecided = v.cls == kShadowOutside;
    if (__ballot(undecided) == 0ull) break;
    const ShadowTexel x = shadow_texel(matrix_of(f), P, (float)side, half, bias);
    if (undecided && x.inside) v = face_verdict(x, map + (size_t)f * texels, side, R, f);
  }
  return v;
}
BB_DEV ShadowVerdict faces_verdict(const ShadowFacesArgs &a, int R, f3 P) {
  return shadow_verdict([&](int f) -> const Mat4 & { return a.m[f]; }, a.map, a.faces, a.side, a.half, a.bias, R, P);
}

template <bool DUMP>
struct ShadowTest {  // one face, R = 0: no loop and no ballot
  const ShadowArgs &a;
  BB_DEV ShadowSkip on(const FrameParams &fp, f3 P, bool valid, int gx, int gy) const {
    const ShadowTexel x = shadow_texel(a.m, P, (float)a.side, a.half, a.bias);
    ShadowVerdict v{kShadowOutside, 255, 255};
    if (x.inside) v = face_verdict(x, a.map, a.side, 0, 0);
    if (DUMP && valid) v.dump(fp, gx, gy, a.mask, nullptr, nullptr);
    return ShadowSkip{a.light, v.cls == kShadowShadowed};
  }
};
template <bool DUMP>
struct ShadowFacesTest {
  const ShadowFacesArgs &a;
  BB_DEV ShadowSkip on(const FrameParams &fp, f3 P, bool valid, int gx, int gy) const {
    const ShadowVerdict v = faces_verdict(a, 0, P);
    if (DUMP && valid) v.dump(fp, gx, gy, a.mask, a.face, nullptr);
    return ShadowSkip{a.light, v.cls == kShadowShadowed};
  }
};
template <bool DUMP>
struct ShadowPcfTest {
  const ShadowPcfArgs &a;
  BB_DEV ShadowScale on(const FrameParams &fp, f3 P, bool valid, int gx, int gy) const {
    const ShadowFacesArgs &s = a.f;
    const ShadowVerdict v = faces_verdict(s, a.radius, P);
    if (DUMP && valid) v.dump(fp, gx, gy, s.mask, s.face, a.taps);
    float intensity = 0.0f, cr = 0.0f, cg = 0.0f, cb = 0.0f;
    if (s.light < a.num_lights) {
      ConstLight l = (ConstLight)a.lights + s.light;
      intensity = l->intensity; cr = l->color[0]; cg = l->color[1]; cb = l->color[2];
    }
    return ShadowScale{s.light, v.cls == kShadowShadowed, v.cls == kShadowPartial, partial_intensity(intensity, v.k, shadow_rk(a.radius)), cr, cg, cb};
  }
};

// Casters (bbr_render_shadow_caster; k_shade_shadow_casters): up to kMaxShadowCasters = 8 caster SLOTS per context, 0 .. 7.  A slot
// in use holds a light index, F = 1 .. 6 view blocks, their F maps of S x S and a bias; S ("shadow_map") and R ("shadow_filter")
// are the context's.  The caster of bbr_render_shadow_map / bbr_render_shadow_faces is slot 0.  The rule (DESIGN.md section 3,
// "Casters"; restated independently in tests/shadow_casters_reference.py):
//   maps    slot s, face f: the map rule above for that view block.  Every rank renders all of them
//   test    for every slot in use, independently of the others: (class_s, face_s, k_s) = the rules above with that slot's
//           matrices, maps and bias, on the P the light loop receives.  R = 0: the first face not OUTSIDE and the hard compare,
//           K = 1, k = 0 or 1.  R >= 1: the box of K = 9 or 25 compares clamped inside the deciding face.  Slots do not see
//           each other
//   loop    iteration li looks for the slot in use whose light index is li (there is at most one).  None, or class OUTSIDE, or
//           k = K: untouched.  k = 0: the iteration contributes nothing (the `continue` of an unknown type).  0 < k < K: it runs
//           with the cooked colour color[c] * (intensity * ((float)k * RK)).  The lights' order, every other operation and the
//           accumulation order are light_surface's.  A slot whose light index is >= NumLights changes nothing
// Hence: one slot in use, whichever, gives the frame of that caster in slot 0; permuting casters over slots changes no bit; a
// caster at bias 2, or on a light beyond the frame's, leaves the frame of the others alone.
// Deviations kept: the deferred background stays untested; a box, one t per window, no fetch across faces.  New: one slot per
// light -- two slots naming one light are refused, not combined.
// The casters do not fit kernel arguments (8 x 6 Mat4 = 3 KB): the kernel gets a pointer to a table the host owns and writes
// only while no frame is in flight, and reads it wave-uniformly through the scalar cache (constant address space, like
// ConstLight): the slot index s and the face index f are scalars.  A lane carries k_s out of on() -- one byte per slot, OUTSIDE
// stored as K, two registers for the eight -- and nothing else; the light loop finds the slot of li in the table's host-built
// light -> slot lookup, extracts that byte and forms the scale from the light's scalars there.  Only lanes inside face f of slot
// s address that map: i, j in [0, S - 1] by the comparisons (and the clamps), f < F_s and s < 8 by the loop bounds.
constexpr int kMaxShadowCasters = 8;
struct ShadowCasterEntry {
  Mat4 m[kMaxShadowFaces];  // proj_view(L_f)
  const float *map;         // F maps of S x S depths, face f at map + f * S * S
  int32_t light;            // the caster's index in the frame's light list
  int32_t faces;            // F; 0: the slot is not in use
  float bias;
  int32_t pad_;
};
struct ShadowCasterTable {
  ShadowCasterEntry slot[kMaxShadowCasters];
  int32_t slot_of_light[kMaxNumLights];  // the slot in use whose light index this is, or -1
};
struct ShadowCastersArgs {
  const ShadowCasterTable *table;
  const Light *lights;  // the frame's light block
  uint8_t *mask;        // the DUMP form's outputs for slot `dump_slot`: class, deciding face and k per pixel, or nullptr
  uint8_t *face;
  uint8_t *taps;
  int32_t num_lights;
  int32_t radius;       // R = 0 .. 2
  int32_t side;         // S
  int32_t dump_slot;
  float half;           // 0.5f * S
};
typedef const ShadowCasterTable __attribute__((address_space(4))) *ConstCasters;
struct ShadowCastersSkip {
  ConstCasters table;
  ConstLight lights;
  int K;           // (scalars)
  float rk;
  uint32_t k[2];   // per lane: byte s & 3 of word s >> 2 = k_s, K where slot s is OUTSIDE, not in use or not evaluated
  BB_DEV int count(int li) const {
    const int s = table->slot_of_light[li];
    if (s < 0) return K;
    return (int)(((s < 4 ? k[0] : k[1]) >> (8 * (s & 3))) & 0xFFu);
  }
  BB_DEV bool operator()(int li) const { return count(li) == 0; }
  BB_DEV void colour(int li, float &cr, float &cg, float &cb) const {
    const int s = table->slot_of_light[li];
    if (s < 0) return;
    ConstLight l = lights + li;
    const float intensity = l->intensity, r = l->color[0], g = l->color[1], b = l->color[2];
    const int n = (int)(((s < 4 ? k[0] : k[1]) >> (8 * (s & 3))) & 0xFFu);
    if (n > 0 && n < K) {
      const float iv = partial_intensity(intensity, n, rk);
      cr = r * iv; cg = g * iv; cb = b * iv;
    }
  }
};
template <bool DUMP>
struct ShadowCastersTest {
  const ShadowCastersArgs &a;
  BB_DEV ShadowCastersSkip on(const FrameParams &fp, f3 P, bool valid, int gx, int gy) const {
    const ConstCasters table = (ConstCasters)a.table;
    const int R = a.radius, K = shadow_taps(R);
    const uint32_t all_k = (uint32_t)K * 0x01010101u;
    uint32_t packed[2] = {all_k, all_k};
#pragma unroll 1
    for (int s = 0; s < kMaxShadowCasters; ++s) {
      const int faces = table->slot[s].faces;
      if (faces == 0) continue;
      // (nothing observable depends on a caster beyond the frame's lights -- but its mask is observable)
      if (!DUMP && table->slot[s].light >= a.num_lights) continue;
      const auto matrix_of = [&](int f) {  // a Mat4 in scalar registers
        Mat4 m;
#pragma unroll
        for (int col = 0; col < 4; ++col)
#pragma unroll
          for (int row = 0; row < 4; ++row) m.M[col][row] = table->slot[s].m[f].M[col][row];
        return m;
      };
      const ShadowVerdict v = shadow_verdict(matrix_of, table->slot[s].map, faces, a.side, a.half, table->slot[s].bias, R, P);
      const uint32_t byte = v.cls == kShadowOutside ? (uint32_t)K : (uint32_t)v.k;
      const uint32_t shift = 8u * (uint32_t)(s & 3);
      uint32_t &word = s < 4 ? packed[0] : packed[1];
      word = (word & ~(0xFFu << shift)) | (byte << shift);
      if (DUMP && valid && s == a.dump_slot) v.dump(fp, gx, gy, a.mask, a.face, a.taps);
    }
    return ShadowCastersSkip{table, (ConstLight)a.lights, K, shadow_rk(R), {packed[0], packed[1]}};
  }
};

// From the filtered surface to the pixel's colour.  Forward: brdf.glsl on the surface.  Deferred: gbuffer.frag:24-32 into
// four RGBA16F attachments (binary16, round to nearest even), then brdf.frag:12-73 on the pixel's own texel -- fused, the
// texel only goes to memory when somebody asked to see it, and only then is the height map sampled (height(): the
// filtered, unrounded value); with gbuffer_view, buffer_visualize.frag:8-12 instead of brdf.frag (recordCommand,
// src/main.cpp:96-121): the rgb of one attachment.
// `shadow` (k_shade_shadow: a ShadowTest) is asked once, on the P the light loop receives.
template <bool DEFERRED, class Lights, class Height, class Shadow = NoShadow>
BB_DEV float4 surface_colour(const FrameParams &fp, const ShadeParams &sp, const Lights lights, f3 P, f3 normal, f3 albedo,
                             float metallic, float roughness, float ao, uint2 *__restrict__ gbuffer, bool valid, int gx, int gy,
                             Height height, const Shadow &shadow = Shadow{}) {
  if (!DEFERRED) return light_surface(sp, lights, P, normal, albedo, metallic, roughness, ao, shadow.on(fp, P, valid, gx, gy));
  P = mk3(bb_half_round(P.x), bb_half_round(P.y), bb_half_round(P.z));
  const auto skip = shadow.on(fp, P, valid, gx, gy);
  normal = mk3(bb_half_round(normal.x), bb_half_round(normal.y), bb_half_round(normal.z));
  albedo = mk3(bb_half_round(albedo.x), bb_half_round(albedo.y), bb_half_round(albedo.z));
  metallic = bb_half_round(metallic); roughness = bb_half_round(roughness); ao = bb_half_round(ao);
  if (gbuffer && valid) {
    const float h = bb_half_round(height());
    _Float16 g[16] = {(_Float16)P.x, (_Float16)P.y, (_Float16)P.z, (_Float16)1.0f,
                      (_Float16)normal.x, (_Float16)normal.y, (_Float16)normal.z, (_Float16)0.0f,
                      (_Float16)albedo.x, (_Float16)albedo.y, (_Float16)albedo.z, (_Float16)0.0f,
                      (_Float16)metallic, (_Float16)roughness, (_Float16)ao, (_Float16)h};
    uint4 *dst = reinterpret_cast<uint4 *>(gbuffer) + 2 * ((size_t)gy * (size_t)fp.width + (size_t)gx);
    uint4 lo, hi;
    __builtin_memcpy(&lo, g, 16);
    __builtin_memcpy(&hi, g + 8, 16);
    dst[0] = lo;
    dst[1] = hi;
  }
  if (fp.gbuffer_view >= 0) {
    const f3 shown = fp.gbuffer_view == 0 ? P : (fp.gbuffer_view == 1 ? normal : (fp.gbuffer_view == 2 ? albedo : mk3(metallic, roughness, ao)));
    return make_float4(shown.x, shown.y, shown.z, 1.0f);
  }
  return light_surface(sp, lights, P, normal, albedo, metallic, roughness, ao, skip);
}

// the pixel's colour into the frame, or (PRESENT) through present_pixel into the presented RGBA8 image
template <bool PRESENT>
BB_DEV void store_colour(bool valid, float4 color, size_t o, float4 *__restrict__ out, uint32_t *__restrict__ out8,
                         const SrgbTables *__restrict__ tables, const ShadeParams &sp) {
  if (!valid) return;
  if (PRESENT) store_pixel(&out8[o], present_pixel(color.x, color.y, color.z, *tables, sp.tone_enable, sp.exposure, 1));
  else store_pixel(&out[o], color);
}

// PRESENT = true (option "present_fused"): the colour goes through present_pixel and is stored as RGBA8 -- the tone-map
// subpass fused into the producing kernel: 4 bytes written per pixel instead of 16, and no k_present pass (16 B read +
// 4 B written per pixel) afterwards.
// TAIL = false: one item per wave -- wave v of workgroup w shades item first_item + 4 w + v and exits; the host sizes the
// grid from the item count of the frame this slot rendered before (frames are coherent), so nearly every wave launched
// has an item.  TAIL = true: a small fixed grid loops over whatever lies behind the part the main launch covered (a
// scene that suddenly grew); normally nothing.  Two instantiations because the loop form costs registers: the compiler
// keeps ~100 live around a loop where the straight-line body fits 64 -- four waves per SIMD instead of eight.  The main
// instantiation asks for eight waves per SIMD (amdgpu_waves_per_eu): the allocator then gets from 67 registers to 64
// without a spill, and the eighth wave is worth 3.4 us of the kernel's 76 at C3 (latency hiding is what this kernel runs on).
// MIXED = false: every material of the frame is packed (its five shaded maps share one size, or are the uniform defaults:
// what bbr_upload_material produces for every ShaderBall material) -- the instantiation then has no per-map sampling path
// at all, and that path's registers and code are not the main launch's problem.  The host knows (upload_material_table).
template <int TILE_W, int TILE_H, bool DEFERRED, bool PRESENT = false, bool TAIL = false, bool MIXED = true>
__global__ __launch_bounds__(kShadeThreads) __attribute__((amdgpu_waves_per_eu(TAIL ? 1 : ((DEFERRED || MIXED) ? 7 : BB_SHADE_WAVES)))) void k_shade(
    // (first: what stands between a wave's launch and its first loads -- the item word, the item count, then the fragment
    //  words and the record: these pointers arrive in scalar registers with the wave, "kernarg preload", 14 dwords at most)
    const uint32_t *__restrict__ items, const uint32_t *__restrict__ item_count, uint32_t first_item,
    const unsigned long long *__restrict__ frags, const uint32_t *__restrict__ frag_count,
    const ShadeRec *__restrict__ recs, const ClipSlot *__restrict__ clip_arena,
    FrameParams fp, ShadeParams sp, const CookedLight *__restrict__ cooked,
    const MaterialDesc *__restrict__ materials, float4 *__restrict__ out,
    uint2 *__restrict__ gbuffer, const SrgbTables *__restrict__ tables, uint32_t *__restrict__ out8,
    Counters *__restrict__ ctr, Counters *__restrict__ ctr_done, uint32_t *__restrict__ item_groups) {
  constexpr int TILE_PIXELS = TILE_W * TILE_H;
  const ConstLights lights_c{(ConstCooked)cooked};
  if (!TAIL) retire_counters(ctr, ctr_done, item_groups);  // (the main launch only)
#ifdef BB_STAMPS
  unsigned long long st_t[8];
  st_t[0] = __builtin_amdgcn_s_memtime();
#define BB_KSTAMP(i) do { asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory"); st_t[i] = __builtin_amdgcn_s_memtime(); } while (0)
#else
#define BB_KSTAMP(i) do { } while (0)
#endif
  // With a LONG light loop (C5's eight lights: two thirds of a wave's instructions) the waves that are still asking for their
  // fragments, records and texels go first: their loads are out sooner and there is always another wave's light loop to
  // issue behind them (C5 frame 509-514 -> 500-503 us on two boxes).  With four lights the same priority costs 2-3 %
  // (C3 101 -> 104 us): there the waves in their light loops are the ones about to give their slots back.
  if (sp.num_lights >= kFrontPriorityLights) __builtin_amdgcn_s_setprio(2);
  const int lane = (int)(threadIdx.x & 63u);
  // this wave's (first) item: wave-uniform, everything derived from it lives in scalar registers.  The item word is read
  // together with the item count, not after it (the list has room for every index a launch can produce): one dependent
  // round trip less in front of the fragments.
  // (Workgroup b runs on XCD b % 8 -- tools/microbench/xcd_map.hip -- so neighbouring items, which share records and
  //  texels, land in eight different L2s.  Giving each XCD a contiguous eighth of the item list cut k_shade's fetch traffic
  //  by 23 % and made it 12 % SLOWER (98 vs 88 us): a hot region then loads one L2 / one XCD's texture units instead of
  //  eight; runs of 4 / 16 / 64 workgroups per XCD: 87 / 89 / 94 us, no traffic gain.  Plain round-robin stays.)
  uint32_t j = first_item + (uint32_t)__builtin_amdgcn_readfirstlane((int)(blockIdx.x * (uint32_t)kShadeWaves + (threadIdx.x >> 6)));
  uint32_t item = items[1u + (TAIL ? 0u : j)];
  uint32_t n_items = *item_count;  // (items[0], or the head word k_raster's tiles appended through: short frames)
  // (both loads are in flight before either is waited for: left to itself the compiler reads the count, branches, and only
  //  then asks for the item word -- one more dependent round trip in front of every wave's fragments)
  //  -- and the frame parameters the item is decoded with arrive in the same round trip, not in one of their own behind it)
  asm volatile("" : "+s"(item), "+s"(n_items), "+s"(fp.tiles_x), "+s"(fp.world), "+s"(fp.rank), "+s"(fp.band_tiles), "+s"(fp.width));
  if (BB_ABLATE(2048u)) sp.num_lights = 0;
  if (j >= n_items) return;  // a wave without an item (the kernel has no barrier: waves come and go on their own)
  do {  // (a loop only in the TAIL instantiation)
  if (TAIL) item = items[1u + j];
  const ItemPlace at = decode_item(fp, item);
  bool valid;
  const unsigned long long frag = fetch_fragment<TILE_PIXELS, true>(item, at, lane, frags, frag_count, valid);
  BB_KSTAMP(1);  // item word, count and fragment arrived
  const uint32_t ref = (uint32_t)frag;
  uint32_t prim = BB_ABLATE(16u) ? 0u : (ref >> 3);
  if (BB_ABLATE(1024u)) prim = (uint32_t)__builtin_amdgcn_readfirstlane((int)prim);  // the record through the scalar cache
  int x, y;
  tile_pixel<TILE_W>(fragment_pixel<TILE_PIXELS>(frag), x, y);
  const int gx = at.tx * TILE_W + x, gy = at.ty * TILE_H + y;
  // the pixel's index in the output (32 bits: a frame has at most 2^30 pixels) -- formed here, so that ONE register, not the
  // pixel's coordinates, lives through the two load groups below (the kernel runs at the 64 registers of eight waves per SIMD)
  uint32_t opix = (uint32_t)(at.out_tile_row * TILE_H + y) * (uint32_t)fp.width + (uint32_t)gx;
  asm volatile("" : "+v"(opix));
  const size_t o = (size_t)opix;

  // ---- The dependent loads between a fragment and its colour, in TWO round trips ----
  //   A  the HEAD of the primitive record (planes, 1/w, the three texture coordinates, the material binding: 80 bytes) and,
  //      for a fragment of a clipped primitive, its sub-triangle's clip slot -- whose index the fragment word carries, so
  //      nothing has to be read first to know whether and where
  //   B  the texels (four 12-byte taps, addressed from the interpolated uv) TOGETHER WITH the body of the record (the other
  //      twelve varyings of each vertex: 144 bytes)
  // Written as one sequence the compiler serialised it into five (round 3's build, by its listing: clip_base -> planes ->
  // barycentrics -> varyings -> material pointer -> texels; it sinks every load to its first use to stay within 64
  // registers): each group below ends in a fence -- an empty asm that takes every loaded value -- so that all loads of the
  // group are in flight before the first of them is waited for.
  // Two forms of the same statements:
  //  * every fragment of the wave belongs to ONE (sub-)triangle -- the ground plane's waves, about half of C3's: record and
  //    clip slot come ONCE through the scalar cache (s_load; constant address space) instead of 64 lanes gathering them;
  //  * otherwise each lane gathers the record of its own fragment's primitive (neighbouring pixels share primitives, so
  //    the loads of a wave hit few L1 lines).
  float a[kNumVary];
  uint32_t packed_dims, material;
  const uint8_t *packed_texels;
  float b0, b1, b2;  // perspective-correct barycentrics with respect to the (unclipped) primitive: plane_bary
  // texels of the packed material (one set of taps, four 12-byte loads of 9-byte records) -- global loads, issued in group B
  BilinearTaps tp = {};
  uint32_t t00[3] = {}, t10[3] = {}, t01[3] = {}, t11[3] = {};
  // (Issued by EVERY lane, without a branch around them: a lane whose material is not packed -- maps of different sizes, the
  //  per-map path further down -- reads twelve bytes of its own record instead and ignores them.  Behind a branch the loads
  //  still in flight at the join are unknown to the compiler, and it waits for all of them where the record's first part
  //  would do.)
  auto issue_taps = [&](const void *harmless) {
    const float u = BB_ABLATE(8u) ? 0.5f : a[0], v = BB_ABLATE(8u) ? 0.5f : a[1];
    const bool packed = !MIXED || packed_dims != 0u;
    tp = bilinear_taps<true>(u, v, packed ? (int)(packed_dims & 0xFFFFu) : 1, packed ? (int)(packed_dims >> 16) : 1);
    const GlobalBytes tb = packed ? (GlobalBytes)packed_texels : (GlobalBytes)harmless;
    const u32x3 q00 = *(GlobalTap)(tb + texel_offset(tp.o00)), q10 = *(GlobalTap)(tb + texel_offset(tp.o10));
    const u32x3 q01 = *(GlobalTap)(tb + texel_offset(tp.o01)), q11 = *(GlobalTap)(tb + texel_offset(tp.o11));
    t00[0] = q00.x; t00[1] = q00.y; t00[2] = q00.z;
    t10[0] = q10.x; t10[1] = q10.y; t10[2] = q10.z;
    t01[0] = q01.x; t01[1] = q01.y; t01[2] = q01.z;
    t11[0] = q11.x; t11[1] = q11.y; t11[2] = q11.z;
  };
  {
    const uint32_t clip1 = (uint32_t)(frag >> (32 + kFragPixBits));  // clip-arena slot + 1 of a clipped sub-triangle, 0: none / unknown
    const uint32_t ref_u = (uint32_t)__builtin_amdgcn_readfirstlane((int)ref);
    if ((__ballot(ref != ref_u) == 0ull && !BB_ABLATE(4096u)) || BB_ABLATE(8192u)) {
      // ---- uniform wave: scalar loads (the constant address space is what makes them scalar -- and keeps the compiler from
      // merging the two forms back into one that gathers: both buffers were written by k_geometry and are read-only here) ----
      typedef const ShadeRec __attribute__((address_space(4))) *ConstRec;
      typedef const ClipSlot __attribute__((address_space(4))) *ConstClip;
      typedef const PlaneHead __attribute__((address_space(4))) *ConstHead;
      const ConstRec rp = (ConstRec)recs + (BB_ABLATE(16u) ? 0u : (ref_u >> 3));
      const uint32_t clip1_u = (uint32_t)__builtin_amdgcn_readfirstlane((int)clip1);
      bool clipped = clip1_u != 0u;
      const ConstClip cp = (ConstClip)clip_arena + (clipped ? clip1_u - 1u : 0u);
      const ConstHead hp = clipped ? &cp->h : &rp->h;
      // group A
      PlaneHead h;
      h.X0 = hp->X0; h.Y0 = hp->Y0; h.l1dx = hp->l1dx; h.l1dy = hp->l1dy; h.l2dx = hp->l2dx; h.l2dy = hp->l2dy;
      h.rw0 = hp->rw0; h.rw1 = hp->rw1; h.rw2 = hp->rw2;
      float uv[3][2], cb[3][3];
#pragma unroll
      for (int k = 0; k < 3; ++k) { uv[k][0] = rp->uv[k][0]; uv[k][1] = rp->uv[k][1]; }
#pragma unroll
      for (int jj = 0; jj < 3; ++jj)
#pragma unroll
        for (int k = 0; k < 3; ++k) cb[jj][k] = cp->bary[jj][k];  // (slot 0 when the fragment is not clipped: loaded, not used)
      packed_dims = rp->packed_dims;
      material = rp->material;
      unsigned long long packed_bits = (unsigned long long)(uintptr_t)rp->packed;
      uint32_t clip_base = rp->clip_base;
      asm volatile("" :: "s"(h.X0), "s"(h.Y0), "s"(h.l1dx), "s"(h.l1dy), "s"(h.l2dx), "s"(h.l2dy), "s"(h.rw0), "s"(h.rw1), "s"(h.rw2), "s"(uv[0][0]), "s"(uv[0][1]), "s"(uv[1][0]), "s"(uv[1][1]), "s"(uv[2][0]), "s"(uv[2][1]), "s"(packed_dims), "s"(material), "s"(packed_bits), "s"(clip_base), "s"(cb[0][0]), "s"(cb[0][1]), "s"(cb[0][2]), "s"(cb[1][0]), "s"(cb[1][1]), "s"(cb[1][2]), "s"(cb[2][0]), "s"(cb[2][1]), "s"(cb[2][2]) : "memory");
      packed_texels = (const uint8_t *)(uintptr_t)packed_bits;
      if (late_clip_slot(clipped, clip_base)) {
        const ConstClip cq = (ConstClip)clip_arena + record_clip_slot(clip_base, ref_u);
        h.X0 = cq->h.X0; h.Y0 = cq->h.Y0; h.l1dx = cq->h.l1dx; h.l1dy = cq->h.l1dy; h.l2dx = cq->h.l2dx; h.l2dy = cq->h.l2dy;
        h.rw0 = cq->h.rw0; h.rw1 = cq->h.rw1; h.rw2 = cq->h.rw2;
#pragma unroll
        for (int jj = 0; jj < 3; ++jj)
#pragma unroll
          for (int k = 0; k < 3; ++k) cb[jj][k] = cq->bary[jj][k];
        clipped = true;
      }
      plane_bary(h, clipped, cb, gx, gy, b0, b1, b2);
      a[0] = interp3(b0, b1, b2, uv[0][0], uv[1][0], uv[2][0]);
      a[1] = interp3(b0, b1, b2, uv[0][1], uv[1][1], uv[2][1]);
      BB_KSTAMP(2);  // head (+ clip slot) arrived, barycentrics and uv done
      // group B: the texel taps first (vector loads, the long pole), the body of the record behind them (scalar loads)
      issue_taps((const void *)(const ShadeRec *)(uintptr_t)rp);
      float body[kNumBodyVary][3];
#pragma unroll
      for (int jj = 0; jj < kNumBodyVary; ++jj)
#pragma unroll
        for (int k = 0; k < 3; ++k) body[jj][k] = rp->vary[jj][k];
#pragma unroll
      for (int q = 0; q < kNumBodyVary; q += 4)
        asm volatile("" :: "s"(body[q][0]), "s"(body[q][1]), "s"(body[q][2]), "s"(body[q + 1][0]), "s"(body[q + 1][1]), "s"(body[q + 1][2]), "s"(body[q + 2][0]), "s"(body[q + 2][1]), "s"(body[q + 2][2]), "s"(body[q + 3][0]), "s"(body[q + 3][1]), "s"(body[q + 3][2]) : "memory");
#pragma unroll
      for (int jj = 0; jj < kNumBodyVary; ++jj) a[2 + jj] = interp3(b0, b1, b2, body[jj][0], body[jj][1], body[jj][2]);
    } else {
      // ---- each lane gathers the record of its own fragment's primitive ----
      const ShadeRec *rp = recs + prim;
      bool clipped = clip1 != 0u;
      const ClipSlot *cp = clip_arena + (clipped ? clip1 - 1u : 0u);
      const PlaneHead *hp = clipped ? &cp->h : &rp->h;
      // group A: three loads of the head (from the record or the clip slot), three of the rest of the record's head,
      // and, for the lanes of clipped fragments, three of the slot's barycentrics
      PlaneHead h = *hp;
      float uv[3][2], cb[3][3] = {};
#pragma unroll
      for (int k = 0; k < 3; ++k) { uv[k][0] = rp->uv[k][0]; uv[k][1] = rp->uv[k][1]; }
      packed_dims = rp->packed_dims;
      material = rp->material;
      unsigned long long packed_bits = (unsigned long long)(uintptr_t)rp->packed;
      uint32_t clip_base = rp->clip_base;
      if (clipped) {
#pragma unroll
        for (int jj = 0; jj < 3; ++jj)
#pragma unroll
          for (int k = 0; k < 3; ++k) cb[jj][k] = cp->bary[jj][k];
      }
      asm volatile("" :: "v"(h.X0), "v"(h.Y0), "v"(h.l1dx), "v"(h.l1dy), "v"(h.l2dx), "v"(h.l2dy), "v"(h.rw0), "v"(h.rw1), "v"(h.rw2), "v"(uv[0][0]), "v"(uv[0][1]), "v"(uv[1][0]), "v"(uv[1][1]), "v"(uv[2][0]), "v"(uv[2][1]), "v"(packed_dims), "v"(material), "v"(packed_bits), "v"(clip_base), "v"(cb[0][0]), "v"(cb[0][1]), "v"(cb[0][2]), "v"(cb[1][0]), "v"(cb[1][1]), "v"(cb[1][2]), "v"(cb[2][0]), "v"(cb[2][1]), "v"(cb[2][2]) : "memory");
      packed_texels = (const uint8_t *)(uintptr_t)packed_bits;
      const bool late = late_clip_slot(clipped, clip_base);
      if (__builtin_expect(__ballot(late) != 0ull, 0)) {
        if (late) {
          const ClipSlot cs = clip_arena[record_clip_slot(clip_base, ref)];
          h = cs.h;
#pragma unroll
          for (int jj = 0; jj < 3; ++jj)
#pragma unroll
            for (int k = 0; k < 3; ++k) cb[jj][k] = cs.bary[jj][k];
          clipped = true;
        }
      }
      plane_bary(h, clipped, cb, gx, gy, b0, b1, b2);
      a[0] = interp3(b0, b1, b2, uv[0][0], uv[1][0], uv[2][0]);
      a[1] = interp3(b0, b1, b2, uv[0][1], uv[1][1], uv[2][1]);
      BB_KSTAMP(2);  // head (+ clip slot) arrived, barycentrics and uv done
      // group B: the first 80 bytes of the record's body (varyings 0..5 whole and two thirds of the sixth), the four texel
      // taps behind them, and -- as soon as the first part has arrived and its six varyings are interpolated, their eighteen
      // registers free again -- the other 64 bytes of the body.  Loads return in order: the second part (the same cache
      // lines as the first: L1 hits) comes back behind the taps, so the group is still one round trip long, and its peak is
      // 20 + 12 loaded registers instead of 36 + 12 (the kernel has 64).
      const float *bp = &rp->vary[0][0];
      float p1[20];
#pragma unroll
      for (int q = 0; q < 20; ++q) p1[q] = bp[q];
      issue_taps(rp);
      asm volatile("" :: "v"(p1[0]), "v"(p1[1]), "v"(p1[2]), "v"(p1[3]), "v"(p1[4]), "v"(p1[5]), "v"(p1[6]), "v"(p1[7]), "v"(p1[8]), "v"(p1[9]), "v"(p1[10]), "v"(p1[11]), "v"(p1[12]), "v"(p1[13]), "v"(p1[14]), "v"(p1[15]), "v"(p1[16]), "v"(p1[17]), "v"(p1[18]), "v"(p1[19]) : "memory");
#pragma unroll
      for (int jj = 0; jj < 6; ++jj) a[2 + jj] = interp3(b0, b1, b2, p1[3 * jj], p1[3 * jj + 1], p1[3 * jj + 2]);
      asm volatile("" :: "v"(a[2]), "v"(a[3]), "v"(a[4]), "v"(a[5]), "v"(a[6]), "v"(a[7]) : "memory");  // (the second part is asked for HERE, not earlier)
      float p2[16];
#pragma unroll
      for (int q = 0; q < 16; ++q) p2[q] = bp[20 + q];
      asm volatile("" :: "v"(p2[0]), "v"(p2[1]), "v"(p2[2]), "v"(p2[3]), "v"(p2[4]), "v"(p2[5]), "v"(p2[6]), "v"(p2[7]), "v"(p2[8]), "v"(p2[9]), "v"(p2[10]), "v"(p2[11]), "v"(p2[12]), "v"(p2[13]), "v"(p2[14]), "v"(p2[15]) : "memory");
      a[8] = interp3(b0, b1, b2, p1[18], p1[19], p2[0]);
#pragma unroll
      for (int jj = 7; jj < kNumBodyVary; ++jj) a[2 + jj] = interp3(b0, b1, b2, p2[3 * jj - 20], p2[3 * jj - 19], p2[3 * jj - 18]);
    }
  }
  // the taps are used from here on: pin them behind the body's fence (they were issued in front of it)
  asm volatile("" :: "v"(t00[0]), "v"(t00[1]), "v"(t00[2]), "v"(t10[0]), "v"(t10[1]), "v"(t10[2]), "v"(t01[0]), "v"(t01[1]), "v"(t01[2]), "v"(t11[0]), "v"(t11[1]), "v"(t11[2]) : "memory");
  __builtin_amdgcn_s_setprio(0);  // (the loads are out: filtering and the light loop at the default priority)

  // texture filtering, forward_brdf.frag:16-22
  const float u = BB_ABLATE(8u) ? 0.5f : a[0], v = BB_ABLATE(8u) ? 0.5f : a[1];
  f3 albedo, normal;
  float metallic, roughness, ao;
  if (!MIXED || packed_dims != 0u) {
    albedo.x = filter_channel(t00[0], t10[0], t01[0], t11[0], 0, tp.fx, tp.fy);
    albedo.y = filter_channel(t00[0], t10[0], t01[0], t11[0], 8, tp.fx, tp.fy);
    albedo.z = filter_channel(t00[0], t10[0], t01[0], t11[0], 16, tp.fx, tp.fy);
    metallic = filter_channel(t00[0], t10[0], t01[0], t11[0], 24, tp.fx, tp.fy);
    roughness = filter_channel(t00[1], t10[1], t01[1], t11[1], 24, tp.fx, tp.fy);
    ao = filter_channel(t00[2], t10[2], t01[2], t11[2], 0, tp.fx, tp.fy);
    normal = surface_normal<DEFERRED>(a, sp.enable_normal_map, [&] {
      return mk3(normal_map_axis(filter_channel(t00[1], t10[1], t01[1], t11[1], 0, tp.fx, tp.fy)),
                 normal_map_axis(filter_channel(t00[1], t10[1], t01[1], t11[1], 8, tp.fx, tp.fy)),
                 normal_map_axis(filter_channel(t00[1], t10[1], t01[1], t11[1], 16, tp.fx, tp.fy)));
    });
  } else {
    // maps of different sizes: one set of taps per map
    const MaterialDesc &md = materials[material];
    albedo = sample_map_rgb(md.maps[kMapAlbedo], u, v);
    metallic = sample_map_r(md.maps[kMapMetallic], u, v);
    roughness = sample_map_r(md.maps[kMapRoughness], u, v);
    ao = sample_map_r(md.maps[kMapAO], u, v);
    normal = surface_normal<DEFERRED>(a, sp.enable_normal_map, [&] {
      const f3 t = sample_map_rgb(md.maps[kMapNormal], u, v);
      return mk3(normal_map_axis(t.x), normal_map_axis(t.y), normal_map_axis(t.z));
    });
  }

  BB_KSTAMP(3);  // varyings, taps arrived, filtered
  float4 color = surface_colour<DEFERRED>(fp, sp, lights_c, mk3(a[2], a[3], a[4]), normal, albedo, metallic, roughness, ao, gbuffer, valid,
                                          gx, gy, [&] { return sample_map_r(materials[material].maps[kMapHeight], u, v); });
  BB_KSTAMP(4);  // light loop done
  if (BB_ABLATE(2u)) color = make_float4(1.f, 1.f, 1.f, 1.f);
  store_colour<PRESENT>(valid, color, o, out, out8, tables, sp);
#ifdef BB_STAMPS
  {
    BB_KSTAMP(5);
    const uint32_t wv = blockIdx.x * (uint32_t)kShadeWaves + (threadIdx.x >> 6);
    if (!TAIL && lane == 0 && wv >= 30000u && wv < 34096u) {  // waves from the middle of the launch: steady state
      unsigned long long *d = g_shade_stamps + (size_t)(wv - 30000u) * 8;
      for (int q = 0; q < 5; ++q) d[q] = st_t[q + 1] - st_t[q];
      d[5] = 1;
    }
  }
#endif
  j += gridDim.x * (uint32_t)kShadeWaves;
  asm volatile("" ::: "memory");
  } while (TAIL && j < n_items);
}

// ------------------------------------------------------------------------------------------------
// k_shade_aniso: k_shade with the sampler's anisotropic filter (option "max_anisotropy" >= 2; src/render.cpp:1349-1350:
// anisotropyEnable, maxAnisotropy = 16, one mip, LOD 0).
//
// With one mip the extra taps are implementation-defined; the rule pinned here is the Vulkan specification's example
// scheme ("Texel Anisotropic Filtering"), in binary32 and in this operand order (restated
// independently in tests/aniso_reference.py):
//   differences  dudx = u(gx + 1, gy) - u(gx, gy), dudy = u(gx, gy + 1) - u(gx, gy), the same for v, where u(X, Y) is this
//                fragment's OWN evaluation of vUV at that pixel centre -- the planes of its (sub-)triangle, its clip-slot
//                matrix -- whatever wins the neighbouring pixel (the hardware's helper lane): nothing is read from another
//                pixel, tile or rank
//   footprint    per map of w x h texels: px2 = (dudx w)^2 + (dvdx h)^2, py2 likewise; the long axis is x iff px2 > py2
//   tap count    N = 1 + #{n in 1..15: n^2 min < max} (= ceil(min(ratio, 16)) without a root or a division), capped by the
//                option; N = 1 when the long axis is at most one texel or a difference is not finite
//   taps         N = 1: the one tap of k_shade, untouched.  Otherwise tap i = 1..N sits at uv + (i / (N + 1) - 1/2) * (the
//                long axis' differences), each a whole bilinear_taps + filter_channel
//   average      the taps summed in order, times the correctly rounded 1 / N
// One launch shades every item (each wave walks the list with the launch's stride), every lane gathers its own record,
// and a lane's tap loop runs two taps per trip so that eight loads are in flight before the first is used; the wave stays
// in the loop until its widest footprint is done.  DUMP = true (bbr_read_surface) also stores what the filter saw and
// produced, 32 floats per covered pixel; the shipped instantiations have no trace of it.
// ------------------------------------------------------------------------------------------------
constexpr int kMaxAnisotropy = 16;
// R[k] = 1 / k correctly rounded, k = 1 .. 17 (R[N + 1] places the taps, R[N] averages them)
__constant__ float kAnisoRcp[kMaxAnisotropy + 2] = {
    0.0f,        1.0f,        1.0f / 2.0f,  1.0f / 3.0f,  1.0f / 4.0f,  1.0f / 5.0f,  1.0f / 6.0f,  1.0f / 7.0f,  1.0f / 8.0f,
    1.0f / 9.0f, 1.0f / 10.0f, 1.0f / 11.0f, 1.0f / 12.0f, 1.0f / 13.0f, 1.0f / 14.0f, 1.0f / 15.0f, 1.0f / 16.0f, 1.0f / 17.0f};
constexpr int kSurfaceFloats = 32;  // one record of bbr_read_surface

// the fragment's vUV at the centre of pixel (px, py), from the planes of its own (sub-)triangle
struct PlaneUV {
  float b0, b1, b2, u, v;
};
BB_DEV PlaneUV plane_uv(const PlaneHead &h, bool clipped, const float (&cb)[3][3], const float (&uv)[3][2], int px, int py) {
  PlaneUV o;
  plane_bary(h, clipped, cb, px, py, o.b0, o.b1, o.b2);
  o.u = interp3(o.b0, o.b1, o.b2, uv[0][0], uv[1][0], uv[2][0]);
  o.v = interp3(o.b0, o.b1, o.b2, uv[0][1], uv[1][1], uv[2][1]);
  return o;
}

struct UvFootprint {
  float u, v, dudx, dvdx, dudy, dvdy;
};
// tap count and the differences of the long axis for a map of w x h texels
struct AnisoTaps {
  int n;
  float du, dv;
  float mx;     // the long axis' squared length in texels (the level rule of k_shade_mip starts from it)
  bool finite;  // all four differences are
};
BB_DEV AnisoTaps aniso_taps(const UvFootprint &f, int w, int h, int max_aniso) {
  const float fw = (float)w, fh = (float)h;
  const float ax = f.dudx * fw, ay = f.dvdx * fh;
  const float px2 = fmaf(ax, ax, ay * ay);
  const float bx = f.dudy * fw, by = f.dvdy * fh;
  const float py2 = fmaf(bx, bx, by * by);
  const bool x_axis = px2 > py2;
  const float mx = x_axis ? px2 : py2, mn = x_axis ? py2 : px2;
  int n = 1;
#pragma unroll
  for (int k = 1; k < kMaxAnisotropy; ++k) n += ((float)(k * k) * mn < mx) ? 1 : 0;
  n = n < max_aniso ? n : max_aniso;
  const float big = 3.402823466e+38f;
  const bool finite = fabsf(f.dudx) <= big && fabsf(f.dvdx) <= big && fabsf(f.dudy) <= big && fabsf(f.dvdy) <= big;
  if (!(mx > 1.0f) || !finite) n = 1;
  AnisoTaps t;
  t.n = n;
  t.du = x_axis ? f.dudx : f.dudy;
  t.dv = x_axis ? f.dvdx : f.dvdy;
  t.mx = mx;
  t.finite = finite;
  return t;
}

// extent of level d of a chain whose level 0 has n texels along this axis: max(1, n >> d)
BB_DEV int level_extent(int n, int d) {
  const int m = n >> d;
  return m > 0 ? m : 1;
}

// What a tap is made of, for the two storage forms.  load() asks for the four texels of the bilinear footprint at (u, v),
// add() filters them and adds every channel to the running sums.
struct PackedFetch {  // the packed material: 9-byte records, block-linear (issue_taps of k_shade)
  static constexpr int kChannels = 9;  // albedo rgb, metallic, roughness, ao, normal xyz
  GlobalBytes texels;
  int w, h;
  struct Raw {
    u32x3 q00, q10, q01, q11;
    float fx, fy;
  };
  BB_DEV Raw load(float u, float v) const {
    const BilinearTaps tp = bilinear_taps<true>(u, v, w, h);
    Raw r;
    r.q00 = *(GlobalTap)(texels + texel_offset(tp.o00)); r.q10 = *(GlobalTap)(texels + texel_offset(tp.o10));
    r.q01 = *(GlobalTap)(texels + texel_offset(tp.o01)); r.q11 = *(GlobalTap)(texels + texel_offset(tp.o11));
    r.fx = tp.fx; r.fy = tp.fy;
    return r;
  }
  BB_DEV int width() const { return w; }
  BB_DEV int height() const { return h; }
  // the same set on level d of its chain, whose texels start at `level`
  BB_DEV PackedFetch at(const uint8_t *level, int d) const { return PackedFetch{(GlobalBytes)level, level_extent(w, d), level_extent(h, d)}; }
  BB_DEV static void add(const Raw &r, float (&acc)[kChannels]) {
    acc[0] = acc[0] + filter_channel(r.q00.x, r.q10.x, r.q01.x, r.q11.x, 0, r.fx, r.fy);
    acc[1] = acc[1] + filter_channel(r.q00.x, r.q10.x, r.q01.x, r.q11.x, 8, r.fx, r.fy);
    acc[2] = acc[2] + filter_channel(r.q00.x, r.q10.x, r.q01.x, r.q11.x, 16, r.fx, r.fy);
    acc[3] = acc[3] + filter_channel(r.q00.x, r.q10.x, r.q01.x, r.q11.x, 24, r.fx, r.fy);
    acc[4] = acc[4] + filter_channel(r.q00.y, r.q10.y, r.q01.y, r.q11.y, 24, r.fx, r.fy);
    acc[5] = acc[5] + filter_channel(r.q00.z, r.q10.z, r.q01.z, r.q11.z, 0, r.fx, r.fy);
    acc[6] = acc[6] + filter_channel(r.q00.y, r.q10.y, r.q01.y, r.q11.y, 0, r.fx, r.fy);
    acc[7] = acc[7] + filter_channel(r.q00.y, r.q10.y, r.q01.y, r.q11.y, 8, r.fx, r.fy);
    acc[8] = acc[8] + filter_channel(r.q00.y, r.q10.y, r.q01.y, r.q11.y, 16, r.fx, r.fy);
  }
};
template <int CHANNELS>
struct MapFetch {  // one RGBA8 map of the material table, its first CHANNELS channels
  static constexpr int kChannels = CHANNELS;
  TexDesc td;
  typedef MapTap Raw;
  BB_DEV Raw load(float u, float v) const { return load_map_tap(td, u, v); }
  BB_DEV int width() const { return td.w; }
  BB_DEV int height() const { return td.h; }
  BB_DEV MapFetch at(const uint8_t *level, int d) const { return MapFetch{TexDesc{level, level_extent(td.w, d), level_extent(td.h, d)}}; }
  BB_DEV static void add(const Raw &r, float (&acc)[kChannels]) {
#pragma unroll
    for (int k = 0; k < kChannels; ++k) acc[k] = acc[k] + map_channel(r, k);
  }
};

// the filtered value of every channel: the average of t.n taps along the long axis (the one tap at (u, v) when t.n = 1)
template <class Fetch>
BB_DEV void aniso_sample(const Fetch &fetch, const UvFootprint &f, const AnisoTaps &t, float (&value)[Fetch::kChannels]) {
  float acc[Fetch::kChannels];
#pragma unroll
  for (int k = 0; k < Fetch::kChannels; ++k) acc[k] = 0.0f;  // (0 + t_1 = t_1 exactly: a tap is never -0)
  const float step = kAnisoRcp[t.n + 1];
  for (int i = 1; i <= t.n; i += 2) {
    // taps i and i + 1: both sets of loads are out before either is filtered
    const bool second = i + 1 <= t.n;
    const float oa = fmaf((float)i, step, -0.5f), ob = fmaf((float)(i + 1), step, -0.5f);
    const float ua = t.n == 1 ? f.u : fmaf(oa, t.du, f.u), va = t.n == 1 ? f.v : fmaf(oa, t.dv, f.v);
    const typename Fetch::Raw ra = fetch.load(ua, va);
    typename Fetch::Raw rb = ra;
    if (second) rb = fetch.load(fmaf(ob, t.du, f.u), fmaf(ob, t.dv, f.v));
    Fetch::add(ra, acc);
    if (second) Fetch::add(rb, acc);
  }
  const float rn = kAnisoRcp[t.n];
#pragma unroll
  for (int k = 0; k < Fetch::kChannels; ++k) value[k] = t.n == 1 ? acc[k] : acc[k] * rn;
}

// The level of detail a filter chose for one texture: level d and the weight delta of level d + 1 (both 0 on level 0 alone)
struct Lod {
  int d;
  float delta;
};

// The filter of "max_anisotropy": level 0 alone.  A filter's sample() takes one texture of a material -- `set` = its map, or
// kMapCount for the packed set -- as the Fetch of its level 0, fills the filtered value of every channel and the level
// choice, and returns the tap count N.
struct AnisoFilter {
  int max_aniso;
  template <class Fetch>
  BB_DEV uint32_t sample(const Fetch &fetch, uint32_t material, int set, const UvFootprint &f, float (&value)[Fetch::kChannels], Lod &lod) const {
    const AnisoTaps t = aniso_taps(f, fetch.width(), fetch.height(), max_aniso);
    aniso_sample(fetch, f, t, value);
    lod = Lod{0, 0.0f};
    return (uint32_t)t.n;
  }
};

// The fragment stage with a footprint: what k_shade_aniso and k_shade_mip are, up to the filter.  One launch shades every
// item (each wave walks the list with the launch's stride) and every lane gathers its own record.
template <int TILE_W, int TILE_H, bool DEFERRED, bool PRESENT, bool DUMP, class Filter, class Shadow = NoShadow>
BB_DEV void shade_item_list(
    const uint32_t *__restrict__ items, const uint32_t *__restrict__ item_count,
    const unsigned long long *__restrict__ frags, const uint32_t *__restrict__ frag_count,
    const ShadeRec *__restrict__ recs, const ClipSlot *__restrict__ clip_arena,
    const FrameParams &fp, const ShadeParams &sp, const CookedLight *__restrict__ cooked,
    const MaterialDesc *__restrict__ materials, float4 *__restrict__ out,
    uint2 *__restrict__ gbuffer, const SrgbTables *__restrict__ tables, uint32_t *__restrict__ out8,
    Counters *__restrict__ ctr, Counters *__restrict__ ctr_done, uint32_t *__restrict__ item_groups, const Filter &filter,
    float *__restrict__ dump, const Shadow &shadow = Shadow{}) {
  constexpr int TILE_PIXELS = TILE_W * TILE_H;
  const ConstLights lights_c{(ConstCooked)cooked};
  retire_counters(ctr, ctr_done, item_groups);
  const int lane = (int)(threadIdx.x & 63u);
  const uint32_t n_items = *item_count;
  for (uint32_t j = (uint32_t)__builtin_amdgcn_readfirstlane((int)(blockIdx.x * (uint32_t)kShadeWaves + (threadIdx.x >> 6)));
       j < n_items; j += gridDim.x * (uint32_t)kShadeWaves) {
    const uint32_t item = items[1u + j];
    const ItemPlace at = decode_item(fp, item);
    bool valid;
    const unsigned long long frag = fetch_fragment<TILE_PIXELS, false>(item, at, lane, frags, frag_count, valid);
    const uint32_t ref = (uint32_t)frag;
    int x, y;
    tile_pixel<TILE_W>(fragment_pixel<TILE_PIXELS>(frag), x, y);
    const int gx = at.tx * TILE_W + x, gy = at.ty * TILE_H + y;
    const size_t o = (size_t)((uint32_t)(at.out_tile_row * TILE_H + y) * (uint32_t)fp.width + (uint32_t)gx);

    // the head of the primitive record and, for a clipped fragment, its sub-triangle's clip slot
    const ShadeRec *rp = recs + (ref >> 3);
    const uint32_t clip1 = (uint32_t)(frag >> (32 + kFragPixBits));  // clip-arena slot + 1 of a clipped sub-triangle, 0: none / unknown
    bool clipped = clip1 != 0u;
    const ClipSlot *cp = clip_arena + (clipped ? clip1 - 1u : 0u);
    PlaneHead h = clipped ? cp->h : rp->h;
    float uv[3][2], cb[3][3] = {};
#pragma unroll
    for (int k = 0; k < 3; ++k) { uv[k][0] = rp->uv[k][0]; uv[k][1] = rp->uv[k][1]; }
    const uint32_t packed_dims = rp->packed_dims, material = rp->material, clip_base = rp->clip_base;
    const GlobalBytes packed_texels = (GlobalBytes)rp->packed;
    if (late_clip_slot(clipped, clip_base)) {
      cp = clip_arena + record_clip_slot(clip_base, ref);
      h = cp->h;
      clipped = true;
    }
    if (clipped) {
#pragma unroll
      for (int jj = 0; jj < 3; ++jj)
#pragma unroll
        for (int k = 0; k < 3; ++k) cb[jj][k] = cp->bary[jj][k];
    }
    const PlaneUV here = plane_uv(h, clipped, cb, uv, gx, gy);
    const PlaneUV right = plane_uv(h, clipped, cb, uv, gx + 1, gy), below = plane_uv(h, clipped, cb, uv, gx, gy + 1);
    UvFootprint f;
    f.u = here.u; f.v = here.v;
    f.dudx = right.u - here.u; f.dvdx = right.v - here.v;
    f.dudy = below.u - here.u; f.dvdy = below.v - here.v;
    const float b0 = here.b0, b1 = here.b1, b2 = here.b2;
    float a[kNumVary];
    a[0] = f.u; a[1] = f.v;
#pragma unroll
    for (int jj = 0; jj < kNumBodyVary; ++jj) a[2 + jj] = interp3(b0, b1, b2, rp->vary[jj][0], rp->vary[jj][1], rp->vary[jj][2]);

    // texture filtering, forward_brdf.frag:16-22 / gbuffer.frag
    const bool normal_map = sp.enable_normal_map != 0;
    f3 albedo, nt = mk3(0.f, 0.f, 0.f);
    float metallic, roughness, ao, height = 0.0f;
    uint32_t taps[kMapCount] = {};  // (DUMP: the tap count used for each map, 0 = not sampled)
    Lod lod = {0, 0.0f}, height_lod = {0, 0.0f};  // (DUMP: the level choice of the packed set / the albedo map, and of the height map)
    const MaterialDesc &md = materials[material];
    if (packed_dims != 0u) {
      const PackedFetch fetch{packed_texels, (int)(packed_dims & 0xFFFFu), (int)(packed_dims >> 16)};
      float s[PackedFetch::kChannels];
      const uint32_t n = filter.sample(fetch, material, kMapCount, f, s, lod);
      albedo = mk3(s[0], s[1], s[2]);
      metallic = s[3]; roughness = s[4]; ao = s[5];
      if (normal_map) nt = mk3(normal_map_axis(s[6]), normal_map_axis(s[7]), normal_map_axis(s[8]));
      taps[kMapAlbedo] = taps[kMapMetallic] = taps[kMapRoughness] = taps[kMapAO] = n;
      if (normal_map) taps[kMapNormal] = n;
    } else {
      // maps of different sizes: a tap count, a level choice and a tap loop per map
      auto one = [&](int map, auto channels, float *value, Lod &map_lod) {
        const MapFetch<decltype(channels)::value> fetch{md.maps[map]};
        float s[decltype(channels)::value];
        taps[map] = filter.sample(fetch, material, map, f, s, map_lod);
#pragma unroll
        for (int k = 0; k < decltype(channels)::value; ++k) value[k] = s[k];
      };
      float s3[3];
      Lod other;
      one(kMapAlbedo, std::integral_constant<int, 3>{}, s3, lod);
      albedo = mk3(s3[0], s3[1], s3[2]);
      one(kMapMetallic, std::integral_constant<int, 1>{}, &metallic, other);
      one(kMapRoughness, std::integral_constant<int, 1>{}, &roughness, other);
      one(kMapAO, std::integral_constant<int, 1>{}, &ao, other);
      if (normal_map) {
        one(kMapNormal, std::integral_constant<int, 3>{}, s3, other);
        nt = mk3(normal_map_axis(s3[0]), normal_map_axis(s3[1]), normal_map_axis(s3[2]));
      }
    }
    const f3 normal = surface_normal<DEFERRED>(a, sp.enable_normal_map, [&] { return nt; });
    if (DEFERRED && (DUMP || gbuffer) && valid) {  // gbuffer.frag's sixth fetch: only when somebody asked to see the texel
      const MapFetch<1> fetch{md.maps[kMapHeight]};
      float s[1];
      taps[kMapHeight] = filter.sample(fetch, material, kMapHeight, f, s, height_lod);
      height = s[0];
    }
    if (DUMP && valid) {
      float *d = dump + ((size_t)gy * (size_t)fp.width + (size_t)gx) * kSurfaceFloats;
      const float rec[kSurfaceFloats] = {f.u, f.v, f.dudx, f.dvdx, f.dudy, f.dvdy, a[2], a[3], a[4], normal.x, normal.y, normal.z,
                                         albedo.x, albedo.y, albedo.z, metallic, roughness, ao, height, nt.x, nt.y, nt.z,
                                         (float)taps[0], (float)taps[1], (float)taps[2], (float)taps[3], (float)taps[4], (float)taps[5],
                                         (float)lod.d, lod.delta, (float)height_lod.d, height_lod.delta};
#pragma unroll
      for (int k = 0; k < kSurfaceFloats; ++k) d[k] = rec[k];
    }

    const float4 color = surface_colour<DEFERRED>(fp, sp, lights_c, mk3(a[2], a[3], a[4]), normal, albedo, metallic, roughness, ao, gbuffer,
                                                  valid, gx, gy, [&] { return height; }, shadow);
    store_colour<PRESENT>(valid, color, o, out, out8, tables, sp);
  }
}

template <int TILE_W, int TILE_H, bool DEFERRED, bool PRESENT, bool DUMP = false>
__global__ __launch_bounds__(kShadeThreads) void k_shade_aniso(
    const uint32_t *__restrict__ items, const uint32_t *__restrict__ item_count,
    const unsigned long long *__restrict__ frags, const uint32_t *__restrict__ frag_count,
    const ShadeRec *__restrict__ recs, const ClipSlot *__restrict__ clip_arena,
    FrameParams fp, ShadeParams sp, const CookedLight *__restrict__ cooked,
    const MaterialDesc *__restrict__ materials, float4 *__restrict__ out,
    uint2 *__restrict__ gbuffer, const SrgbTables *__restrict__ tables, uint32_t *__restrict__ out8,
    Counters *__restrict__ ctr, Counters *__restrict__ ctr_done, uint32_t *__restrict__ item_groups, int max_aniso,
    float *__restrict__ dump) {
  shade_item_list<TILE_W, TILE_H, DEFERRED, PRESENT, DUMP>(items, item_count, frags, frag_count, recs, clip_arena, fp, sp, cooked, materials, out,
                                                           gbuffer, tables, out8, ctr, ctr_done, item_groups, AnisoFilter{max_aniso}, dump);
}

// k_shade_shadow: the fragment stage of k_shade_aniso ("max_anisotropy" 1 .. 16) with the shadow test in front of the caster's
// iteration of the light loop (the rule: at the head of "Shadow mapping").  The test is evaluated in surface_colour, behind the filter,
// where the footprint's registers are dead.  DUMP as in k_shade_aniso, plus the class of every pixel where `shadow.mask` is set.
template <int TILE_W, int TILE_H, bool DEFERRED, bool PRESENT, bool DUMP = false>
__global__ __launch_bounds__(kShadeThreads) void k_shade_shadow(
    const uint32_t *__restrict__ items, const uint32_t *__restrict__ item_count,
    const unsigned long long *__restrict__ frags, const uint32_t *__restrict__ frag_count,
    const ShadeRec *__restrict__ recs, const ClipSlot *__restrict__ clip_arena,
    FrameParams fp, ShadeParams sp, const CookedLight *__restrict__ cooked,
    const MaterialDesc *__restrict__ materials, float4 *__restrict__ out,
    uint2 *__restrict__ gbuffer, const SrgbTables *__restrict__ tables, uint32_t *__restrict__ out8,
    Counters *__restrict__ ctr, Counters *__restrict__ ctr_done, uint32_t *__restrict__ item_groups, int max_aniso,
    float *__restrict__ dump, ShadowArgs shadow) {
  shade_item_list<TILE_W, TILE_H, DEFERRED, PRESENT, DUMP>(items, item_count, frags, frag_count, recs, clip_arena, fp, sp, cooked, materials, out,
                                                           gbuffer, tables, out8, ctr, ctr_done, item_groups, AnisoFilter{max_aniso}, dump,
                                                           ShadowTest<DUMP>{shadow});
}

// k_shade_shadow_faces: k_shade_shadow with 2 .. 6 faces for the caster (the rule: in front of ShadowFacesArgs).  DUMP as in
// k_shade_shadow, plus the deciding face of every pixel where `shadow.face` is set.
template <int TILE_W, int TILE_H, bool DEFERRED, bool PRESENT, bool DUMP = false>
__global__ __launch_bounds__(kShadeThreads) void k_shade_shadow_faces(
    const uint32_t *__restrict__ items, const uint32_t *__restrict__ item_count,
    const unsigned long long *__restrict__ frags, const uint32_t *__restrict__ frag_count,
    const ShadeRec *__restrict__ recs, const ClipSlot *__restrict__ clip_arena,
    FrameParams fp, ShadeParams sp, const CookedLight *__restrict__ cooked,
    const MaterialDesc *__restrict__ materials, float4 *__restrict__ out,
    uint2 *__restrict__ gbuffer, const SrgbTables *__restrict__ tables, uint32_t *__restrict__ out8,
    Counters *__restrict__ ctr, Counters *__restrict__ ctr_done, uint32_t *__restrict__ item_groups, int max_aniso,
    float *__restrict__ dump, ShadowFacesArgs shadow) {
  shade_item_list<TILE_W, TILE_H, DEFERRED, PRESENT, DUMP>(items, item_count, frags, frag_count, recs, clip_arena, fp, sp, cooked, materials, out,
                                                           gbuffer, tables, out8, ctr, ctr_done, item_groups, AnisoFilter{max_aniso}, dump,
                                                           ShadowFacesTest<DUMP>{shadow});
}

// k_shade_shadow_pcf: k_shade_shadow / k_shade_shadow_faces with option "shadow_filter" (the rule: in front of ShadowPcfArgs), one
// kernel for 1 .. 6 faces and both radii.  DUMP as in k_shade_shadow_faces, plus k of every pixel where `shadow.taps` is set.
template <int TILE_W, int TILE_H, bool DEFERRED, bool PRESENT, bool DUMP = false>
__global__ __launch_bounds__(kShadeThreads) void k_shade_shadow_pcf(
    const uint32_t *__restrict__ items, const uint32_t *__restrict__ item_count,
    const unsigned long long *__restrict__ frags, const uint32_t *__restrict__ frag_count,
    const ShadeRec *__restrict__ recs, const ClipSlot *__restrict__ clip_arena,
    FrameParams fp, ShadeParams sp, const CookedLight *__restrict__ cooked,
    const MaterialDesc *__restrict__ materials, float4 *__restrict__ out,
    uint2 *__restrict__ gbuffer, const SrgbTables *__restrict__ tables, uint32_t *__restrict__ out8,
    Counters *__restrict__ ctr, Counters *__restrict__ ctr_done, uint32_t *__restrict__ item_groups, int max_aniso,
    float *__restrict__ dump, ShadowPcfArgs shadow) {
  shade_item_list<TILE_W, TILE_H, DEFERRED, PRESENT, DUMP>(items, item_count, frags, frag_count, recs, clip_arena, fp, sp, cooked, materials, out,
                                                           gbuffer, tables, out8, ctr, ctr_done, item_groups, AnisoFilter{max_aniso}, dump,
                                                           ShadowPcfTest<DUMP>{shadow});
}

// k_shade_shadow_casters: the kernel of a context with a caster slot other than 0 in use (the rule: in front of
// ShadowCasterEntry), one kernel for every number of casters, 1 .. 6 faces each and R = 0 .. 2.  DUMP as in k_shade_shadow_pcf,
// for the slot `shadow.dump_slot`.
template <int TILE_W, int TILE_H, bool DEFERRED, bool PRESENT, bool DUMP = false>
__global__ __launch_bounds__(kShadeThreads) void k_shade_shadow_casters(
    const uint32_t *__restrict__ items, const uint32_t *__restrict__ item_count,
    const unsigned long long *__restrict__ frags, const uint32_t *__restrict__ frag_count,
    const ShadeRec *__restrict__ recs, const ClipSlot *__restrict__ clip_arena,
    FrameParams fp, ShadeParams sp, const CookedLight *__restrict__ cooked,
    const MaterialDesc *__restrict__ materials, float4 *__restrict__ out,
    uint2 *__restrict__ gbuffer, const SrgbTables *__restrict__ tables, uint32_t *__restrict__ out8,
    Counters *__restrict__ ctr, Counters *__restrict__ ctr_done, uint32_t *__restrict__ item_groups, int max_aniso,
    float *__restrict__ dump, ShadowCastersArgs shadow) {
  shade_item_list<TILE_W, TILE_H, DEFERRED, PRESENT, DUMP>(items, item_count, frags, frag_count, recs, clip_arena, fp, sp, cooked, materials, out,
                                                           gbuffer, tables, out8, ctr, ctr_done, item_groups, AnisoFilter{max_aniso}, dump,
                                                           ShadowCastersTest<DUMP>{shadow});
}

// ------------------------------------------------------------------------------------------------
// Mip chains and the trilinear filter (option "mip_levels" >= 2; src/render.cpp:1363-1365: the reference's sampler has
// mipmapMode LINEAR, on images of one level).  The rule, in binary32 and in this operand order (DESIGN.md section 3;
// restated independently in tests/mip_reference.py):
//   chain      a map of w x h texels has L = min(mip_levels, 1 + floor(log2 max(w, h))) levels, level k of max(1, w >> k) x
//              max(1, h >> k) texels.  Per channel byte, texel (x, y) of level k + 1 = (s + 2) >> 2, s the integer sum of
//              the level-k bytes at columns min(2x, w_k - 1), min(2x + 1, w_k - 1) and the same two rows.  A packed
//              material's level k is the packed form (bb_pack.h) of the five level-k maps.
//   N          the anisotropic rule's footprint and tap count on the LEVEL-0 size (mx: the long axis' squared length)
//   level      P = mx * R2[N], R2[k] the binary32 nearest to 1 / k^2.  A difference not finite, or !(P > 1): d = 0, delta = 0.
//              Otherwise from P's bits b: e = (b >> 23) - 127, d = e >> 1, delta = 0.5 * ((float)(e & 1) + (float)(b &
//              0x7FFFFF) * 2^-23), every step exact; d >= L - 1 (+inf included): d = L - 1, delta = 0.  (lambda = 1/2 log2 P
//              with log2(1 + t) taken as t: low by at most 0.043 level)
//   value      hi = the anisotropic rule's taps and average on level d's size (tap offsets are in uv: the same on every
//              level; wrapping and the 2^30 cutoff per level); delta == 0: value = hi, nothing else happens; otherwise lo =
//              the same on level d + 1 and value = fmaf(delta, lo - hi, hi) per channel.
// The chain is built at upload / option time by k_mip_reduce and k_mip_pack; the shading kernel finds the levels through
// a table per material (MipTable) that only it reads.
// ------------------------------------------------------------------------------------------------
constexpr int kMaxMipLevels = 15;        // the full chain of the largest map the ABI takes (16384)
constexpr int kMipSets = kMapCount + 1;  // the six maps, and the packed set (index kMapCount)
struct MipSet {
  int32_t levels;  // L >= 1 of a live material
  int32_t pad;
  const uint8_t *level[kMaxMipLevels];  // where level k's texels start (level 0: the material's own allocation)
};
struct MipTable {
  MipSet set[kMipSets];
};
static_assert(sizeof(MipSet) == 128 && sizeof(MipTable) == 896, "MipTable");

// R2[k] = 1 / k^2 correctly rounded, k = 1 .. 16
__constant__ float kMipRcp2[kMaxAnisotropy + 1] = {
    0.0f,         1.0f,          1.0f / 4.0f,   1.0f / 9.0f,   1.0f / 16.0f,  1.0f / 25.0f,  1.0f / 36.0f,  1.0f / 49.0f, 1.0f / 64.0f,
    1.0f / 81.0f, 1.0f / 100.0f, 1.0f / 121.0f, 1.0f / 144.0f, 1.0f / 169.0f, 1.0f / 196.0f, 1.0f / 225.0f, 1.0f / 256.0f};

// the level rule: d and delta from the footprint's long axis mx, the tap count n and the number of levels
BB_DEV Lod mip_level(const AnisoTaps &t, int levels) {
  Lod lod = {0, 0.0f};
  const float P = t.mx * kMipRcp2[t.n];
  if (t.finite && P > 1.0f) {
    const uint32_t b = __float_as_uint(P);
    const int e = (int)(b >> 23) - 127;
    lod.d = e >> 1;
    lod.delta = 0.5f * ((float)(e & 1) + (float)(b & 0x7FFFFFu) * 1.1920928955078125e-07f);
    if (lod.d >= levels - 1) lod = Lod{levels - 1, 0.0f};
  }
  return lod;
}

struct MipFilter {
  int max_aniso;
  const MipTable *__restrict__ tables;
  template <class Fetch>
  BB_DEV uint32_t sample(const Fetch &fetch, uint32_t material, int set, const UvFootprint &f, float (&value)[Fetch::kChannels], Lod &lod) const {
    const MipSet &ms = tables[material].set[set];
    const AnisoTaps t = aniso_taps(f, fetch.width(), fetch.height(), max_aniso);
    lod = mip_level(t, ms.levels);
    aniso_sample(fetch.at(ms.level[lod.d], lod.d), f, t, value);
    if (lod.delta != 0.0f) {  // (d + 1 <= L - 1 here; a wave whose lanes all sit on one level skips this)
      float lo[Fetch::kChannels];
      aniso_sample(fetch.at(ms.level[lod.d + 1], lod.d + 1), f, t, lo);
#pragma unroll
      for (int k = 0; k < Fetch::kChannels; ++k) value[k] = fmaf(lod.delta, lo[k] - value[k], value[k]);
    }
    return (uint32_t)t.n;
  }
};

// k_shade_mip: the fragment stage with the trilinear filter, whatever "max_anisotropy" is.  DUMP as in k_shade_aniso.
template <int TILE_W, int TILE_H, bool DEFERRED, bool PRESENT, bool DUMP = false>
__global__ __launch_bounds__(kShadeThreads) __attribute__((amdgpu_waves_per_eu(4))) void k_shade_mip(
    const uint32_t *__restrict__ items, const uint32_t *__restrict__ item_count,
    const unsigned long long *__restrict__ frags, const uint32_t *__restrict__ frag_count,
    const ShadeRec *__restrict__ recs, const ClipSlot *__restrict__ clip_arena,
    FrameParams fp, ShadeParams sp, const CookedLight *__restrict__ cooked,
    const MaterialDesc *__restrict__ materials, float4 *__restrict__ out,
    uint2 *__restrict__ gbuffer, const SrgbTables *__restrict__ tables, uint32_t *__restrict__ out8,
    Counters *__restrict__ ctr, Counters *__restrict__ ctr_done, uint32_t *__restrict__ item_groups, int max_aniso,
    const MipTable *__restrict__ mip_tables, float *__restrict__ dump) {
  shade_item_list<TILE_W, TILE_H, DEFERRED, PRESENT, DUMP>(items, item_count, frags, frag_count, recs, clip_arena, fp, sp, cooked, materials, out,
                                                           gbuffer, tables, out8, ctr, ctr_done, item_groups,
                                                           MipFilter{max_aniso, mip_tables}, dump);
}

// One level of a row-major RGBA8 chain from the one above: texel (x, y) of the w1 x h1 level below a w0 x h0 level.  One
// thread per texel; the four bytes of a texel are reduced side by side.
constexpr int kMipThreads = 256;
__global__ __launch_bounds__(kMipThreads) void k_mip_reduce(const uint32_t *__restrict__ src, int w0, int h0, uint32_t *__restrict__ dst,
                                                            int w1, int h1) {
  const uint32_t i = blockIdx.x * (uint32_t)kMipThreads + threadIdx.x;
  if (i >= (uint32_t)w1 * (uint32_t)h1) return;
  const int x = (int)(i % (uint32_t)w1), y = (int)(i / (uint32_t)w1);
  const int x0 = min(2 * x, w0 - 1), x1 = min(2 * x + 1, w0 - 1), y0 = min(2 * y, h0 - 1), y1 = min(2 * y + 1, h0 - 1);
  const uint32_t a = src[(size_t)y0 * w0 + x0], b = src[(size_t)y0 * w0 + x1], c = src[(size_t)y1 * w0 + x0], d = src[(size_t)y1 * w0 + x1];
  uint32_t r = 0;
#pragma unroll
  for (int k = 0; k < 32; k += 8) {
    const uint32_t s = ((a >> k) & 255u) + ((b >> k) & 255u) + ((c >> k) & 255u) + ((d >> k) & 255u);
    r |= ((s + 2u) >> 2) << k;
  }
  dst[i] = r;
}

// One packed level from the row-major level of the five shaded maps (PBRMapType order; nullptr: the map is not supplied
// and broadcasts its texel of `defaults`, kMapCount RGBA8 texels): the records of bb_pack.h, block-linear.  One thread
// per record SLOT of the ceil(w / 4) x ceil(h / 4) blocks, so the padding records of the last block column / row are
// written (zero), and the first kPackedTexelPad threads also zero the bytes behind the last record: every byte of the level.
struct MipPackMaps {
  const uint8_t *map[5];
};
__global__ __launch_bounds__(kMipThreads) void k_mip_pack(MipPackMaps maps, const uint8_t *__restrict__ defaults, int w, int h,
                                                          uint8_t *__restrict__ out) {
  const uint32_t w4 = ((uint32_t)w + 3u) >> 2, h4 = ((uint32_t)h + 3u) >> 2, n_slots = w4 * h4 * 16u;
  const uint32_t i = blockIdx.x * (uint32_t)kMipThreads + threadIdx.x;
  if (i < kPackedTexelPad) out[(size_t)n_slots * kPackedTexelBytes + i] = 0;
  if (i >= n_slots) return;
  const uint32_t block = i >> 4, x = (block % w4) * 4u + (i & 3u), y = (block / w4) * 4u + ((i >> 2) & 3u);
  uint8_t t[kPackedTexelBytes] = {};
  if (x < (uint32_t)w && y < (uint32_t)h) {
    const size_t at = ((size_t)y * (size_t)w + x) * 4;
    auto texel = [&](int k) { return maps.map[k] ? maps.map[k] + at : defaults + 4 * k; };
    const uint8_t *al = texel(kMapAlbedo), *me = texel(kMapMetallic), *ro = texel(kMapRoughness), *ao = texel(kMapAO), *no = texel(kMapNormal);
    t[0] = al[0]; t[1] = al[1]; t[2] = al[2]; t[3] = me[0];
    t[4] = no[0]; t[5] = no[1]; t[6] = no[2]; t[7] = ro[0];
    t[8] = ao[0];
  }
  uint8_t *o = out + (size_t)i * kPackedTexelBytes;
#pragma unroll
  for (int k = 0; k < (int)kPackedTexelBytes; ++k) o[k] = t[k];
}

// ------------------------------------------------------------------------------------------------
// small utility kernels
// ------------------------------------------------------------------------------------------------

// bb_rcp / bb_rcp_normal against the IEEE division and max0 against its select form, for every float with bit pattern
// in [lo, hi) and its negation: number of differing results
__global__ void k_selftest_rcp(unsigned long long *__restrict__ mismatches, uint32_t lo, uint32_t hi) {
  const uint32_t stride = gridDim.x * blockDim.x;
  unsigned long long bad = 0;
  for (uint64_t u = (uint64_t)lo + blockIdx.x * blockDim.x + threadIdx.x; u < hi; u += stride) {
    const float x = __uint_as_float((uint32_t)u);
    const float a = bb_rcp(x), b = 1.0f / x, c = bb_rcp(-x);
    bad += (__float_as_uint(a) != __float_as_uint(b) && !(a != a && b != b)) || (__float_as_uint(c) != (__float_as_uint(b) ^ 0x80000000u) && !(c != c && b != b));
    // the unguarded variant on its documented domain [2^-100, 2^100]
    if (u >= 0x0D800000u && u <= 0x71800000u) bad += __float_as_uint(bb_rcp_normal(x)) != __float_as_uint(b);
    // max0 == (a > 0 ? a : 0), both signs, every pattern (NaN -> +0, -0 -> +0)
    const float nx = -x;
    bad += __float_as_uint(max0(x)) != __float_as_uint(x > 0.0f ? x : 0.0f);
    bad += __float_as_uint(max0(nx)) != __float_as_uint(nx > 0.0f ? nx : 0.0f);
    bad += __float_as_uint(__builtin_fmaxf(x, 0.001f)) != __float_as_uint(!(x > 0.001f) ? 0.001f : x);
    bad += __float_as_uint(__builtin_fmaxf(nx, 0.001f)) != __float_as_uint(!(nx > 0.001f) ? 0.001f : nx);
  }
  if (bad) atomicAdd(mismatches, bad);
}

// ------------------------------------------------------------------------------------------------
// presentation: HDR attachment (binary16) -> hdr_tone_mapping.frag:9-18 -> sRGB UNORM8.
// Same fixed sequences as the CPU oracle (binary16 rounding, exp, threshold table): byte-exact.
// ------------------------------------------------------------------------------------------------

// hdr_tone_mapping.frag:9-18 on the fp32 frame, in place
__global__ void k_tone_map(float4 *__restrict__ frame, size_t n, int enable, float exposure) {
  size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  float4 c = frame[i];
  if (enable) {
    c.x = 1.0f - bb_exp(-c.x * exposure);
    c.y = 1.0f - bb_exp(-c.y * exposure);
    c.z = 1.0f - bb_exp(-c.z * exposure);
  }
  c.w = 1.0f;
  frame[i] = c;
}

// 16 B read + 4 B written per pixel: 20 algorithmic bytes, HBM-bound by construction.  A workgroup loads the 4.3 KB
// of tables once and converts 2048 pixels (eight coalesced rounds of 256).
constexpr int kPresentThreads = 256;
constexpr int kPresentPerThread = 8;
// k_present's whole body, stated once: k_present takes the exposure as a kernel argument, k_present_auto (option
// "auto_exposure") loads it from device memory and calls the same text
BB_DEV void present_body(const float4 *__restrict__ frame, uint32_t *__restrict__ out_rgba8, size_t n,
                         const SrgbTables *__restrict__ tables, int enable, float exposure, int hdr16) {
  __shared__ SrgbTables t;
  {
    const uint32_t *src = reinterpret_cast<const uint32_t *>(tables);
    uint32_t *dst = reinterpret_cast<uint32_t *>(&t);
    for (uint32_t w = threadIdx.x; w < sizeof(SrgbTables) / 4; w += kPresentThreads) dst[w] = src[w];
  }
  __syncthreads();
  const size_t base = (size_t)blockIdx.x * (kPresentThreads * kPresentPerThread) + threadIdx.x;
#pragma unroll 2
  for (int j = 0; j < kPresentPerThread; ++j) {
    const size_t i = base + (size_t)j * kPresentThreads;
    if (i >= n) break;
    // (the fp32 frame is read once, the presented image written once: both non-temporal)
    const v4f c = __builtin_nontemporal_load(reinterpret_cast<const v4f *>(frame) + i);
    const uint32_t px = present_pixel(c.x, c.y, c.z, t, enable, exposure, hdr16);
    store_pixel(&out_rgba8[i], px);
  }
}
__global__ __launch_bounds__(kPresentThreads) void k_present(const float4 *__restrict__ frame, uint32_t *__restrict__ out_rgba8,
                                                              size_t n, const SrgbTables *__restrict__ tables, int enable,
                                                              float exposure, int hdr16) {
  present_body(frame, out_rgba8, n, tables, enable, exposure, hdr16);
}

// ------------------------------------------------------------------------------------------------
// supersampling (option "supersample", n = 2..4): the resolve of the fine frame, VK_RESOLVE_MODE_AVERAGE over the n x n
// regular grid.  Output pixel (x, y) of the W x rows frame, all four channels, in binary32 without contraction:
//   acc = f(nx, ny);  acc += f(nx + i, ny + j) for (i, j) != (0, 0), row-major, i fastest;  out = acc * R[n]
// A streaming kernel: 16 n^2 B read + 16 B written per output pixel (PRESENT: + 4 B), nothing reused.  One lane per output
// pixel; per fine row it loads its n contiguous float4 (16-byte non-temporal loads: the 64 lanes of a wave cover 64 * 16 n
// contiguous bytes of the row), adds them in the pinned order, and stores non-temporally like k_present.  blockIdx.y is the
// output row, so no lane divides; addresses are size_t (a 32768-wide fine frame passes 2^32 bytes within a few rows).
// The rows below the first are a rolled loop: a lane then holds one fine row of its pixel at a time (n float4) instead of
// all n^2, and the kernel keeps the 64-register allocation of eight waves per SIMD.
// PRESENT (option "present_fused" with n >= 2): the resolved pixel goes through present_pixel (binary16 stage included)
// and is stored as RGBA8; the tables are staged in LDS as k_present stages them -- once per workgroup, i.e. per 256 pixels
// of one row: 4.3 KB of L2 reads beside the 16 KB of samples at n = 2.  A form in which a workgroup covered eight rows with one
// staging measured no faster (116.0 against 115.1 us at 3840 x 2160), so the tables' traffic is not what the form costs.
// ------------------------------------------------------------------------------------------------
constexpr int kResolveThreads = 256;
template <int N>
BB_DEV constexpr float resolve_scale() {
  static_assert(N >= 2 && N <= 4, "supersample: n = 2 .. 4 are resolved");
  return N == 2 ? 0.25f : (N == 3 ? 1.0f / 9.0f : 0.0625f);  // R[3]: the binary32 nearest 1/9 (0x3DE38E39), a constant
}
BB_DEV v4f resolve_add(v4f a, v4f b) {
  // (plain adds: nothing here may become an fma, and the order is the rule's)
  return v4f{__fadd_rn(a.x, b.x), __fadd_rn(a.y, b.y), __fadd_rn(a.z, b.z), __fadd_rn(a.w, b.w)};
}
template <int N>
BB_DEV v4f resolve_row(const v4f *__restrict__ row, v4f acc, bool first) {
  v4f v[N];
#pragma unroll
  for (int i = 0; i < N; ++i) v[i] = __builtin_nontemporal_load(row + i);
  if (first) acc = v[0];
  else acc = resolve_add(acc, v[0]);
#pragma unroll
  for (int i = 1; i < N; ++i) acc = resolve_add(acc, v[i]);
  return acc;
}
template <int N>
BB_DEV float4 resolve_pixel(const float4 *__restrict__ fine, int32_t width, int32_t x, size_t y) {
  const size_t fine_pitch = (size_t)width * N;
  const v4f *row = reinterpret_cast<const v4f *>(fine) + (y * N) * fine_pitch + (size_t)x * N;
  v4f acc = resolve_row<N>(row, v4f{0.f, 0.f, 0.f, 0.f}, true);
#pragma unroll 1
  for (int j = 1; j < N; ++j) {
    row += fine_pitch;
    acc = resolve_row<N>(row, acc, false);
  }
  constexpr float r = resolve_scale<N>();
  return make_float4(__fmul_rn(acc.x, r), __fmul_rn(acc.y, r), __fmul_rn(acc.z, r), __fmul_rn(acc.w, r));
}
// PRESENT: the workgroup's copy of the presentation tables (every thread calls this; it ends in a barrier)
BB_DEV void resolve_stage_tables(SrgbTables &t, const SrgbTables *__restrict__ tables) {
  const uint32_t *src = reinterpret_cast<const uint32_t *>(tables);
  uint32_t *dst = reinterpret_cast<uint32_t *>(&t);
  for (uint32_t w = threadIdx.x; w < sizeof(SrgbTables) / 4; w += kResolveThreads) dst[w] = src[w];
  __syncthreads();
}
template <int N, bool PRESENT>
__global__ __launch_bounds__(kResolveThreads) void k_resolve(const float4 *__restrict__ fine, float4 *__restrict__ out,
                                                              uint32_t *__restrict__ out_rgba8, int32_t width,
                                                              const SrgbTables *__restrict__ tables, int enable, float exposure) {
  const int32_t x = (int32_t)(blockIdx.x * kResolveThreads + threadIdx.x);
  const size_t y = blockIdx.y, o = y * (size_t)width + (size_t)x;
  if constexpr (PRESENT) {
    __shared__ SrgbTables t;
    resolve_stage_tables(t, tables);
    if (x >= width) return;
    const float4 px = resolve_pixel<N>(fine, width, x, y);
    store_pixel(&out_rgba8[o], present_pixel(px.x, px.y, px.z, t, enable, exposure, 1));
  } else {
    if (x >= width) return;
    store_pixel(&out[o], resolve_pixel<N>(fine, width, x, y));
  }
}

// ------------------------------------------------------------------------------------------------
// bloom (option "bloom", L = 1..8; the rule: include/bibim_hip.h "bloom").  Between the fp32 frame and the
// presented image: a bright pass, L box-filtered levels down (w_k = (w_{k-1} + 1) >> 1), a tent filter back up that adds
// level to level, and k_present_bloom, which is k_present with I * up(U_1) added in front of present_pixel.  The frame itself
// is only read.  Every + - * is one IEEE operation (__fadd_rn / __fsub_rn / __fmul_rn): nothing may contract into an fma.
// A level is w_k x h_k float4 texels (r, g, b, 0): 16-byte accesses like the frame's; the levels of one pyramid lie one
// behind the other in one allocation, each starting on a 16-byte boundary by construction.
// All four are streaming kernels shaped like k_resolve: one lane per texel of the grid they write, blockIdx.y its row (no
// lane divides), size_t addresses (a 32768-wide frame passes 2^32 bytes).  The levels are read again by the next launch,
// so their accesses are ordinary ones, and so is k_bloom_first's read of the frame (k_present_bloom reads it again); that
// second read and the image's store are non-temporal as in k_present.
//   k_bloom_first    F -> D_1: per D_1 texel the two contiguous float4 of each of its two source rows (k_resolve<2>'s access
//                    shape), the bright pass on each, the box.  Odd W / H: the last column / row is read twice (the clamp).
//   k_bloom_down     D_k -> D_{k+1}: the box alone.
//   k_bloom_up       U_k = D_k + up(U_{k+1}), in place over D_k: a lane reads and writes its own texel of level k only.
//   k_present_bloom  LDS: the sRGB tables (sizeof(SrgbTables)) and nothing else; the four U_1 taps come from the L2.
// ------------------------------------------------------------------------------------------------
constexpr int kMaxBloomLevels = 8;
constexpr int kBloomThreads = 256;
constexpr float kBloomMax = 65504.0f;  // the bright pass's ceiling: the largest binary16 (every level stays finite)
BB_DEV v4f bloom_bright(v4f f, float threshold) {
  // max0: NaN -> +0, -0 -> +0, -inf -> 0; the min: +inf -> 65504
  return v4f{__builtin_fminf(max0(__fsub_rn(f.x, threshold)), kBloomMax), __builtin_fminf(max0(__fsub_rn(f.y, threshold)), kBloomMax),
             __builtin_fminf(max0(__fsub_rn(f.z, threshold)), kBloomMax), 0.0f};
}
// ((a + b) + (c + d)) * 0.25, per channel
BB_DEV v4f bloom_box(v4f a, v4f b, v4f c, v4f d) {
  const v4f s = resolve_add(resolve_add(a, b), resolve_add(c, d));
  return v4f{__fmul_rn(s.x, 0.25f), __fmul_rn(s.y, 0.25f), __fmul_rn(s.z, 0.25f), 0.0f};
}
BB_DEV float bloom_lerp4(float a, float b) { return __fadd_rn(a, __fmul_rn(__fsub_rn(b, a), 0.25f)); }
BB_DEV v4f bloom_lerp4(v4f a, v4f b) { return v4f{bloom_lerp4(a.x, b.x), bloom_lerp4(a.y, b.y), bloom_lerp4(a.z, b.z), 0.0f}; }
// up(G, w, h)(x, y), (x, y) a texel of the next finer grid: the near texel and its neighbour towards (x, y), 9 3 3 1 / 16
BB_DEV v4f bloom_up(const float4 *__restrict__ g, int32_t w, int32_t h, int32_t x, int32_t y) {
  const int32_t px = x >> 1, py = y >> 1;
  const int32_t qx = min(max(px + ((x & 1) ? 1 : -1), 0), w - 1), qy = min(max(py + ((y & 1) ? 1 : -1), 0), h - 1);
  const v4f *rp = reinterpret_cast<const v4f *>(g) + (size_t)py * (size_t)w, *rq = reinterpret_cast<const v4f *>(g) + (size_t)qy * (size_t)w;
  const v4f r0 = bloom_lerp4(rp[px], rp[qx]), r1 = bloom_lerp4(rq[px], rq[qx]);
  return bloom_lerp4(r0, r1);
}

template <bool FIRST>  // FIRST: the source is the frame (the bright pass in front of the box); else a level
BB_DEV void bloom_down(const float4 *__restrict__ src, int32_t w, int32_t h, float4 *__restrict__ dst, int32_t wd, float threshold) {
  const int32_t x = (int32_t)(blockIdx.x * kBloomThreads + threadIdx.x);
  if (x >= wd) return;
  const size_t y = blockIdx.y;
  const int32_t x0 = 2 * x, x1 = min(2 * x + 1, w - 1);  // (2x <= w - 1 for every x < wd = (w + 1) >> 1)
  const size_t y0 = 2 * y, y1 = 2 * y + 1 < (size_t)h ? 2 * y + 1 : (size_t)h - 1;
  const v4f *r0 = reinterpret_cast<const v4f *>(src) + y0 * (size_t)w, *r1 = reinterpret_cast<const v4f *>(src) + y1 * (size_t)w;
  v4f a, b, c, d;
  if constexpr (FIRST) {
    // The frame is read again by k_present_bloom a few launches later: an ORDINARY load here leaves it where that second read
    // finds part of it (k_present_bloom 69 -> 55 us, the chain 34 -> 29 us at 3840 x 2160, profiles/bloom.txt section 3).
#ifdef BB_BLOOM_NT_READ  // diagnostic build (make EXTRA=-DBB_BLOOM_NT_READ): the other side of that A/B
    a = bloom_bright(__builtin_nontemporal_load(r0 + x0), threshold), b = bloom_bright(__builtin_nontemporal_load(r0 + x1), threshold);
    c = bloom_bright(__builtin_nontemporal_load(r1 + x0), threshold), d = bloom_bright(__builtin_nontemporal_load(r1 + x1), threshold);
#else
    a = bloom_bright(r0[x0], threshold), b = bloom_bright(r0[x1], threshold), c = bloom_bright(r1[x0], threshold), d = bloom_bright(r1[x1], threshold);
#endif
  } else {
    a = r0[x0], b = r0[x1], c = r1[x0], d = r1[x1];
  }
  reinterpret_cast<v4f *>(dst)[y * (size_t)wd + (size_t)x] = bloom_box(a, b, c, d);
}
__global__ __launch_bounds__(kBloomThreads) void k_bloom_first(const float4 *__restrict__ frame, int32_t w, int32_t h,
                                                                float4 *__restrict__ d1, int32_t w1, float threshold) {
  bloom_down<true>(frame, w, h, d1, w1, threshold);
}
__global__ __launch_bounds__(kBloomThreads) void k_bloom_down(const float4 *__restrict__ src, int32_t w, int32_t h,
                                                               float4 *__restrict__ dst, int32_t wd) {
  bloom_down<false>(src, w, h, dst, wd, 0.0f);
}
// level: D_k on entry, U_k on return (w x its rows); coarse: U_{k+1}, wc x hc
__global__ __launch_bounds__(kBloomThreads) void k_bloom_up(const float4 *__restrict__ coarse, int32_t wc, int32_t hc,
                                                             float4 *level, int32_t w) {
  const int32_t x = (int32_t)(blockIdx.x * kBloomThreads + threadIdx.x);
  if (x >= w) return;
  v4f *t = reinterpret_cast<v4f *>(level) + (size_t)blockIdx.y * (size_t)w + (size_t)x;
  const v4f u = bloom_up(coarse, wc, hc, x, (int32_t)blockIdx.y);
  const v4f d = *t;
  *t = v4f{__fadd_rn(d.x, u.x), __fadd_rn(d.y, u.y), __fadd_rn(d.z, u.z), 0.0f};
}
// v = F + I * up(U_1), then present_pixel as k_present (tables staged in LDS as k_resolve's PRESENT form stages them).
// The body is stated once for k_present_bloom and k_present_bloom_auto, as present_body is for k_present.
BB_DEV void present_bloom_body(const float4 *__restrict__ frame, const float4 *__restrict__ u1, int32_t w1, int32_t h1,
                               uint32_t *__restrict__ out_rgba8, int32_t width, const SrgbTables *__restrict__ tables, int enable,
                               float exposure, int hdr16, float intensity) {
  static_assert(kBloomThreads == kResolveThreads, "resolve_stage_tables strides by kResolveThreads");
  __shared__ SrgbTables t;
  resolve_stage_tables(t, tables);
  const int32_t x = (int32_t)(blockIdx.x * kBloomThreads + threadIdx.x);
  if (x >= width) return;
  const size_t o = (size_t)blockIdx.y * (size_t)width + (size_t)x;
  const v4f f = __builtin_nontemporal_load(reinterpret_cast<const v4f *>(frame) + o);
  const v4f b = bloom_up(u1, w1, h1, x, (int32_t)blockIdx.y);
  const float r = __fadd_rn(f.x, __fmul_rn(intensity, b.x)), g = __fadd_rn(f.y, __fmul_rn(intensity, b.y)),
              bl = __fadd_rn(f.z, __fmul_rn(intensity, b.z));
  store_pixel(&out_rgba8[o], present_pixel(r, g, bl, t, enable, exposure, hdr16));
}
__global__ __launch_bounds__(kBloomThreads) void k_present_bloom(const float4 *__restrict__ frame, const float4 *__restrict__ u1,
                                                                  int32_t w1, int32_t h1, uint32_t *__restrict__ out_rgba8,
                                                                  int32_t width, const SrgbTables *__restrict__ tables, int enable,
                                                                  float exposure, int hdr16, float intensity) {
  present_bloom_body(frame, u1, w1, h1, out_rgba8, width, tables, enable, exposure, hdr16, intensity);
}

// ------------------------------------------------------------------------------------------------
// auto exposure (option "auto_exposure"; the rule: include/bibim_hip.h "auto exposure").  In front of the
// conversion: k_luminance counts the frame's pixels into 256 bins of log2 luminance, k_exposure turns the histogram into the
// exposure E of this presentation and adapts it against the history of its source, k_present_auto / k_present_bloom_auto are
// k_present / k_present_bloom with E loaded from device memory.  The histogram is integer arithmetic: the order in which
// pixels are counted does not matter, the result is exact.  The floating-point steps are single IEEE operations
// (__fadd_rn / __fsub_rn / __fmul_rn: nothing may contract).
//   k_luminance   streaming: 16 B read per pixel and nothing else, ordinary loads (k_bloom_first and the present kernel read
//                 the same bytes a few launches later).  A workgroup converts kLumaThreads * kLumaPerThread pixels, in
//                 coalesced rounds like k_present.  LDS: kLumaWords = 257 words (the 256 bins and `ignored`), 1028 bytes.
//                 Neighbouring pixels mostly share a bin, so equal bins are combined in front of the LDS add: a lane adds a
//                 run of equal bins among its own pixels once, and a wave whose lanes all hold the same (bin, count) adds it
//                 once for all of them (luma_add).  At the end the non-zero words go to the presentation's device histogram,
//                 one global atomic each.
//   k_exposure    one workgroup of 256: lane k owns bin k.  Prefix sums, trim, S, the 64-bit division, the reciprocal, the
//                 clamp, the adapt step against the history word; writes the record, the history, and leaves the device
//                 histogram zeroed for its next use.
// ------------------------------------------------------------------------------------------------
constexpr int kLumaThreads = 256;
constexpr int kLumaPerThread = 8;
constexpr int kLumaBins = 256;
constexpr int kLumaWords = kLumaBins + 1;      // [256]: the ignored pixels
constexpr uint32_t kLumaSkip = 0xFFFFFFFFu;    // no pixel (behind the frame's end)
constexpr int kLumaFirstBin = (127 - 16) * 8;  // 888: bits >> 20 of 2^-16
// bbr_exposure_record (include/bibim_hip.h), as the kernels write it; the host asserts that the two agree
struct ExposureRecord {
  uint32_t hist[kLumaBins];
  uint32_t ignored, counted, kept, mean_bits;
  unsigned long long sum;
  float target, clamped, previous, applied;
  uint32_t flags, reserved;
};
struct ExposureHistory {  // one per source
  float value;
  uint32_t valid;
};
struct ExposureParams {  // bbr_set_auto_exposure
  float key, e_min, e_max, rate;
  int32_t lo, hi;
};

// the word of the histogram a pixel is counted in
BB_DEV uint32_t luma_word(v4f p) {
  const float y = __fadd_rn(__fadd_rn(__fmul_rn(0.2126f, p.x), __fmul_rn(0.7152f, p.y)), __fmul_rn(0.0722f, p.z));
  if (!(y > 0.0f)) return (uint32_t)kLumaBins;  // NaN, +-0, negative, -inf: ignored
  const int32_t k = (int32_t)(__float_as_uint(y) >> 20) - kLumaFirstBin;
  return (uint32_t)min(max(k, 0), kLumaBins - 1);
}
// BB_LUMA_FORM: the one diagnostic switch of these kernels (make EXTRA=-DBB_LUMA_FORM=n), the A/B of
// profiles/auto_exposure.txt on how equal bins are combined in front of the LDS add.  0 = one LDS add per pixel, 1 = a lane adds a run of equal
// bins among its own pixels once, 2 (what ships) = that, and a wave whose lanes all hold the same (bin, count) adds it once.
#ifndef BB_LUMA_FORM
#define BB_LUMA_FORM 2
#endif
// `cnt` pixels of word `w` into the workgroup's histogram; called by any subset of a wave's lanes
BB_DEV void luma_add(uint32_t *h, uint32_t w, uint32_t cnt) {
#if BB_LUMA_FORM == 2
  const unsigned long long here = __ballot(1);
  const uint32_t w0 = __builtin_amdgcn_readfirstlane(w), c0 = __builtin_amdgcn_readfirstlane(cnt);
  if (__ballot(w == w0 && cnt == c0) == here) {  // the expected case: one add for the wave
    if ((uint32_t)__lane_id() == (uint32_t)__ffsll((long long)here) - 1u) atomicAdd(&h[w0], c0 * (uint32_t)__popcll(here));
    return;
  }
#endif
  atomicAdd(&h[w], cnt);
}
// a lane's kLumaPerThread words (kLumaSkip: no pixel) into the workgroup's histogram
BB_DEV void luma_count(uint32_t *h, const uint32_t (&w)[kLumaPerThread]) {
#if BB_LUMA_FORM == 0
#pragma unroll
  for (int j = 0; j < kLumaPerThread; ++j)
    if (w[j] != kLumaSkip) atomicAdd(&h[w[j]], 1u);
#else
  uint32_t run = kLumaSkip, cnt = 0u;
#pragma unroll
  for (int j = 0; j < kLumaPerThread; ++j) {
    if (w[j] == run) {
      ++cnt;
    } else {
      if (run != kLumaSkip) luma_add(h, run, cnt);
      run = w[j], cnt = 1u;
    }
  }
  if (run != kLumaSkip) luma_add(h, run, cnt);
#endif
}
__global__ __launch_bounds__(kLumaThreads) void k_luminance(const float4 *__restrict__ frame, size_t n, uint32_t *__restrict__ hist) {
  __shared__ uint32_t h[kLumaWords];
  for (uint32_t w = threadIdx.x; w < (uint32_t)kLumaWords; w += kLumaThreads) h[w] = 0u;
  __syncthreads();
  const size_t base = (size_t)blockIdx.x * (kLumaThreads * kLumaPerThread) + threadIdx.x;
  v4f px[kLumaPerThread];
#pragma unroll
  for (int j = 0; j < kLumaPerThread; ++j) {
    const size_t i = base + (size_t)j * kLumaThreads;
    px[j] = i < n ? reinterpret_cast<const v4f *>(frame)[i] : v4f{0.f, 0.f, 0.f, 0.f};
  }
  uint32_t w[kLumaPerThread];
#pragma unroll
  for (int j = 0; j < kLumaPerThread; ++j) w[j] = base + (size_t)j * kLumaThreads < n ? luma_word(px[j]) : kLumaSkip;
  luma_count(h, w);
  __syncthreads();
  for (uint32_t k = threadIdx.x; k < (uint32_t)kLumaWords; k += kLumaThreads)
    if (const uint32_t v = h[k]) atomicAdd(&hist[k], v);
}

constexpr int kExposureThreads = kLumaBins;
// the sum of v over the workgroup, in every lane (two barriers; `s` holds kExposureThreads words)
BB_DEV unsigned long long exposure_sum(unsigned long long v, unsigned long long *s) {
  __syncthreads();
  s[threadIdx.x] = v;
  __syncthreads();
  for (int d = kExposureThreads / 2; d > 0; d >>= 1) {
    if ((int)threadIdx.x < d) s[threadIdx.x] += s[threadIdx.x + d];
    __syncthreads();
  }
  return s[0];
}
// hist: the presentation's kLumaWords words; fallback: the frame's own Exposure, applied when nothing was counted and there is no history
__global__ __launch_bounds__(kExposureThreads) void k_exposure(uint32_t *__restrict__ hist, ExposureRecord *__restrict__ rec,
                                                                ExposureHistory *__restrict__ history, ExposureParams p, float fallback) {
  __shared__ unsigned long long s[kExposureThreads];
  __shared__ uint32_t scan[kExposureThreads];
  const int k = (int)threadIdx.x;
  const uint32_t mine = hist[k];
  // P_k + hist[k]: an inclusive scan (the counts sum to at most 2^30 pixels: 32 bits hold every partial sum)
  scan[k] = mine;
  __syncthreads();
  for (int d = 1; d < kExposureThreads; d <<= 1) {
    const uint32_t below = k >= d ? scan[k - d] : 0u;
    __syncthreads();
    scan[k] += below;
    __syncthreads();
  }
  const long long above = (long long)scan[k], below = above - (long long)mine;
  const long long n = (long long)scan[kExposureThreads - 1];
  const long long skip_lo = n * p.lo / 1000, skip_hi = n * (1000 - p.hi) / 1000;
  const long long c = max(0ll, min(above, n - skip_hi) - max(below, skip_lo));
  const unsigned long long kept = exposure_sum((unsigned long long)c, s);
  const unsigned long long sum = exposure_sum((unsigned long long)c * (unsigned long long)k, s);
  rec->hist[k] = mine;
  hist[k] = 0u;
  if (k != 0) return;
  const uint32_t ignored = hist[kLumaBins];
  hist[kLumaBins] = 0u;
  const ExposureHistory past = *history;
  uint32_t mean_bits = 0u;
  float target = 0.f, clamped = 0.f, applied;
  if (n > 0) {
    mean_bits = ((uint32_t)kLumaFirstBin << 20) + (uint32_t)((sum << 20) / kept) + (1u << 19);
    // the centre of a bin of [2^-16, 2^16): a normal number with a normal reciprocal, bb_rcp_normal's correctly rounded range
    const float r = bb_rcp_normal(__uint_as_float(mean_bits));
    target = __fmul_rn(p.key, r);
    clamped = __builtin_fminf(__builtin_fmaxf(target, p.e_min), p.e_max);
    applied = (past.valid && p.rate != 1.0f) ? __fadd_rn(past.value, __fmul_rn(__fsub_rn(clamped, past.value), p.rate)) : clamped;
    *history = ExposureHistory{applied, 1u};
  } else {
    applied = past.valid ? past.value : fallback;
  }
  rec->ignored = ignored, rec->counted = (uint32_t)n, rec->kept = (uint32_t)kept, rec->mean_bits = mean_bits;
  rec->sum = sum;
  rec->target = target, rec->clamped = clamped, rec->previous = past.valid ? past.value : 0.f, rec->applied = applied;
  rec->flags = (past.valid ? 1u : 0u) | (n > 0 ? 0u : 2u);
  rec->reserved = 0u;
}

// k_present / k_present_bloom with the exposure of the presentation's record in the argument's place: one uniform load per workgroup
__global__ __launch_bounds__(kPresentThreads) void k_present_auto(const float4 *__restrict__ frame, uint32_t *__restrict__ out_rgba8,
                                                                   size_t n, const SrgbTables *__restrict__ tables, int enable,
                                                                   const float *__restrict__ exposure, int hdr16) {
  present_body(frame, out_rgba8, n, tables, enable, *exposure, hdr16);
}
__global__ __launch_bounds__(kBloomThreads) void k_present_bloom_auto(const float4 *__restrict__ frame, const float4 *__restrict__ u1,
                                                                       int32_t w1, int32_t h1, uint32_t *__restrict__ out_rgba8,
                                                                       int32_t width, const SrgbTables *__restrict__ tables,
                                                                       int enable, const float *__restrict__ exposure, int hdr16,
                                                                       float intensity) {
  present_bloom_body(frame, u1, w1, h1, out_rgba8, width, tables, enable, *exposure, hdr16, intensity);
}
// ------------------------------------------------------------------------------------------------
// multisampling (option "sample_shading" 0 with "supersample" n = 2 or 4): one fragment is shaded per primitive and output
// pixel.  The block of output pixel (x, y) is the fine pixels (nx + i, ny + j), indexed k = j * n + i; P(s) is the primitive
// (reference >> 3: the sub-triangles of one clipped primitive are one primitive) that wins fine pixel s.
//   rep(s) = the first s' of s's block, in index order, with P(s') == P(s)   (covered s);   rep(s) = s   (uncovered s)
//   g(s)   = f(rep(s));   out = the resolve rule above applied to g
// Only the samples with rep(s) == s, the representatives, are shaded -- as the fine pixels they are -- so the fine frame
// holds f at them (and the background at uncovered samples) and nothing defined anywhere else.
//
// The SAMPLE MAP: one word per output pixel, a 4-bit field per sample holding rep(k) (16 bits at n = 2, 64 at n = 4), laid out
// like the output frame (a rank's shard rows on a partitioned context).
//
// k_sample_merge, between k_raster and k_shade_items: one workgroup per fine tile, the tiles the rank owns in plain screen
// order.  It reads the tile's fragment list (a kFullTile tile: the one word stands for all pixels) into registers, writes the
// winner of every pixel into LDS, derives the map words of the tile's output pixels from that (written for empty tiles too:
// identity), and rewrites the list in place with the representatives only -- their words unchanged, in their original
// order: the list k_raster would have written had only they been covered, padded to 64 with its first word as k_raster
// pads.  A full tile becomes an explicit list of TILE_PIXELS / n^2 words, in ascending pixel-field order, without the flag.
// It does the accounting k_raster leaves out in this mode (frag_count, item_groups).
// Blocks never straddle a tile (n divides 8, the side of the pixel field's 8 x 8 blocks) nor the frame (its extent is n x
// the output's), so a tile's map words depend on that tile alone.
// ------------------------------------------------------------------------------------------------
constexpr int kMergeThreads = 256;
constexpr uint32_t kNoPrim = 0xFFFFFFFFu;  // (a primitive index has 29 bits)
template <int N> struct SampleMap;
template <> struct SampleMap<2> { typedef uint16_t Word; };
template <> struct SampleMap<4> { typedef unsigned long long Word; };
// rep(k) of a map word
template <int N>
BB_DEV int sample_rep(typename SampleMap<N>::Word w, int k) { return (int)((w >> (4 * k)) & (typename SampleMap<N>::Word)(N * N - 1)); }

template <int TILE_W, int TILE_H, int N>
__global__ __launch_bounds__(kMergeThreads) void k_sample_merge(FrameParams fp, uint32_t *__restrict__ frag_count,
                                                                unsigned long long *__restrict__ frags,
                                                                typename SampleMap<N>::Word *__restrict__ map,
                                                                uint32_t *__restrict__ item_groups) {
  typedef typename SampleMap<N>::Word Word;
  constexpr int TILE_PIXELS = TILE_W * TILE_H;
  constexpr int PASSES = TILE_PIXELS / kMergeThreads;  // list words per thread
  constexpr int WAVES = kMergeThreads / 64;
  constexpr int OUT_W = TILE_W / N, OUT_H = TILE_H / N, OUT_PIXELS = OUT_W * OUT_H;
  static_assert(8 % N == 0 && TILE_W % 8 == 0 && TILE_H % 8 == 0, "a block lies inside one 8 x 8 block of the pixel field");
  static_assert(PASSES * WAVES <= 64, "the runs of kept words are scanned by one wave");
  __shared__ uint32_t s_prim[TILE_PIXELS];       // P of every pixel of the tile, by pixel field; kNoPrim: nothing drawn
  __shared__ Word s_map[OUT_PIXELS];             // the tile's map words
  __shared__ uint32_t s_kept[PASSES * WAVES];    // representatives in each run of 64 list words
  __shared__ unsigned long long s_pad_frag;      // the new list's first word
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int tx = blockIdx.x;
  int ty, out_tile_row;
  if (!tile_row(fp, (int)blockIdx.y, ty, out_tile_row)) return;
  const uint32_t tile = (uint32_t)ty * (uint32_t)fp.tiles_x + (uint32_t)tx;
  unsigned long long *list = frags + (size_t)tile * TILE_PIXELS;

  // ---- the whole list, into registers ----
  const uint32_t raw = frag_count[tile];
  const bool full = (raw & kFullTile) != 0u;
  const uint32_t count = full ? (uint32_t)TILE_PIXELS : min(raw, (uint32_t)TILE_PIXELS);
  unsigned long long fw[PASSES];
  const unsigned long long word0 = full ? list[0] : 0ull;  // (pixel field 0: word i of the implied list is this one with pixel i)
#pragma unroll
  for (int k = 0; k < PASSES; ++k) {
    const uint32_t i = (uint32_t)(k * kMergeThreads + tid);
    fw[k] = full ? word0 + ((unsigned long long)i << 32) : (i < count ? list[i] : 0ull);
    s_prim[i] = kNoPrim;
  }
  __syncthreads();
#pragma unroll
  for (int k = 0; k < PASSES; ++k)
    if ((uint32_t)(k * kMergeThreads + tid) < count) s_prim[fragment_pixel<TILE_PIXELS>(fw[k])] = (uint32_t)fw[k] >> 3;
  __syncthreads();

  // ---- the map words of the tile's output pixels ----
  const int out_width = fp.width / N;
  for (int o = tid; o < OUT_PIXELS; o += kMergeThreads) {
    const int bx = o % OUT_W, by = o / OUT_W;
    uint32_t prim[N * N];
#pragma unroll
    for (int k = 0; k < N * N; ++k) prim[k] = s_prim[tile_index<TILE_W>(bx * N + k % N, by * N + k / N)];
    Word w = 0;
#pragma unroll
    for (int k = 0; k < N * N; ++k) {
      int rep = k;
#pragma unroll
      for (int e = k - 1; e >= 0; --e)
        if (prim[k] != kNoPrim && prim[e] == prim[k]) rep = e;
      w |= (Word)((Word)rep << (4 * k));
    }
    s_map[o] = w;
    if (tx * TILE_W + bx * N < fp.width && ty * TILE_H + by * N < fp.height)
      map[(size_t)(out_tile_row * OUT_H + by) * (size_t)out_width + (size_t)(tx * OUT_W + bx)] = w;
  }
  __syncthreads();

  // ---- which words stay, and where ----
  unsigned long long kept_mask[PASSES];
#pragma unroll
  for (int k = 0; k < PASSES; ++k) {
    bool keep = false;
    if ((uint32_t)(k * kMergeThreads + tid) < count) {
      int x, y;
      tile_pixel<TILE_W>(fragment_pixel<TILE_PIXELS>(fw[k]), x, y);
      const int s = (y % N) * N + (x % N);
      keep = sample_rep<N>(s_map[(y / N) * OUT_W + (x / N)], s) == s;
    }
    kept_mask[k] = __ballot(keep);
    if (lane == 0) s_kept[k * WAVES + wave] = (uint32_t)__popcll(kept_mask[k]);
  }
  __syncthreads();  // (every load of the list has returned: its words went into the ballots above)
  // the runs in list order: run r = k * WAVES + wave holds words [64 r, 64 r + 64); every wave scans the totals itself
  const uint32_t mine = lane < PASSES * WAVES ? s_kept[lane] : 0u;
  uint32_t incl = mine;
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const uint32_t up = (uint32_t)__shfl_up((int)incl, d);
    if (lane >= d) incl += up;
  }
  const uint32_t m = (uint32_t)__shfl((int)incl, 63);
#pragma unroll
  for (int k = 0; k < PASSES; ++k) {
    const uint32_t base = (uint32_t)__shfl((int)(incl - mine), k * WAVES + wave);
    if ((kept_mask[k] >> lane) & 1ull) {
      const uint32_t at = base + (uint32_t)__popcll(kept_mask[k] & ((1ull << lane) - 1ull));
      list[at] = fw[k];
      if (at == 0u) s_pad_frag = fw[k];
    }
  }
  __syncthreads();
  // (k_shade loads 64 words before it knows the count: padded to a multiple of 64 with copies of the first, as k_raster pads)
  if (m != 0u && (m & 63u) != 0u && tid < (int)(64u - (m & 63u))) list[m + (uint32_t)tid] = s_pad_frag;
  if (tid == 0) {
    frag_count[tile] = m;  // (N_shaded = sum of these: the representatives)
    const uint32_t slot = blockIdx.y * gridDim.x + blockIdx.x;
    if (item_groups && m) atomicAdd(&item_groups[(slot / kItemGroupSlots) * kItemGroupStride], (m + 63u) >> 6);
  }
}
// Instantiated HERE, not where the host launches them: the compiler lays kernels out in the order they are instantiated, and
// a kernel instantiated between k_raster's and k_shade_items' launches would move the kernels of the default path against
// each other in the code object (they run side by side on pipelined frames).  From here all of them move together.
template __global__ void k_sample_merge<32, 32, 2>(FrameParams, uint32_t *__restrict__, unsigned long long *__restrict__, SampleMap<2>::Word *__restrict__, uint32_t *__restrict__);
template __global__ void k_sample_merge<32, 32, 4>(FrameParams, uint32_t *__restrict__, unsigned long long *__restrict__, SampleMap<4>::Word *__restrict__, uint32_t *__restrict__);
template __global__ void k_sample_merge<64, 64, 2>(FrameParams, uint32_t *__restrict__, unsigned long long *__restrict__, SampleMap<2>::Word *__restrict__, uint32_t *__restrict__);
template __global__ void k_sample_merge<64, 64, 4>(FrameParams, uint32_t *__restrict__, unsigned long long *__restrict__, SampleMap<4>::Word *__restrict__, uint32_t *__restrict__);

// k_resolve_merged: k_resolve on g.  Per output pixel the map word, then fine[block + rep(k)] for k = 0 .. n^2 - 1 added in
// the pinned order, a fine row of the block at a time as k_resolve does.  A pixel whose fields are all 0 (one primitive
// covers the block: most pixels of a frame) loads its one value once; the n^2 - 1 additions stay, they are the rule.
// Traffic per output pixel: the map word, 16 B per distinct representative, the store.
template <int N>
BB_DEV float4 resolve_merged_pixel(const float4 *__restrict__ fine, typename SampleMap<N>::Word w, int32_t width, int32_t x, size_t y) {
  const size_t fine_pitch = (size_t)width * N;
  const v4f *block = reinterpret_cast<const v4f *>(fine) + (y * N) * fine_pitch + (size_t)x * N;
  v4f acc;
  if (w == 0) {
    const v4f v = __builtin_nontemporal_load(block);
    acc = v;
#pragma unroll
    for (int k = 1; k < N * N; ++k) acc = resolve_add(acc, v);
  } else {
    acc = v4f{0.f, 0.f, 0.f, 0.f};
#pragma unroll 1
    for (int j = 0; j < N; ++j) {
      v4f v[N];
#pragma unroll
      for (int i = 0; i < N; ++i) {
        const int r = sample_rep<N>(w, i);
        v[i] = __builtin_nontemporal_load(block + (size_t)(r / N) * fine_pitch + (size_t)(r % N));
      }
      acc = j == 0 ? v[0] : resolve_add(acc, v[0]);
#pragma unroll
      for (int i = 1; i < N; ++i) acc = resolve_add(acc, v[i]);
      w = (typename SampleMap<N>::Word)(w >> (4 * N));
    }
  }
  constexpr float r = resolve_scale<N>();
  return make_float4(__fmul_rn(acc.x, r), __fmul_rn(acc.y, r), __fmul_rn(acc.z, r), __fmul_rn(acc.w, r));
}
template <int N, bool PRESENT>
__global__ __launch_bounds__(kResolveThreads) void k_resolve_merged(const float4 *__restrict__ fine,
                                                                     const typename SampleMap<N>::Word *__restrict__ map,
                                                                     float4 *__restrict__ out, uint32_t *__restrict__ out_rgba8,
                                                                     int32_t width, const SrgbTables *__restrict__ tables, int enable,
                                                                     float exposure) {
  const int32_t x = (int32_t)(blockIdx.x * kResolveThreads + threadIdx.x);
  const size_t y = blockIdx.y, o = y * (size_t)width + (size_t)x;
  if constexpr (PRESENT) {
    __shared__ SrgbTables t;
    resolve_stage_tables(t, tables);
    if (x >= width) return;
    const float4 px = resolve_merged_pixel<N>(fine, map[o], width, x, y);
    store_pixel(&out_rgba8[o], present_pixel(px.x, px.y, px.z, t, enable, exposure, 1));
  } else {
    if (x >= width) return;
    store_pixel(&out[o], resolve_merged_pixel<N>(fine, map[o], width, x, y));
  }
}

// ------------------------------------------------------------------------------------------------
// depth resolve (option "depth_resolve" with "supersample" n = 2..4): one depth, and on the dump path one winner, per output
// pixel, taken from ONE sample k* of the pixel's block (k = j * n + i, the colour resolve's block and index):
//   kDepthZero  k* = 0
//   kDepthMin   k* = the first k, in index order, whose depth bit pattern (an unsigned 32-bit integer) is smallest
//   kDepthMax   k* = the first k, in index order, whose depth bit pattern is largest
// Stored depths lie in [0, 1] and an uncovered sample holds the cleared 0.0, so the order of the bit patterns is the order
// of the values, and it is the comparison k_raster's keys make (reverse-Z: MAX is the nearest sample).  The fine depth (and,
// PRIM, the fine winners: 0xFFFFFFFF where a sample is uncovered) is what k_raster stored through depth_io (vis_depth,
// vis_prim) at the render extent; nothing here interprets a depth as a number.
// A streaming kernel shaped like k_resolve: one lane per output pixel, blockIdx.y the output row, size_t addresses, the n
// contiguous depths of a fine row in one load where the address allows it (8 bytes at n = 2, 16 at n = 4; at n = 3 a row
// starts at a multiple of 12 bytes, so three 4-byte loads), the rows below the first a rolled loop.  kDepthZero loads
// sample 0 alone.  4 n^2 B read + 4 B written per output pixel (PRIM: + 4 B read at k* and 4 B written); no LDS, no scratch.
// ------------------------------------------------------------------------------------------------
enum : int { kDepthZero = 1, kDepthMin = 4, kDepthMax = 8 };  // VkResolveModeFlagBits
typedef uint32_t depth_u32x2 __attribute__((ext_vector_type(2)));
typedef uint32_t depth_u32x4 __attribute__((ext_vector_type(4)));
template <int N>
BB_DEV void depth_row_load(const uint32_t *__restrict__ row, uint32_t (&v)[N]) {
  static_assert(N >= 2 && N <= 4, "supersample: n = 2 .. 4 are resolved");
  if constexpr (N == 2) {
    const depth_u32x2 w = __builtin_nontemporal_load(reinterpret_cast<const depth_u32x2 *>(row));
    v[0] = w.x; v[1] = w.y;
  } else if constexpr (N == 4) {
    const depth_u32x4 w = __builtin_nontemporal_load(reinterpret_cast<const depth_u32x4 *>(row));
    v[0] = w.x; v[1] = w.y; v[2] = w.z; v[3] = w.w;
  } else {
#pragma unroll
    for (int i = 0; i < N; ++i) v[i] = __builtin_nontemporal_load(row + i);
  }
}
// one fine row of the block against the best so far; `k` is the index of the row's first sample (strict: the first k stays)
template <int N, int MODE>
BB_DEV void depth_row_select(const uint32_t *__restrict__ row, uint32_t k, bool first, uint32_t &best, uint32_t &best_k) {
  uint32_t v[N];
  depth_row_load<N>(row, v);
#pragma unroll
  for (int i = 0; i < N; ++i) {
    const bool better = (first && i == 0) || (MODE == kDepthMin ? v[i] < best : v[i] > best);
    best = better ? v[i] : best;
    best_k = better ? k + (uint32_t)i : best_k;
  }
}
template <int N, int MODE, bool PRIM>
__global__ __launch_bounds__(kResolveThreads) void k_resolve_depth(const uint32_t *__restrict__ fine_depth,
                                                                    const uint32_t *__restrict__ fine_prim,
                                                                    uint32_t *__restrict__ out_depth, uint32_t *__restrict__ out_prim,
                                                                    int32_t width) {
  static_assert(MODE == kDepthZero || MODE == kDepthMin || MODE == kDepthMax, "depth_resolve: SAMPLE_ZERO, MIN or MAX");
  const int32_t x = (int32_t)(blockIdx.x * kResolveThreads + threadIdx.x);
  if (x >= width) return;
  const size_t y = blockIdx.y, o = y * (size_t)width + (size_t)x;
  const size_t fine_pitch = (size_t)width * N, block = (y * N) * fine_pitch + (size_t)x * N;
  uint32_t best, best_k = 0u;
  if constexpr (MODE == kDepthZero) {
    best = __builtin_nontemporal_load(fine_depth + block);
  } else {
    const uint32_t *row = fine_depth + block;
    best = 0u;
    depth_row_select<N, MODE>(row, 0u, true, best, best_k);
#pragma unroll 1
    for (int j = 1; j < N; ++j) {
      row += fine_pitch;
      depth_row_select<N, MODE>(row, (uint32_t)(j * N), false, best, best_k);
    }
  }
  store_pixel(&out_depth[o], best);
  if constexpr (PRIM)
    store_pixel(&out_prim[o], __builtin_nontemporal_load(fine_prim + block + (size_t)(best_k / N) * fine_pitch + (size_t)(best_k % N)));
}
// Instantiated HERE, behind every kernel above, for the reason given at k_sample_merge: the kernels of the default path keep
// their places against each other in the code object.
#define BB_RESOLVE_DEPTH(N, MODE)                                                                                                      \
  template __global__ void k_resolve_depth<N, MODE, false>(const uint32_t *__restrict__, const uint32_t *__restrict__, uint32_t *__restrict__, \
                                                           uint32_t *__restrict__, int32_t);                                          \
  template __global__ void k_resolve_depth<N, MODE, true>(const uint32_t *__restrict__, const uint32_t *__restrict__, uint32_t *__restrict__,  \
                                                          uint32_t *__restrict__, int32_t);
BB_RESOLVE_DEPTH(2, kDepthZero) BB_RESOLVE_DEPTH(2, kDepthMin) BB_RESOLVE_DEPTH(2, kDepthMax)
BB_RESOLVE_DEPTH(3, kDepthZero) BB_RESOLVE_DEPTH(3, kDepthMin) BB_RESOLVE_DEPTH(3, kDepthMax)
BB_RESOLVE_DEPTH(4, kDepthZero) BB_RESOLVE_DEPTH(4, kDepthMin) BB_RESOLVE_DEPTH(4, kDepthMax)
#undef BB_RESOLVE_DEPTH

// ------------------------------------------------------------------------------------------------
// The wire forms of the exchange (include/bibim_hip.h, BBR_SHARD_*): what a rank's shard of n = shard_rows * width pixels
// looks like while it travels.  One struct per form: Whole = pixel of the whole frame it unpacks to, block_bytes(n) = size
// of one rank's block, load(block, j, n) = pixel j of a block, kLoadAlign = the widest access load() makes (what a gather
// buffer must be aligned to; every block size is a multiple of it, so every block of the buffer is aligned with its first).
// How a block is made from the shard: bibim_hip.hip, kWireForms.
// ------------------------------------------------------------------------------------------------

// the shard as it is, [shard_rows][width] pixels: the fp32 one, or the presented RGBA8 one
template <class Pixel>
struct WirePlain {
  using Whole = Pixel;
  static constexpr size_t kLoadAlign = sizeof(Pixel);
  static constexpr __host__ __device__ size_t block_bytes(size_t n) { return n * sizeof(Pixel); }
  static __device__ Whole load(const uint8_t *block, size_t j, size_t) { return reinterpret_cast<const Pixel *>(block)[j]; }
};
using WireRgba32f = WirePlain<float4>;
using WireRgba8 = WirePlain<uint32_t>;

// Lossless 12.1-byte form (a quarter less than RGBA32F over links that are the bottleneck at N > 1): alpha is 1.0 where
// geometry was shaded and 0.0 on cleared pixels (forward_brdf.frag:75 writes 1, the clear colour is 0, src/main.cpp:84;
// the deferred path writes 1 everywhere), so it travels as one bit.
//   block = rgb[n][3] float, padding to 8 bytes, one 64-bit mask per 64 pixels (bit k of word w = pixel 64 w + k), padding
//   to 16 bytes; the padding bytes are zero
struct WirePacked {
  using Whole = float4;
  static constexpr size_t kLoadAlign = 8;  // the mask words
  static constexpr __host__ __device__ size_t mask_offset(size_t n) { return (n * 12 + 7) & ~(size_t)7; }
  static constexpr __host__ __device__ size_t block_bytes(size_t n) { return (mask_offset(n) + ((n + 63) / 64) * 8 + 15) & ~(size_t)15; }
  static __device__ Whole load(const uint8_t *block, size_t j, size_t n) {
    const float *rgb = reinterpret_cast<const float *>(block) + 3 * j;
    const unsigned long long m = reinterpret_cast<const unsigned long long *>(block + mask_offset(n))[j >> 6];
    return make_float4(rgb[0], rgb[1], rgb[2], ((m >> (j & 63)) & 1ull) ? 1.0f : 0.0f);
  }
};

// The reference's own HDR attachment format (R16G16B16A16_SFLOAT, src/render.h:94, src/main.cpp:463-472): 8 bytes per
// pixel, half of the fp32 shard.  Lossy -- every channel is rounded to the nearest binary16 value (ties to even, the
// rounding an attachment write performs: bb_half_round) -- and therefore a separate output, never the default.  The whole
// frame is widened back to RGBA32F (every binary16 value is a binary32 value).
struct WireRgba16f {
  using Whole = float4;
  static constexpr size_t kLoadAlign = 8;  // a pixel's four halves in one load
  static constexpr __host__ __device__ size_t block_bytes(size_t n) { return n * 8; }
  static __device__ Whole load(const uint8_t *block, size_t j, size_t) {
    const uint2 w = reinterpret_cast<const uint2 *>(block)[j];
    _Float16 h[4];
    __builtin_memcpy(h, &w, 8);
    return make_float4((float)h[0], (float)h[1], (float)h[2], (float)h[3]);
  }
};

// fp32 shard -> WirePacked block (`mask` = block + mask_offset(n))
__global__ void k_pack_shard(const float4 *__restrict__ shard, float *__restrict__ rgb, unsigned long long *__restrict__ mask,
                             size_t n) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  const bool live = i < n;
  float4 p = make_float4(0.f, 0.f, 0.f, 0.f);
  if (live) {
    p = shard[i];
    rgb[3 * i + 0] = p.x;
    rgb[3 * i + 1] = p.y;
    rgb[3 * i + 2] = p.z;
  }
  const unsigned long long m = __ballot(live && __float_as_uint(p.w) == 0x3F800000u);
  if ((threadIdx.x & 63) == 0 && live) mask[i >> 6] = m;
  if (i == 0) {
    // the block's padding is zero: a block is a function of the shard alone, whatever the buffer held before
    const size_t words = (n + 63) / 64;
    if (n & 1) rgb[3 * n] = 0.f;                                                // 12 n mod 8 = 4: four bytes in front of the masks
    if ((WirePacked::mask_offset(n) + words * 8) & 15) mask[words] = 0ull;      // eight bytes behind them
  }
}

// fp32 shard -> WireRgba16f block
__global__ void k_pack_shard_half(const float4 *__restrict__ shard, uint2 *__restrict__ out, size_t n) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const float4 p = shard[i];
  const _Float16 h[4] = {(_Float16)p.x, (_Float16)p.y, (_Float16)p.z, (_Float16)p.w};
  uint2 w;
  __builtin_memcpy(&w, h, 8);
  out[i] = w;
}

// The screen-band un-interleave: pixel i of the row-major frame -> the rank whose shard holds it, and its index there
// (band b = band_rows framebuffer rows belongs to rank b % world; a shard is its rank's bands stacked in order).
__device__ __forceinline__ size_t shard_index(size_t i, int width, int world, int band_rows, int &rank) {
  const int y = (int)(i / (size_t)width), x = (int)(i - (size_t)y * width);
  const int band = y / band_rows, r = y - band * band_rows;
  rank = band % world;
  return ((size_t)(band / world) * band_rows + r) * (size_t)width + x;
}

// [world] blocks of `shard_pixels` pixels each, back to back (what the all-gather leaves) -> the row-major whole frame
template <class Form>
__global__ void k_unpack_gathered(const uint8_t *__restrict__ gathered, typename Form::Whole *__restrict__ frame, int width,
                                  int height, int world, int band_rows, size_t shard_pixels) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= (size_t)width * (size_t)height) return;
  int rank;
  const size_t j = shard_index(i, width, world, band_rows, rank);
  frame[i] = Form::load(gathered + (size_t)rank * Form::block_bytes(shard_pixels), j, shard_pixels);
}

// The peer form of the exchange as ONE kernel (bbr_push_shard, option "push_mode" 1): a workgroup loads a piece of this
// rank's block once and stores it into the same place of EVERY peer's gather buffer -- world - 1 stores per load, each going
// out over its own xGMI link, so all links of the full mesh carry a block at the same time (the direct pattern of SURVEY
// section 5 / 8(e): shard / link bandwidth, where copies queued one behind the other take world - 1 times that).  The
// peers' buffers are peer-accessible device memory (hipDeviceEnablePeerAccess or an opened IPC handle).
constexpr int kMaxPushPeers = 15;
struct PushTargets {
  void *dst[kMaxPushPeers];
};
constexpr int kPushThreads = 256;
template <typename V>
__global__ __launch_bounds__(kPushThreads) void k_push_block(const V *__restrict__ src, PushTargets t, int n_targets, size_t n) {
  for (size_t i = (size_t)blockIdx.x * kPushThreads + threadIdx.x; i < n; i += (size_t)gridDim.x * kPushThreads) {
    const V v = src[i];
#pragma unroll 1
    for (int k = 0; k < n_targets; ++k) reinterpret_cast<V *>(t.dst[k])[i] = v;
  }
}

// ------------------------------------------------------------------------------------------------
// k_shade_overlay: light.frag / gizmo.frag on the fragments of the overlay pass, written sRGB-encoded into the
// presented RGBA8 image (the overlay subpass draws into the swapchain image, src/main.cpp:128-171).
// ------------------------------------------------------------------------------------------------
template <int TILE_W, int TILE_H>
__global__ __launch_bounds__(kShadeThreads) void k_shade_overlay(
    FrameParams fp, const ShadeRec *__restrict__ recs, const ClipSlot *__restrict__ clip_arena,
    const unsigned long long *__restrict__ frags, const uint32_t *__restrict__ frag_count,
    const SrgbTables *__restrict__ tables, uint32_t *__restrict__ out_rgba8) {
  constexpr int TILE_PIXELS = TILE_W * TILE_H;
  constexpr int CHUNKS = TILE_PIXELS / kShadeThreads;
  const int tx = blockIdx.x / CHUNKS, chunk = blockIdx.x - tx * CHUNKS;
  const int ty = blockIdx.y;
  if (ty >= fp.tiles_y) return;
  const uint32_t tile = (uint32_t)ty * (uint32_t)fp.tiles_x + (uint32_t)tx;
  const uint32_t i = (uint32_t)chunk * kShadeThreads + threadIdx.x;
  const uint32_t n_frag = frag_count[tile];
  if (i >= n_frag) return;
  const unsigned long long frag = frags[(size_t)tile * TILE_PIXELS + i];
  const uint32_t ref = (uint32_t)frag, prim = ref >> 3;
  int x, y;
  tile_pixel<TILE_W>(fragment_pixel<TILE_PIXELS>(frag), x, y);
  const int gx = tx * TILE_W + x, gy = ty * TILE_H + y;
  const ShadeRec pa = recs[prim];
  // the overlay pass writes no slot into its fragment words: a clipped primitive's slot is always found through the record
  const bool clipped = pa.clip_base != kNotClipped;
  const ClipSlot *cs = clipped ? &clip_arena[record_clip_slot(pa.clip_base, ref)] : nullptr;
  const PlaneHead h = clipped ? cs->h : pa.h;
  float cb[3][3] = {};
  if (clipped) {
#pragma unroll
    for (int jj = 0; jj < 3; ++jj)
#pragma unroll
      for (int k = 0; k < 3; ++k) cb[jj][k] = cs->bary[jj][k];
  }
  float b0, b1, b2;
  plane_bary(h, clipped, cb, gx, gy, b0, b1, b2);
  // varyings 0..5 of the overlay programs (k_geometry<..., OVERLAY>): 0, 1 sit in the record's head, 2..5 in its body
  float a[6];
#pragma unroll
  for (int k = 0; k < 2; ++k) a[k] = interp3(b0, b1, b2, pa.uv[0][k], pa.uv[1][k], pa.uv[2][k]);
#pragma unroll
  for (int k = 0; k < 4; ++k) a[2 + k] = interp3(b0, b1, b2, pa.vary[k][0], pa.vary[k][1], pa.vary[k][2]);
  float col[3] = {a[0], a[1], a[2]};  // light.frag: outColor = vec4(vColor, 1)
  if (pa.material == 2u) {             // gizmo.frag:10-17: L = -(0,0,1); diff = max(dot(L, normalize(vNormal)), 0)
    const f3 N = normalize3(mk3(a[3], a[4], a[5]));
    const float diff = max0(dot3(mk3(-0.0f, -0.0f, -1.0f), N));
    col[0] = a[0] * diff; col[1] = a[1] * diff; col[2] = a[2] * diff;
  }
  uint32_t px = 0xFF000000u;
#pragma unroll
  for (int k = 0; k < 3; ++k) px |= srgb8(col[k], *tables) << (8 * k);
  out_rgba8[(size_t)gy * (size_t)fp.width + (size_t)gx] = px;
}

// ------------------------------------------------------------------------------------------------
// TBN line overlay (option "tbn"): tbn.vert:18-41 + tbn.geom:14-73 per triangle, then 1-pixel lines with
// the diamond-exit rule, depth-tested against the scene, resolved in primitive order
// ------------------------------------------------------------------------------------------------

constexpr int kTbnTile = 32;          // k_tbn_raster: one 32 x 32 tile per workgroup (fixed, whatever tile_mode is)
constexpr int kTbnThreads = 256;
constexpr float kTbnGuard = 4.0f;     // |x|, |y| <= 4 w: snapped coordinates stay below 2^25, every product below 2^53
constexpr float kTbnLength = 0.05f;   // tbn.geom:3

struct TbnParams {
  int32_t width, height, tiles_x, tiles_y;
  uint32_t bin_cap;
  float half_w, half_h;
};

// Everything specific to TBN is plain IEEE fp32 in the order written (the file is compiled with -ffp-contract=off);
// nothing here goes through a helper that uses fmaf.
BB_DEV f3 tbn_cross(f3 a, f3 b) { return f3{a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x}; }
BB_DEV f3 tbn_mean(f3 a, f3 b, f3 c) {
  return f3{((a.x + b.x) + c.x) / 3.0f, ((a.y + b.y) + c.y) / 3.0f, ((a.z + b.z) + c.z) / 3.0f};
}
BB_DEV f3 tbn_normalize(f3 v) {
  const float l = sqrtf((v.x * v.x + v.y * v.y) + v.z * v.z);
  return f3{v.x / l, v.y / l, v.z / l};
}
// vCombined * (p, 1): the centroid's w is ((1 + 1) + 1) / 3 = 1 and the offsets carry w = 0
BB_DEV void tbn_to_clip(const Mat4 &m, f3 p, float *c) {
#pragma unroll
  for (int i = 0; i < 4; ++i) c[i] = ((m.M[0][i] * p.x + m.M[1][i] * p.y) + m.M[2][i] * p.z) + m.M[3][i] * 1.0f;
}

BB_DEV float tbn_plane(const float *c, int k) {
  switch (k) {
    case 0: return c[3] - c[2];  // z <= w
    case 1: return c[2];         // z >= 0
    case 2: return kTbnGuard * c[3] + c[0];
    case 3: return kTbnGuard * c[3] - c[0];
    case 4: return kTbnGuard * c[3] + c[1];
    default: return kTbnGuard * c[3] - c[1];
  }
}

// Liang-Barsky in clip space, then project_vertex on both ends.  False: no segment (non-finite, outside, behind the
// camera, or zero length once snapped).
BB_DEV bool tbn_make_segment(const float *p0, const float *p1, const Viewport &vp, TbnSeg &r) {
#pragma unroll
  for (int k = 0; k < 4; ++k)
    if (!isfinite(p0[k]) || !isfinite(p1[k])) return false;
  float t0 = 0.0f, t1 = 1.0f;
#pragma unroll
  for (int k = 0; k < 6; ++k) {
    const float d0 = tbn_plane(p0, k), d1 = tbn_plane(p1, k);
    if (d0 < 0.0f && d1 < 0.0f) return false;
    if (d0 < 0.0f) t0 = fmaxf(t0, d0 / (d0 - d1));
    else if (d1 < 0.0f) t1 = fminf(t1, d0 / (d0 - d1));
  }
  if (t0 > t1) return false;
  float q0[4], q1[4];
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    q0[k] = t0 > 0.0f ? p0[k] + t0 * (p1[k] - p0[k]) : p0[k];
    q1[k] = t1 < 1.0f ? p0[k] + t1 * (p1[k] - p0[k]) : p1[k];
  }
  float rw;
  if (!project_vertex(q0, vp, r.X0, r.Y0, rw, r.za) || !project_vertex(q1, vp, r.X1, r.Y1, rw, r.zb)) return false;
  return r.X0 != r.X1 || r.Y0 != r.Y1;
}

// Bin a segment (valid) to every tile its pixel bounding box (one pixel of slack each side) meets inside the target; the
// lanes of a wave walk their tile ranges in lock-step.  A full bin raises overflow bit 0 and reports the count it needed;
// the host grows the bins and redoes the pass.  Called by every active lane of the wave.
BB_DEV void tbn_bin(bool valid, const TbnSeg &s, uint32_t index, const TbnParams &tp, uint32_t *tile_count, uint32_t *bins,
                    uint32_t *ctr) {
  const int px0 = max((min(s.X0, s.X1) >> 8) - 1, 0), px1 = min((max(s.X0, s.X1) >> 8) + 1, tp.width - 1);
  const int py0 = max((min(s.Y0, s.Y1) >> 8) - 1, 0), py1 = min((max(s.Y0, s.Y1) >> 8) + 1, tp.height - 1);
  const int tx0 = px0 / kTbnTile, ty0 = py0 / kTbnTile, tw = px1 / kTbnTile - tx0 + 1;
  const int nt = (valid && px0 <= px1 && py0 <= py1) ? tw * (py1 / kTbnTile - ty0 + 1) : 0;
  for (int k = 0; __ballot(k < nt) != 0ull; ++k) {
    const bool has = k < nt;
    const uint32_t t = has ? (uint32_t)(ty0 + k / tw) * (uint32_t)tp.tiles_x + (uint32_t)(tx0 + k % tw) : 0u;
    const uint32_t slot = bin_slot(wave_bin_reserve(has, t, tile_count));
    if (!has) continue;
    if (slot < tp.bin_cap) {
      bins[(size_t)t * tp.bin_cap + slot] = index;
    } else {
      atomicOr(&ctr[0], 1u);
      atomicMax(&ctr[1], slot + 1u);
    }
  }
}

// One lane per triangle of the frame's draw list: the vertex stage's N, T, B and posWorld (the forward pass's own
// expressions), the normal-map branch of tbn.vert, the face frame of tbn.geom, and the strip's eight segments clipped
// and snapped into slot prim * 8 + s (kTbnNoSeg where segment s produced nothing).
__global__ __launch_bounds__(256) void k_tbn_segments(const DrawDesc *__restrict__ draws, uint32_t n_draws, uint32_t n_prims,
                                                      Mat4 pv, int32_t enable_normal_map,
                                                      const MaterialDesc *__restrict__ materials, TbnParams tp,
                                                      TbnSeg *__restrict__ segs, uint32_t *__restrict__ tile_count,
                                                      uint32_t *__restrict__ bins, uint32_t *__restrict__ ctr) {
  const uint32_t prim = blockIdx.x * blockDim.x + threadIdx.x;
  if (prim >= n_prims) return;
  const DrawDesc draw = draws[find_draw(draws, n_draws, prim)];
  const PrimSource src = prim_source(draw, prim);
  float im_[3][3];
#pragma unroll
  for (int r = 0; r < 3; ++r)
#pragma unroll
    for (int cc = 0; cc < 3; ++cc) im_[r][cc] = src.ib->inv_model.M[r][cc];
  f3 P[3], T[3], B[3], N[3];
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    const GlobalVertex v = src.v[k];
    // tbn.vert:18-25 is the forward pass's vertex program: the same functions as k_geometry
    const float pos[3] = {v->pos[0], v->pos[1], v->pos[2]};
    const f4 w = vertex_world(src.ib->model, pos);
    f3 Nk = normal_dir(im_, mk3(v->normal[0], v->normal[1], v->normal[2]));
    f3 Tk = normal_dir(im_, mk3(v->tangent[0], v->tangent[1], v->tangent[2]));
    f3 Bk = cross3(Nk, Tk);
    if (enable_normal_map != 0) {
      // tbn.vert:27-42: a vertex-stage fetch with k_shade's sampler (bilinear, REPEAT, LOD 0), then the TBN product
      const TexDesc td = materials[draw.material].maps[kMapNormal];
      const BilinearTaps tp_ = bilinear_taps(v->uv[0], v->uv[1], td.w, td.h);
      const uint32_t *tx32 = reinterpret_cast<const uint32_t *>(td.texels);
      const uint32_t t00 = tx32[tp_.o00], t10 = tx32[tp_.o10], t01 = tx32[tp_.o01], t11 = tx32[tp_.o11];
      const float sx = filter_channel(t00, t10, t01, t11, 0, tp_.fx, tp_.fy) * 2.0f - 1.0f;
      const float sy = filter_channel(t00, t10, t01, t11, 8, tp_.fx, tp_.fy) * 2.0f - 1.0f;
      const float sz = filter_channel(t00, t10, t01, t11, 16, tp_.fx, tp_.fy) * 2.0f - 1.0f;
      const f3 nm = mk3((Tk.x * sx + Bk.x * sy) + Nk.x * sz, (Tk.y * sx + Bk.y * sy) + Nk.y * sz,
                        (Tk.z * sx + Bk.z * sy) + Nk.z * sz);
      f3 bn = mk3(1.0f, 0.0f, 0.0f);
      if (nm.x == 1.0f && nm.y == 0.0f && nm.z == 0.0f) bn = mk3(0.0f, 0.0f, 1.0f);
      const f3 tn = tbn_cross(nm, bn);
      Bk = tbn_cross(nm, tn);
      Tk = tn;
      Nk = nm;
    }
    P[k] = mk3(w.x, w.y, w.z);
    T[k] = Tk; B[k] = Bk; N[k] = Nk;
  }
  // tbn.geom:18-35
  const f3 C = tbn_mean(P[0], P[1], P[2]);
  const f3 e[3] = {scale3(tbn_normalize(tbn_mean(T[0], T[1], T[2])), kTbnLength),
                   scale3(tbn_normalize(tbn_mean(B[0], B[1], B[2])), kTbnLength),
                   scale3(tbn_normalize(tbn_mean(N[0], N[1], N[2])), kTbnLength)};
  float strip[9][4];  // C,T,C, C,B,C, C,N,C (tbn.geom:39-71)
  tbn_to_clip(pv, C, strip[0]);
#pragma unroll
  for (int j = 0; j < 3; ++j) {
    tbn_to_clip(pv, add3(C, e[j]), strip[3 * j + 1]);
#pragma unroll
    for (int k = 0; k < 4; ++k) strip[3 * j][k] = strip[3 * j + 2][k] = strip[0][k];
  }
  const Viewport vp = {tp.half_w, tp.half_h, tp.half_w, tp.half_h};
#pragma unroll  // (static indices into strip: no scratch)
  for (int s = 0; s < 8; ++s) {
    TbnSeg r = {};
    const uint32_t slot = prim * 8u + (uint32_t)s;
    const bool valid = tbn_make_segment(strip[s], strip[s + 1], vp, r);
    r.key = valid ? slot : kTbnNoSeg;
    segs[slot] = r;
    tbn_bin(valid, r, slot, tp, tile_count, bins, ctr);
  }
}

// bbr_selftest_lines: bin segments the caller supplied (record i is bin entry i)
__global__ __launch_bounds__(256) void k_tbn_bin(const TbnSeg *__restrict__ segs, uint32_t n, TbnParams tp,
                                                 uint32_t *__restrict__ tile_count, uint32_t *__restrict__ bins,
                                                 uint32_t *__restrict__ ctr) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  TbnSeg s = {};
  if (i < n) s = segs[i];
  tbn_bin(i < n && (s.X0 != s.X1 || s.Y0 != s.Y1), s, i, tp, tile_count, bins, ctr);
}

// OpenGL 4.6 §14.5.1 diamond-exit rule on 1/256-pixel integers, endpoints relative to the fragment centre, with the
// spec's perturbation p' = p - (eps, eps^2).  A fragment is produced iff the perturbed segment meets the open diamond
// |x| + |y| < 128 and its perturbed end point is not inside it.  After the perturbation nothing touches a boundary, so
// separation along one of three axes decides: the diamond's two edge normals and the segment's normal.
BB_DEV bool tbn_covers(long long ax, long long ay, long long bx, long long by) {
  const long long eb = llabs(bx) + llabs(by);
  if (eb < 128 || (eb == 128 && bx > 0)) return false;  // b - (eps, eps^2) inside the diamond
  const long long au = ax + ay, bu = bx + by;           // axis (1, 1): shifted by -(eps + eps^2)
  if (max(au, bu) <= -128 || min(au, bu) >= 129) return false;
  const long long av = ax - ay, bv = bx - by;           // axis (1, -1): shifted by -eps + eps^2
  if (max(av, bv) <= -128 || min(av, bv) >= 129) return false;
  const long long dx = bx - ax, dy = by - ay;           // axis (-dy, dx): the segment is the point c + dy eps - dx eps^2
  const long long c = dx * ay - dy * ax, h = 128 * max(llabs(dx), llabs(dy));
  if (c > h || (c == h && (dy > 0 || (dy == 0 && dx < 0)))) return false;
  if (c < -h || (c == -h && (dy < 0 || (dy == 0 && dx > 0)))) return false;
  return true;
}

// Walk the segment's major axis through the tile: per column (row) of an x-major (y-major) segment only the four pixels
// around the line's crossing of the pixel centre can hold a fragment; tbn_covers decides exactly.
BB_DEV void tbn_raster_segment(const TbnSeg &s, int tx0, int ty0, const TbnParams &tp, const float *s_depth,
                               uint32_t *s_key) {
  const long long dx = (long long)s.X1 - s.X0, dy = (long long)s.Y1 - s.Y0;
  if (dx == 0 && dy == 0) return;
  const bool xmajor = llabs(dx) >= llabs(dy);
  const int ma0 = xmajor ? s.X0 : s.Y0, ma1 = xmajor ? s.X1 : s.Y1, mi0 = xmajor ? s.Y0 : s.X0;
  const long long dma = xmajor ? dx : dy, dmi = xmajor ? dy : dx;
  const int tma = xmajor ? tx0 : ty0, tmi = xmajor ? ty0 : tx0;
  const int lima = xmajor ? tp.width : tp.height, limi = xmajor ? tp.height : tp.width;
  const int i0 = max(max((min(ma0, ma1) >> 8) - 1, tma), 0);
  const int i1 = min(min((max(ma0, ma1) >> 8) + 1, tma + kTbnTile - 1), lima - 1);
  const int jlo = max(tmi, 0), jhi = min(tmi + kTbnTile - 1, limi - 1);
  const long long den = dx * dx + dy * dy;
  for (int i = i0; i <= i1; ++i) {
    const long long cm = 256ll * i + 128;
    const double mc = (double)mi0 + (double)(cm - ma0) * (double)dmi / (double)dma;
    const int j0 = (int)floor((mc - 128.0) / 256.0);
    for (int j = max(j0 - 1, jlo); j <= min(j0 + 2, jhi); ++j) {
      const int px = xmajor ? i : j, py = xmajor ? j : i;
      const long long fx = 256ll * px + 128, fy = 256ll * py + 128;
      if (!tbn_covers(s.X0 - fx, s.Y0 - fy, s.X1 - fx, s.Y1 - fy)) continue;
      const long long num = (fx - s.X0) * dx + (fy - s.Y0) * dy;
      const double t = (double)num / (double)den;
      const float z = (float)((1.0 - t) * (double)s.za + t * (double)s.zb);
      const int l = (py - ty0) * kTbnTile + (px - tx0);
      if (z >= s_depth[l]) atomicMax(&s_key[l], s.key + 1u);
    }
  }
}

// One workgroup per 32 x 32 tile and slice of kTbnThreads bin entries (blockIdx.z; a slice strides by kTbnSplit slices,
// so that a far ball's few tiles with thousands of segments each are spread over many CUs): the tile's scene depth and
// its keys (ds_max_u32) in LDS, lanes walk the slice's segments, then every touched pixel folds its key into the frame's
// key buffer with one atomicMax (per pixel and slice, lanes on consecutive pixels; never per fragment).
constexpr int kTbnSplit = 16;
__global__ __launch_bounds__(kTbnThreads) void k_tbn_raster(const TbnSeg *__restrict__ segs,
                                                            const uint32_t *__restrict__ tile_count,
                                                            const uint32_t *__restrict__ bins, TbnParams tp,
                                                            const float *__restrict__ depth, uint32_t *__restrict__ keys) {
  __shared__ uint32_t s_key[kTbnTile * kTbnTile];
  __shared__ float s_depth[kTbnTile * kTbnTile];
  const int tx0 = blockIdx.x * kTbnTile, ty0 = blockIdx.y * kTbnTile;
  const uint32_t tile = blockIdx.y * (uint32_t)tp.tiles_x + blockIdx.x;
  const uint32_t n = min(tile_count[tile], tp.bin_cap);
  const uint32_t first = blockIdx.z * kTbnThreads;
  if (first >= n) return;  // (workgroup-uniform)
  for (int l = threadIdx.x; l < kTbnTile * kTbnTile; l += kTbnThreads) {
    const int px = tx0 + (l & (kTbnTile - 1)), py = ty0 + l / kTbnTile;
    s_key[l] = 0u;
    s_depth[l] = (px < tp.width && py < tp.height) ? depth[(size_t)py * tp.width + px] : 0.0f;
  }
  __syncthreads();
  for (uint32_t j = first + threadIdx.x; j < n; j += kTbnThreads * kTbnSplit)
    tbn_raster_segment(segs[bins[(size_t)tile * tp.bin_cap + j]], tx0, ty0, tp, s_depth, s_key);
  __syncthreads();
  for (int l = threadIdx.x; l < kTbnTile * kTbnTile; l += kTbnThreads) {
    const int px = tx0 + (l & (kTbnTile - 1)), py = ty0 + l / kTbnTile;
    const uint32_t k = s_key[l];
    if (k && px < tp.width && py < tp.height) atomicMax(&keys[(size_t)py * tp.width + px], k);
  }
}

// The winning keys to the presented image: flat colour of segment s = (key - 1) & 7, red, green, blue for s / 3 = 0, 1, 2,
// sRGB-encoded (tbn.frag:8-10); pixels without a key are not written.
__global__ __launch_bounds__(256) void k_tbn_colour(const uint32_t *__restrict__ keys, uint32_t *__restrict__ present, size_t n) {
  const size_t o = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (o >= n) return;
  const uint32_t k = keys[o];
  if (!k) return;
  const uint32_t c = ((k - 1u) & 7u) / 3u;
  present[o] = c == 0u ? 0xFF0000FFu : (c == 1u ? 0xFF00FF00u : 0xFFFF0000u);
}

// A queued shadow pass (bbr_queue_shadow_caster) has rendered its faces in front of its frame, each counting in a block of
// its own (`face_ctr`, `n_blocks` <= kShadowPassBlocks of them, zero before the pass).  What the synchronous pass does on
// the host after a wait happens here, one wave behind the last face and in front of the frame's k_geometry: the blocks are
// folded into the frame's own words and cleared for the next pass.
//   overflow, bin_need   or / max into the frame's block `frame_ctr` (zero since the slot's last frame retired it, and only
//                        ever or-ed and max-ed by k_geometry): the frame's k_raster publishes them in the pinned flag words,
//                        its shading retires them (retire_counters) -- an overflow in the pass is the frame's
//   n_broad, n_clip_slots   are allocators in the frame's block, so the largest among the faces goes beside them
//                        (Counters::pass_broad / pass_clip, which travel with the block) and into the pinned words of their own
// (A frame whose pass overflowed the every-tile list then ignores its own list, k_raster: it is rendered again anyway.)
constexpr int kShadowPassBlocks = kMaxShadowCasters * kMaxShadowFaces;
constexpr int kPassRetireThreads = 64;
static_assert(kShadowPassBlocks <= kPassRetireThreads, "one lane per block");
__global__ __launch_bounds__(kPassRetireThreads) void k_shadow_pass_retire(Counters *__restrict__ face_ctr, uint32_t n_blocks,
                                                                          Counters *__restrict__ frame_ctr,
                                                                          uint32_t *__restrict__ host_flags) {
  const uint32_t lane = threadIdx.x;
  uint32_t overflow = 0u, bin_need = 0u, broad = 0u, clip = 0u;
  if (lane < n_blocks) {
    const Counters &b = face_ctr[lane];
    overflow = b.overflow, bin_need = b.bin_need, broad = b.n_broad, clip = b.n_clip_slots;
  }
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) {  // (butterfly: every lane ends with the wave's value)
    overflow |= (uint32_t)__shfl_xor((int)overflow, d);
    bin_need = max(bin_need, (uint32_t)__shfl_xor((int)bin_need, d));
    broad = max(broad, (uint32_t)__shfl_xor((int)broad, d));
    clip = max(clip, (uint32_t)__shfl_xor((int)clip, d));
  }
  __syncthreads();  // (every block has been read)
  for (uint32_t i = lane; i < n_blocks * (uint32_t)(sizeof(Counters) / 4); i += kPassRetireThreads)
    reinterpret_cast<uint32_t *>(face_ctr)[i] = 0u;
  if (lane == 0) {
    if (overflow) atomicOr(&frame_ctr->overflow, overflow);
    if (bin_need) atomicMax(&frame_ctr->bin_need, bin_need);
    frame_ctr->pass_broad = broad;
    frame_ctr->pass_clip = clip;
    host_flags[kFlagPassBroadNeed] = broad;
    host_flags[kFlagPassClipNeed] = clip;
  }
}

// ------------------------------------------------------------------------------------------------
// Option "surface_keep": a slot's shaded SURFACE, kept under a kept view (option "view_keep").
//
// What light_surface receives of a fragment -- P, the normal as surface_normal<false> returns it, albedo, metallic, roughness,
// ao -- depends on the slot's visibility, the draws' contents, the materials and enable_normal_map; not on the lights, the
// exposure or tone mapping.  k_surface_store writes it once per stop of the camera and slot, k_shade_lit reads it back in
// every frame behind: no item word, no fragment list, no record, no texel, one round trip of four coalesced loads per wave.
//
// The layout: three float4 planes and one uint32 plane of `plane` = 64 x (item capacity) entries each, one behind the other,
// entry [item * 64 + lane] the fragment slot k_shade's wave `item` shades in lane `lane`:
//   plane 0  P.x  P.y  P.z  n.x      plane 1  n.y  n.z  albedo.r  albedo.g      plane 2  albedo.b  metallic  roughness  ao
//   plane 3  the pixel's index in the output as k_shade forms it, or kSurfaceNoPixel for a lane that is not `valid`
// Every access is one full-width vector instruction: 1 KB (256 B) contiguous per wave.
// Both kernels stand HERE, behind every kernel above, for the reason given at k_sample_merge.
// ------------------------------------------------------------------------------------------------
constexpr uint32_t kSurfaceNoPixel = 0xFFFFFFFFu;  // (a frame has at most 2^30 pixels)
constexpr int kSurfacePlanes = 3;
// float4 entries of a surface of `items` items: the three planes, and the index plane (four words per entry)
constexpr size_t surface_keep_entries(size_t items) { return items * 64 * kSurfacePlanes + items * 64 / 4; }

// The fragment stage of k_shade up to the light loop, through the functions the fragment kernels share -- the bits are k_shade's
// by construction -- in shade_item_list's shape: every lane gathers its own record, each wave walks the list with the launch's
// stride.  One tap at (u, v): the filter of "max_anisotropy" 1, "mip_levels" 1.  Packed and mixed materials, per lane.
// `n_cap`: the item capacity of `surface` (the host sized it from the slot's exact item count: never exceeded, and checked here).
template <int TILE_W, int TILE_H>
__global__ __launch_bounds__(kShadeThreads) void k_surface_store(
    const uint32_t *__restrict__ items, const uint32_t *__restrict__ item_count, uint32_t n_cap,
    const unsigned long long *__restrict__ frags, const uint32_t *__restrict__ frag_count,
    const ShadeRec *__restrict__ recs, const ClipSlot *__restrict__ clip_arena, FrameParams fp, int enable_normal_map,
    const MaterialDesc *__restrict__ materials, float4 *__restrict__ surface) {
  constexpr int TILE_PIXELS = TILE_W * TILE_H;
  const int lane = (int)(threadIdx.x & 63u);
  const uint32_t n_items = min(*item_count, n_cap);
  const size_t plane = (size_t)n_cap * 64;
  uint32_t *const index = reinterpret_cast<uint32_t *>(surface + kSurfacePlanes * plane);
  for (uint32_t j = (uint32_t)__builtin_amdgcn_readfirstlane((int)(blockIdx.x * (uint32_t)kShadeWaves + (threadIdx.x >> 6)));
       j < n_items; j += gridDim.x * (uint32_t)kShadeWaves) {
    const uint32_t item = items[1u + j];
    const ItemPlace at = decode_item(fp, item);
    bool valid;
    const unsigned long long frag = fetch_fragment<TILE_PIXELS, false>(item, at, lane, frags, frag_count, valid);
    const uint32_t ref = (uint32_t)frag;
    int x, y;
    tile_pixel<TILE_W>(fragment_pixel<TILE_PIXELS>(frag), x, y);
    const int gx = at.tx * TILE_W + x, gy = at.ty * TILE_H + y;
    const uint32_t opix = (uint32_t)(at.out_tile_row * TILE_H + y) * (uint32_t)fp.width + (uint32_t)gx;

    // the head of the primitive record and, for a clipped fragment, its sub-triangle's clip slot
    const ShadeRec *rp = recs + (ref >> 3);
    const uint32_t clip1 = (uint32_t)(frag >> (32 + kFragPixBits));  // clip-arena slot + 1 of a clipped sub-triangle, 0: none / unknown
    bool clipped = clip1 != 0u;
    const ClipSlot *cp = clip_arena + (clipped ? clip1 - 1u : 0u);
    PlaneHead h = clipped ? cp->h : rp->h;
    float uv[3][2], cb[3][3] = {};
#pragma unroll
    for (int k = 0; k < 3; ++k) { uv[k][0] = rp->uv[k][0]; uv[k][1] = rp->uv[k][1]; }
    const uint32_t packed_dims = rp->packed_dims, material = rp->material, clip_base = rp->clip_base;
    const GlobalBytes packed_texels = (GlobalBytes)rp->packed;
    if (late_clip_slot(clipped, clip_base)) {
      cp = clip_arena + record_clip_slot(clip_base, ref);
      h = cp->h;
      clipped = true;
    }
    if (clipped) {
#pragma unroll
      for (int jj = 0; jj < 3; ++jj)
#pragma unroll
        for (int k = 0; k < 3; ++k) cb[jj][k] = cp->bary[jj][k];
    }
    const PlaneUV here = plane_uv(h, clipped, cb, uv, gx, gy);
    float a[kNumVary];
    a[0] = here.u; a[1] = here.v;
#pragma unroll
    for (int jj = 0; jj < kNumBodyVary; ++jj) a[2 + jj] = interp3(here.b0, here.b1, here.b2, rp->vary[jj][0], rp->vary[jj][1], rp->vary[jj][2]);

    // texture filtering, forward_brdf.frag:16-22: k_shade's statements
    f3 albedo, normal;
    float metallic, roughness, ao;
    if (packed_dims != 0u) {
      const PackedFetch fetch{packed_texels, (int)(packed_dims & 0xFFFFu), (int)(packed_dims >> 16)};
      const PackedFetch::Raw r = fetch.load(here.u, here.v);
      albedo.x = filter_channel(r.q00.x, r.q10.x, r.q01.x, r.q11.x, 0, r.fx, r.fy);
      albedo.y = filter_channel(r.q00.x, r.q10.x, r.q01.x, r.q11.x, 8, r.fx, r.fy);
      albedo.z = filter_channel(r.q00.x, r.q10.x, r.q01.x, r.q11.x, 16, r.fx, r.fy);
      metallic = filter_channel(r.q00.x, r.q10.x, r.q01.x, r.q11.x, 24, r.fx, r.fy);
      roughness = filter_channel(r.q00.y, r.q10.y, r.q01.y, r.q11.y, 24, r.fx, r.fy);
      ao = filter_channel(r.q00.z, r.q10.z, r.q01.z, r.q11.z, 0, r.fx, r.fy);
      normal = surface_normal<false>(a, enable_normal_map, [&] {
        return mk3(normal_map_axis(filter_channel(r.q00.y, r.q10.y, r.q01.y, r.q11.y, 0, r.fx, r.fy)),
                   normal_map_axis(filter_channel(r.q00.y, r.q10.y, r.q01.y, r.q11.y, 8, r.fx, r.fy)),
                   normal_map_axis(filter_channel(r.q00.y, r.q10.y, r.q01.y, r.q11.y, 16, r.fx, r.fy)));
      });
    } else {
      // maps of different sizes: one set of taps per map
      const MaterialDesc &md = materials[material];
      albedo = sample_map_rgb(md.maps[kMapAlbedo], here.u, here.v);
      metallic = sample_map_r(md.maps[kMapMetallic], here.u, here.v);
      roughness = sample_map_r(md.maps[kMapRoughness], here.u, here.v);
      ao = sample_map_r(md.maps[kMapAO], here.u, here.v);
      normal = surface_normal<false>(a, enable_normal_map, [&] {
        const f3 t = sample_map_rgb(md.maps[kMapNormal], here.u, here.v);
        return mk3(normal_map_axis(t.x), normal_map_axis(t.y), normal_map_axis(t.z));
      });
    }
    const size_t e = (size_t)j * 64 + (size_t)lane;
    surface[e] = make_float4(a[2], a[3], a[4], normal.x);
    surface[plane + e] = make_float4(normal.y, normal.z, albedo.x, albedo.y);
    surface[2 * plane + e] = make_float4(albedo.z, metallic, roughness, ao);
    index[e] = valid ? opix : kSurfaceNoPixel;
  }
}

// One item per wave, four waves per workgroup, the grid sized by the host from the exact item count (the pinned word the slot's
// last full frame left): no tail launch and no TAIL form.  A wave's four loads depend on nothing but its own index; then the
// light loop on the slot's cooked table, as surface_colour<false> runs it without a shadow, and the store.  No LDS, no barrier.
// The surface is read with non-temporal loads: a slot reads its surface again three frames later, three slots' surfaces exceed
// the Infinity Cache, and what they would push out of the L2 are the pixels and light tables of the frames in flight.  Alone the
// two policies measure the same; with three frames in flight plain loads cost 1.9 us per frame (profiles/r18_surface_keep.txt).
template <bool PRESENT = false>
__global__ __launch_bounds__(kShadeThreads) __attribute__((amdgpu_waves_per_eu(8))) void k_shade_lit(
    const float4 *__restrict__ surface, const uint32_t *__restrict__ item_count, uint32_t n_cap, ShadeParams sp,
    const CookedLight *__restrict__ cooked, float4 *__restrict__ out, const SrgbTables *__restrict__ tables,
    uint32_t *__restrict__ out8, Counters *__restrict__ ctr, Counters *__restrict__ ctr_done, uint32_t *__restrict__ item_groups) {
  const ConstLights lights_c{(ConstCooked)cooked};
  retire_counters(ctr, ctr_done, item_groups);
  const uint32_t j = (uint32_t)__builtin_amdgcn_readfirstlane((int)(blockIdx.x * (uint32_t)kShadeWaves + (threadIdx.x >> 6)));
  if (j >= n_cap) return;  // (never: the host's grid; what keeps the loads below inside the buffer)
  const size_t plane = (size_t)n_cap * 64, e = (size_t)j * 64 + (size_t)(threadIdx.x & 63u);
  const uint32_t *const index = reinterpret_cast<const uint32_t *>(surface + kSurfacePlanes * plane);
  const v4f *const sv = reinterpret_cast<const v4f *>(surface);
  const v4f q0 = __builtin_nontemporal_load(sv + e), q1 = __builtin_nontemporal_load(sv + plane + e),
            q2 = __builtin_nontemporal_load(sv + 2 * plane + e);
  const uint32_t opix = __builtin_nontemporal_load(index + e);
  if (j >= *item_count) return;  // a wave without an item (the grid is rounded up to whole workgroups)
  const float4 color = light_surface(sp, lights_c, mk3(q0.x, q0.y, q0.z), mk3(q0.w, q1.x, q1.y), mk3(q1.z, q1.w, q2.x), q2.y, q2.z, q2.w);
  store_colour<PRESENT>(opix != kSurfaceNoPixel, color, (size_t)opix, out, out8, tables, sp);
}

}  // namespace bbr
