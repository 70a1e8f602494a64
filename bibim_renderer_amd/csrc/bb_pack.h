// bb_pack.h -- the packed form of a material, decided and filled on the host.  No HIP: compiles with any C++17 compiler.
//
// The five shaded maps (albedo, metallic, roughness, ao, normal) are interleaved into 9-byte records (bb_types.h) when
// every SUPPLIED one of them has the same size; a missing map is uniform and broadcasts its default texel.  A supplied
// map of another size -- 1 x 1 included, wherever it stands in map order -- leaves the material unpacked: each map then
// has its own size and its own tap count.  No map supplied: packed at 1 x 1.
//
// Layout: block-linear, 4 x 4 texel blocks of 144 bytes, blocks in row-major order:
//   texel (x, y) = record ((y >> 2) * ceil(w / 4) + (x >> 2)) * 16 + (y & 3) * 4 + (x & 3)
// Records of texels outside w x h (the padding of the last block column / row) and the kPackedTexelPad bytes behind the
// last record (the 12-byte load of the last texel reaches 3 bytes past it) are zero.
#pragma once
#include <cstddef>
#include <cstdint>
#include <cstring>

#include "bb_types.h"
#include "bibim_hip.h"

namespace bbr {

// the `default` material's texels (resources/pbr/default/*.png are uniform images), PBRMapType order
constexpr uint8_t kDefaultTexel[kMapCount][4] = {{255, 255, 255, 255}, {0, 0, 0, 255},       {0, 0, 0, 255},
                                                 {255, 255, 255, 255}, {127, 127, 255, 255}, {0, 0, 0, 255}};

inline bool map_supplied(const bbr_image &im) { return im.rgba && im.width > 0 && im.height > 0; }

struct PackPlan {
  bool packable;
  int pw, ph;    // the shared size (1 x 1 when no shaded map is supplied); meaningless when !packable
  size_t bytes;  // of the packed form, pad included; 0 when !packable
};

inline PackPlan pack_plan(const bbr_image maps[kMapCount]) {
  const int used[5] = {kMapAlbedo, kMapMetallic, kMapRoughness, kMapAO, kMapNormal};
  PackPlan p{true, 1, 1, 0};
  bool seen = false;
  for (int k : used) {
    const bbr_image &im = maps[k];
    if (!map_supplied(im)) continue;
    if (!seen) {
      p.pw = im.width;
      p.ph = im.height;
      seen = true;
    } else if (im.width != p.pw || im.height != p.ph) {
      p.packable = false;
    }
  }
  if (p.packable) {
    const size_t w4 = ((size_t)p.pw + 3) / 4, h4 = ((size_t)p.ph + 3) / 4;
    p.bytes = w4 * h4 * 16 * kPackedTexelBytes + kPackedTexelPad;
  }
  return p;
}

// fills out[0 .. plan.bytes) for a packable plan of these maps
inline void pack_fill(const bbr_image maps[kMapCount], const PackPlan &plan, uint8_t *out) {
  std::memset(out, 0, plan.bytes);
  const size_t pw = (size_t)plan.pw, n_texels = pw * (size_t)plan.ph, w4 = (pw + 3) / 4;
  auto texel = [&](int k, size_t i) -> const uint8_t * { return map_supplied(maps[k]) ? maps[k].rgba + 4 * i : kDefaultTexel[k]; };
  for (size_t i = 0; i < n_texels; ++i) {
    const uint8_t *al = texel(kMapAlbedo, i), *me = texel(kMapMetallic, i), *ro = texel(kMapRoughness, i);
    const uint8_t *ao = texel(kMapAO, i), *no = texel(kMapNormal, i);
    const size_t x = i % pw, y = i / pw;
    uint8_t *t = out + (((y >> 2) * w4 + (x >> 2)) * 16 + (y & 3) * 4 + (x & 3)) * kPackedTexelBytes;
    t[0] = al[0]; t[1] = al[1]; t[2] = al[2]; t[3] = me[0];
    t[4] = no[0]; t[5] = no[1]; t[6] = no[2]; t[7] = ro[0];
    t[8] = ao[0];
  }
}

}  // namespace bbr
