// Stand-alone check of csrc/bb_pack.h on heap images allocated at their exact sizes, for a build with
// -fsanitize=address,undefined (tests/test_texture_chart.py compiles and runs it): a read past a map or a write past the
// size the plan reports ends the program with the sanitizer's report; a wrong decision or byte ends it with exit code 1.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "bb_pack.h"

using namespace bbr;

namespace {

struct Case {
  const char *name;
  int size[kMapCount][2];  // w, h per map in PBRMapType order; 0 = the map is not supplied
  bool packable;
  int pw, ph;
};

int run(const Case &c) {
  bbr_image maps[kMapCount];
  uint8_t *own[kMapCount] = {};
  for (int k = 0; k < kMapCount; ++k) {
    const int w = c.size[k][0], h = c.size[k][1];
    maps[k] = bbr_image{nullptr, 0, 0};
    if (!w) continue;
    const size_t n = (size_t)w * h * 4;
    own[k] = (uint8_t *)std::malloc(n);  // exactly the image: one byte further is the sanitizer's red zone
    for (size_t i = 0; i < n; ++i) own[k][i] = (uint8_t)(i * 131u + k * 17u + 1u);
    maps[k] = bbr_image{own[k], w, h};
  }
  int bad = 0;
  const PackPlan plan = pack_plan(maps);
  if (plan.packable != c.packable) bad = 1;
  if (plan.packable) {  // (whatever the case expects: a wrong "packable" is then also the sanitizer's finding)
    if (plan.pw != c.pw || plan.ph != c.ph) bad = 1;
    uint8_t *out = (uint8_t *)std::malloc(plan.bytes);
    pack_fill(maps, plan, out);
    const size_t w4 = ((size_t)plan.pw + 3) / 4;
    auto texel = [&](int k, size_t i) { return own[k] ? own[k] + 4 * i : kDefaultTexel[k]; };
    for (size_t y = 0; y < (size_t)plan.ph && !bad; ++y)
      for (size_t x = 0; x < (size_t)plan.pw; ++x) {
        const size_t i = y * plan.pw + x;
        const uint8_t *t = out + (((y / 4) * w4 + x / 4) * 16 + (y % 4) * 4 + x % 4) * kPackedTexelBytes;
        const uint8_t *al = texel(kMapAlbedo, i), *no = texel(kMapNormal, i);
        if (t[0] != al[0] || t[1] != al[1] || t[2] != al[2] || t[3] != texel(kMapMetallic, i)[0] || t[4] != no[0] || t[5] != no[1] ||
            t[6] != no[2] || t[7] != texel(kMapRoughness, i)[0] || t[8] != texel(kMapAO, i)[0]) {
          bad = 1;
          break;
        }
      }
    for (size_t i = plan.bytes - kPackedTexelPad; i < plan.bytes; ++i)
      if (out[i]) bad = 1;
    std::free(out);
  }
  for (auto p : own) std::free(p);
  std::printf("%-28s %s\n", c.name, bad ? "WRONG" : "ok");
  return bad;
}

}  // namespace

int main() {
  const Case cases[] = {
      {"1x1 first, then 6x10", {{1, 1}, {6, 10}, {6, 10}, {6, 10}, {6, 10}, {0, 0}}, false, 0, 0},
      {"6x10 first, then 1x1", {{6, 10}, {0, 0}, {1, 1}, {0, 0}, {0, 0}, {0, 0}}, false, 0, 0},
      {"5x3", {{5, 3}, {5, 3}, {5, 3}, {5, 3}, {5, 3}, {5, 3}}, true, 5, 3},
      {"16384x3", {{16384, 3}, {16384, 3}, {16384, 3}, {16384, 3}, {16384, 3}, {0, 0}}, true, 16384, 3},
      {"all maps absent", {{0, 0}, {0, 0}, {0, 0}, {0, 0}, {0, 0}, {0, 0}}, true, 1, 1},
      {"all five at 1x1", {{1, 1}, {1, 1}, {1, 1}, {1, 1}, {1, 1}, {0, 0}}, true, 1, 1},
      {"only the normal map, 6x10", {{0, 0}, {0, 0}, {0, 0}, {0, 0}, {6, 10}, {0, 0}}, true, 6, 10},
  };
  int bad = 0;
  for (const Case &c : cases) bad |= run(c);
  return bad;
}
