// ui_validate_check.cpp -- csrc/bb_ui.h under AddressSanitizer + UBSan, outside python: heap arrays of exactly the sizes the
// draw data declares, so that a read past a count (or before a check) is an error of the run, and every rejection of
// bbr_ui_validate on data that would otherwise send a kernel out of bounds.  Built and run by tests/test_ui_validate.py.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <memory>
#include <vector>

#include "bb_ui.h"

namespace {

struct Vert {
  float pos[2], uv[2];
  uint32_t col;
};
static_assert(sizeof(Vert) == bbr::kUiVertexBytes && sizeof(bbr_ui_cmd) == 32, "layouts");

// draw data on the heap at its exact size (no slack behind any array)
struct Data {
  std::unique_ptr<uint8_t[]> v;
  std::unique_ptr<uint16_t[]> i;
  std::unique_ptr<bbr_ui_cmd[]> c;
  bbr_ui_draw d;
};

Data make(const std::vector<Vert> &v, const std::vector<uint16_t> &i, const std::vector<bbr_ui_cmd> &c) {
  Data o;
  o.v.reset(new uint8_t[v.size() * sizeof(Vert)]);
  o.i.reset(new uint16_t[i.size()]);
  o.c.reset(new bbr_ui_cmd[c.size()]);
  if (!v.empty()) std::memcpy(o.v.get(), v.data(), v.size() * sizeof(Vert));
  if (!i.empty()) std::memcpy(o.i.get(), i.data(), i.size() * sizeof(uint16_t));
  if (!c.empty()) std::memcpy(o.c.get(), c.data(), c.size() * sizeof(bbr_ui_cmd));
  o.d = bbr_ui_draw{v.empty() ? nullptr : o.v.get(), (uint32_t)v.size(), i.empty() ? nullptr : o.i.get(), (uint32_t)i.size(),
                    c.empty() ? nullptr : o.c.get(), (uint32_t)c.size(), {0.0f, 0.0f}, {64.0f, 48.0f}, {1.0f, 1.0f}};
  return o;
}

const std::vector<Vert> kQuad = {{{4, 4}, {0, 0}, 0x80FFFFFFu}, {{20, 4}, {1, 0}, 0x80FFFFFFu}, {{20, 12}, {1, 1}, 0x80FFFFFFu},
                                 {{4, 12}, {0, 1}, 0x80FFFFFFu}};
const std::vector<uint16_t> kQuadIdx = {0, 1, 2, 0, 2, 3};
bbr_ui_cmd cmd(float x0, float y0, float x1, float y1, uint32_t vtx, uint32_t idx, uint32_t n) {
  return bbr_ui_cmd{{x0, y0, x1, y1}, 1, vtx, idx, n};
}

int failures = 0;
void expect(const char *name, int rc, int want, const int32_t *box = nullptr, const int32_t *want_box = nullptr) {
  bool ok = rc == want;
  if (ok && want_box) ok = std::memcmp(box, want_box, 4 * sizeof(int32_t)) == 0;
  std::printf("%-28s %s\n", name, ok ? "ok" : "WRONG");
  failures += !ok;
}

}  // namespace

int main() {
  const float inf = std::numeric_limits<float>::infinity(), nan = std::numeric_limits<float>::quiet_NaN();
  int32_t box[4];
  {
    Data a = make(kQuad, kQuadIdx, {cmd(2.5f, -3.0f, 30.2f, 20.9f, 0, 0, 6), cmd(40.0f, 10.0f, 90.0f, 47.5f, 0, 0, 6), cmd(70.0f, 0, 90.0f, 9.0f, 0, 0, 6),
                                    cmd(0, 0, 64.0f, 48.0f, 0, 0, 0)});
    const int32_t want[4] = {2, 0, 64, 47};  // [2, 29) x [0, 20) and [40, 64) x [10, 47); beyond the frame and elem_count 0 add nothing
    expect("valid, union box", bbr::ui_validate(&a.d, 64, 48, box), BBR_OK, box, want);
    expect("valid, no box wanted", bbr::ui_validate(&a.d, 64, 48, nullptr), BBR_OK);
  }
  {
    Data a = make({}, {}, {});
    const int32_t want[4] = {0, 0, 0, 0};
    expect("empty draw data", bbr::ui_validate(&a.d, 64, 48, box), BBR_OK, box, want);
    expect("NULL draw data", bbr::ui_validate(nullptr, 64, 48, box), BBR_ERR_INVALID_ARGUMENT);
    expect("frame 0 x 48", bbr::ui_validate(&a.d, 0, 48, box), BBR_ERR_INVALID_ARGUMENT);
  }
  {
    Data a = make(kQuad, kQuadIdx, {cmd(0, 0, 64, 48, 0, 0, 5)});
    expect("elem_count % 3", bbr::ui_validate(&a.d, 64, 48, box), BBR_ERR_INVALID_ARGUMENT);
  }
  {
    Data a = make(kQuad, kQuadIdx, {cmd(0, 0, 64, 48, 0, 3, 6)});
    expect("idx_offset + elem_count", bbr::ui_validate(&a.d, 64, 48, box), BBR_ERR_INVALID_ARGUMENT);
    Data b = make(kQuad, kQuadIdx, {cmd(0, 0, 64, 48, 0, 0xFFFFFFFDu, 6)});
    expect("idx_offset wraps", bbr::ui_validate(&b.d, 64, 48, box), BBR_ERR_INVALID_ARGUMENT);
  }
  {
    Data a = make(kQuad, kQuadIdx, {cmd(0, 0, 64, 48, 1, 0, 6)});
    expect("vtx_offset + index", bbr::ui_validate(&a.d, 64, 48, box), BBR_ERR_INVALID_ARGUMENT);
    Data b = make(kQuad, {0, 1, 4, 0, 2, 3}, {cmd(0, 0, 64, 48, 0, 0, 6)});
    expect("index past the vertices", bbr::ui_validate(&b.d, 64, 48, box), BBR_ERR_INVALID_ARGUMENT);
    Data c = make(kQuad, kQuadIdx, {cmd(0, 0, 64, 48, 0xFFFFFFFFu, 0, 6)});
    expect("vtx_offset wraps", bbr::ui_validate(&c.d, 64, 48, box), BBR_ERR_INVALID_ARGUMENT);
    Data d = make(kQuad, kQuadIdx, {cmd(90, 0, 99, 48, 1, 0, 6)});  // a skipped command's indices are checked as well
    expect("bad index, dead scissor", bbr::ui_validate(&d.d, 64, 48, box), BBR_ERR_INVALID_ARGUMENT);
  }
  for (int field = 0; field < 4; ++field)
    for (float bad : {inf, -inf, nan}) {
      std::vector<Vert> v = kQuad;
      (field < 2 ? v[3].pos[field] : v[3].uv[field - 2]) = bad;
      Data a = make(v, kQuadIdx, {cmd(0, 0, 64, 48, 0, 0, 6)});
      expect("non-finite pos / uv", bbr::ui_validate(&a.d, 64, 48, box), BBR_ERR_INVALID_ARGUMENT);
    }
  {
    std::vector<Vert> v = kQuad;
    v[1].pos[0] = 32768.0f;  // snaps to 2^23 exactly: the last admitted coordinate
    v[2].pos[1] = -32000.0f;
    Data a = make(v, kQuadIdx, {cmd(0, 0, 64, 48, 0, 0, 6)});
    expect("snap at +-2^23", bbr::ui_validate(&a.d, 64, 48, box), BBR_OK);
    v[1].pos[0] = 32768.01f;
    Data b = make(v, kQuadIdx, {cmd(0, 0, 64, 48, 0, 0, 6)});
    expect("snap beyond 2^23", bbr::ui_validate(&b.d, 64, 48, box), BBR_ERR_INVALID_ARGUMENT);
    v[1].pos[0] = 3.0e38f;
    Data c = make(v, kQuadIdx, {cmd(0, 0, 64, 48, 0, 0, 6)});
    expect("huge position", bbr::ui_validate(&c.d, 64, 48, box), BBR_ERR_INVALID_ARGUMENT);
  }
  for (float bad : {0.0f, -64.0f, nan, inf}) {
    Data a = make(kQuad, kQuadIdx, {cmd(0, 0, 64, 48, 0, 0, 6)});
    a.d.display_size[1] = bad;
    expect("display_size", bbr::ui_validate(&a.d, 64, 48, box), BBR_ERR_INVALID_ARGUMENT);
  }
  {
    Data a = make(kQuad, kQuadIdx, {cmd(0, 0, 64, 48, 0, 0, 6)});
    a.d.vertices = nullptr;
    expect("NULL vertices, count 4", bbr::ui_validate(&a.d, 64, 48, box), BBR_ERR_INVALID_ARGUMENT);
  }
  {  // scissor quirks on their own
    Data a = make(kQuad, kQuadIdx, {});
    int32_t b[4];
    const float c1[4] = {10.9f, -3.0f, 20.1f, 9.9f};
    const bool live = bbr::ui_scissor(c1, a.d, 64, 48, b);
    const int32_t want[4] = {10, 0, 19, 9};
    expect("scissor truncates z - x", live ? 0 : 1, 0, b, want);
    const float c2[4] = {12.0f, 0.0f, 5.0f, 10.0f};
    expect("scissor z < x is empty", bbr::ui_scissor(c2, a.d, 64, 48, b) ? 1 : 0, 0);
    const float c3[4] = {-inf, -inf, inf, inf};
    const int32_t all[4] = {0, 0, 64, 48};
    expect("scissor of infinities", bbr::ui_scissor(c3, a.d, 64, 48, b) ? 0 : 1, 0, b, all);
  }
  float dec[256];
  bbr::ui_dec_table(dec);
  std::printf("dec");
  for (int b = 0; b < 256; ++b) {
    uint32_t u;
    std::memcpy(&u, &dec[b], 4);
    std::printf(" %08x", u);
  }
  std::printf("\n");
  return failures ? 1 : 0;
}
