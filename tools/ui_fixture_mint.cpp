// ui_fixture_mint.cpp -- mints the draw data behind tests/golden/ui_drawdata.npz (authoring container only).
//
// A headless GUI context lays out one window and renders three frames; the draw data of the last one is flattened the way
// INTEGRATION.md shows (all command lists in order, offsets made global) and dumped next to the font atlas' alpha.  Compiled by
// tools/make_fixtures.py ui_drawdata against the reference's copy of the GUI library (imgui.cpp, imgui_draw.cpp,
// imgui_widgets.cpp); nothing of it runs on a GPU machine and nothing compiled from it is committed.
//
// File layout (little endian): u32 n_vertices, n_indices, n_cmds, n_lists, atlas_w, atlas_h; f32 display_pos[2],
// display_size[2], framebuffer_scale[2]; ImDrawVert[n_vertices] (20 B); u16[n_indices]; bbr_ui_cmd[n_cmds] (32 B);
// u8[atlas_w * atlas_h].
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "imgui/imgui.h"

struct Cmd {
  float clip_rect[4];
  int32_t texture;
  uint32_t vtx_offset, idx_offset, elem_count;
};
static_assert(sizeof(Cmd) == 32 && sizeof(ImDrawVert) == 20 && sizeof(ImDrawIdx) == 2, "layouts of include/bibim_hip.h");

int main(int argc, char **argv) {
  if (argc != 2) {
    std::fprintf(stderr, "usage: %s OUT\n", argv[0]);
    return 2;
  }
  IMGUI_CHECKVERSION();
  ImGui::CreateContext();
  ImGuiIO &io = ImGui::GetIO();
  io.IniFilename = nullptr;
  io.DisplaySize = ImVec2(1280.0f, 720.0f);
  io.DeltaTime = 1.0f / 60.0f;
  unsigned char *alpha = nullptr;
  int aw = 0, ah = 0;
  io.Fonts->GetTexDataAsAlpha8(&alpha, &aw, &ah);  // default font
  io.Fonts->TexID = (ImTextureID)(intptr_t)1;      // the atlas is texture 1, the image below texture 2

  bool normal_map = true;
  float exposure = 1.25f;
  int pass = 1;
  for (int frame = 0; frame < 3; ++frame) {
    ImGui::NewFrame();
    ImGui::SetNextWindowPos(ImVec2(37.0f, -41.0f));  // partly off the top edge
    ImGui::SetNextWindowSize(ImVec2(430.0f, 520.0f));
    ImGui::Begin("Render settings");
    ImGui::Checkbox("Enable Normal Map", &normal_map);
    ImGui::SliderFloat("Exposure", &exposure, 0.0f, 4.0f);
    ImGui::RadioButton("Forward", &pass, 0);
    ImGui::SameLine();
    ImGui::RadioButton("Deferred", &pass, 1);
    ImGui::SameLine();
    ImGui::RadioButton("G-buffer", &pass, 2);
    ImGui::BeginChild("materials", ImVec2(0.0f, 170.0f), true);
    for (int i = 0; i < 30; ++i) ImGui::Text("material %02d  roughness %.2f", i, 0.03f * (float)i);
    ImGui::EndChild();
    ImGui::Image((ImTextureID)(intptr_t)2, ImVec2(150.0f, 110.0f), ImVec2(-0.25f, -0.5f), ImVec2(1.75f, 1.5f),
                 ImVec4(1.0f, 0.9f, 0.8f, 0.85f), ImVec4(1.0f, 1.0f, 1.0f, 0.5f));
    ImGui::End();
    ImGui::Render();
  }
  const ImDrawData *dd = ImGui::GetDrawData();

  std::vector<ImDrawVert> vertices;
  std::vector<ImDrawIdx> indices;
  std::vector<Cmd> cmds;
  for (int n = 0; n < dd->CmdListsCount; ++n) {
    const ImDrawList *list = dd->CmdLists[n];
    const uint32_t v0 = (uint32_t)vertices.size(), i0 = (uint32_t)indices.size();
    for (int c = 0; c < list->CmdBuffer.Size; ++c) {
      const ImDrawCmd &pc = list->CmdBuffer[c];
      if (pc.UserCallback) continue;
      Cmd out;
      out.clip_rect[0] = pc.ClipRect.x; out.clip_rect[1] = pc.ClipRect.y; out.clip_rect[2] = pc.ClipRect.z; out.clip_rect[3] = pc.ClipRect.w;
      out.texture = (int32_t)(intptr_t)pc.TextureId;
      out.vtx_offset = pc.VtxOffset + v0;
      out.idx_offset = pc.IdxOffset + i0;
      out.elem_count = pc.ElemCount;
      cmds.push_back(out);
    }
    vertices.insert(vertices.end(), list->VtxBuffer.Data, list->VtxBuffer.Data + list->VtxBuffer.Size);
    indices.insert(indices.end(), list->IdxBuffer.Data, list->IdxBuffer.Data + list->IdxBuffer.Size);
  }

  std::FILE *f = std::fopen(argv[1], "wb");
  if (!f) return 1;
  const uint32_t head[6] = {(uint32_t)vertices.size(), (uint32_t)indices.size(), (uint32_t)cmds.size(), (uint32_t)dd->CmdListsCount,
                            (uint32_t)aw, (uint32_t)ah};
  const float geo[6] = {dd->DisplayPos.x, dd->DisplayPos.y, dd->DisplaySize.x, dd->DisplaySize.y, dd->FramebufferScale.x,
                        dd->FramebufferScale.y};
  std::fwrite(head, sizeof head, 1, f);
  std::fwrite(geo, sizeof geo, 1, f);
  std::fwrite(vertices.data(), sizeof(ImDrawVert), vertices.size(), f);
  std::fwrite(indices.data(), sizeof(ImDrawIdx), indices.size(), f);
  std::fwrite(cmds.data(), sizeof(Cmd), cmds.size(), f);
  std::fwrite(alpha, 1, (size_t)aw * ah, f);
  std::fclose(f);
  std::printf("%d lists, %zu commands, %zu vertices, %zu triangles, atlas %d x %d\n", dd->CmdListsCount, cmds.size(), vertices.size(),
              indices.size() / 3, aw, ah);
  ImGui::DestroyContext();
  return 0;
}
