// Sanitizer driver for the texture side of the scene-edit rebuild (qa_scene_build.cpp RebuildSceneSide, qa_texel_dev.h; built by
// tests/test_texture_edit_host.py with -fsanitize=address,undefined, no GPU):
//   texture_edit_check <blob>...
// Per blob A: BuildScene(A), then what a texture edit may touch is rewritten step by step - a rectangle of a file texture's texels,
// a texmap's transform, a texmap's texture index, a checker's colours, the two backdrop colours - and after every step
// RebuildSceneSide on the kept tables must equal BuildScene of the patched blob: DScene, the plan and every vector that survives
// DropMeshSide, byte for byte, on tables as BuildScene left them and on tables that went through DropMeshSide (what a context
// keeps).  The texel table is the caller's to keep up: the kept tables' entries of the rectangle are made again with
// texelsTabulateHost and must equal the fresh build's.  Then the records an edit may not change - a texture's type, size or texel
// offset, a texmap's texture index beyond the table, the backdrop's texmap - are refused with QA_EINVAL and leave the tables as they were.
// One line per blob: what was patched.  Exit code 0 = every check passed.
#include <algorithm>
#include <cstdio>
#include <cstring>
#include <fstream>
#include <iterator>
#include <string>
#include <vector>

#include "qa_scene_build.h"
#include "qa_texel_dev.h"
#include "qaray_host.h"

using namespace qa;
typedef std::vector<unsigned char> Bytes;

static int fails = 0;
static const char *scene = "";

static void Fail(const char *step, const char *what)
{
  printf("%s: after '%s': %s differs\n", scene, step, what);
  ++fails;
}

template <class T> static bool Same(const std::vector<T> &a, const std::vector<T> &b)
{
  return a.size() == b.size() && (a.empty() || memcmp(a.data(), b.data(), a.size() * sizeof(T)) == 0);
}

// DScene, the plan and every vector DropMeshSide keeps (the image: kept by a resident scene only)
static void CompareSceneSide(const char *step, const SceneTables &a, const SceneTables &b)
{
  if (memcmp(&a.ds, &b.ds, sizeof(DScene))) Fail(step, "DScene");
  const ScenePlan &p = a.plan, &q = b.plan;
  if (!Same(p.meshes, q.meshes)) Fail(step, "ScenePlan::meshes");
  if (p.meshInstanced != q.meshInstanced) Fail(step, "ScenePlan::meshInstanced");
  if (!Same(p.shadowLights, q.shadowLights)) Fail(step, "ScenePlan::shadowLights");
  if (p.textured != q.textured || p.area != q.area || p.resident != q.resident || p.csFits != q.csFits || p.csCullOk != q.csCullOk ||
      p.syncAuto != q.syncAuto || p.ldsBytes != q.ldsBytes)
    Fail(step, "ScenePlan");
  if (!Same(a.csInst, b.csInst)) Fail(step, "csInst");
  if (!Same(a.csCull, b.csCull)) Fail(step, "csCull");
  if (!Same(a.materials, b.materials)) Fail(step, "materials");
  if (!Same(a.mtlTex, b.mtlTex)) Fail(step, "mtlTex");
  if (!Same(a.texOff, b.texOff)) Fail(step, "texOff");
  if (!Same(a.taps, b.taps)) Fail(step, "taps");
  if (!Same(a.texLayout, b.texLayout)) Fail(step, "texLayout");
  if (a.csFitsMeshes != b.csFitsMeshes) Fail(step, "csFitsMeshes");
  if (b.plan.resident && !Same(a.image, b.image)) Fail(step, "image");
}

static void Check(const char *path)
{
  scene = path;
  std::ifstream f(path, std::ios::binary);
  Bytes blob((std::istreambuf_iterator<char>(f)), std::istreambuf_iterator<char>());
  blob.shrink_to_fit();
  std::string err;
  SceneTables kept, slim;
  if (blob.size() < sizeof(qa_flat_header) || BuildScene(blob.data(), blob.size(), BuildKnobs{}, kept, &err) != QA_OK ||
      BuildScene(blob.data(), blob.size(), BuildKnobs{}, slim, &err) != QA_OK) {
    printf("%s: BuildScene failed: %s\n", path, err.c_str());
    ++fails;
    return;
  }
  const uint32_t buildsOfUpload = kept.meshBuilds;
  DropMeshSide(slim);
  qa_flat_header *h = reinterpret_cast<qa_flat_header *>(blob.data());
  qa_texmap *maps = reinterpret_cast<qa_texmap *>(blob.data() + h->off_texmaps);
  qa_texture *tex = reinterpret_cast<qa_texture *>(blob.data() + h->off_textures);
  std::string did;

  auto step = [&](const char *name) {
    SceneTables fresh;
    std::string e1, e2, e3;
    const int rcFresh = BuildScene(blob.data(), blob.size(), BuildKnobs{}, fresh, &e1);
    const int rcKept = RebuildSceneSide(blob.data(), blob.size(), BuildKnobs{}, kept, &e2);
    const int rcSlim = RebuildSceneSide(blob.data(), blob.size(), BuildKnobs{}, slim, &e3);
    if (rcFresh != QA_OK || rcKept != QA_OK || rcSlim != QA_OK) {
      printf("%s: after '%s': rc %d (%s) / %d (%s) / %d (%s)\n", path, name, rcFresh, e1.c_str(), rcKept, e2.c_str(), rcSlim, e3.c_str());
      ++fails;
      return;
    }
    CompareSceneSide(name, kept, fresh);
    if (!Same(kept.texels, fresh.texels)) Fail(name, "texels");
    if (kept.meshBuilds != buildsOfUpload) Fail(name, "meshBuilds (a rebuild ran the per-mesh builder)");
    CompareSceneSide(name, slim, fresh);
    did += std::string(did.empty() ? "" : ", ") + name;
  };

  int file = -1, other = -1, checker = -1;
  for (uint32_t i = 0; i < h->num_textures; ++i) {
    if (tex[i].type == QA_TEX_FILE && tex[i].width > 0 && tex[i].height > 0 &&
        (file < 0 || (int64_t) tex[i].width * tex[i].height > (int64_t) tex[file].width * tex[file].height))
      file = (int) i;
    if (tex[i].type == QA_TEX_CHECKER && checker < 0) checker = (int) i;
  }
  for (uint32_t i = 0; i < h->num_textures; ++i)
    if ((int) i != file && other < 0) other = (int) i;
  if (file >= 0 && h->num_texmaps > 0) {
    // a rectangle that starts at an odd column and is not a multiple of 4 wide where the texture allows it
    const qa_texture &t = tex[file];
    const int x0 = t.width > 2 ? 1 : 0, x1 = std::max(x0 + 1, t.width - (t.width > 4 ? 2 : 0)), y0 = t.height / 3, y1 = std::max(y0 + 1, t.height - t.height / 4);
    const size_t w = (size_t) (x1 - x0), rows = (size_t) (y1 - y0), stride = 3 * w + 5;
    Bytes src(stride * rows);
    for (size_t i = 0; i < src.size(); ++i) src[i] = (unsigned char) (i * 37 + 11);
    for (size_t r = 0; r < rows; ++r) {
      memcpy(blob.data() + t.off_texels + 3 * ((y0 + r) * (size_t) t.width + x0), src.data() + r * stride, 3 * w);
      // the texel table of tables that still have one: the rectangle's entries from the source an upload uses
      texelsTabulateHost(src.data() + r * stride, w, 1, stride, kept.texels.data() + 4 * ((size_t) kept.texOff[file] + (y0 + r) * (size_t) t.width + x0));
    }
    step("texel rectangle");
  } else did += "no file texture";
  int moved = -1;
  for (uint32_t k = 0; k < h->num_texmaps && moved < 0; ++k)
    if (maps[k].texture >= 0) moved = (int) k;
  if (moved >= 0) {
    for (int i = 0; i < 9; ++i) maps[moved].itm[i] *= 1.25f;
    maps[moved].pos[0] += 0.375f; maps[moved].pos[1] -= 0.125f;
    step("texmap transform");
    if (other >= 0) {
      const int k = (int) h->num_texmaps - 1;
      maps[k].texture = maps[k].texture == other ? file : other;
      step("texmap rebound");
      maps[k].texture = -1;
      step("texmap without texture");
    }
  }
  if (checker >= 0) {
    tex[checker].color1[0] = 0.875f; tex[checker].color1[1] = 0.125f; tex[checker].color2[2] = 0.5f;
    step("checker colours");
  }
  h->background.color[0] = 0.25f; h->background.color[2] *= 0.5f;
  h->environment.color[1] = 0.75f; h->environment.color[0] += 0.125f;
  step("backdrop colours");

  // what an edit may not change: refused, and the tables stay what they were
  SceneTables before;
  BuildScene(blob.data(), blob.size(), BuildKnobs{}, before, &err);
  auto refused = [&](const char *name) {
    std::string e;
    const int rcKept = RebuildSceneSide(blob.data(), blob.size(), BuildKnobs{}, kept, &e);
    const int rcSlim = RebuildSceneSide(blob.data(), blob.size(), BuildKnobs{}, slim, &e);
    if (rcKept != QA_EINVAL || rcSlim != QA_EINVAL) { printf("%s: '%s' gave rc %d / %d\n", path, name, rcKept, rcSlim); ++fails; }
    CompareSceneSide(name, kept, before);
    if (!Same(kept.texels, before.texels)) Fail(name, "texels");
    CompareSceneSide(name, slim, before);
    did += std::string(", refused: ") + name;
  };
  if (file >= 0) {
    const qa_texture was = tex[file];
    tex[file].type = QA_TEX_CHECKER; refused("texture type"); tex[file] = was;
    tex[file].width = was.width > 1 ? was.width - 1 : 2; refused("texture width"); tex[file] = was;
    std::swap(tex[file].width, tex[file].height);
    if (was.width != was.height) refused("texture size swapped");
    tex[file] = was;
    tex[file].off_texels = was.off_texels >= 3 ? was.off_texels - 3 : was.off_texels + 3; refused("texel offset"); tex[file] = was;
  }
  if (h->num_texmaps) {
    const qa_texmap was = maps[0];
    maps[0].texture = (int32_t) h->num_textures; refused("texture index = count"); maps[0] = was;
    maps[0].texture = -2; refused("texture index -2"); maps[0] = was;
    const int32_t bg = h->background.texmap, env = h->environment.texmap;
    h->background.texmap = bg < 0 ? 0 : -1; refused("background texmap"); h->background.texmap = bg;
    h->environment.texmap = env < 0 ? 0 : -1; refused("environment texmap"); h->environment.texmap = env;
  }
  step("after the refusals");
  printf("%s: %s\n", path, did.c_str());
}

int main(int argc, char **argv)
{
  if (argc < 2) { printf("usage: texture_edit_check <blob>...\n"); return 2; }
  for (int i = 1; i < argc; ++i) Check(argv[i]);
  if (fails) printf("texture_edit_check: %d failure(s)\n", fails);
  else printf("texture_edit_check: clean\n");
  return fails ? 1 : 0;
}
