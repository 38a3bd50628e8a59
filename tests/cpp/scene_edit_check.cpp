// Sanitizer driver for the scene-edit rebuild (qa_scene_build.cpp RebuildSceneSide, built by tests/test_scene_edit_host.py with
// -fsanitize=address,undefined, no GPU):
//   scene_edit_check <blob>...
// Per blob A: BuildScene(A), then the records an edit may touch are rewritten step by step - camera, a light (moved and dimmed; then
// made an area light; then ambient), a material (diffuse and reflection colours), a depth-1 node and a depth-2 node (translated
// and rotated), the root node - and after every step RebuildSceneSide on the kept tables must equal BuildScene of the patched blob:
// every vector, DScene and ScenePlan, byte for byte.  The same steps once more on tables that went through DropMeshSide (what a
// context keeps): the scene-side tables must still come out equal.  A blob whose counts differ is refused and changes nothing.
// One line per blob: what was patched.  Exit code 0 = every check passed.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <fstream>
#include <iterator>
#include <string>
#include <vector>

#include "qa_scene_build.h"
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
  if (a.csFitsMeshes != b.csFitsMeshes) Fail(step, "csFitsMeshes");
}

static void CompareAll(const char *step, const SceneTables &a, const SceneTables &b)
{
  CompareSceneSide(step, a, b);
  if (a.mesh.size() != b.mesh.size()) { Fail(step, "mesh count"); return; }
  for (size_t i = 0; i < a.mesh.size(); ++i) {
    const MeshTables &m = a.mesh[i], &n = b.mesh[i];
    if (!Same(m.nodes, n.nodes) || !Same(m.fnodes, n.fnodes) || !Same(m.tris, n.tris) || !Same(m.ftris, n.ftris) || !Same(m.wtris, n.wtris) ||
        !Same(m.shade, n.shade) || !Same(m.fmap, n.fmap) || !Same(m.vt, n.vt) || !Same(m.normals, n.normals) || !Same(m.wide.nodes, n.wide.nodes) ||
        !Same(m.wide.order, n.wide.order) || m.wide.rootWord != n.wide.rootWord || m.wide.depth != n.wide.depth)
      Fail(step, "MeshTables");
  }
  if (!Same(a.csNodes, b.csNodes)) Fail(step, "csNodes");
  if (!Same(a.csTris, b.csTris)) Fail(step, "csTris");
  if (!Same(a.csLeafBox, b.csLeafBox)) Fail(step, "csLeafBox");
  if (!Same(a.texels, b.texels)) Fail(step, "texels");
  if (!Same(a.image, b.image)) Fail(step, "image");
}

// tm <- R * tm with R a rotation about (1, 2, 3) / |.| by `deg`, itm <- itm * R^T, pos <- R * pos + shift (column-major 3x3)
static void MoveNode(qa_instance &in, float deg, const float shift[3])
{
  const float l = std::sqrt(14.f), x = 1 / l, y = 2 / l, z = 3 / l, a = deg * 3.14159265f / 180.f, c = std::cos(a), s = std::sin(a), t = 1 - c;
  const float R[9] = {t * x * x + c, t * x * y + s * z, t * x * z - s * y, t * x * y - s * z, t * y * y + c, t * y * z + s * x,
                      t * x * z + s * y, t * y * z - s * x, t * z * z + c};
  float tm[9], itm[9], pos[3];
  for (int col = 0; col < 3; ++col)
    for (int r = 0; r < 3; ++r) {
      tm[3 * col + r] = R[r] * in.tm[3 * col] + R[3 + r] * in.tm[3 * col + 1] + R[6 + r] * in.tm[3 * col + 2];
      itm[3 * col + r] = in.itm[r] * R[col] + in.itm[3 + r] * R[3 + col] + in.itm[6 + r] * R[6 + col];
    }
  for (int r = 0; r < 3; ++r) pos[r] = R[r] * in.pos[0] + R[3 + r] * in.pos[1] + R[6 + r] * in.pos[2] + shift[r];
  memcpy(in.tm, tm, 36); memcpy(in.itm, itm, 36); memcpy(in.pos, pos, 12);
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
  qa_light *lights = reinterpret_cast<qa_light *>(blob.data() + h->off_lights);
  qa_material *mats = reinterpret_cast<qa_material *>(blob.data() + h->off_materials);
  qa_instance *inst = reinterpret_cast<qa_instance *>(blob.data() + h->off_instances);
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
    CompareAll(name, kept, fresh);
    if (kept.meshBuilds != buildsOfUpload) Fail(name, "meshBuilds (a rebuild ran the per-mesh builder)");
    // (a dropped image: only a scene that is not resident lost it, and then no kernel reads it)
    DScene a = slim.ds, b = fresh.ds;
    if (memcmp(&a, &b, sizeof(DScene))) Fail(name, "DScene (tables without their mesh side)");
    CompareSceneSide(name, slim, fresh);
    if (fresh.plan.resident && !Same(slim.image, fresh.image)) Fail(name, "image (tables without their mesh side)");
    did += std::string(did.empty() ? "" : ", ") + name;
  };

  // camera: moved, turned, depth of field
  h->cam_pos[0] += 0.75f; h->cam_pos[2] -= 0.5f;
  for (int i = 0; i < 3; ++i) { h->screenA[i] += 0.25f * h->screenX[i]; h->screenU[i] *= 1.0625f; }
  h->dof = h->dof * 1.5f + 0.125f;
  step("camera");
  int point = -1;
  for (uint32_t i = 0; i < h->num_lights && point < 0; ++i)
    if (lights[i].type == QA_LIGHT_POINT || lights[i].type == QA_LIGHT_SPOT) point = (int) i;
  if (point < 0 && h->num_lights) point = (int) h->num_lights - 1;
  if (point >= 0) {
    qa_light &l = lights[point];
    l.position[0] += 1.5f; l.position[1] -= 0.5f;
    for (int i = 0; i < 3; ++i) l.intensity[i] *= 0.5f;
    step("light moved and dimmed");
  } else did += ", no lights";
  if (h->num_materials) {
    qa_material &m = mats[h->num_materials / 2];
    m.diffuse.color[0] = 0.125f; m.diffuse.color[1] = 0.75f; m.diffuse.color[2] = 0.25f;
    m.reflection.color[0] = m.reflection.color[0] != 0.f ? 0.f : 0.5f;   // (flips the material's lobe flag on most scenes)
    m.reflection.color[1] = m.reflection.color[2] = m.reflection.color[0];
    step("material colours");
  }
  const float shift[3] = {0.5f, -0.25f, 0.125f};
  for (int depth = 1; depth <= 2; ++depth)
    for (uint32_t k = 1; k < h->num_instances; ++k)
      if (inst[k].depth == depth && inst[k].obj_type != QA_OBJ_NONE) {
        MoveNode(inst[k], depth == 1 ? 20.f : -35.f, shift);
        step(depth == 1 ? "depth-1 node" : "depth-2 node");
        break;
      }
  // plan changes: an area light, back, an ambient light, a root node that is not the identity
  if (point >= 0) {
    const qa_light was = lights[point];
    if (lights[point].type == QA_LIGHT_POINT || lights[point].type == QA_LIGHT_SPOT) {
      lights[point].size = was.size > 0.01f ? 0.f : 0.75f;
      step("light size across 0.01");
      lights[point] = was;
      step("light size back");
    }
    lights[point].type = QA_LIGHT_AMBIENT;
    step("light made ambient");
    lights[point] = was;
  }
  inst[0].pos[1] += 0.5f;
  step("root node moved");
  inst[0].pos[1] -= 0.5f;
  step("root node back");

  // a blob of another shape is refused, and the tables stay what they were
  if (h->num_lights) {
    SceneTables before;
    std::string e;
    BuildScene(blob.data(), blob.size(), BuildKnobs{}, before, &e);
    h->num_lights -= 1;
    const int rc = RebuildSceneSide(blob.data(), blob.size(), BuildKnobs{}, kept, &e);
    h->num_lights += 1;
    if (rc != QA_EINVAL) { printf("%s: a blob with another light count gave rc %d\n", path, rc); ++fails; }
    CompareAll("refused blob", kept, before);
  }
  printf("%s: %s\n", path, did.c_str());
}

int main(int argc, char **argv)
{
  if (argc < 2) { printf("usage: scene_edit_check <blob>...\n"); return 2; }
  for (int i = 1; i < argc; ++i) Check(argv[i]);
  if (fails) printf("scene_edit_check: %d failure(s)\n", fails);
  else printf("scene_edit_check: clean\n");
  return fails ? 1 : 0;
}
