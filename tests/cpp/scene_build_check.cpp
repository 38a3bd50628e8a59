// Sanitizer driver for the scene builder (qa_scene_build.cpp, built by tests/test_sanitizers.py with
// -fsanitize=address,undefined, no GPU):
//   scene_build_check plan <blob>...      one line per blob: the build's return code and the plan it made
//   scene_build_check malformed <blob>    mutations of a valid blob, each with the QA_E* code it must give
// Exit code 0 = every check passed.
#include <cstdio>
#include <cstring>
#include <fstream>
#include <functional>
#include <iterator>
#include <string>
#include <vector>

#include "qa_scene_build.h"
#include "qaray_host.h"

using namespace qa;
typedef std::vector<unsigned char> Bytes;

static int fails = 0;

static Bytes Read(const char *path)
{
  std::ifstream f(path, std::ios::binary);
  return Bytes(std::istreambuf_iterator<char>(f), std::istreambuf_iterator<char>());
}

static int Build(const Bytes &b, SceneTables &t, std::string *err)
{
  // a copy of exactly the blob's size: the sanitizer sees every read past its end
  std::vector<unsigned char> exact(b);
  exact.shrink_to_fit();
  return BuildScene(exact.data(), exact.size(), BuildKnobs{}, t, err);
}

static void Plan(const char *path)
{
  SceneTables t;
  std::string err;
  const int rc = Build(Read(path), t, &err);
  const ScenePlan &p = t.plan;
  printf("%s rc=%d resident=%d csFits=%d csCullOk=%d stackNeedMax=%u ldsBytes=%zu useFast=", path, rc, (int) p.resident, (int) p.csFits,
         (int) p.csCullOk, t.ds.stackNeed, p.ldsBytes);
  for (const DMesh &m : p.meshes) printf("%u", m.useFast);
  printf(" useWide=");
  for (const DMesh &m : p.meshes) printf("%u", m.useWide);
  printf("%s%s\n", rc ? " err=" : "", rc ? err.c_str() : "");
}

// the tables of a blob, writable (the flattener's 8-byte alignment keeps every record aligned)
struct View {
  Bytes b;
  qa_flat_header *h() { return reinterpret_cast<qa_flat_header *>(b.data()); }
  template <class T> T *at(uint64_t off) { return reinterpret_cast<T *>(b.data() + off); }
  qa_mesh &mesh(uint32_t i) { return at<qa_mesh>(h()->off_meshes)[i]; }
  qa_instance &inst(uint32_t i) { return at<qa_instance>(h()->off_instances)[i]; }
};

static void Expect(const char *what, const Bytes &valid, int code, const std::function<void(View &)> &mutate)
{
  View v{valid};
  mutate(v);
  SceneTables t;
  std::string err;
  const int rc = Build(v.b, t, &err);
  printf("%-44s rc=%d %s\n", what, rc, err.c_str());
  if (rc != code) { printf("  expected rc=%d\n", code); ++fails; }
}

static void Malformed(const char *path)
{
  const Bytes valid = Read(path);
  View v{valid};
  const qa_flat_header *h = v.h();
  // a mesh with texture vertices on every face, a tree of more than one leaf and an instance that shows it
  uint32_t mi = h->num_meshes, ii = 0;
  for (uint32_t k = 0; k < h->num_instances && mi == h->num_meshes; ++k) {
    const qa_instance &in = v.inst(k);
    if (in.obj_type != QA_OBJ_MESH) continue;
    const qa_mesh &m = v.mesh(in.mesh);
    const qa_face *f = v.at<qa_face>(m.off_faces);
    if (m.num_bvh_nodes > 3 && m.num_faces > 1 && f[0].vt[0] >= 0) { mi = (uint32_t) in.mesh; ii = k; }
  }
  if (mi == h->num_meshes || h->num_texmaps == 0) { printf("%s: no textured mesh with texture vertices\n", path); ++fails; return; }
  const qa_mesh m = v.mesh(mi);
  Expect("valid", valid, QA_OK, [](View &) {});
  Expect("truncated", valid, QA_EINVAL, [](View &x) { x.b.resize(x.b.size() / 2); });
  Expect("shorter than the header", valid, QA_EINVAL, [](View &x) { x.b.resize(sizeof(qa_flat_header) - 1); });
  Expect("wrong magic", valid, QA_EINVAL, [](View &x) { x.h()->magic ^= 1u; });
  Expect("table offset past the end", valid, QA_EINVAL, [](View &x) { x.h()->off_meshes = x.b.size(); });
  // (the instance, material-set, light and texmap tables are read before the alignment check: misalign another one)
  Expect("misaligned table offset", valid, QA_EINVAL, [](View &x) { x.h()->off_materials += 4; });
  Expect("misaligned mesh array", valid, QA_EINVAL, [&](View &x) { x.mesh(mi).off_faces += 2; });
  Expect("bad mesh index", valid, QA_EINVAL, [&](View &x) { x.inst(ii).mesh = (int32_t) x.h()->num_meshes; });
  Expect("bad material index", valid, QA_EINVAL, [&](View &x) { x.inst(ii).mtlset = (int32_t) x.h()->num_mtlsets; });
  Expect("bad texture index", valid, QA_EINVAL, [](View &x) { x.at<qa_texmap>(x.h()->off_texmaps)[0].texture = (int32_t) x.h()->num_textures; });
  Expect("BVH child out of range", valid, QA_EINVAL, [&](View &x) {
    qa_bvh_node *n = x.at<qa_bvh_node>(m.off_bvh_nodes);
    n[1].data = m.num_bvh_nodes & ~1u;   // inner node whose second child is past the end
  });
  Expect("BVH element out of range", valid, QA_EINVAL, [&](View &x) { x.at<uint32_t>(m.off_elements)[0] = m.num_faces; });
  Expect("face vertex out of range", valid, QA_EINVAL, [&](View &x) { x.at<qa_face>(m.off_faces)[0].v[1] = (int32_t) m.num_vertices; });
  Expect("texcoord index out of range", valid, QA_EINVAL, [&](View &x) { x.at<qa_face>(m.off_faces)[0].vt[2] = (int32_t) m.num_texcoords; });
  Expect("texture vertices on only some faces", valid, QA_EUNSUPPORTED, [&](View &x) {
    qa_face &f = x.at<qa_face>(m.off_faces)[0];
    f.vt[0] = f.vt[1] = f.vt[2] = -1;
  });
  // its tree words (leaves among them) are never followed: the mesh is simply empty
  Expect("mesh without faces, with leaf words", valid, QA_OK, [&](View &x) { x.mesh(mi).num_faces = 0; });
}

int main(int argc, char **argv)
{
  if (argc >= 3 && !strcmp(argv[1], "plan"))
    for (int i = 2; i < argc; ++i) Plan(argv[i]);
  else if (argc == 3 && !strcmp(argv[1], "malformed"))
    Malformed(argv[2]);
  else {
    printf("usage: scene_build_check plan <blob>... | malformed <blob>\n");
    return 2;
  }
  if (fails) printf("scene_build_check: %d failure(s)\n", fails);
  return fails ? 1 : 0;
}
