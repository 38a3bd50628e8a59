// qa_scene_build.h — the host-only half of a scene upload: validate a flat blob (include/qa_flat_scene.h), derive every table the
// kernels read and the decisions that follow from them.  No HIP runtime call and no environment: qa_capi.hip fills the knobs and
// copies the tables to the device (UploadScene); tests/cpp/scene_build_check.cpp runs the builder under the sanitizers.
#pragma once
#include <hip/hip_runtime.h>   // uint4 / float4

#include <cstdio>
#include <string>
#include <vector>

#include "qa_scene_dev.h"
#include "qa_tilecull.h"
#include "qa_widebvh.h"

namespace qa {

constexpr size_t kMaxLdsPerBlock = 64 * 1024;      // dynamic LDS a workgroup may ask for without opt-in
constexpr size_t kResidentLdsBudget = 40 * 1024;   // image + stacks: keeps 4 workgroups per CU (160 KB LDS)

// Developer knobs (qa_capi.hip reads them once per upload; the defaults are the product's)
struct BuildKnobs {
  bool wide = true;                      // QA_WIDE=0: no 4-wide trees
  unsigned wideLeaf = 3;                 // QA_WIDE_LEAF: triangles per leaf of the 4-wide trees
  unsigned fastLeaf = 2;                 // QA_FAST_LEAF: triangles per leaf of the own SAH trees
  uint32_t fastMaxFaces = 0xFFFFFFFFu;   // QA_FAST_MAXFACES: larger meshes keep the reference tree
  uint32_t csItems = 576, csSlots = 80;  // QA_CS_ITEMS, QA_CS_SLOTS: qa_integrate_cs's pool items and ray slots per wave
  FILE *report = nullptr;                // per-mesh tree report ("verbose", QA_FAST_VERBOSE), else null
};

struct MeshTables {
  std::vector<DNode> nodes, fnodes;      // reference tree (even count), own SAH tree (qa_fastbvh.h)
  std::vector<DTri> tris, ftris, wtris;  // element order, own tree's leaf order, 4-wide tree's leaf order
  std::vector<DTriShade> shade;
  std::vector<uint32_t> fmap;
  std::vector<DNode> leaves;             // the own tree's leaves (qa_tilecull.h); empty beyond QA_TILE_LEAF_CAP
  std::vector<DNode> sweepLeaves;        // the same records, largest box first: the order in which a last-cast query takes its candidates (qa_kernel.h sweepLeaves)
  std::vector<float> vt;                 // 6 floats per element (textured scenes)
  std::vector<float> normals;            // distinct face normals, 4 floats each (resident image)
  WideBvh wide;                          // qa_widebvh.h
};

// What one upload decides; the launch paths read it from qa_ctx::plan
struct ScenePlan {
  std::vector<DMesh> meshes;             // the device mesh table, its pointer fields still null
  std::vector<bool> meshInstanced;       // some scene-graph node shows the mesh
  std::vector<int32_t> shadowLights;     // table indices of the non-ambient lights
  bool textured = false, area = false, resident = false;
  bool csFits = false;                   // the scene fits qa_integrate_cs's limits (20-bit scene-wide indices, <= 256 nodes, ...)
  bool csCullOk = false;                 // the instance-culling constants are finite (otherwise every instance is visited)
  int syncAuto = 0;                      // samples of a wave start together unless the frame decides otherwise
  size_t ldsBytes = 0;                   // dynamic LDS of qa_integrate: resident image + stacks, or stacks
  size_t tileListBytes = 0;              // + the waves' tile lists behind them (qa_tilecull.h), where they cost no workgroup per CU; else 0
  // Unlit scenes whose bounce rays need nothing of their hit but which emitter it is (PlanLastCast, qa_scene_build.cpp): the
  // resident ones run qa_integrate_lastcast (qa_kernel.h lastCastQuery).  lastCastGlow: bit k = node k is a glow node
  bool lastCastQuery = false;
  uint32_t lastCastGlow = 0;
};
// a mesh hit without texture vertices keeps the uvw of an earlier, farther hit: history only a sequential walk has
inline bool MissesTexcoords(const ScenePlan &p, const DMesh &m) { return p.textured && m.num_faces > 0 && !m.hasVT; }

// type, size and texel offset of a qa_texture as the texel table was laid out with them
struct TexLayout { int32_t type, width, height, pad; uint64_t off_texels; };

struct SceneTables {
  ScenePlan plan;
  DScene ds{};                           // camera, background, counts, LDS and culling constants; no device pointer yet
  std::vector<MeshTables> mesh;
  std::vector<DWideNode> csNodes;        // qa_integrate_cs: the 4-wide trees of all meshes (empty unless plan.csFits)
  std::vector<DTri> csTris;
  std::vector<float> csLeafBox;
  std::vector<CsInst> csInst;
  std::vector<CsCull> csCull;
  std::vector<DMaterial> materials;
  std::vector<int32_t> mtlTex;           // textured scenes: texmaps per material, float texels, their offsets, filter taps
  std::vector<float> texels;
  std::vector<uint32_t> texOff;
  std::vector<float> taps;
  std::vector<TexLayout> texLayout;      // per texture, textured or not: what no edit may change
  std::vector<uint4> image;              // the resident image (uploaded when plan.resident): the LDS part, then the meshes' leaf tables
  size_t imageLdsVec4 = 0;               // its LDS part: [nodes | tris | shade | own tree] per mesh, then the materials
  // what RebuildSceneSide needs of the mesh-side stages beside the tables above
  bool csFitsMeshes = false;             // plan.csFits as BuildMeshes and BuildCsTrees left it (the node transforms may still veto)
  uint32_t meshBuilds = 0;               // calls of the per-mesh builder this BuildScene made
};

// byte j = first | (count - 1) << 7 of leaf j of a sorted leaf table (MeshTables::sweepLeaves); false, and zeros, where a leaf does not fit
bool LeafPairBytes(const std::vector<DNode> &sorted, unsigned char bytes[QA_TILE_LEAF_CAP]);
float HaltonF(int index, int base);   // Halton sequence in the reference's fp32 order
// QA_OK, or a QA_E* code with the reason in *err
int BuildScene(const unsigned char *blob, size_t nbytes, const BuildKnobs &knobs, SceneTables &out, std::string *err);
// Scene edits (qa_scene_edit_*): `blob` is the blob `tables` was built from with its camera, light, material and instance records
// rewritten (same counts, same mesh side), and of its texture side the texmap records, the textures' colours, the texels and the
// colours of the header's background / environment.  Runs every stage again that reads them - the light plan, BuildMaterials,
// BuildCsInstances, PlanScene, and the material table at the end of the resident image - and leaves `tables` as BuildScene(blob)
// would, without a mesh build: BuildMeshes, BuildCsTrees and BuildTextures keep their results (no table is derived from a texmap
// or a texture colour; SceneTables::texels, the one table derived from the texels, is the caller's to keep up: on a context it
// lives on the device only, qa_texture_edit.hip).  A texture whose type, size or texel offset differs, or a backdrop that shows
// another texmap, is refused with QA_EINVAL.  QA_OK or a QA_E* code with the reason in *err; a refused blob leaves `tables` as
// it was.
int RebuildSceneSide(const unsigned char *blob, size_t nbytes, const BuildKnobs &knobs, SceneTables &tables, std::string *err);
// Drops the vectors RebuildSceneSide never reads (a context calls it once the tables are on the device: mesh arrays, scene-wide
// trees, texels, and the image of a scene that is not LDS-resident)
void DropMeshSide(SceneTables &tables);

}  // namespace qa
