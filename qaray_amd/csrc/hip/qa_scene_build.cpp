// qa_scene_build.cpp — BuildScene (qa_scene_build.h): blob -> validated host tables and the scene's plan.
#include "qa_scene_build.h"

#include <algorithm>
#include <cmath>
#include <cstring>
#include <new>

#include "qa_device_math.h"
#include "qa_fastbvh.h"
#include "qa_texel_dev.h"
#include "qa_tilecull.h"
#include "qaray_host.h"

namespace qa {
namespace {

struct Refused { int code; const char *msg; };
[[noreturn]] void Refuse(int code, const char *msg) { throw Refused{code, msg}; }

struct Blob {
  const unsigned char *p;
  size_t n;
  const qa_flat_header *h;
  bool inside(uint64_t off, uint64_t bytes) const { return off <= n && bytes <= n - off; }
  template <class T> const T *at(uint64_t off) const { return QA_BLOB_PTR(T, p, off); }
};

void CheckHeader(const Blob &b)
{
  if (b.n < sizeof(qa_flat_header)) Refuse(QA_EINVAL, "blob smaller than its header");
  const qa_flat_header *h = b.h;
  if (h->magic != QA_FLAT_MAGIC || h->version != QA_FLAT_VERSION) Refuse(QA_EINVAL, "not a qaray flat scene (magic/version)");
  if (h->total_bytes != b.n) Refuse(QA_EINVAL, "blob size does not match its header");
  if (!b.inside(h->off_instances, (uint64_t) h->num_instances * sizeof(qa_instance)) ||
      !b.inside(h->off_meshes, (uint64_t) h->num_meshes * sizeof(qa_mesh)) ||
      !b.inside(h->off_mtlsets, (uint64_t) h->num_mtlsets * sizeof(qa_mtlset)) ||
      !b.inside(h->off_materials, (uint64_t) h->num_materials * sizeof(qa_material)) ||
      !b.inside(h->off_lights, (uint64_t) h->num_lights * sizeof(qa_light)) ||
      !b.inside(h->off_texmaps, (uint64_t) h->num_texmaps * sizeof(qa_texmap)) ||
      !b.inside(h->off_textures, (uint64_t) h->num_textures * sizeof(qa_texture)))
    Refuse(QA_EINVAL, "table outside the blob");
  if (h->num_instances == 0 || h->width == 0 || h->height == 0) Refuse(QA_EINVAL, "empty scene");
  const qa_instance *inst = b.at<qa_instance>(h->off_instances);
  const qa_mtlset *mtlset = b.at<qa_mtlset>(h->off_mtlsets);
  for (uint32_t k = 0; k < h->num_instances; ++k) {
    const qa_instance &in = inst[k];
    if (in.depth > QA_MAX_NODE_DEPTH) Refuse(QA_EUNSUPPORTED, "node nesting deeper than QA_MAX_NODE_DEPTH");
    if (in.parent >= (int) k || (k > 0 && in.parent < 0)) Refuse(QA_EINVAL, "instances are not in pre-order");
    if (in.obj_type == QA_OBJ_MESH && (in.mesh < 0 || in.mesh >= (int) h->num_meshes)) Refuse(QA_EINVAL, "bad mesh index");
    if (in.mtlset >= (int) h->num_mtlsets) Refuse(QA_EINVAL, "bad material index");
  }
  for (uint32_t i = 0; i < h->num_mtlsets; ++i)
    if (mtlset[i].first < 0 || mtlset[i].count < 0 || (uint32_t) (mtlset[i].first + mtlset[i].count) > h->num_materials)
      Refuse(QA_EINVAL, "bad material range");
  const qa_texmap *texmaps = b.at<qa_texmap>(h->off_texmaps);
  const qa_texture *textures = b.at<qa_texture>(h->off_textures);
  for (uint32_t i = 0; i < h->num_texmaps; ++i)
    if (texmaps[i].texture < -1 || texmaps[i].texture >= (int) h->num_textures) Refuse(QA_EINVAL, "bad texture index");
  if (h->background.texmap < -1 || h->background.texmap >= (int) h->num_texmaps || h->environment.texmap < -1 ||
      h->environment.texmap >= (int) h->num_texmaps)
    Refuse(QA_EINVAL, "bad background / environment texmap index");
  // the tables are read in place (4- and 8-byte fields): offsets must be 8-byte aligned
  for (uint64_t off : {h->off_instances, h->off_meshes, h->off_mtlsets, h->off_materials, h->off_lights, h->off_texmaps, h->off_textures})
    if (off % 8) Refuse(QA_EINVAL, "table offset is not 8-byte aligned");
  for (uint32_t i = 0; i < h->num_textures; ++i)
    if (textures[i].type == QA_TEX_FILE &&
        (textures[i].width < 0 || textures[i].height < 0 ||
         !b.inside(textures[i].off_texels, (uint64_t) textures[i].width * (uint64_t) textures[i].height * 3)))
      Refuse(QA_EINVAL, "texel array outside the blob");
}

// Per mesh: everything derived from its own arrays
struct MeshBuild {
  const Blob &b;
  const qa_mesh &m;
  const BuildKnobs &k;
  MeshTables &t;
  DMesh &dm;
  const qa_bvh_node *nodes;
  const uint32_t *elements;
  const qa_face *faces;
  const float *V;

  // every inner box of the reference tree contains its children's (cy::BVH's inner boxes are unions): the own trees' order
  // checks test a leaf's box only.  (The words of a mesh without faces are not validated: a child out of range fails.)
  bool Nested() const
  {
    for (uint32_t i = 1; i < m.num_bvh_nodes; ++i) {
      if (nodes[i].data & QA_BVH_LEAF_BIT) continue;
      const uint32_t ch = nodes[i].data & QA_BVH_CHILD_MASK;
      if (ch + 1 >= m.num_bvh_nodes) return false;
      for (uint32_t q = ch; q < ch + 2; ++q)
        for (int a = 0; a < 3; ++a)
          if (!(nodes[q].box[a] >= nodes[i].box[a] && nodes[q].box[a + 3] <= nodes[i].box[a + 3])) return false;
    }
    return true;
  }

  // the reference tree, validated, and the deepest stack its walk can need = its depth (one pending sibling per level);
  // children always have larger indices than their parent, so a forward sweep computes node depths.  The words of a mesh
  // without faces are copied, never followed.
  uint32_t RefTree()
  {
    t.nodes.assign(m.num_bvh_nodes + (m.num_bvh_nodes & 1), DNode{});  // even count: sibling pairs are 64-byte units
    for (uint32_t i = 0; i < m.num_bvh_nodes; ++i) {
      memcpy(t.nodes[i].box, nodes[i].box, sizeof(t.nodes[i].box));
      t.nodes[i].data = nodes[i].data;
      if (i >= 1 && m.num_faces > 0) {
        if (!(nodes[i].data & QA_BVH_LEAF_BIT)) {
          const uint32_t ch = nodes[i].data & QA_BVH_CHILD_MASK;
          if (ch + 1 >= m.num_bvh_nodes || ch <= i || (ch & 1)) Refuse(QA_EINVAL, "BVH child index out of range");
        } else {
          const uint32_t cnt = ((nodes[i].data >> QA_BVH_COUNT_SHIFT) & QA_BVH_COUNT_MASK) + 1;
          if ((nodes[i].data & QA_BVH_OFFSET_MASK) + cnt > m.num_faces) Refuse(QA_EINVAL, "BVH leaf range out of range");
          if (nodes[i].data == QA_DONE) Refuse(QA_EUNSUPPORTED, "leaf word collides with the traversal sentinel");
        }
      }
    }
    uint32_t stackNeed = 1;
    if (m.num_faces > 0 && m.num_bvh_nodes > 1) {
      std::vector<uint32_t> level(m.num_bvh_nodes, 0);
      level[1] = 1;
      for (uint32_t i = 1; i < m.num_bvh_nodes; ++i) {
        if (level[i] == 0 || (nodes[i].data & QA_BVH_LEAF_BIT)) continue;
        const uint32_t ch = nodes[i].data & QA_BVH_CHILD_MASK;
        level[ch] = level[ch + 1] = level[i] + 1;
        stackNeed = std::max(stackNeed, level[i] + 1);
      }
    }
    return stackNeed;
  }

  // intersection and shading records in element order; DTriShade::pad = the reference-tree leaf of the element (refReaches)
  void Triangles()
  {
    const float *VN = b.at<float>(m.off_normals);
    t.tris.resize(m.num_faces);
    t.shade.resize(m.num_faces);
    for (uint32_t e = 0; e < m.num_faces; ++e) {
      const uint32_t fid = elements[e];
      if (fid >= m.num_faces) Refuse(QA_EINVAL, "BVH element out of range");
      const qa_face &f = faces[fid];
      for (int q = 0; q < 3; ++q) {
        if (f.v[q] < 0 || (uint32_t) f.v[q] >= m.num_vertices) Refuse(QA_EINVAL, "vertex index out of range");
        if (f.vn[q] < 0 || (uint32_t) f.vn[q] >= m.num_normals) Refuse(QA_EINVAL, "normal index out of range");
      }
      const f3 A = ld3(V + 3 * f.v[0]), B = ld3(V + 3 * f.v[1]), C = ld3(V + 3 * f.v[2]);
      // src/objects/objects.cpp:220-246
      const f3 N = normalize(cross(B - A, C - A));
      uint32_t axis;
      const float ax = qabs(N.x), ay = qabs(N.y), az = qabs(N.z);
      if (ax > ay && ax > az) axis = 0;
      else if (ay > az) axis = 1;
      else axis = 2;
      auto U = [&](f3 p) { return axis == 0 ? p.y : p.x; };
      auto W = [&](f3 p) { return axis == 2 ? p.y : p.z; };
      DTri &r = t.tris[e];
      r.N[0] = N.x; r.N[1] = N.y; r.N[2] = N.z;
      r.A[0] = A.x; r.A[1] = A.y; r.A[2] = A.z;
      r.bu = U(B); r.bv = W(B); r.cu = U(C); r.cv = W(C);
      // TriangleArea(axis, A, B, C) (objects.cpp:30-41)
      const float area = (r.bu - U(A)) * (r.cv - W(A)) - (r.cu - U(A)) * (r.bv - W(A));
      r.s = 1.f / area;
      r.axis = axis;
      DTriShade &s = t.shade[e];
      memcpy(s.n0, VN + 3 * f.vn[0], 12);
      memcpy(s.n1, VN + 3 * f.vn[1], 12);
      memcpy(s.n2, VN + 3 * f.vn[2], 12);
      s.mtl = f.mtl;
      s.face = fid;
      s.pad = 0;
    }
    for (uint32_t i = 1; i < m.num_bvh_nodes && m.num_faces > 0; ++i)
      if (nodes[i].data & QA_BVH_LEAF_BIT) {
        const uint32_t cnt = ((nodes[i].data >> QA_BVH_COUNT_SHIFT) & QA_BVH_COUNT_MASK) + 1, off = nodes[i].data & QA_BVH_OFFSET_MASK;
        for (uint32_t q = 0; q < cnt; ++q) t.shade[off + q].pad = i;
      }
  }

  // smallest altitude over all triangles: 2 * area / longest edge (degenerate triangles never pass the reference's test - their
  // normal is NaN - and are left out)
  double MinAltitude() const
  {
    double hMin = 1e300;
    for (uint32_t e = 0; e < m.num_faces; ++e) {
      const qa_face &f = faces[elements[e]];
      const float *A = V + 3 * (size_t) f.v[0], *B = V + 3 * (size_t) f.v[1], *C = V + 3 * (size_t) f.v[2];
      const double ab[3] = {(double) B[0] - A[0], (double) B[1] - A[1], (double) B[2] - A[2]};
      const double ac[3] = {(double) C[0] - A[0], (double) C[1] - A[1], (double) C[2] - A[2]};
      const double bc[3] = {(double) C[0] - B[0], (double) C[1] - B[1], (double) C[2] - B[2]};
      const double cr[3] = {ab[1] * ac[2] - ab[2] * ac[1], ab[2] * ac[0] - ab[0] * ac[2], ab[0] * ac[1] - ab[1] * ac[0]};
      const double area2 = std::sqrt(cr[0] * cr[0] + cr[1] * cr[1] + cr[2] * cr[2]);
      const double L = std::sqrt(std::max({ab[0] * ab[0] + ab[1] * ab[1] + ab[2] * ab[2], ac[0] * ac[0] + ac[1] * ac[1] + ac[2] * ac[2],
                                           bc[0] * bc[0] + bc[1] * bc[1] + bc[2] * bc[2]}));
      if (area2 > 0 && L > 0) hMin = std::min(hMin, area2 / L);
    }
    return hMin;
  }

  // distinct face normals up to sign, merged within 1e-5 (the DTri records hold the reference's own normalize(cross()))
  void Normals()
  {
    std::vector<float> &nl = t.normals;
    for (uint32_t e = 0; e < m.num_faces; ++e) {
      const float *N = t.tris[e].N;
      if (!(N[0] == N[0])) continue;   // degenerate triangle: NaN normal, never accepted
      bool seen = false;
      for (size_t q = 0; q + 3 < nl.size() + 1 && !seen; q += 4) {
        // same direction up to sign within 1e-5 (the kernel's parallelism threshold allows for it)
        const float dp = std::fabs(nl[q] * N[0] + nl[q + 1] * N[1] + nl[q + 2] * N[2]);
        const float cx = nl[q + 1] * N[2] - nl[q + 2] * N[1], cy = nl[q + 2] * N[0] - nl[q] * N[2], cz = nl[q] * N[1] - nl[q + 1] * N[0];
        seen = dp > 0.5f && std::sqrt(cx * cx + cy * cy + cz * cz) < 1e-5f;
      }
      if (seen) continue;
      if (nl.size() >= 4 * 24) { nl.clear(); return; }   // too many: no list
      nl.insert(nl.end(), {N[0], N[1], N[2], 0.f});
    }
  }

  // global-memory scene: the 4-wide tree over the reference leaves, and the inside test's fp32 slack
  MeshSlack WideTree()
  {
    std::vector<float> ev(9 * (size_t) m.num_faces), tb(6 * (size_t) m.num_faces);
    std::vector<unsigned char> skip(m.num_faces, 0);
    for (uint32_t e = 0; e < m.num_faces; ++e) {
      const qa_face &f = faces[elements[e]];
      for (int v = 0; v < 3; ++v) memcpy(&ev[9 * (size_t) e + 3 * v], V + 3 * (size_t) f.v[v], 12);
      const float *p = &ev[9 * (size_t) e];
      for (int a = 0; a < 3; ++a) {
        tb[6 * (size_t) e + a] = std::min(p[a], std::min(p[3 + a], p[6 + a]));
        tb[6 * (size_t) e + 3 + a] = std::max(p[a], std::max(p[3 + a], p[6 + a]));
      }
      skip[e] = !(t.tris[e].N[0] == t.tris[e].N[0]);   // degenerate: NaN normal, the inside test never accepts it
    }
    // triangles per leaf: 3 (same-box A/B of 1 / 2 / 3 / 4 / 6 / 8: C3 288 / 363 / 373 / 382 / 389 / 371, C5 391 / 612 / 614 / 594 /
    // 565 / 539 Msamples/s on the megakernel; the staged integrator is flat between 2 and 4)
    WideBvhBuilder(tb.data(), skip.data(), m.num_faces, k.wideLeaf).Run(t.wide);
    // the triangle records once more in the wide tree's leaf order; the element id rides above the 2-bit axis
    t.wtris.resize(t.wide.order.size());
    for (size_t i = 0; i < t.wide.order.size(); ++i) {
      t.wtris[i] = t.tris[t.wide.order[i]];
      t.wtris[i].axis |= t.wide.order[i] << 2;
    }
    return ComputeMeshSlack(t.tris.data(), m.num_faces, ev.data());
  }

  // LDS-resident candidates: the own SAH tree over the element bounds; returns its depth
  uint32_t FastTree(uint32_t mi, double hMin)
  {
    std::vector<float> bounds(6 * (size_t) m.num_faces);
    for (uint32_t e = 0; e < m.num_faces; ++e) {
      const qa_face &f = faces[elements[e]];
      float *bb = &bounds[6 * (size_t) e];
      for (int a = 0; a < 3; ++a) { bb[a] = 1e30f; bb[3 + a] = -1e30f; }
      for (int v = 0; v < 3; ++v)
        for (int a = 0; a < 3; ++a) {
          const float x = V[3 * (size_t) f.v[v] + a];
          if (x < bb[a]) bb[a] = x;
          if (x > bb[3 + a]) bb[3 + a] = x;
        }
    }
    FastBvh fb;
    FastBvhBuilder(bounds.data(), m.num_faces, k.fastLeaf).Run(fb);
    if (fb.nodes.size() & 1) fb.nodes.push_back(DNode{});
    if (k.report) {
      float rootBox[6];
      memcpy(rootBox, m.bmin, 12);
      memcpy(rootBox + 3, m.bmax, 12);
      const double costRef = (m.num_faces > 0 && m.num_bvh_nodes > 1) ? TreeCost(t.nodes.data(), nodes[1].data, rootBox) : 0;
      const double costFast = TreeCost(fb.nodes.data(), fb.rootData, rootBox);
      fprintf(k.report, "mesh %u: %u triangles, expected ray cost reference tree %.2f, own tree %.2f (depth %u), smallest altitude %g, |coord| <= %g, %zu distinct normals\n",
              mi, m.num_faces, costRef, costFast, fb.depth, hMin, (double) dm.absMax, t.normals.size() / 4);
    }
    t.fnodes = fb.nodes;
    t.fmap = fb.order;
    t.ftris.resize(m.num_faces);
    // DTri::axis of the own tree's copies = axis | element << 2 | reference-tree leaf << 17: the walk hands back the
    // element and its leaf (refReaches) with the accepted record itself instead of through two more dependent reads
    // (fmap, DTriShade::pad) after it.  Meshes beyond 15 bits of either keep the reference tree (useFast below).
    for (uint32_t i = 0; i < m.num_faces; ++i) {
      const uint32_t e = fb.order[i];
      t.ftris[i] = t.tris[e];
      t.ftris[i].axis = (t.tris[e].axis & 3u) | ((e & 0x7FFFu) << 2) | ((t.shade[e].pad & 0x7FFFu) << 17);
    }
    // the leaves alone, for the per-tile lists of camera rays (qa_tilecull.h); a tree of more leaves than one ballot covers has none
    // (every slot from 1 on is the root or a child; slot 0 and a padding slot carry no leaf bit)
    for (size_t i = 1; i < fb.nodes.size() && m.num_faces > 0; ++i)
      if (fb.nodes[i].data & QA_BVH_LEAF_BIT) t.leaves.push_back(fb.nodes[i]);
    if (t.leaves.size() > QA_TILE_LEAF_CAP || m.num_faces > QA_TILE_ENTRY_FACES) t.leaves.clear();
    // ... and once more by descending half-area of the box (the table's order among equals), for the any-hit queries of bounce rays
    // that sweep the table (qa_kernel.h sweepLeaves): such a query wants the likeliest blocker first, and large walls block most rays
    // (profiles/leaf_sweep_cost.txt).  A table of its own: the list builder's order, and with it the tile lists, stay what they are
    t.sweepLeaves = t.leaves;
    auto halfArea = [](const DNode &n) {
      const float dx = n.box[3] - n.box[0], dy = n.box[4] - n.box[1], dz = n.box[5] - n.box[2];
      return (dx * dy + dy * dz) + dz * dx;
    };
    std::stable_sort(t.sweepLeaves.begin(), t.sweepLeaves.end(), [&](const DNode &a, const DNode &b) { return halfArea(a) > halfArea(b); });
    return fb.depth;
  }

  // texture vertices per triangle (element order); a mesh must have them on every face or none
  void Texcoords(bool textured)
  {
    const float *VT = b.at<float>(m.off_texcoords);
    uint32_t withVT = 0;
    for (uint32_t e = 0; e < m.num_faces; ++e) {
      const qa_face &f = faces[elements[e]];
      if (f.vt[0] >= 0 && f.vt[1] >= 0 && f.vt[2] >= 0) {
        for (int q = 0; q < 3; ++q) if ((uint32_t) f.vt[q] >= m.num_texcoords) Refuse(QA_EINVAL, "texcoord index out of range");
        ++withVT;
      }
    }
    if (withVT != 0 && withVT != m.num_faces) Refuse(QA_EUNSUPPORTED, "mesh with texture vertices on only some faces");
    dm.hasVT = (withVT && textured) ? 1 : 0;
    if (!dm.hasVT) return;
    t.vt.resize(6 * (size_t) m.num_faces);
    for (uint32_t e = 0; e < m.num_faces; ++e) {
      const qa_face &f = faces[elements[e]];
      for (int q = 0; q < 3; ++q) { t.vt[6 * e + 2 * q] = VT[2 * f.vt[q]]; t.vt[6 * e + 2 * q + 1] = VT[2 * f.vt[q] + 1]; }
    }
  }

  // fills the mesh's tables and its DMesh record; returns the depth of its reference tree alone
  uint32_t Run(uint32_t mi, uint64_t totalFaces, bool textured)
  {
    uint32_t stackNeed = RefTree();
    const uint32_t stackNeedRef = stackNeed;   // depth of the reference tree alone
    Triangles();
    const double hMin = MinAltitude();
    dm.invH = hMin < 1e300 ? (float) (1.0 / hMin) : 0.f;
    for (int a = 0; a < 3; ++a) dm.absMax = std::max(dm.absMax, std::max(std::fabs(m.bmin[a]), std::fabs(m.bmax[a])));
    Normals();
    MeshSlack slack{0.f, 0.f};
    // only LDS-resident scenes search their own trees, and residency needs the whole image within 40 KB (~140 B per
    // triangle before the own tree): skip the build where that is out of reach
    if (totalFaces > 512) {
      t.fnodes.assign(2, DNode{});
      if (m.num_faces > 0 && m.num_bvh_nodes > 1 && k.wide) {
        slack = WideTree();
        stackNeed = std::max(stackNeed, 3 * t.wide.depth + 2);
        if (k.report)
          fprintf(k.report, "mesh %u: %u triangles, reference tree %u nodes depth %u; wide tree %zu nodes depth %u; inside-test slack %g, cancel distance %g, |coord| <= %g\n",
                  mi, m.num_faces, m.num_bvh_nodes, stackNeed, t.wide.nodes.size(), t.wide.depth, (double) slack.nearPad,
                  (double) slack.cancelDist, (double) dm.absMax);
      }
    } else stackNeed = std::max(stackNeed, FastTree(mi, hMin));
    Texcoords(textured);
    memcpy(dm.bmin, m.bmin, 12);
    memcpy(dm.bmax, m.bmax, 12);
    dm.num_faces = m.num_faces;
    dm.num_nodes = m.num_bvh_nodes;
    dm.rootData = m.num_bvh_nodes > 1 ? nodes[1].data : QA_DONE;
    dm.frootData = (m.num_faces && t.fnodes.size() > 1) ? t.fnodes[1].data : QA_DONE;
    // needle-like triangles would widen the own trees' boxes (200 eps P^2 / h, see hitMesh; the slack) to a sizeable part of
    // the mesh: such a mesh keeps the reference tree
    const double P = 2.0 * dm.absMax + 1e-30, diag = std::sqrt((double) (m.bmax[0] - m.bmin[0]) * (m.bmax[0] - m.bmin[0]) +
                                                               (double) (m.bmax[1] - m.bmin[1]) * (m.bmax[1] - m.bmin[1]) +
                                                               (double) (m.bmax[2] - m.bmin[2]) * (m.bmax[2] - m.bmin[2]));
    const bool nested = Nested();
    dm.useFast = (totalFaces <= 512 && m.num_bvh_nodes < 0x8000u && m.num_faces <= k.fastMaxFaces &&
                  1.2e-5 * dm.invH * P * P < 0.01 * diag && nested) ? 1u : 0u;
    dm.useWide = (t.wide.rootWord != QA_DONE && slack.nearPad < 0.01 * diag && nested) ? 1u : 0u;
    dm.stackNeed = stackNeed;
    dm.wrootWord = t.wide.rootWord;
    dm.wideStack = 3 * t.wide.depth + 2;
    dm.wnodeCount = (uint32_t) t.wide.nodes.size();
    // QA_SLACK_SCALE is 1 except in the test-only library lib_noslack (qa_scene_dev.h)
    dm.nearPad = slack.nearPad * QA_SLACK_SCALE;
    dm.cancelDist = QA_SLACK_SCALE == 1.0f ? slack.cancelDist : QA_SLACK_SCALE > 0 ? slack.cancelDist / QA_SLACK_SCALE : 1e30f;
    dm.gateIsRoot = (m.num_bvh_nodes > 1 && memcmp(nodes[1].box, m.bmin, 12) == 0 && memcmp(nodes[1].box + 3, m.bmax, 12) == 0) ? 1u : 0u;
    return stackNeedRef;
  }
};

void BuildMeshes(const Blob &b, const BuildKnobs &k, SceneTables &out, uint32_t *stackNeedMax)
{
  const qa_flat_header *h = b.h;
  const qa_mesh *mesh = b.at<qa_mesh>(h->off_meshes);
  ScenePlan &plan = out.plan;
  plan.meshes.resize(h->num_meshes);
  out.mesh.resize(h->num_meshes);
  uint64_t totalFaces = 0;
  for (uint32_t mi = 0; mi < h->num_meshes; ++mi) totalFaces += mesh[mi].num_faces;
  for (uint32_t mi = 0; mi < h->num_meshes; ++mi) {
    const qa_mesh &m = mesh[mi];
    if (!b.inside(m.off_bvh_nodes, (uint64_t) m.num_bvh_nodes * sizeof(qa_bvh_node)) ||
        !b.inside(m.off_elements, (uint64_t) m.num_faces * 4) || !b.inside(m.off_faces, (uint64_t) m.num_faces * sizeof(qa_face)) ||
        !b.inside(m.off_vertices, (uint64_t) m.num_vertices * 12) || !b.inside(m.off_normals, (uint64_t) m.num_normals * 12) ||
        !b.inside(m.off_texcoords, (uint64_t) m.num_texcoords * 8))
      Refuse(QA_EINVAL, "mesh array outside the blob");
    if (m.off_bvh_nodes % 4 || m.off_elements % 4 || m.off_faces % 4 || m.off_vertices % 4 || m.off_normals % 4 || m.off_texcoords % 4)
      Refuse(QA_EINVAL, "mesh array offset is not 4-byte aligned");
    DMesh &dm = plan.meshes[mi];
    MeshBuild mb{b, m, k, out.mesh[mi], dm, b.at<qa_bvh_node>(m.off_bvh_nodes), b.at<uint32_t>(m.off_elements), b.at<qa_face>(m.off_faces),
                 b.at<float>(m.off_vertices)};
    const uint32_t stackNeedRef = mb.Run(mi, totalFaces, plan.textured);
    ++out.meshBuilds;
    *stackNeedMax = std::max(*stackNeedMax, dm.stackNeed);
    if (m.num_faces > QA_CS_INDEX_MASK) plan.csFits = false;     // a key holds instance << 20 | element (qa_kernel_cs.h)
    if (stackNeedRef > QA_CS_EXACT_STACK) plan.csFits = false;   // private stacks of the exact walks
    if (MissesTexcoords(plan, dm)) plan.csFits = false;
  }
}

// qa_integrate_cs: the 4-wide trees of all meshes in one node array and one triangle array (qa_kernel_cs.h)
void BuildCsTrees(const Blob &b, SceneTables &out)
{
  const qa_mesh *mesh = b.at<qa_mesh>(b.h->off_meshes);
  std::vector<float> &leafBox = out.csLeafBox;   // 8 floats per triangle: box of its leaf in the reference tree, 1.0f = that leaf is the root
  for (uint32_t mi = 0; mi < b.h->num_meshes; ++mi) {
    const MeshTables &mt = out.mesh[mi];
    const WideBvh &wb = mt.wide;
    const uint32_t nodeBase = (uint32_t) out.csNodes.size(), triBase = (uint32_t) out.csTris.size();
    auto rebase = [&](uint32_t w) -> uint32_t {
      if (w == QA_DONE) return w;
      if (w & QA_BVH_LEAF_BIT) return (w & ~QA_BVH_OFFSET_MASK) | ((w & QA_BVH_OFFSET_MASK) + triBase);
      return w + nodeBase;
    };
    for (const DWideNode &nd : wb.nodes) {
      DWideNode d = nd;
      for (int q = 0; q < 4; ++q) d.child[q] = rebase(nd.child[q]);
      out.csNodes.push_back(d);
    }
    const qa_bvh_node *rnodes = b.at<qa_bvh_node>(mesh[mi].off_bvh_nodes);
    for (size_t i = 0; i < mt.wtris.size(); ++i) {
      out.csTris.push_back(mt.wtris[i]);
      const uint32_t leaf = mt.shade[wb.order[i]].pad;
      float rec[8] = {0, 0, 0, 0, 0, 0, leaf <= 1 ? 1.0f : 0.0f, 0};
      if (leaf < mesh[mi].num_bvh_nodes) memcpy(rec, rnodes[leaf].box, 24);
      leafBox.insert(leafBox.end(), rec, rec + 8);
    }
    out.plan.meshes[mi].csRootWord = rebase(wb.rootWord);
  }
  ScenePlan &plan = out.plan;
  if (out.csNodes.size() > QA_CS_INDEX_MASK || out.csTris.size() > QA_CS_INDEX_MASK || b.h->num_instances > 256) plan.csFits = false;
  if (b.h->width > 0xFFFFu || b.h->height > 0xFFFFu || b.h->num_materials > 0xFFFEu) plan.csFits = false;   // pixel and material ride in 16-bit halves of the kernel's state words
  if (out.csTris.empty()) plan.csFits = false;
  if (!plan.csFits) { out.csNodes.clear(); out.csTris.clear(); leafBox.clear(); }
  else if (out.csNodes.empty()) out.csNodes.push_back(DWideNode{});
}

// one flat record per scene-graph node for qa_integrate_cs's sweeps, their root-space bounds and the culling constants
void BuildCsInstances(const Blob &b, SceneTables &out)
{
  const qa_flat_header *h = b.h;
  const qa_instance *inst = b.at<qa_instance>(h->off_instances);
  ScenePlan &plan = out.plan;
  if (!out.ds.rootIdentity) plan.csFits = false;   // (XML scenes: always the identity)
  out.csInst.assign(h->num_instances, CsInst{});
  out.csCull.resize(h->num_instances);
  for (CsCull &cb : out.csCull) { cb.lo[0] = cb.lo[1] = cb.lo[2] = 3e38f; cb.hi[0] = cb.hi[1] = cb.hi[2] = -3e38f; cb.pad0 = cb.pad1 = 0.f; }   // empty: never entered
  double cullS1 = 1, cullS2 = 1, cullK3 = 0, cullK4 = 0;
  bool cullOk = true;
  for (uint32_t k = 1; k < h->num_instances; ++k) {
    const qa_instance &in = inst[k];
    CsInst &r = out.csInst[k];
    r.type = in.obj_type;
    r.depth = in.depth;
    r.parent = in.parent;
    if (in.obj_type == QA_OBJ_NONE) continue;
    if (in.depth < 1 || in.depth > 2) { plan.csFits = false; continue; }
    const qa_instance &a = in.depth == 2 ? inst[in.parent] : in;
    memcpy(r.itmA, a.itm, 36); memcpy(r.posA, a.pos, 12); memcpy(r.tmA, a.tm, 36);
    if (in.depth == 2) { memcpy(r.itmB, in.itm, 36); memcpy(r.posB, in.pos, 12); memcpy(r.tmB, in.tm, 36); }
    double lo[3] = {-1, -1, -1}, hi[3] = {1, 1, 1};   // sphere: the unit ball; plane: the unit square at z = 0
    if (in.obj_type == QA_OBJ_PLANE) lo[2] = hi[2] = 0;
    if (in.obj_type == QA_OBJ_MESH) {
      const DMesh &dm = plan.meshes[in.mesh];
      r.mesh = (uint32_t) in.mesh;
      r.useWide = dm.useWide;
      r.csRootWord = dm.csRootWord;
      r.num_faces = dm.num_faces;
      memcpy(r.bmin, dm.bmin, 12); memcpy(r.bmax, dm.bmax, 12);
      r.nearPad = dm.nearPad; r.absMax = dm.absMax; r.cancelDist = dm.cancelDist;
      for (int q = 0; q < 3; ++q) { lo[q] = dm.bmin[q]; hi[q] = dm.bmax[q]; }
    }
    // bounds in root space: the eight corners through tm * p + pos of every level (double), padded below
    double wlo[3] = {1e300, 1e300, 1e300}, whi[3] = {-1e300, -1e300, -1e300};
    for (int corner = 0; corner < 8; ++corner) {
      double pnt[3] = {(corner & 1) ? hi[0] : lo[0], (corner & 2) ? hi[1] : lo[1], (corner & 4) ? hi[2] : lo[2]};
      for (int lvl = in.depth; lvl >= 1; --lvl) {
        const qa_instance &t = (lvl == in.depth) ? in : inst[in.parent];
        double o[3];
        for (int rr = 0; rr < 3; ++rr) o[rr] = (double) t.tm[rr] * pnt[0] + (double) t.tm[3 + rr] * pnt[1] + (double) t.tm[6 + rr] * pnt[2] + (double) t.pos[rr];
        memcpy(pnt, o, sizeof(o));
      }
      for (int q = 0; q < 3; ++q) { wlo[q] = std::min(wlo[q], pnt[q]); whi[q] = std::max(whi[q], pnt[q]); }
    }
    for (int q = 0; q < 3; ++q) { r.wmin[q] = (float) wlo[q]; r.wmax[q] = (float) whi[q]; }
    // instance culling (qa_kernel_cs.h csCullRay): bounds rounded outwards, and this node's share of the scene's widening constants
    CsCull &cb = out.csCull[k];
    double boxAbs = 0;
    for (int q = 0; q < 3; ++q) {
      cb.lo[q] = std::nextafterf((float) wlo[q], -INFINITY);
      cb.hi[q] = std::nextafterf((float) whi[q], INFINITY);
      boxAbs = std::max({boxAbs, std::fabs(wlo[q]), std::fabs(whi[q])});
    }
    auto normInf = [](const float *m) { double n = 0; for (int rr = 0; rr < 3; ++rr) n = std::max(n, (double) std::fabs(m[rr]) + std::fabs(m[3 + rr]) + std::fabs(m[6 + rr])); return n; };
    auto vecInf = [](const float *v) { return std::max({(double) std::fabs(v[0]), (double) std::fabs(v[1]), (double) std::fabs(v[2])}); };
    double cond = normInf(a.tm) * normInf(a.itm), tmNorm = normInf(a.tm), posAbs = vecInf(a.pos);
    if (in.depth == 2) {
      cond *= normInf(in.tm) * normInf(in.itm);
      posAbs += normInf(a.tm) * vecInf(in.pos);
      tmNorm *= normInf(in.tm);
    }
    cullS1 = std::max(cullS1, posAbs + 1.0);
    cullS2 = std::max(cullS2, boxAbs + 1.0);
    cullK3 = std::max(cullK3, 2e-5 * cond);
    cullK4 = std::max(cullK4, 2.0 * tmNorm * (in.obj_type == QA_OBJ_MESH ? (double) r.nearPad : 0.0) + 1e-5 * (boxAbs + 1.0));
    if (!std::isfinite(cond) || !std::isfinite(boxAbs) || !std::isfinite(posAbs) || !std::isfinite(tmNorm)) cullOk = false;
  }
  DScene &ds = out.ds;
  ds.csCullS1 = (float) cullS1; ds.csCullS2 = (float) cullS2; ds.csCullK3 = (float) cullK3; ds.csCullK4 = (float) cullK4;
  plan.csCullOk = cullOk && std::isfinite(ds.csCullS1) && std::isfinite(ds.csCullS2) && std::isfinite(ds.csCullK3) && std::isfinite(ds.csCullK4);
}

// plain colours; returns whether any material has reflective / refractive lobes
bool BuildMaterials(const Blob &b, SceneTables &out)
{
  const qa_material *mats = b.at<qa_material>(b.h->off_materials);
  out.materials.resize(b.h->num_materials);
  bool anySpecularLobes = false;
  for (uint32_t i = 0; i < b.h->num_materials; ++i) {
    const qa_material &m = mats[i];
    DMaterial &d = out.materials[i];
    memcpy(d.diffuse, m.diffuse.color, 12);       d.kill = m.kill;
    memcpy(d.specular, m.specular.color, 12);     d.gloss_spec = m.gloss_spec;
    memcpy(d.emission, m.emission.color, 12);     d.ior = m.ior;
    memcpy(d.reflection, m.reflection.color, 12); d.gloss_refl = m.gloss_refl;
    memcpy(d.refraction, m.refraction.color, 12); d.gloss_refr = m.gloss_refr;
    memcpy(d.absorption, m.absorption, 12);
    d.flags = 0;
    for (int k = 0; k < 3; ++k) {
      if (m.reflection.color[k] != 0.f || m.refraction.color[k] != 0.f) d.flags |= QA_MTL_SPECULAR_LOBES;
      if (m.specular.color[k] != 0.f) d.flags |= QA_MTL_HAS_SPECULAR;
    }
    anySpecularLobes |= (d.flags & QA_MTL_SPECULAR_LOBES) != 0;
  }
  return anySpecularLobes;
}

// texture-side tables (TEX kernel variants)
void BuildTextures(const Blob &b, SceneTables &out)
{
  const qa_flat_header *h = b.h;
  const qa_material *mats = b.at<qa_material>(h->off_materials);
  const qa_texture *textures = b.at<qa_texture>(h->off_textures);
  out.mtlTex.assign(8 * (size_t) h->num_materials, -1);
  for (uint32_t i = 0; i < h->num_materials; ++i) {
    int32_t *mt = &out.mtlTex[8 * (size_t) i];
    mt[0] = mats[i].diffuse.texmap;
    mt[1] = mats[i].specular.texmap;
    mt[2] = mats[i].emission.texmap;
    mt[3] = mats[i].reflection.texmap;
    mt[4] = mats[i].refraction.texmap;
    for (int k = 0; k < 5; ++k) if (mt[k] >= (int) h->num_texmaps) Refuse(QA_EINVAL, "bad texmap index");
  }
  // file textures as float RGB: TextureFile::Sample divides every byte it reads by 255.0f (src/textures/texture.cpp:120-131) - 12
  // divisions per bilinear tap, 384 per filtered lookup; the same IEEE division once per texel here gives the same bits
  out.texOff.assign(std::max<uint32_t>(h->num_textures, 1u), 0u);
  std::vector<float> &tex4 = out.texels;
  for (uint32_t i = 0; i < h->num_textures; ++i) {
    const qa_texture &tx = textures[i];
    out.texOff[i] = (uint32_t) (tex4.size() / 4);
    if (tx.type == QA_TEX_CHECKER || tx.width <= 0 || tx.height <= 0) continue;
    const size_t n = (size_t) tx.width * (size_t) tx.height;
    if (!b.inside(tx.off_texels, 3 * n)) Refuse(QA_EINVAL, "texture texels outside the blob");
    const unsigned char *px = b.p + tx.off_texels;
    const size_t at = tex4.size();
    tex4.resize(at + 4 * n);
    texelsTabulateHost(px, n, 1, 3 * n, tex4.data() + at);   // (qa_texel_dev.h: a texel edit recomputes entries from the same source)
  }
  if (tex4.size() / 4 > 0xFFFFFFFFull) Refuse(QA_EUNSUPPORTED, "more than 2^32 texels");
  if (tex4.empty()) tex4.assign(4, 0.f);
  // Texture::Sample's elliptical taps (src/core/texture.cpp:39-46), i = 1..31, host libm
  out.taps.resize(62);
  for (int i = 1; i < 32; ++i) {
    float x = HaltonF(i, 2), y = HaltonF(i, 3);
    const float r = sqrtf(x) * 0.5f;
    x = r * sinf(y * (float) M_PI * 2);
    y = r * cosf(y * (float) M_PI * 2);
    out.taps[2 * (i - 1)] = x;
    out.taps[2 * (i - 1) + 1] = y;
  }
}

// resident image: [nodes | tris | shade] per mesh, then materials, in 16-byte units
void BuildImage(SceneTables &out)
{
  std::vector<uint4> &image = out.image;
  auto append = [&](const void *p, size_t bytes) {
    const uint32_t off = (uint32_t) image.size();
    const size_t n = (bytes + 15) / 16;
    image.resize(image.size() + n, uint4{0, 0, 0, 0});
    if (bytes) memcpy(image.data() + off, p, bytes);
    return off;
  };
  auto pad64 = [&] { while (image.size() % 4) image.push_back(uint4{0, 0, 0, 0}); };   // node pairs on 64-byte boundaries
  for (size_t mi = 0; mi < out.mesh.size(); ++mi) {
    const MeshTables &mt = out.mesh[mi];
    DMesh &dm = out.plan.meshes[mi];
    pad64();
    dm.resNodes = append(mt.nodes.data(), mt.nodes.size() * sizeof(DNode));
    dm.resTris = append(mt.tris.data(), mt.tris.size() * sizeof(DTri));
    dm.resShade = append(mt.shade.data(), mt.shade.size() * sizeof(DTriShade));
    pad64();
    dm.resFNodes = append(mt.fnodes.data(), mt.fnodes.size() * sizeof(DNode));
    dm.resFTris = append(mt.ftris.data(), mt.ftris.size() * sizeof(DTri));
    dm.resFMap = append(mt.fmap.data(), mt.fmap.size() * sizeof(uint32_t));
    dm.resNormals = append(mt.normals.data(), mt.normals.size() * sizeof(float));
    dm.numNormals = (uint32_t) (mt.normals.size() / 4);
  }
  out.ds.resMaterials = append(out.materials.data(), out.materials.size() * sizeof(DMaterial));
  // what follows stays in global memory: the leaf tables are read once per work item (qa_integrate, section A), their sorted copies by
  // scalar loads, once per bounce ray's query of the mesh (qa_kernel.h sweepLeaves)
  out.imageLdsVec4 = image.size();
  for (size_t mi = 0; mi < out.mesh.size(); ++mi) {
    DMesh &dm = out.plan.meshes[mi];
    dm.numLeaves = dm.useFast ? (uint32_t) out.mesh[mi].leaves.size() : 0u;
    dm.resLeaves = dm.numLeaves ? append(out.mesh[mi].leaves.data(), out.mesh[mi].leaves.size() * sizeof(DNode)) : 0u;
    if (dm.numLeaves) append(out.mesh[mi].sweepLeaves.data(), out.mesh[mi].sweepLeaves.size() * sizeof(DNode));   // at resLeaves + 2 * numLeaves
    unsigned char pairs[QA_TILE_LEAF_CAP];
    dm.leafPairs = dm.numLeaves && LeafPairBytes(out.mesh[mi].sweepLeaves, pairs) ? 1u : 0u;
    if (dm.numLeaves) append(pairs, sizeof(pairs));   // at resLeaves + 4 * numLeaves, always all 64 bytes: the kernel copies them whole
  }
}

void PlanLastCast(const Blob &b, SceneTables &out);
// the DScene fields that come from the header, the stack and LDS sizes, and residency; the last-cast predicate
void PlanScene(const Blob &b, const BuildKnobs &k, uint32_t stackNeedMax, SceneTables &out)
{
  const qa_flat_header *h = b.h;
  DScene &ds = out.ds;
  ScenePlan &plan = out.plan;
  ds.stackNeed = stackNeedMax;
  ds.stackDepth = std::max(stackNeedMax, 8u);
  // LDS per workgroup: traversal stacks + 6 accumulator floats per lane (mean, variance); small scenes stay entirely on the CU
  const size_t stackBytes = ((size_t) ds.stackDepth + QA_LANE_SLOTS) * QA_BLOCK * sizeof(uint32_t);
  const size_t imageBytes = out.imageLdsVec4 * sizeof(uint4);
  if (stackBytes > kMaxLdsPerBlock) Refuse(QA_EUNSUPPORTED, "BVH too deep for the LDS traversal stack");
  // workgroups of a resident scene also keep the cold path state in LDS columns (QA_LANE_SLOTS_RES)
  const size_t stackBytesRes = ((size_t) ds.stackDepth + QA_LANE_SLOTS_RES) * QA_BLOCK * sizeof(uint32_t);
  plan.resident = imageBytes > 0 && imageBytes + stackBytesRes <= kResidentLdsBudget && h->num_instances <= QA_KARG_INST &&
                  h->num_meshes <= QA_KARG_MESH;
  plan.ldsBytes = plan.resident ? stackBytesRes + imageBytes : stackBytes;
  // the waves' tile lists: only where some mesh has a leaf table and the workgroups per CU stay what they are.  A CU's 160 KB of
  // LDS are handed out in units of 1280 bytes: the Cornell box's 31 520 B are 25 units, five workgroups per CU; with 960 B more
  // (26 units) four were resident and the frame took 80 ms instead of 71 (profiles/tile_lists.txt)
  plan.tileListBytes = 0;
  const size_t listBytes = (QA_BLOCK / 64) * QA_TILE_LIST_DWORDS * sizeof(uint32_t), cuLds = 160 * 1024, unit = 1280;
  auto perCU = [&](size_t bytes) { return cuLds / ((bytes + unit - 1) / unit * unit); };
  bool anyLeaves = false;
  for (const DMesh &dm : plan.meshes) anyLeaves = anyLeaves || dm.numLeaves > 0;
  if (plan.resident && anyLeaves && perCU(plan.ldsBytes + listBytes) == perCU(plan.ldsBytes)) plan.tileListBytes = listBytes;
  if (plan.resident) {
    ds.residentVec4 = (uint32_t) out.imageLdsVec4;
    std::copy(b.at<qa_instance>(h->off_instances), b.at<qa_instance>(h->off_instances) + h->num_instances, ds.instv);
  } else ds.resMaterials = 0;
  ds.csSlots = std::min(std::max(k.csSlots, 64u), 256u);   // an instance enters up to 64 rays at once; 8 bits of an item
  ds.csItems = std::max(k.csItems, 128u);
  memcpy(ds.cam.screenA, h->screenA, 12);
  memcpy(ds.cam.screenU, h->screenU, 12);
  memcpy(ds.cam.screenV, h->screenV, 12);
  memcpy(ds.cam.screenX, h->screenX, 12);
  memcpy(ds.cam.screenY, h->screenY, 12);
  memcpy(ds.cam.pos, h->cam_pos, 12);
  ds.cam.dof = h->dof;
  ds.cam.width = (int) h->width;
  ds.cam.height = (int) h->height;
  memcpy(ds.background, h->background.color, 12);
  memcpy(ds.environment, h->environment.color, 12);
  ds.bgTexmap = h->background.texmap;
  ds.envTexmap = h->environment.texmap;
  ds.num_inst = (int) h->num_instances;
  ds.num_lights = (int) h->num_lights;
  ds.num_materials = (int) h->num_materials;
  PlanLastCast(b, out);
}

// what follows from the lights and the root node alone
void PlanLightsAndRoot(const Blob &b, SceneTables &out)
{
  const qa_flat_header *h = b.h;
  ScenePlan &plan = out.plan;
  const qa_light *light = b.at<qa_light>(h->off_lights);
  plan.area = false;
  plan.shadowLights.clear();
  for (uint32_t i = 0; i < h->num_lights; ++i) {
    if ((light[i].type == QA_LIGHT_POINT || light[i].type == QA_LIGHT_SPOT) && light[i].size > 0.01f) plan.area = true;
    if (light[i].type != QA_LIGHT_AMBIENT) plan.shadowLights.push_back((int32_t) i);
  }
  const qa_instance *inst = b.at<qa_instance>(h->off_instances);
  static const float I9[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1}, Z3[3] = {0, 0, 0};
  out.ds.rootIdentity = (memcmp(inst[0].tm, I9, 36) == 0 && memcmp(inst[0].itm, I9, 36) == 0 && memcmp(inst[0].pos, Z3, 12) == 0) ? 1 : 0;
}

// what a scene edit must leave alone of the texture records: the float texel table is laid out by them (RebuildSceneSide)
void KeepTexLayout(const Blob &b, SceneTables &out)
{
  const qa_texture *textures = b.at<qa_texture>(b.h->off_textures);
  out.texLayout.resize(b.h->num_textures);
  for (uint32_t i = 0; i < b.h->num_textures; ++i)
    out.texLayout[i] = TexLayout{textures[i].type, textures[i].width, textures[i].height, 0, textures[i].off_texels};
}

// May the bounce rays of this scene be asked "which emitter do you meet" instead of "what do you hit" (qa_kernel.h lastCastQuery)?
// Without lights, textures and reflective / refractive lobes a path is camera ray, diffuse hit, one bounce ray, and the bounce ray's
// hit adds its material's emission, draws RandomSelectMtl's one number and spawns nothing (shadeSurface: !fromDiffuse fails).  Then
// the hit itself is not needed where
//   * no material absorbs (Beer's factor of a back-face hit is exp(-0 * z) = 1 exactly),
//   * every node with an object has a material, a plane or sphere a single one (a MultiMtl on them is indexed by the mtlID an earlier
//     mesh hit left behind), and a mesh under a MultiMtl no face id outside it (that hit adds white and draws nothing),
//   * the emitting materials belong to planes and spheres only ("glow nodes", at most 32 nodes: one mask word): a mesh hit adds
//     T * 0 whichever triangle it is.  A scene with an emitting mesh material keeps the closest-hit kernel.
// Every edit that can change any of this ends in PlanScene (RebuildSceneSide).
void PlanLastCast(const Blob &b, SceneTables &out)
{
  const qa_flat_header *h = b.h;
  ScenePlan &plan = out.plan;
  plan.lastCastQuery = false;
  plan.lastCastGlow = 0;
  if (h->num_lights != 0 || plan.textured || plan.area || h->num_instances > 32) return;
  const qa_material *mats = b.at<qa_material>(h->off_materials);
  const qa_mtlset *sets = b.at<qa_mtlset>(h->off_mtlsets);
  const qa_instance *inst = b.at<qa_instance>(h->off_instances);
  const qa_mesh *meshes = b.at<qa_mesh>(h->off_meshes);
  auto emits = [&](int32_t mi) { const float *e = mats[mi].emission.color; return !(e[0] == 0.f && e[1] == 0.f && e[2] == 0.f); };
  for (uint32_t i = 0; i < h->num_materials; ++i) {
    const qa_material &m = mats[i];
    for (int k = 0; k < 3; ++k)
      if (m.reflection.color[k] != 0.f || m.refraction.color[k] != 0.f || !(m.absorption[k] == 0.f)) return;
  }
  uint32_t glow = 0;
  for (uint32_t k = 0; k < h->num_instances; ++k) {
    const qa_instance &in = inst[k];
    if (in.obj_type == QA_OBJ_NONE) continue;
    if (k == 0) continue;   // (the sweeps start at node 1: an object on the root is never traced)
    if (in.mtlset < 0 || (uint32_t) in.mtlset >= h->num_mtlsets) return;
    const qa_mtlset &ms = sets[in.mtlset];
    const int32_t count = ms.multi ? ms.count : 1;
    if (ms.first < 0 || count < 1 || (uint64_t) ms.first + (uint64_t) count > h->num_materials) return;
    bool glows = false;
    for (int32_t i = 0; i < count; ++i) glows = glows || emits(ms.first + i);
    if (in.obj_type == QA_OBJ_MESH) {
      if (glows) return;
      if (in.mesh < 0 || (uint32_t) in.mesh >= h->num_meshes) return;
      if (ms.multi) {
        const qa_mesh &m = meshes[in.mesh];
        const qa_face *faces = b.at<qa_face>(m.off_faces);
        for (uint32_t f = 0; f < m.num_faces; ++f)
          if (faces[f].mtl < 0 || faces[f].mtl >= ms.count) return;
      }
    } else {
      if (ms.multi) return;
      if (glows) glow |= 1u << k;
    }
  }
  plan.lastCastQuery = true;
  plan.lastCastGlow = glow;
}

// Without reflective / refractive lobes a path is at most camera ray + one diffuse bounce: starting
// the samples of a wave together keeps its coherent camera rays apart from the incoherent bounce
// rays (+21 % on the Cornell box).  Long specular chains would make lanes wait for the longest path.
// Textured scenes also start samples together: the 32-tap filtered lookups of camera hits are the
// expensive part of their shading and stay coherent that way (+18 % on project7_object, whereas the
// untextured glossy-caustics scene loses 14 % to waiting for its long specular chains).
int SyncAuto(const ScenePlan &plan, bool anySpecularLobes) { return (!anySpecularLobes || plan.textured) ? 1 : 0; }

}  // namespace

// Where the leaves of a sorted leaf table have their triangles in DMesh::ftris, one byte a leaf: first | (count - 1) << 7.  A lane of
// qa_integrate_lastcast's sweep reads its candidate's byte from LDS instead of the leaf word from global memory (qa_kernel.h
// sweepLeaves).  -> false, and all bytes zero, where some leaf has more than two triangles or starts beyond 127
bool LeafPairBytes(const std::vector<DNode> &sorted, unsigned char bytes[QA_TILE_LEAF_CAP])
{
  memset(bytes, 0, QA_TILE_LEAF_CAP);
  if (sorted.empty() || sorted.size() > QA_TILE_LEAF_CAP) return false;
  for (size_t j = 0; j < sorted.size(); ++j) {
    const uint32_t word = sorted[j].data;
    const uint32_t count = ((word >> QA_BVH_COUNT_SHIFT) & QA_BVH_COUNT_MASK) + 1, first = word & QA_BVH_OFFSET_MASK;
    if (count > 2 || first > 127) {
      memset(bytes, 0, QA_TILE_LEAF_CAP);
      return false;
    }
    bytes[j] = (unsigned char) (first | (count - 1) << 7);
  }
  return true;
}

// core/sampler.cpp:31-40, evaluated on the host in the reference's fp32 order
float HaltonF(int index, int base)
{
  float r = 0;
  float f = 1.0f / (float) base;
  for (int i = index; i > 0; i /= base) {
    r += f * (i % base);
    f /= (float) base;
  }
  return r;
}

int BuildScene(const unsigned char *blob, size_t nbytes, const BuildKnobs &knobs, SceneTables &out, std::string *err)
{
  out = SceneTables{};
  memset(&out.ds, 0, sizeof(out.ds));   // (padding included: the record is a kernel argument)
  try {
    const Blob b{blob, nbytes, reinterpret_cast<const qa_flat_header *>(blob)};
    CheckHeader(b);
    const qa_flat_header *h = b.h;
    ScenePlan &plan = out.plan;
    PlanLightsAndRoot(b, out);
    const qa_instance *inst = b.at<qa_instance>(h->off_instances);
    plan.meshInstanced.assign(h->num_meshes, false);
    for (uint32_t k = 0; k < h->num_instances; ++k) if (inst[k].obj_type == QA_OBJ_MESH) plan.meshInstanced[inst[k].mesh] = true;
    plan.textured = h->num_texmaps > 0;
    KeepTexLayout(b, out);
    plan.csFits = true;
    uint32_t stackNeedMax = 1;
    BuildMeshes(b, knobs, out, &stackNeedMax);
    const bool anySpecularLobes = BuildMaterials(b, out);
    BuildImage(out);
    BuildCsTrees(b, out);
    out.csFitsMeshes = plan.csFits;
    BuildCsInstances(b, out);
    plan.syncAuto = SyncAuto(plan, anySpecularLobes);
    if (plan.textured) BuildTextures(b, out);
    PlanScene(b, knobs, stackNeedMax, out);
  } catch (const Refused &r) {
    *err = r.msg;
    return r.code;
  } catch (const std::bad_alloc &) {
    *err = "out of memory";
    return QA_ENOMEM;
  }
  return QA_OK;
}

}  // namespace qa

namespace qa {

int RebuildSceneSide(const unsigned char *blob, size_t nbytes, const BuildKnobs &knobs, SceneTables &out, std::string *err)
{
  try {
    const Blob b{blob, nbytes, reinterpret_cast<const qa_flat_header *>(blob)};
    CheckHeader(b);   // (the only stage below that can refuse: nothing is changed before it has passed)
    const qa_flat_header *h = b.h;
    if (h->num_instances != out.csInst.size() || h->num_materials != out.materials.size() || h->num_meshes != out.plan.meshes.size() ||
        (int) h->num_lights != out.ds.num_lights || (int) h->width != out.ds.cam.width || (int) h->height != out.ds.cam.height)
      Refuse(QA_EINVAL, "not an edit of the blob these tables were built from (counts or image size differ)");
    // texture side: the texmap records, the textures' colours and the two header colours are read in place (by the kernels, or by
    // PlanScene below); what lays out the texel table, and which map the backdrop shows, stays
    if (h->num_textures != out.texLayout.size() || (h->num_texmaps > 0) != out.plan.textured)
      Refuse(QA_EINVAL, "not an edit of the blob these tables were built from (texture counts differ)");
    const qa_texture *textures = b.at<qa_texture>(h->off_textures);
    for (uint32_t i = 0; i < h->num_textures; ++i) {
      const TexLayout &l = out.texLayout[i];
      if (textures[i].type != l.type || textures[i].width != l.width || textures[i].height != l.height || textures[i].off_texels != l.off_texels)
        Refuse(QA_EINVAL, "a texture edit can change color1 and color2 only (type, size and texel offset stay: the texel table is not laid out again): upload the scene instead");
    }
    if (h->background.texmap != out.ds.bgTexmap || h->environment.texmap != out.ds.envTexmap)
      Refuse(QA_EINVAL, "a backdrop edit can change the two colours only (their texture maps stay): upload the scene instead");
    ScenePlan &plan = out.plan;
    PlanLightsAndRoot(b, out);
    plan.csFits = out.csFitsMeshes;
    const bool anySpecularLobes = BuildMaterials(b, out);
    // the resident image's LDS part ends with the material table (BuildImage); everything before it is mesh data
    const size_t mtlVec4 = (out.materials.size() * sizeof(DMaterial) + 15) / 16;
    if (out.image.size() >= out.imageLdsVec4 && out.imageLdsVec4 >= mtlVec4 && mtlVec4) memcpy(out.image.data() + (out.imageLdsVec4 - mtlVec4), out.materials.data(), out.materials.size() * sizeof(DMaterial));
    BuildCsInstances(b, out);
    plan.syncAuto = SyncAuto(plan, anySpecularLobes);
    PlanScene(b, knobs, out.ds.stackNeed, out);
  } catch (const Refused &r) {
    *err = r.msg;
    return r.code;
  } catch (const std::bad_alloc &) {
    *err = "out of memory";
    return QA_ENOMEM;
  }
  return QA_OK;
}

void DropMeshSide(SceneTables &t)
{
  for (MeshTables &m : t.mesh) m = MeshTables{};
  std::vector<DWideNode>().swap(t.csNodes);
  std::vector<DTri>().swap(t.csTris);
  std::vector<float>().swap(t.csLeafBox);
  std::vector<float>().swap(t.texels);
  if (!t.plan.resident) std::vector<uint4>().swap(t.image);
}

}  // namespace qa
