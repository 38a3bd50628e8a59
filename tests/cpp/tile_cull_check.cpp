// Host check of the per-tile leaf lists of camera rays (qa_tilecull.h; built by tests/test_tile_cull_host.py with
// -fsanitize=address,undefined, no GPU):
//   tile_cull_check rays <blob>...   for every 8x8 tile of the blob's frame and every mesh node with a leaf table: the tile's
//                                    list as qa_integrate builds it, then 256 random sub-pixel camera rays per tile; every
//                                    leaf whose widened box passes the walk's own non-strict test (either form, no distance
//                                    limit) for one of them must be on the list.  One line per node; exit code 1 on an omission.
//   tile_cull_check leaves <blob>    the leaf tables
//   tile_cull_check hist <blob>      histogram of list lengths over the tiles whose pyramid meets the mesh bounds, and the
//                                    mean number of listed leaves and triangles
#include <cmath>
#include <cstdio>
#include <cstring>
#include <fstream>
#include <iterator>
#include <string>
#include <vector>

#include "qa_scene_build.h"
#include "qa_tilecull.h"
#include "qaray_host.h"

using namespace qa;
typedef std::vector<unsigned char> Bytes;

static Bytes Read(const char *path)
{
  std::ifstream f(path, std::ios::binary);
  return Bytes(std::istreambuf_iterator<char>(f), std::istreambuf_iterator<char>());
}

struct Scene {
  Bytes blob;
  SceneTables t;
  const qa_flat_header *h = nullptr;
  const qa_instance *inst = nullptr;
  bool Load(const char *path)
  {
    blob = Read(path);
    blob.shrink_to_fit();
    std::string err;
    const int rc = BuildScene(blob.data(), blob.size(), BuildKnobs{}, t, &err);
    if (rc != QA_OK) { printf("%s: BuildScene rc=%d %s\n", path, rc, err.c_str()); return false; }
    h = reinterpret_cast<const qa_flat_header *>(blob.data());
    inst = QA_BLOB_PTR(qa_instance, blob.data(), h->off_instances);
    return true;
  }
  // the node chain of instance k, outermost first, as localRay / buildTileLists apply it
  std::vector<int> Chain(int k) const
  {
    std::vector<int> c;
    for (int a = k; a > 0 && (int) c.size() < QA_MAX_NODE_DEPTH; a = inst[a].parent) c.insert(c.begin(), a);
    if (!t.ds.rootIdentity) c.insert(c.begin(), 0);
    return c;
  }
};

// the tile's list for node k: bit i = leaf i of the table is listed
struct TileList { unsigned long long mask = 0; TileCone cone; float pad = 0; };
static TileList ListOf(const Scene &s, int k, const std::vector<int> &chain, int X0, int Y0)
{
  const DCamera &cam = s.t.ds.cam;
  const DMesh &m = s.t.plan.meshes[s.inst[k].mesh];
  const std::vector<DNode> &leaves = s.t.mesh[s.inst[k].mesh].leaves;
  const f3 oW = ld3(cam.pos);
  f3 cW[4], c[4];
  tileWindow(ld3(cam.screenA), ld3(cam.screenU), ld3(cam.screenV), (float) X0, (float) Y0, cW);
  f3 o = oW;
  for (int i = 0; i < 4; ++i) c[i] = cW[i];
  for (int a : chain) {
    o = tileNodePoint(s.inst[a], o);
    for (int i = 0; i < 4; ++i) c[i] = tileNodePoint(s.inst[a], c[i]);
  }
  TileList L;
  tileCone(tileLens(oW, cW), o, c, &L.cone);
  L.pad = fastWalkPad(m.invH, m.absMax, L.cone.oAbs);
  for (size_t i = 0; i < leaves.size(); ++i) {
    float tLow;
    if (tileConeMeetsBox(&L.cone, ld3(leaves[i].box), ld3(leaves[i].box + 3), L.pad, &tLow)) L.mask |= 1ull << i;
    if (!(tLow >= 0)) { printf("entry bound %g is not a number >= 0\n", (double) tLow); L.mask = 0; }
  }
  return L;
}

static uint32_t g_rng = 0x9E3779B9u;
static float Rnd()   // [0, 1), the ends included now and then
{
  g_rng ^= g_rng << 13; g_rng ^= g_rng >> 17; g_rng ^= g_rng << 5;
  const uint32_t pick = g_rng & 31u;
  if (pick == 0) return 0.f;
  if (pick == 1) return std::nextafterf(1.f, 0.f);
  return (float) (g_rng >> 8) / 16777216.0f;
}

static int Rays(const char *path)
{
  Scene s;
  if (!s.Load(path)) return 1;
  const DCamera &cam = s.t.ds.cam;
  const int W = cam.width, H = cam.height;
  int bad = 0, nodes = 0;
  for (int k = 1; k < (int) s.h->num_instances; ++k) {
    if (s.inst[k].obj_type != QA_OBJ_MESH) continue;
    const DMesh &m = s.t.plan.meshes[s.inst[k].mesh];
    if (!m.useFast || !m.numLeaves) continue;
    ++nodes;
    const std::vector<DNode> &leaves = s.t.mesh[s.inst[k].mesh].leaves;
    const std::vector<int> chain = s.Chain(k);
    // the pose: where the origin is in node space, and what of the mesh lies behind it along the view axis
    f3 o = ld3(cam.pos), fwd = (ld3(cam.screenA) + ld3(cam.screenU) * (0.5f * W)) + ld3(cam.screenV) * (0.5f * H);
    for (int a : chain) { fwd = tileNodePoint(s.inst[a], fwd); o = tileNodePoint(s.inst[a], o); }
    fwd = fwd - o;
    auto inside = [&](const float *b) { return o.x >= b[0] && o.y >= b[1] && o.z >= b[2] && o.x <= b[3] && o.y <= b[4] && o.z <= b[5]; };
    const float mb[6] = {m.bmin[0], m.bmin[1], m.bmin[2], m.bmax[0], m.bmax[1], m.bmax[2]};
    int insideLeaf = 0, cornersBehind = 0;
    for (const DNode &l : leaves) insideLeaf += inside(l.box) ? 1 : 0;
    for (int q = 0; q < 8; ++q)
      cornersBehind += dot(F3(mb[(q & 1) ? 3 : 0], mb[(q & 2) ? 4 : 1], mb[(q & 4) ? 5 : 2]) - o, fwd) < 0 ? 1 : 0;
    unsigned long long rays = 0, required = 0, listed = 0, omissions = 0, tiles = 0, slowForm = 0;
    for (int Y0 = 0; Y0 < H; Y0 += 8)
      for (int X0 = 0; X0 < W; X0 += 8) {
        const TileList L = ListOf(s, k, chain, X0, Y0);
        ++tiles;
        listed += (unsigned long long) __builtin_popcountll(L.mask);
        for (int r = 0; r < 256; ++r) {
          const int px = X0 + (int) (g_rng % (unsigned) std::min(8, W - X0)), py = Y0 + (int) ((g_rng >> 8) % (unsigned) std::min(8, H - Y0));
          const f3 texpos = F3(Rnd(), Rnd(), 0.f) + F3((float) px, (float) py, 0.f);
          // qa_integrate section B (src/renderers/renderer.cpp:312-328), then rootRay and localRay
          const f3 cpt = (ld3(cam.screenA) + ld3(cam.screenU) * texpos.x) + ld3(cam.screenV) * texpos.y;
          Ray ray;
          ray.p = ld3(cam.pos);
          ray.d = normalize(cpt - ray.p);
          if (s.t.ds.rootIdentity) ray.d = (ray.p + ray.d) - ray.p;
          for (int a : chain) ray = toNode(s.inst[a], ray);
          ++rays;
          const float oMax = qmax(qmax(qabs(ray.p.x), qabs(ray.p.y)), qabs(ray.p.z));
          const float pad = fastWalkPad(m.invH, m.absMax, oMax);
          const f3 pLo = ray.p + F3(pad, pad, pad), pHi = ray.p - F3(pad, pad, pad);
          const f3 drcp = F3(1.f / ray.d.x, 1.f / ray.d.y, 1.f / ray.d.z);
          const bool fastSlab = !(qabs(ray.d.x) < 1e-7f || qabs(ray.d.y) < 1e-7f || qabs(ray.d.z) < 1e-7f);
          slowForm += fastSlab ? 0 : 1;
          for (size_t i = 0; i < leaves.size(); ++i) {
            const f3 bmin = ld3(leaves[i].box), bmax = ld3(leaves[i].box + 3);
            float e0, x0, e1, x1;
            boxEntryExitPad(pLo, pHi, ray.d, drcp, bmin, bmax, e0, x0);
            bool pass = e0 <= x0;
            if (fastSlab) {   // (the walk takes this form only when no lane of the wave has a near-zero component)
              boxEntryExitPadFast(pLo, pHi, drcp, bmin, bmax, e1, x1);
              pass = pass || e1 <= x1;
            }
            if (!pass) continue;
            ++required;
            if (!((L.mask >> i) & 1ull)) {
              if (omissions++ < 5) printf("  omitted: tile (%d, %d) leaf %zu, ray through (%.9g, %.9g)\n", X0, Y0, i, (double) texpos.x, (double) texpos.y);
            }
          }
        }
      }
    printf("%s node=%d leaves=%u originInBounds=%d originInLeaves=%d cornersBehind=%d tiles=%llu rays=%llu exactFormRays=%llu required=%llu listedPerTile=%.2f omissions=%llu\n",
           path, k, m.numLeaves, inside(mb) ? 1 : 0, insideLeaf, cornersBehind, tiles, rays, slowForm, required, (double) listed / (double) tiles, omissions);
    bad += omissions ? 1 : 0;
  }
  if (!nodes) { printf("%s: no mesh node with a leaf table\n", path); return 1; }
  return bad ? 1 : 0;
}

static int Hist(const char *path)
{
  Scene s;
  if (!s.Load(path)) return 1;
  const DCamera &cam = s.t.ds.cam;
  printf("%s: %dx%d, dynamic LDS %zu B + %zu B of tile lists\n", path, cam.width, cam.height, s.t.plan.ldsBytes, s.t.plan.tileListBytes);
  for (int k = 1; k < (int) s.h->num_instances; ++k) {
    if (s.inst[k].obj_type != QA_OBJ_MESH) continue;
    const DMesh &m = s.t.plan.meshes[s.inst[k].mesh];
    if (!m.useFast || !m.numLeaves) continue;
    const std::vector<DNode> &leaves = s.t.mesh[s.inst[k].mesh].leaves;
    const std::vector<int> chain = s.Chain(k);
    unsigned long long hist[QA_TILE_LEAF_CAP + 1] = {0}, tiles = 0, meet = 0, sumLeaves = 0, sumTris = 0;
    for (int Y0 = 0; Y0 < cam.height; Y0 += 8)
      for (int X0 = 0; X0 < cam.width; X0 += 8) {
        const TileList L = ListOf(s, k, chain, X0, Y0);
        ++tiles;
        float tLow;
        if (!tileConeMeetsBox(&L.cone, ld3(m.bmin), ld3(m.bmax), 0.f, &tLow)) continue;
        ++meet;
        const int n = __builtin_popcountll(L.mask);
        hist[n]++;
        sumLeaves += (unsigned long long) n;
        for (size_t i = 0; i < leaves.size(); ++i)
          if ((L.mask >> i) & 1ull) sumTris += ((leaves[i].data >> QA_BVH_COUNT_SHIFT) & QA_BVH_COUNT_MASK) + 1;
      }
    printf("node %d: %u triangles in %u leaves; %llu of %llu tiles meet the mesh bounds; listed per such tile: %.2f leaves, %.2f triangles\n", k, m.num_faces,
           m.numLeaves, meet, tiles, (double) sumLeaves / (double) std::max(meet, 1ull), (double) sumTris / (double) std::max(meet, 1ull));
    unsigned long long cum = 0;
    for (int n = 0; n <= QA_TILE_LEAF_CAP; ++n) {
      if (!hist[n]) continue;
      cum += hist[n];
      printf("  %2d leaves: %7llu tiles  (%5.1f %%, cumulative %5.1f %%)\n", n, hist[n], 100.0 * hist[n] / meet, 100.0 * cum / meet);
    }
  }
  return 0;
}

int main(int argc, char **argv)
{
  int rc = 0;
  if (argc >= 3 && !strcmp(argv[1], "rays"))
    for (int i = 2; i < argc; ++i) rc |= Rays(argv[i]);
  else if (argc == 3 && !strcmp(argv[1], "hist"))
    rc = Hist(argv[2]);
  else if (argc == 3 && !strcmp(argv[1], "leaves")) {   // the leaf tables themselves
    Scene s;
    if (!s.Load(argv[2])) return 1;
    for (size_t mi = 0; mi < s.t.mesh.size(); ++mi)
      for (const DNode &l : s.t.mesh[mi].leaves)
        printf("mesh %zu leaf %08x box %g %g %g  %g %g %g\n", mi, l.data, (double) l.box[0], (double) l.box[1], (double) l.box[2], (double) l.box[3], (double) l.box[4], (double) l.box[5]);
  }
  else {
    printf("usage: tile_cull_check rays <blob>... | hist <blob> | leaves <blob>\n");
    return 2;
  }
  printf(rc ? "tile_cull_check: FAILED\n" : "tile_cull_check: clean\n");
  return rc;
}
