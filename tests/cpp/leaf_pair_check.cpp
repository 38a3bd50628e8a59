// Host model of the two triangle phases of the leaf sweep of qa_integrate_lastcast's bounce rays (qa_kernel.h sweepLeaves; built by
// tests/test_leaf_pair_host.py with -fsanitize=address,undefined, no GPU):
//   leaf_pair_check rays <rays per tile> <blob>...
//     the rays of last_cast_check.cpp (random sub-pixel camera rays per 8x8 tile, one cosine-distributed bounce ray from every hit).
//     Every bounce ray is put to every mesh node that the query would ask (no glow node), at the limit the query would ask it with,
//     and - where the ray is accepted - once more at exactly the accepted distance (the limit at which that triangle is a tie).  For
//     a mesh that blocksMesh sweeps, the box phase gives the lane's candidates, and the candidates go through
//       single    one triangle per turn: the leaf word of the sorted table, first and count from it, a return from the inner loop
//                 (the sweep as commit 55d1672's parent had it: the specification)
//       pair      one leaf per turn: first and count from the byte table (qa_scene_build.cpp LeafPairBytes), both records tested
//                 against the same limit, then the selection; a leaf of one triangle reads its one record twice
//     and the two must give the same hit, best, tie and hz.  Every record index the pair form reads is checked against the mesh's
//     record count.  Before the rays, per mesh: the byte table the builder put behind the sorted copy (SceneTables::image at
//     resLeaves + 4 * numLeaves) must decode to every sorted leaf's first and count, DMesh::leafPairs must say so, and a mesh
//     without a table to sweep must have neither.
//     Per blob one line of counts; exit code 1 on any difference.
//   leaf_pair_check bytes
//     LeafPairBytes on tables made here: a leaf of three triangles, a leaf that starts at 128, 64 leaves, 65 leaves, none.
#include <algorithm>
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

// the triangle test, the slab forms and the scene model of the last-cast check, as they stand there (its main() becomes lcc::main)
namespace lcc {
#include "last_cast_check.cpp"
}
using namespace lcc;

static bool Sweeps(const DMesh &m) { return m.useFast && m.numLeaves >= 2 && m.numLeaves <= QA_TILE_LEAF_CAP; }

struct Found {
  bool hit = false, tie = false;
  uint32_t best = 0;
  float hz = 0;
  bool operator==(const Found &o) const { return hit == o.hit && tie == o.tie && best == o.best && memcmp(&hz, &o.hz, 4) == 0; }
};

// box phase of sweepLeaves on the sorted table -> the lane's candidates, bit j = leaf j
static unsigned long long Candidates(const DMesh &m, const MeshTables &mt, const Ray &ray, f3 drcp, bool fastSlab, float pad, float limit)
{
  const f3 pLo = ray.p + F3(pad, pad, pad), pHi = ray.p - F3(pad, pad, pad);
  const f3 cLo = slabRayTerm(pLo, drcp), cHi = slabRayTerm(pHi, drcp);
  unsigned long long mask = 0;
  for (uint32_t j = 0; j < m.numLeaves; ++j) {
    const DNode &n = mt.sweepLeaves[j];
    float entry, exit_;
    if (fastSlab) boxEntryExitPadFma(cLo, cHi, drcp, ld3(n.box), ld3(n.box + 3), entry, exit_);
    else boxEntryExitPad(pLo, pHi, ray.d, drcp, ld3(n.box), ld3(n.box + 3), entry, exit_);
    if (entry <= limit && entry <= exit_) mask |= 1ull << j;
  }
  return mask;
}

// the loop of sweepLeaves as commit 55d1672's parent had it: while (lo | hi) around for (i < count), a return from the inner one
static Found Single(const MeshTables &mt, unsigned long long cand, const Ray &ray, float limit, unsigned long long &turns)
{
  Found f;
  f.hz = limit;
  for (; cand; cand &= cand - 1) {
    const uint32_t j = (uint32_t) __builtin_ctzll(cand);
    const uint32_t word = mt.sweepLeaves[j].data;
    const uint32_t count = ((word >> QA_BVH_COUNT_SHIFT) & QA_BVH_COUNT_MASK) + 1, first = word & QA_BVH_OFFSET_MASK;
    for (uint32_t i = 0; i < count; ++i) {
      ++turns;
      const DTri &t = mt.ftris.at(first + i);
      if (TriangleZTie(t, ray, f.hz, f.tie)) {
        f.best = t.axis >> 2;
        f.hit = true;
        return f;
      }
    }
  }
  return f;
}

// the loop of sweepLeaves: one leaf per turn, its byte, both records, one selection
static Found Pair(const MeshTables &mt, const unsigned char *bytes, unsigned long long cand, const Ray &ray, float limit, unsigned long long &turns,
                  unsigned long long &outside)
{
  Found f;
  f.hz = limit;
  while (cand && !f.hit) {
    ++turns;
    const uint32_t j = (uint32_t) __builtin_ctzll(cand);
    cand &= cand - 1;
    const uint32_t byte = bytes[j];
    const uint32_t i1 = byte & 127u, i2 = i1 + (byte >> 7);
    if (i1 >= mt.ftris.size() || i2 >= mt.ftris.size()) { ++outside; return f; }
    const DTri &t = mt.ftris[i1], &u = mt.ftris[i2];
    float h1 = f.hz, h2 = f.hz;
    bool tie1 = false, tie2 = false;
    const bool ok1 = TriangleZTie(t, ray, h1, tie1);
    const bool ok2 = TriangleZTie(u, ray, h2, tie2);
    f.tie = f.tie || tie1 || (!ok1 && tie2);
    f.hit = ok1 || ok2;
    if (f.hit) {
      f.best = (ok1 ? t.axis : u.axis) >> 2;
      f.hz = ok1 ? h1 : h2;
    }
  }
  return f;
}

struct Counts {
  unsigned long long meshes = 0, tables = 0, noTable = 0, oneTriLeaves = 0, lastRecordLeaves = 0, tableErrors = 0;
  unsigned long long camRays = 0, bounce = 0, queries = 0, walked = 0, atTie = 0, hits = 0, ties = 0, second = 0, secondTieMasked = 0, oneTriTurns = 0;
  unsigned long long singleTurns = 0, pairTurns = 0, outside = 0, mismatches = 0;
};

// the byte table of every mesh as the builder left it
static void CheckTables(const Scene &s, Counts &c)
{
  for (size_t mi = 0; mi < s.t.plan.meshes.size(); ++mi) {
    const DMesh &m = s.t.plan.meshes[mi];
    const MeshTables &mt = s.t.mesh[mi];
    ++c.meshes;
    if (!m.numLeaves) {
      ++c.noTable;
      if (m.leafPairs) { ++c.tableErrors; printf("  mesh %zu: no leaf table, but leafPairs is set\n", mi); }
      continue;
    }
    unsigned char want[QA_TILE_LEAF_CAP];
    const bool fits = LeafPairBytes(mt.sweepLeaves, want);
    const size_t at = (size_t) m.resLeaves + 4 * (size_t) m.numLeaves;
    if ((m.leafPairs != 0) != fits || mt.sweepLeaves.size() != m.numLeaves || at + QA_TILE_LEAF_CAP / 16 > s.t.image.size()) {
      ++c.tableErrors;
      printf("  mesh %zu: leafPairs %u, the bytes fit %d, %zu sorted leaves of %u, image of %zu\n", mi, m.leafPairs, (int) fits, mt.sweepLeaves.size(), m.numLeaves, s.t.image.size());
      continue;
    }
    const unsigned char *bytes = reinterpret_cast<const unsigned char *>(s.t.image.data() + at);
    if (memcmp(bytes, want, QA_TILE_LEAF_CAP)) { ++c.tableErrors; printf("  mesh %zu: the image's bytes are not LeafPairBytes'\n", mi); }
    if (!fits) continue;
    ++c.tables;
    for (uint32_t j = 0; j < m.numLeaves; ++j) {
      const uint32_t word = mt.sweepLeaves[j].data;
      const uint32_t count = ((word >> QA_BVH_COUNT_SHIFT) & QA_BVH_COUNT_MASK) + 1, first = word & QA_BVH_OFFSET_MASK;
      if ((bytes[j] & 127u) != first || (bytes[j] >> 7) + 1u != count || first + count > mt.ftris.size()) {
        ++c.tableErrors;
        printf("  mesh %zu leaf %u: byte %u, first %u count %u of %zu records\n", mi, j, bytes[j], first, count, mt.ftris.size());
      }
      c.oneTriLeaves += count == 1;
      c.lastRecordLeaves += first + count == mt.ftris.size();
    }
    for (uint32_t j = m.numLeaves; j < QA_TILE_LEAF_CAP; ++j) c.tableErrors += bytes[j] != 0;
  }
}

static void Ask(const Scene &s, int mi, const Ray &ray, float limit, bool again, Counts &c)
{
  const DMesh &m = s.t.plan.meshes[mi];
  const MeshTables &mt = s.t.mesh[mi];
  if (!Sweeps(m) || !m.leafPairs) { ++c.walked; return; }   // (the walk: nothing of this check's)
  const f3 drcp = F3(1.f / ray.d.x, 1.f / ray.d.y, 1.f / ray.d.z);
  const bool fastSlab = !(qabs(ray.d.x) < 1e-7f || qabs(ray.d.y) < 1e-7f || qabs(ray.d.z) < 1e-7f);
  const float oMax = qmax(qmax(qabs(ray.p.x), qabs(ray.p.y)), qabs(ray.p.z));
  const float pad = fastWalkPad(m.invH, m.absMax, oMax);
  const unsigned long long cand = Candidates(m, mt, ray, drcp, fastSlab, pad, limit);
  const unsigned char *bytes = reinterpret_cast<const unsigned char *>(s.t.image.data() + (size_t) m.resLeaves + 4 * (size_t) m.numLeaves);
  ++c.queries;
  const Found a = Single(mt, cand, ray, limit, c.singleTurns);
  const Found b = Pair(mt, bytes, cand, ray, limit, c.pairTurns, c.outside);
  if (!(a == b) && c.mismatches++ < 5)
    printf("  mismatch: mesh %d limit %.9g candidates %llx: single hit %d best %u tie %d hz %.9g, pair hit %d best %u tie %d hz %.9g\n", mi, limit, cand,
           (int) a.hit, a.best, (int) a.tie, a.hz, (int) b.hit, b.best, (int) b.tie, b.hz);
  c.hits += a.hit;
  c.ties += a.tie;
  // which cases the rays met: the accepted triangle is its leaf's second; that leaf's second is a tie the first's acceptance hides
  for (unsigned long long rest = cand; rest; rest &= rest - 1) {
    const uint32_t byte = bytes[__builtin_ctzll(rest)];
    const DTri &t = mt.ftris[byte & 127u], &u = mt.ftris[(byte & 127u) + (byte >> 7)];
    float h1 = limit, h2 = limit;
    bool tie1 = false, tie2 = false;
    const bool ok1 = TriangleZTie(t, ray, h1, tie1), ok2 = TriangleZTie(u, ray, h2, tie2);
    c.oneTriTurns += !(byte >> 7);
    if (ok1 || ok2) {
      c.second += !ok1 && (byte >> 7);
      c.secondTieMasked += ok1 && tie2 && !tie1 && (byte >> 7);
      break;
    }
  }
  if (a.hit && !again) {
    ++c.atTie;
    Ask(s, mi, ray, a.hz, true, c);   // the accepted triangle at exactly the limit: a tie, and the sweep goes on behind it
  }
}

static int PairRaysOf(const char *path, int raysPerTile)
{
  Model M;
  if (!M.Load(path)) return 1;
  const Scene &s = M.s;
  const ScenePlan &plan = s.t.plan;
  if (!plan.lastCastQuery) { printf("%s: the plan has no lastCastQuery\n", path); return 1; }
  Counts c;
  CheckTables(s, c);
  const DCamera &cam = s.t.ds.cam;
  const int W = cam.width, H = cam.height;
  const uint32_t glow = plan.lastCastGlow;
  for (int Y0 = 0; Y0 < H; Y0 += 8)
    for (int X0 = 0; X0 < W; X0 += 8)
      for (int r = 0; r < raysPerTile; ++r) {
        const int px = X0 + (int) (g_rng % (unsigned) std::min(8, W - X0)), py = Y0 + (int) ((g_rng >> 8) % (unsigned) std::min(8, H - Y0));
        const f3 texpos = F3(Rnd(), Rnd(), 0.f) + F3((float) px, (float) py, 0.f);
        const f3 cpt = (ld3(cam.screenA) + ld3(cam.screenU) * texpos.x) + ld3(cam.screenV) * texpos.y;
        Ray world;
        world.p = ld3(cam.pos);
        world.d = normalize(cpt - world.p);
        ++c.camRays;
        const Model::Closest h = M.RefSweep(world);
        if (h.node < 0) continue;
        // the hit and its geometric normal in world space (Node::FromNodeCoords up the chain), the normal turned against the ray
        f3 p = h.local.p + h.local.d * h.z, N;
        const int type = s.inst[h.node].obj_type;
        if (type == QA_OBJ_SPHERE) N = normalize(p);
        else if (type == QA_OBJ_PLANE) N = F3(0, 0, 1);
        else N = ld3(s.t.mesh[s.inst[h.node].mesh].tris[h.elem].N);
        if (dot(N, h.local.d) > 0) N = -N;
        for (int a = h.node; a >= 0; a = s.inst[a].parent) {
          if (a == 0 && s.t.ds.rootIdentity) break;
          p = mulMV(s.inst[a].tm, p) + ld3(s.inst[a].pos);
          N = normalize(mulTMV(s.inst[a].itm, N));
        }
        const f3 ax = qabs(N.x) < 0.5f ? F3(1, 0, 0) : F3(0, 1, 0);
        const f3 u = normalize(cross(ax, N)), v = cross(N, u);
        const float r1 = Rnd(), phi = 2.f * QA_PI * Rnd(), rad = qsqrt(r1);
        Ray b;
        b.p = p;
        b.d = normalize((u * (rad * cosf(phi)) + v * (rad * sinf(phi))) + N * qsqrt(qmax(0.f, 1.f - r1)));
        ++c.bounce;
        // lastCastQuery's limits: the glow nodes first, then every other mesh node at its limit
        const Ray r0 = M.RootRay(b);
        float tG = QA_BIGFLOAT;
        int G = -1;
        for (int k = 1; k < (int) s.h->num_instances && k < 32; ++k) {
          if (!((glow >> k) & 1u)) continue;
          const Ray lr = M.Local(k, r0);
          if (s.inst[k].obj_type == QA_OBJ_SPHERE ? SphereZ(lr, tG) : PlaneZ(lr, tG)) G = k;
        }
        uint32_t up;
        memcpy(&up, &tG, 4);
        ++up;
        float tGup;
        memcpy(&tGup, &up, 4);
        for (int k = 1; k < (int) s.h->num_instances; ++k) {
          if (k < 32 && ((glow >> k) & 1u)) continue;
          if (s.inst[k].obj_type != QA_OBJ_MESH) continue;
          const DMesh &m = plan.meshes[s.inst[k].mesh];
          if (m.num_faces == 0 || !m.useFast) continue;
          Ask(s, s.inst[k].mesh, M.Local(k, r0), G < 0 ? QA_BIGFLOAT : (k < G ? tGup : tG), false, c);
        }
      }
  const bool bad = c.mismatches || c.outside || c.tableErrors;
  printf("%s frame=%dx%d meshes=%llu tables=%llu noTable=%llu oneTriLeaves=%llu lastRecordLeaves=%llu tableErrors=%llu cameraRays=%llu bounce=%llu queries=%llu walked=%llu atTie=%llu "
         "hits=%llu ties=%llu second=%llu secondTieMasked=%llu oneTriTurns=%llu singleTurns=%llu pairTurns=%llu outside=%llu mismatches=%llu\n",
         path, W, H, c.meshes, c.tables, c.noTable, c.oneTriLeaves, c.lastRecordLeaves, c.tableErrors, c.camRays, c.bounce, c.queries, c.walked, c.atTie, c.hits, c.ties, c.second,
         c.secondTieMasked, c.oneTriTurns, c.singleTurns, c.pairTurns, c.outside, c.mismatches);
  return bad ? 1 : 0;
}

// LeafPairBytes on tables made here
static int ByteTables()
{
  auto leaf = [](uint32_t first, uint32_t count) {
    DNode n{};
    n.data = (first & QA_BVH_OFFSET_MASK) | ((count - 1) << QA_BVH_COUNT_SHIFT) | QA_BVH_LEAF_BIT;
    return n;
  };
  int bad = 0;
  unsigned char b[QA_TILE_LEAF_CAP];
  auto zero = [&] { return std::all_of(b, b + QA_TILE_LEAF_CAP, [](unsigned char x) { return x == 0; }); };
  auto expect = [&](const char *what, bool ok) {
    printf("  %-44s %s\n", what, ok ? "ok" : "WRONG");
    bad += !ok;
  };
  std::vector<DNode> t = {leaf(4, 2), leaf(0, 1), leaf(126, 2), leaf(127, 1)};
  expect("two, one, the last pair, the last record", LeafPairBytes(t, b) && b[0] == (4 | 128) && b[1] == 0 && b[2] == (126 | 128) && b[3] == 127 && b[4] == 0);
  t = {leaf(0, 2), leaf(2, 3)};
  expect("a leaf of three triangles: no table", !LeafPairBytes(t, b) && zero());
  t = {leaf(0, 2), leaf(128, 1)};
  expect("a leaf that starts at record 128: no table", !LeafPairBytes(t, b) && zero());
  t.clear();
  for (uint32_t j = 0; j < QA_TILE_LEAF_CAP; ++j) t.push_back(leaf(2 * (QA_TILE_LEAF_CAP - 1 - j), j & 1 ? 1 : 2));
  bool ok = LeafPairBytes(t, b);
  for (uint32_t j = 0; ok && j < QA_TILE_LEAF_CAP; ++j) ok = b[j] == ((2 * (QA_TILE_LEAF_CAP - 1 - j)) | (j & 1 ? 0u : 128u));
  expect("64 leaves: every byte", ok);
  t.push_back(leaf(1, 1));
  expect("65 leaves: no table", !LeafPairBytes(t, b) && zero());
  t.clear();
  expect("no leaves: no table", !LeafPairBytes(t, b) && zero());
  return bad ? 1 : 0;
}

int main(int argc, char **argv)
{
  int rc = 0;
  if (argc == 2 && !strcmp(argv[1], "bytes")) rc = ByteTables();
  else if (argc >= 4 && !strcmp(argv[1], "rays") && atoi(argv[2]) >= 1)
    for (int i = 3; i < argc; ++i) rc |= PairRaysOf(argv[i], atoi(argv[2]));
  else {
    printf("usage: leaf_pair_check rays <rays per tile> <blob>... | leaf_pair_check bytes\n");
    return 2;
  }
  printf(rc ? "leaf_pair_check: FAILED\n" : "leaf_pair_check: clean\n");
  return rc;
}
