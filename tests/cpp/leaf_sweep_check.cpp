// Host model of the leaf sweep of qa_integrate_lastcast's bounce rays (qa_kernel.h sweepLeaves, used by blocksMesh; built by
// tests/test_leaf_sweep_host.py with -fsanitize=address,undefined, no GPU):
//   leaf_sweep_check rays <rays per tile> <fast|slow> <blob>...
//     the rays of last_cast_check.cpp (random sub-pixel camera rays per 8x8 tile, one cosine-distributed bounce ray from every hit).
//     Every bounce ray is answered by the reference's closest-hit sweep, by the query with the any-hit walk of the own tree (what
//     the kernel did before) and by the query with the leaf sweep - once for every order in which a lane may take its candidates
//     and for both rules after a found triangle whose leaf the reference does not reach:
//       table     the leaf table's order
//       area      the leaves by descending half-area of their stored boxes (the table's order among equals): MeshTables::sweepLeaves,
//                 the copy of the table that the kernel sweeps
//       nearest   by entry distance (the table's order among equals)
//       +go-on    the lane goes on with its remaining candidates instead of asking again
//     and each answer that is not "ask again" must be the reference's.  slow: every ray takes the exact slab form (boxEntryExitPad),
//     as the lanes of a wave do in which one ray has a direction component below 1e-7.
//     Per blob: the outcome line of the shipped form (area order, ask again), and per form the mean and the per-tile envelope (the
//     largest count among a tile's bounce rays: lanes of one wave work until the last of them is done) of box tests and triangle
//     tests, the rays that ask again, and the estimate of issued instructions per wave and query from the envelope.
//     Exit code 1 on a mismatch of any form.
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

// the query, the reference's sweep and the ray generator of the last-cast check, as they stand there (its main() becomes lcc::main)
namespace lcc {
#include "last_cast_check.cpp"
}
using namespace lcc;

enum Order { kTable = 0, kArea, kNearest, kOrders };
static const char *const kOrderName[kOrders] = {"table", "area", "nearest"};

// estimate of issued vector instructions: a pair step of the walk with its hit selection and stack traffic, a swept leaf, a triangle test
static const double kStepCost = 40, kSweptLeafCost = 17, kTriCost = 30;

struct Sweep {
  unsigned long long boxes = 0, tris = 0;
};

// May blocksMesh sweep this mesh's leaf table?  (a tree that is a single leaf has no box to test: it keeps the walk)
static bool Sweeps(const DMesh &m) { return m.useFast && m.numLeaves >= 2 && m.numLeaves <= QA_TILE_LEAF_CAP; }

// sweepLeaves: the box phase over the whole table, then the lane's candidates one by one until a triangle is accepted.
// -> accepted; best = element | reference leaf << 15.  goOn: the caller's test of the found triangle, asked per triangle here
template <class Reached>
static bool SweepLeaves(const DMesh &m, const MeshTables &mt, const Ray &ray, f3 drcp, bool fastSlab, float pad, float limit, Order order, bool goOn,
                        const Reached &reached, uint32_t &best, bool &tie, Sweep &st)
{
  const f3 pLo = ray.p + F3(pad, pad, pad), pHi = ray.p - F3(pad, pad, pad);
  const f3 cLo = slabRayTerm(pLo, drcp), cHi = slabRayTerm(pHi, drcp);
  const std::vector<DNode> &leaves = order == kArea ? mt.sweepLeaves : mt.leaves;   // (area: the table the host sorted, in its order)
  std::vector<std::pair<float, uint32_t>> cand;   // (sort key, leaf)
  for (uint32_t j = 0; j < m.numLeaves; ++j) {
    ++st.boxes;
    float entry, exit_;
    if (fastSlab) boxEntryExitPadFma(cLo, cHi, drcp, ld3(leaves[j].box), ld3(leaves[j].box + 3), entry, exit_);
    else boxEntryExitPad(pLo, pHi, ray.d, drcp, ld3(leaves[j].box), ld3(leaves[j].box + 3), entry, exit_);
    if (!(entry <= limit && entry <= exit_)) continue;
    const float key = order == kNearest ? entry : 0.f;
    cand.push_back({key, j});
  }
  std::stable_sort(cand.begin(), cand.end(), [](const std::pair<float, uint32_t> &a, const std::pair<float, uint32_t> &b) { return a.first < b.first; });
  bool found = false;
  for (const auto &c : cand) {
    const uint32_t word = leaves[c.second].data;
    const uint32_t count = ((word >> QA_BVH_COUNT_SHIFT) & QA_BVH_COUNT_MASK) + 1, first = word & QA_BVH_OFFSET_MASK;
    for (uint32_t i = 0; i < count; ++i) {
      ++st.tris;
      float hz = limit;
      if (TriangleZTie(mt.ftris[first + i], ray, hz, tie)) {
        best = mt.ftris[first + i].axis >> 2;
        found = true;
        if (!goOn || reached(best)) return true;
      }
    }
  }
  return found;   // (goOn: the last accepted triangle, which the reference does not reach)
}

struct SweepModel {
  const Model &M;
  bool slow;
  unsigned long long swept = 0, walked = 0, refWalks = 0;   // meshes answered by the sweep | by the walk | untrusted misses walked again in place

  // blocksMesh with the sweep where the mesh allows it
  bool BlocksMesh(const DMesh &m, const MeshTables &mt, const Ray &ray, float limit, Order order, bool goOn, int &again, Sweep &st)
  {
    const f3 drcp = F3(1.f / ray.d.x, 1.f / ray.d.y, 1.f / ray.d.z);
    const bool fastSlab = !slow && !(qabs(ray.d.x) < 1e-7f || qabs(ray.d.y) < 1e-7f || qabs(ray.d.z) < 1e-7f);
    const float mb[6] = {m.bmin[0], m.bmin[1], m.bmin[2], m.bmax[0], m.bmax[1], m.bmax[2]};
    float entry, meshExit;
    RefBox(ray, drcp, mb, entry, meshExit);
    if (entry > meshExit) return false;
    const bool gate = !(entry > limit);
    if (m.num_faces == 0) return false;
    if (!m.useFast) { again = kNoOwnTree; return false; }
    const float oMax = qmax(qmax(qabs(ray.p.x), qabs(ray.p.y)), qabs(ray.p.z));
    const float pad = fastWalkPad(m.invH, m.absMax, oMax);
    uint32_t bestF = 0;
    bool tie = false, hit;
    auto reached = [&](uint32_t best) {
      const uint32_t leaf = best >> 15;
      if (!gate) return false;
      if (leaf <= 1) return true;
      float e, x;
      RefBox(ray, drcp, mt.nodes[leaf].box, e, x);
      return refLeafReached(e, x, limit, false);
    };
    if (Sweeps(m)) {
      ++swept;
      hit = SweepLeaves(m, mt, ray, drcp, fastSlab, pad, limit, order, goOn, reached, bestF, tie, st);
    } else {
      ++walked;
      Steps ws;
      float hz = limit;
      hit = FastWalk(mt, m.frootData, ray, drcp, fastSlab, pad, hz, false, bestF, tie, ws);
      st.boxes += 2 * ws.nodes;
      st.tris += ws.tris;
    }
    if (tie) { again = kTie; return false; }
    if (!hit) {
      if (limit > meshExit) {
        const float theta = ((QA_SLACK_SCALE * 1.8e-5f) * m.invH) * (oMax + m.absMax) + QA_SLACK_SCALE * 2e-5f;
        const float lim = (theta * theta) * dot(ray.d, ray.d);
        bool parallel = mt.normals.empty();
        for (size_t i = 0; i + 3 < mt.normals.size(); i += 4) {
          const float dn = __builtin_fmaf(ray.d.x, mt.normals[i], __builtin_fmaf(ray.d.y, mt.normals[i + 1], ray.d.z * mt.normals[i + 2]));
          parallel = parallel || (dn * dn <= lim);
        }
        if (parallel) {
          ++refWalks;
          uint32_t e = 0;
          float hz = limit;
          return RefWalkAny(mt, ray, drcp, hz, e);
        }
      }
      return false;
    }
    if (!reached(bestF)) { again = kLeaf; return false; }
    return true;
  }

  // lastCastQuery -> 0, or why the lane asks again
  int Query(const Ray &world, uint32_t glow, Order order, bool goOn, Answer &a, bool &glowHit, Sweep &st)
  {
    const Scene &s = M.s;
    const Ray r0 = M.RootRay(world);
    float tG = QA_BIGFLOAT;
    int G = -1;
    for (int k = 1; k < (int) s.h->num_instances && k < 32; ++k) {
      if (!((glow >> k) & 1u)) continue;
      const Ray r = M.Local(k, r0);
      if (s.inst[k].obj_type == QA_OBJ_SPHERE ? SphereZ(r, tG) : PlaneZ(r, tG)) G = k;
    }
    uint32_t up;
    memcpy(&up, &tG, 4);
    ++up;
    float tGup;
    memcpy(&tGup, &up, 4);
    bool blocked = false;
    int again = 0;
    for (int k = 1; k < (int) s.h->num_instances && !blocked && !again; ++k) {
      if (k < 32 && ((glow >> k) & 1u)) continue;
      const int type = s.inst[k].obj_type;
      if (type == QA_OBJ_NONE) continue;
      const float limit = G < 0 ? QA_BIGFLOAT : (k < G ? tGup : tG);
      const Ray r = M.Local(k, r0);
      float z = limit;
      if (type == QA_OBJ_SPHERE) blocked = SphereZ(r, z);
      else if (type == QA_OBJ_PLANE) blocked = PlaneZ(r, z);
      else blocked = BlocksMesh(s.t.plan.meshes[s.inst[k].mesh], s.t.mesh[s.inst[k].mesh], r, limit, order, goOn, again, st);
    }
    a.drawn = blocked || G >= 0;
    a.emits = (!blocked && G >= 0) ? M.sets[s.inst[G].mtlset].first : -1;
    glowHit = !blocked && G >= 0;
    return again;
  }
};

struct Tally {
  unsigned long long boxes = 0, tris = 0, envBoxes = 0, envTris = 0, again = 0, mismatches = 0;
  unsigned long long tileBoxes = 0, tileTris = 0;
  void Ray(unsigned long long b, unsigned long long t)
  {
    boxes += b; tris += t;
    tileBoxes = std::max(tileBoxes, b); tileTris = std::max(tileTris, t);
  }
  void Tile() { envBoxes += tileBoxes; envTris += tileTris; tileBoxes = tileTris = 0; }
};

static int RaysOf(const char *path, int raysPerTile, bool slow)
{
  Model M;
  if (!M.Load(path)) return 1;
  const Scene &s = M.s;
  const ScenePlan &plan = s.t.plan;
  if (!plan.lastCastQuery) { printf("%s: the plan has no lastCastQuery\n", path); return 1; }
  const DCamera &cam = s.t.ds.cam;
  const int W = cam.width, H = cam.height;
  unsigned long long camRays = 0, bounce = 0, glowHits = 0, blockedRays = 0, escaped = 0, groups = 0, why[5] = {0};
  Tally walk, form[kOrders][2];
  SweepModel shipped{M, slow};
  SweepModel other{M, slow};
  unsigned sweptMeshes = 0, walkedMeshes = 0, leavesMax = 0;
  for (int k = 1; k < (int) s.h->num_instances; ++k)
    if (s.inst[k].obj_type == QA_OBJ_MESH) {
      const DMesh &m = plan.meshes[s.inst[k].mesh];
      (Sweeps(m) ? sweptMeshes : walkedMeshes) += 1;
      leavesMax = std::max(leavesMax, m.numLeaves);
    }
  for (int Y0 = 0; Y0 < H; Y0 += 8)
    for (int X0 = 0; X0 < W; X0 += 8) {
      bool some = false;
      for (int r = 0; r < raysPerTile; ++r) {
        const int px = X0 + (int) (g_rng % (unsigned) std::min(8, W - X0)), py = Y0 + (int) ((g_rng >> 8) % (unsigned) std::min(8, H - Y0));
        const f3 texpos = F3(Rnd(), Rnd(), 0.f) + F3((float) px, (float) py, 0.f);
        const f3 cpt = (ld3(cam.screenA) + ld3(cam.screenU) * texpos.x) + ld3(cam.screenV) * texpos.y;
        Ray world;
        world.p = ld3(cam.pos);
        world.d = normalize(cpt - world.p);
        ++camRays;
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
        if (slow && (bounce & 7u) == 0) (&b.d.x)[(bounce >> 3) % 3] = 0.f;   // the ray that makes its wave take the exact form
        ++bounce;
        some = true;
        const Answer ref = M.RefAnswer(b);
        // the walk (the fast form is the ray's own choice there: the model of the shipped kernel's cost)
        {
          Answer q;
          bool glowHit = false;
          Steps sa;
          const int asks = M.Query(b, plan.lastCastGlow, q, glowHit, sa);
          walk.Ray(sa.nodes, sa.tris);
          walk.again += asks ? 1 : 0;
          walk.mismatches += (!asks && !(q == ref)) ? 1 : 0;
        }
        for (int o = 0; o < kOrders; ++o)
          for (int go = 0; go < 2; ++go) {
            const bool isShipped = o == kArea && go == 0;
            SweepModel &sm = isShipped ? shipped : other;
            Answer q;
            bool glowHit = false;
            Sweep st;
            const int asks = sm.Query(b, plan.lastCastGlow, (Order) o, go != 0, q, glowHit, st);
            Tally &t = form[o][go];
            t.Ray(st.boxes, st.tris);
            t.again += asks ? 1 : 0;
            const bool wrong = !asks && !(q == ref);
            if (wrong && t.mismatches++ < 3)
              printf("  mismatch (%s%s): tile (%d, %d): the query says material %d drawn %d, the reference's sweep material %d drawn %d\n", kOrderName[o],
                     go ? "+go-on" : "", X0, Y0, q.emits, (int) q.drawn, ref.emits, (int) ref.drawn);
            if (isShipped) {
              if (asks) ++why[asks];
              else {
                glowHits += glowHit ? 1 : 0;
                blockedRays += (q.drawn && !glowHit) ? 1 : 0;
                escaped += q.drawn ? 0 : 1;
              }
            }
          }
      }
      if (some) {
        ++groups;
        walk.Tile();
        for (int o = 0; o < kOrders; ++o)
          for (int go = 0; go < 2; ++go) form[o][go].Tile();
      }
    }
  const double n = (double) std::max(bounce, 1ull), g = (double) std::max(groups, 1ull);
  unsigned long long mismatches = walk.mismatches, againMax = 0;
  for (int o = 0; o < kOrders; ++o)
    for (int go = 0; go < 2; ++go) { mismatches += form[o][go].mismatches; againMax = std::max(againMax, form[o][go].again); }
  const Tally &sh = form[kArea][0];
  printf("%s frame=%dx%d form=%s resident=%d sweptMeshes=%u walkedMeshes=%u leavesMax=%u cameraRays=%llu bounce=%llu swept=%llu walked=%llu glowHits=%llu blocked=%llu escaped=%llu again=%llu againTie=%llu againLeaf=%llu againNoOwnTree=%llu missRewalks=%llu againWalk=%llu againMax=%llu mismatches=%llu\n",
         path, W, H, slow ? "slow" : "fast", (int) plan.resident, sweptMeshes, walkedMeshes, leavesMax, camRays, bounce, shipped.swept, shipped.walked, glowHits, blockedRays, escaped, sh.again, why[kTie],
         why[kLeaf], why[kNoOwnTree], shipped.refWalks, walk.again, againMax, mismatches);
  // node visits of the walk: inner nodes (pair steps: two box tests, the choice, the stack) and leaves
  const double walkEst = kStepCost * (walk.envBoxes / g) + kTriCost * (walk.envTris / g);
  printf("  %-16s per ray %6.2f node visits %6.2f triangle tests | envelope of %d rays a tile (%llu tiles) %6.2f node visits %6.2f triangle tests | again %llu | estimate %7.0f\n",
         "walk", walk.boxes / n, walk.tris / n, raysPerTile, groups, walk.envBoxes / g, walk.envTris / g, walk.again, walkEst);
  for (int o = 0; o < kOrders; ++o)
    for (int go = 0; go < 2; ++go) {
      const Tally &t = form[o][go];
      const double est = kSweptLeafCost * (t.envBoxes / g) + kTriCost * (t.envTris / g);
      char name[32];
      snprintf(name, sizeof(name), "%s%s", kOrderName[o], go ? "+go-on" : "");
      printf("  %-16s per ray %6.2f box tests    %6.2f triangle tests | envelope of %d rays a tile (%llu tiles) %6.2f box tests    %6.2f triangle tests | again %llu | estimate %7.0f (%+.1f %%)\n",
             name, t.boxes / n, t.tris / n, raysPerTile, groups, t.envBoxes / g, t.envTris / g, t.again, est, 100.0 * (est - walkEst) / std::max(walkEst, 1.0));
    }
  return mismatches ? 1 : 0;
}

int main(int argc, char **argv)
{
  int rc = 0;
  if (argc >= 5 && !strcmp(argv[1], "rays") && atoi(argv[2]) >= 1 && (!strcmp(argv[3], "fast") || !strcmp(argv[3], "slow")))
    for (int i = 4; i < argc; ++i) rc |= RaysOf(argv[i], atoi(argv[2]), !strcmp(argv[3], "slow"));
  else {
    printf("usage: leaf_sweep_check rays <rays per tile> <fast|slow> <blob>...\n");
    return 2;
  }
  printf(rc ? "leaf_sweep_check: FAILED\n" : "leaf_sweep_check: clean\n");
  return rc;
}
