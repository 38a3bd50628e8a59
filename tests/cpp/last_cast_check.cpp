// Host model of the last-cast query of qa_integrate_lastcast (qa_kernel.h lastCastQuery / blocksMesh; built by
// tests/test_last_cast_host.py with -fsanitize=address,undefined, no GPU):
//   last_cast_check rays <rays per tile> <blob>...   for every 8x8 tile of the blob's frame: random sub-pixel camera rays, and from
//                                                    every hit (the reference's sweep over all nodes) one cosine-distributed
//                                                    bounce ray.  Every bounce ray is answered twice:
//       the reference's sweep  Scene::TraceNodeNormal restated: the nodes in pre-order, the intersectors against the distance held,
//                              a mesh by its bounds test and walkBVH<false> -> (the hit's material if it emits, else none; drawn)
//       the query              lastCastQuery restated: the glow nodes, then the any-hit sweep with the per-node limits on the own
//                              tree (walkBVH<true>, closest = false), the leaf test at the limit, the rule for misses
//     and the two must agree wherever the query does not answer "ask again".  Per blob: the share of rays with a glow hit, the
//     share that asks again, and node visits / triangle tests per ray of the closest-hit walk of the own tree (what a bounce ray
//     costs without the query) and of the query's any-hit walk - also as an envelope: per tile, the largest count among the
//     tile's bounce rays (lanes of one wave walk until the last of them is done).  Exit code 1 on a mismatch.
//   last_cast_check predicate <blob>                 ScenePlan::lastCastQuery and the glow mask of the built scene
#define main tile_cull_check_main   // the scene loader of the tile lists' check
#include "tile_cull_check.cpp"
#undef main

// (the inside test, the reference's slab interval and its walk as tests/cpp/reach_rule_check.cpp restates them)
#define QA_BIAS 0.005f   /* qa_kernel.h */

// hitTriangleZ (qa_kernel.h) on a DTri: accept / reject against the distance held, and the distance
static bool TriangleZ(const DTri &q, const Ray &ray, float &hz)
{
  const f3 N = ld3(q.N), A = ld3(q.A);
  const float dz = dot(ray.d, N);
  const float pz = dot(ray.p - A, N);
  const float t = -pz / dz;
  bool ok = !(qabs(dz) < 1e-7f) && !(t <= QA_BIAS) && (hz > t);
  const f3 p = ray.p + ray.d * t;
  const bool ax0 = (q.axis == 0), ax2 = (q.axis == 2);
  const float pu = ax0 ? p.y : p.x, pv = ax2 ? p.y : p.z;
  const float au = ax0 ? A.y : A.x, av = ax2 ? A.y : A.z;
  const float a = ((q.bu - pu) * (q.cv - pv) - (q.cu - pu) * (q.bv - pv)) * q.s;
  const float b = ((q.cu - pu) * (av - pv) - (au - pu) * (q.cv - pv)) * q.s;
  const float c = 1.f - a - b;
  ok = ok && !(a < 0 || b < 0 || c < 0);
  if (ok) hz = t;
  return ok;
}

// boxEntryExit / boxEntryExitFast (qa_kernel.h): the reference's slab interval; the two forms give the same values where the
// fast one runs
static void RefBox(const Ray &ray, f3 drcp, const float *box, float &entry, float &exit_)
{
  const f3 p0 = (-(ray.p - ld3(box))) * drcp;
  const f3 p1 = (-(ray.p - ld3(box + 3))) * drcp;
  f3 t0, t1;
  slab(ray.d.x, p0.x, p1.x, t0.x, t1.x);
  slab(ray.d.y, p0.y, p1.y, t0.y, t1.y);
  slab(ray.d.z, p0.z, p1.z, t0.z, t1.z);
  entry = qmax(t0.x, qmax(t0.y, t0.z));
  exit_ = qmin(t1.x, qmin(t1.y, t1.z));
}

// walkBVH<false> (TriObj::TraceBVHNode): near child first, far child stacked, strict tests, a leaf's triangles in element order
static bool RefWalk(const MeshTables &mt, const Ray &ray, f3 drcp, float &hz, uint32_t &best)
{
  std::vector<uint32_t> stack;
  bool hasHit = false;
  uint32_t cur = mt.nodes[1].data;
  for (;;) {
    while (!(cur & QA_BVH_LEAF_BIT)) {
      const DNode &n0 = mt.nodes[cur & QA_BVH_CHILD_MASK], &n1 = mt.nodes[(cur & QA_BVH_CHILD_MASK) + 1];
      float entry0, exit0, entry1, exit1;
      RefBox(ray, drcp, n0.box, entry0, exit0);
      RefBox(ray, drcp, n1.box, entry1, exit1);
      const bool hit0 = entry0 < hz && entry0 < exit0, hit1 = entry1 < hz && entry1 < exit1;
      if (hit0 && hit1) {
        const bool nearFirst = entry0 < entry1;
        stack.push_back(nearFirst ? n1.data : n0.data);
        cur = nearFirst ? n0.data : n1.data;
      } else if (hit0) cur = n0.data;
      else if (hit1) cur = n1.data;
      else if (!stack.empty()) { cur = stack.back(); stack.pop_back(); }
      else return hasHit;
    }
    const uint32_t count = ((cur >> QA_BVH_COUNT_SHIFT) & QA_BVH_COUNT_MASK) + 1, first = cur & QA_BVH_OFFSET_MASK;
    for (uint32_t i = 0; i < count; ++i)
      if (TriangleZ(mt.tris[first + i], ray, hz)) { hasHit = true; best = first + i; }
    if (stack.empty()) return hasHit;
    cur = stack.back();
    stack.pop_back();
  }
}


// the same walk with closest = false: it ends at the first accepted triangle
static bool RefWalkAny(const MeshTables &mt, const Ray &ray, f3 drcp, float &hz, uint32_t &best)
{
  std::vector<uint32_t> stack;
  bool hasHit = false;
  uint32_t cur = mt.nodes[1].data;
  for (;;) {
    while (!(cur & QA_BVH_LEAF_BIT)) {
      const DNode &n0 = mt.nodes[cur & QA_BVH_CHILD_MASK], &n1 = mt.nodes[(cur & QA_BVH_CHILD_MASK) + 1];
      float entry0, exit0, entry1, exit1;
      RefBox(ray, drcp, n0.box, entry0, exit0);
      RefBox(ray, drcp, n1.box, entry1, exit1);
      const bool hit0 = entry0 < hz && entry0 < exit0, hit1 = entry1 < hz && entry1 < exit1;
      if (hit0 && hit1) {
        const bool nearFirst = entry0 < entry1;
        stack.push_back(nearFirst ? n1.data : n0.data);
        cur = nearFirst ? n0.data : n1.data;
      } else if (hit0) cur = n0.data;
      else if (hit1) cur = n1.data;
      else if (!stack.empty()) { cur = stack.back(); stack.pop_back(); }
      else return hasHit;
    }
    const uint32_t count = ((cur >> QA_BVH_COUNT_SHIFT) & QA_BVH_COUNT_MASK) + 1, first = cur & QA_BVH_OFFSET_MASK;
    for (uint32_t i = 0; i < count; ++i)
      if (TriangleZ(mt.tris[first + i], ray, hz)) { best = first + i; return true; }
    if (stack.empty()) return hasHit;
    cur = stack.back();
    stack.pop_back();
  }
}


// hitSphere / hitPlane (qa_kernel.h) with closest = false: accept against the distance held, and the distance
static bool SphereZ(const Ray &ray, float &hz)
{
  const float a = dot(ray.d, ray.d);
  const float b = 2.f * dot(ray.p, ray.d);
  const float c = dot(ray.p, ray.p) - 1;
  const float rcp2a = 1.f / (2.f * a);
  const float delta = b * b - 4 * a * c;
  float t = QA_BIGFLOAT;
  if (delta < 0) return false;
  if (delta == 0) {
    const float t0 = -b * rcp2a;
    if (t0 <= QA_BIAS) return false;
    t = t0;
  } else {
    const float sq = qsqrt(delta);
    const float t1 = (-b - sq) * rcp2a;
    const float t2 = (-b + sq) * rcp2a;
    if (t1 <= QA_BIAS && t2 <= QA_BIAS) return false;
    else if (t1 > QA_BIAS) t = qmin(t, t1);
    else if (t2 > QA_BIAS) t = qmin(t, t2);
  }
  if (hz > t) { hz = t; return true; }
  return false;
}
static bool PlaneZ(const Ray &ray, float &hz)
{
  const float dz = ray.d.z;
  if (qabs(dz) < 1e-7f) return false;
  const float t = -ray.p.z / dz;
  if (t <= QA_BIAS) return false;
  if (hz > t) {
    const f3 p = ray.p + ray.d * t;
    if (qabs(p.x) > 1.f || qabs(p.y) > 1.f) return false;
    hz = t;
    return true;
  }
  return false;
}

struct Steps { unsigned long long nodes = 0, tris = 0; };
enum Why { kNoOwnTree = 1, kTie, kMiss, kLeaf };   // why a query asks again (kMiss: it does not - that mesh is walked again in place)


// hitTriangleZTie<true> on a record of DMesh::ftris
static bool TriangleZTie(const DTri &q, const Ray &ray, float &hz, bool &tie)
{
  DTri plain = q;
  plain.axis = q.axis & 3u;
  float t = QA_BIGFLOAT;
  const bool inside = TriangleZ(plain, ray, t);   // against nothing held: the inside test alone, t = the distance
  const bool ok = inside && hz > t;
  tie = tie || (inside && hz == t);
  if (ok) hz = t;
  return ok;
}

// walkBVH<true> (the own tree: padded boxes, non-strict tests; the fma slab step where the ray allows the fast form)
static bool FastWalk(const MeshTables &mt, uint32_t rootData, const Ray &ray, f3 drcp, bool fastSlab, float pad, float &hz, bool closest,
                     uint32_t &best, bool &tie, Steps &st)
{
  f3 pLo = ray.p + F3(pad, pad, pad), pHi = ray.p - F3(pad, pad, pad);
  const f3 cLo = slabRayTerm(pLo, drcp), cHi = slabRayTerm(pHi, drcp);
  std::vector<uint32_t> stack;
  bool hasHit = false;
  uint32_t cur = rootData;
  for (;;) {
    while (!(cur & QA_BVH_LEAF_BIT)) {
      ++st.nodes;
      const DNode &n0 = mt.fnodes[cur & QA_BVH_CHILD_MASK], &n1 = mt.fnodes[(cur & QA_BVH_CHILD_MASK) + 1];
      float entry0, exit0, entry1, exit1;
      if (fastSlab) {
        boxEntryExitPadFma(cLo, cHi, drcp, ld3(n0.box), ld3(n0.box + 3), entry0, exit0);
        boxEntryExitPadFma(cLo, cHi, drcp, ld3(n1.box), ld3(n1.box + 3), entry1, exit1);
      } else {
        boxEntryExitPad(pLo, pHi, ray.d, drcp, ld3(n0.box), ld3(n0.box + 3), entry0, exit0);
        boxEntryExitPad(pLo, pHi, ray.d, drcp, ld3(n1.box), ld3(n1.box + 3), entry1, exit1);
      }
      const bool hit0 = entry0 <= hz && entry0 <= exit0, hit1 = entry1 <= hz && entry1 <= exit1;
      if (hit0 && hit1) {
        const bool nearFirst = entry0 < entry1;
        stack.push_back(nearFirst ? n1.data : n0.data);
        cur = nearFirst ? n0.data : n1.data;
      } else if (hit0) cur = n0.data;
      else if (hit1) cur = n1.data;
      else if (!stack.empty()) { cur = stack.back(); stack.pop_back(); }
      else return hasHit;
    }
    ++st.nodes;
    const uint32_t count = ((cur >> QA_BVH_COUNT_SHIFT) & QA_BVH_COUNT_MASK) + 1, first = cur & QA_BVH_OFFSET_MASK;
    for (uint32_t i = 0; i < count; ++i) {
      ++st.tris;
      if (TriangleZTie(mt.ftris[first + i], ray, hz, tie)) {
        hasHit = true;
        best = mt.ftris[first + i].axis >> 2;   // element | reference leaf << 15
        if (!closest) return true;
      }
    }
    if (stack.empty()) return hasHit;
    cur = stack.back();
    stack.pop_back();
  }
}

struct Answer {
  int emits = -1;      // the material that adds its emission, -1: none
  bool drawn = false;  // something is hit: RandomSelectMtl draws
  bool operator==(const Answer &o) const { return emits == o.emits && drawn == o.drawn; }
};

struct Model {
  Scene s;
  const qa_mtlset *sets = nullptr;
  const qa_material *mats = nullptr;
  std::vector<std::vector<int>> chain;
  bool Load(const char *path)
  {
    if (!s.Load(path)) return false;
    sets = QA_BLOB_PTR(qa_mtlset, s.blob.data(), s.h->off_mtlsets);
    mats = QA_BLOB_PTR(qa_material, s.blob.data(), s.h->off_materials);
    chain.resize(s.h->num_instances);
    for (int k = 1; k < (int) s.h->num_instances; ++k) {
      chain[k] = s.Chain(k);
      if (!s.t.ds.rootIdentity) chain[k].erase(chain[k].begin());   // (the root's level is rootRay's)
    }
    return true;
  }
  Ray RootRay(const Ray &world) const
  {
    if (!s.t.ds.rootIdentity) return toNode(s.inst[0], world);
    Ray o = world;
    o.d = (world.p + world.d) - world.p;
    return o;
  }
  Ray Local(int k, Ray r) const
  {
    for (int a : chain[k]) r = toNode(s.inst[a], r);
    return r;
  }
  bool Emits(int mi) const { const float *e = mats[mi].emission.color; return !(e[0] == 0.f && e[1] == 0.f && e[2] == 0.f); }
  // the material qa_integrate's section D shades the hit with (-1: none, -2: MultiMtl's white)
  int MaterialOf(int node, int mtlID) const
  {
    const qa_instance &in = s.inst[node];
    if (in.mtlset < 0) return -1;
    const qa_mtlset &ms = sets[in.mtlset];
    if (!ms.multi) return ms.first;
    return (mtlID >= 0 && mtlID < ms.count) ? ms.first + mtlID : -2;
  }

  // Scene::TraceNodeNormal: the closest hit over every node in pre-order (traceClosest on the reference's tree)
  struct Closest { int node = -1; uint32_t elem = 0; int mtlID = 0; float z = QA_BIGFLOAT; Ray local; };
  Closest RefSweep(const Ray &world) const
  {
    Closest h;
    const Ray r0 = RootRay(world);
    for (int k = 1; k < (int) s.h->num_instances; ++k) {
      const int type = s.inst[k].obj_type;
      if (type == QA_OBJ_NONE) continue;
      const Ray r = Local(k, r0);
      bool hit = false;
      uint32_t e = 0;
      if (type == QA_OBJ_SPHERE) hit = SphereZ(r, h.z);
      else if (type == QA_OBJ_PLANE) hit = PlaneZ(r, h.z);
      else {
        const DMesh &m = s.t.plan.meshes[s.inst[k].mesh];
        const MeshTables &mt = s.t.mesh[s.inst[k].mesh];
        const f3 drcp = F3(1.f / r.d.x, 1.f / r.d.y, 1.f / r.d.z);
        const float mb[6] = {m.bmin[0], m.bmin[1], m.bmin[2], m.bmax[0], m.bmax[1], m.bmax[2]};
        float entry, exit_;
        RefBox(r, drcp, mb, entry, exit_);
        if (entry > h.z || entry > exit_ || m.num_faces == 0) continue;
        hit = RefWalk(mt, r, drcp, h.z, e);
        if (hit) h.mtlID = mt.shade[e].mtl;
      }
      if (hit) { h.node = k; h.elem = e; h.local = r; }
    }
    return h;
  }
  Answer RefAnswer(const Ray &world) const
  {
    const Closest h = RefSweep(world);
    Answer a;
    if (h.node < 0) return a;
    const int mi = MaterialOf(h.node, h.mtlID);
    a.drawn = mi >= 0;
    a.emits = (mi >= 0 && Emits(mi)) ? mi : -1;
    return a;
  }

  // blocksMesh
  bool BlocksMesh(const DMesh &m, const MeshTables &mt, const Ray &ray, float limit, int &again, Steps &st) const
  {
    const f3 drcp = F3(1.f / ray.d.x, 1.f / ray.d.y, 1.f / ray.d.z);
    const bool fastSlab = !(qabs(ray.d.x) < 1e-7f || qabs(ray.d.y) < 1e-7f || qabs(ray.d.z) < 1e-7f);
    const float mb[6] = {m.bmin[0], m.bmin[1], m.bmin[2], m.bmax[0], m.bmax[1], m.bmax[2]};
    float entry, meshExit;
    RefBox(ray, drcp, mb, entry, meshExit);
    if (entry > meshExit) return false;
    const bool gate = !(entry > limit);
    if (m.num_faces == 0) return false;
    if (!m.useFast) { again = kNoOwnTree; return false; }
    const float oMax = qmax(qmax(qabs(ray.p.x), qabs(ray.p.y)), qabs(ray.p.z));
    const float pad = fastWalkPad(m.invH, m.absMax, oMax);
    float hz = limit;
    uint32_t bestF = 0;
    bool tie = false;
    const bool hit = FastWalk(mt, m.frootData, ray, drcp, fastSlab, pad, hz, false, bestF, tie, st);
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
        if (parallel) {   // the reference's tree at the fixed limit, as hitMesh walks it for such a miss
          again = kMiss;  // (counted, not asked again: Query)
          uint32_t e = 0;
          hz = limit;
          return RefWalkAny(mt, ray, drcp, hz, e);
        }
      }
      return false;
    }
    const uint32_t leaf = bestF >> 15;
    bool reached = true;
    if (leaf > 1) {
      float e, x;
      RefBox(ray, drcp, mt.nodes[leaf].box, e, x);
      reached = refLeafReached(e, x, limit, false);
    }
    if (!gate || !reached) { again = kLeaf; return false; }
    return true;
  }
  // lastCastQuery -> 0, or why the lane asks again
  mutable unsigned long long refWalks = 0;   // misses of an own tree that were not trusted: that mesh walked again on the reference's tree
  int Query(const Ray &world, uint32_t glow, Answer &a, bool &glowHit, Steps &st) const
  {
    const Ray r0 = RootRay(world);
    float tG = QA_BIGFLOAT;
    int G = -1;
    for (int k = 1; k < (int) s.h->num_instances && k < 32; ++k) {
      if (!((glow >> k) & 1u)) continue;
      const Ray r = Local(k, r0);
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
      const Ray r = Local(k, r0);
      float z = limit;
      if (type == QA_OBJ_SPHERE) blocked = SphereZ(r, z);
      else if (type == QA_OBJ_PLANE) blocked = PlaneZ(r, z);
      else {
        blocked = BlocksMesh(s.t.plan.meshes[s.inst[k].mesh], s.t.mesh[s.inst[k].mesh], r, limit, again, st);
        if (again == kMiss) { ++refWalks; again = 0; }
      }
    }
    a.drawn = blocked || G >= 0;
    a.emits = (!blocked && G >= 0) ? sets[s.inst[G].mtlset].first : -1;
    glowHit = !blocked && G >= 0;
    return again;
  }
  // what a bounce ray's closest-hit sweep costs on the own trees (traceClosest of the variant without the query)
  void ClosestCost(const Ray &world, Steps &st) const
  {
    const Ray r0 = RootRay(world);
    float hz = QA_BIGFLOAT;
    for (int k = 1; k < (int) s.h->num_instances; ++k) {
      const int type = s.inst[k].obj_type;
      if (type == QA_OBJ_NONE) continue;
      const Ray r = Local(k, r0);
      if (type == QA_OBJ_SPHERE) SphereZ(r, hz);
      else if (type == QA_OBJ_PLANE) PlaneZ(r, hz);
      else {
        const DMesh &m = s.t.plan.meshes[s.inst[k].mesh];
        const MeshTables &mt = s.t.mesh[s.inst[k].mesh];
        if (!m.useFast || m.num_faces == 0) continue;
        const f3 drcp = F3(1.f / r.d.x, 1.f / r.d.y, 1.f / r.d.z);
        const bool fastSlab = !(qabs(r.d.x) < 1e-7f || qabs(r.d.y) < 1e-7f || qabs(r.d.z) < 1e-7f);
        const float mb[6] = {m.bmin[0], m.bmin[1], m.bmin[2], m.bmax[0], m.bmax[1], m.bmax[2]};
        float entry, exit_;
        RefBox(r, drcp, mb, entry, exit_);
        if (entry > hz || entry > exit_) continue;
        const float oMax = qmax(qmax(qabs(r.p.x), qabs(r.p.y)), qabs(r.p.z));
        uint32_t best = 0;
        bool tie = false;
        FastWalk(mt, m.frootData, r, drcp, fastSlab, fastWalkPad(m.invH, m.absMax, oMax), hz, true, best, tie, st);
      }
    }
  }
};

static int RaysOf(const char *path, int raysPerTile)
{
  Model M;
  if (!M.Load(path)) return 1;
  const Scene &s = M.s;
  const ScenePlan &plan = s.t.plan;
  if (!plan.lastCastQuery) { printf("%s: the plan has no lastCastQuery\n", path); return 1; }
  const DCamera &cam = s.t.ds.cam;
  const int W = cam.width, H = cam.height;
  unsigned long long camRays = 0, bounce = 0, glowHits = 0, blockedRays = 0, escaped = 0, again = 0, mismatches = 0, groups = 0, why[5] = {0};
  Steps closest, anyhit, closestEnv, anyEnv;
  for (int Y0 = 0; Y0 < H; Y0 += 8)
    for (int X0 = 0; X0 < W; X0 += 8) {
      Steps cMax, aMax;
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
        ++bounce;
        some = true;
        const Answer ref = M.RefAnswer(b);
        Answer q;
        bool glowHit = false;
        Steps sa, sc;
        const int asks = M.Query(b, plan.lastCastGlow, q, glowHit, sa);
        M.ClosestCost(b, sc);
        anyhit.nodes += sa.nodes; anyhit.tris += sa.tris;
        closest.nodes += sc.nodes; closest.tris += sc.tris;
        cMax.nodes = std::max(cMax.nodes, sc.nodes); cMax.tris = std::max(cMax.tris, sc.tris);
        aMax.nodes = std::max(aMax.nodes, sa.nodes); aMax.tris = std::max(aMax.tris, sa.tris);
        if (asks) { ++again; ++why[asks]; continue; }
        glowHits += glowHit ? 1 : 0;
        blockedRays += (q.drawn && !glowHit) ? 1 : 0;
        escaped += q.drawn ? 0 : 1;
        if (!(q == ref)) {
          if (mismatches++ < 5)
            printf("  mismatch: tile (%d, %d): the query says material %d drawn %d, the reference's sweep material %d drawn %d\n", X0, Y0, q.emits, (int) q.drawn,
                   ref.emits, (int) ref.drawn);
        }
      }
      if (some) {
        ++groups;
        closestEnv.nodes += cMax.nodes; closestEnv.tris += cMax.tris;
        anyEnv.nodes += aMax.nodes; anyEnv.tris += aMax.tris;
      }
    }
  const double n = (double) std::max(bounce, 1ull), g = (double) std::max(groups, 1ull);
  printf("%s frame=%dx%d glowMask=%u cameraRays=%llu bounce=%llu glowHits=%llu blocked=%llu escaped=%llu again=%llu againNoOwnTree=%llu againTie=%llu missRewalks=%llu againLeaf=%llu mismatches=%llu glowShare=%.4f againShare=%.5f\n", path, W, H,
         plan.lastCastGlow, camRays, bounce, glowHits, blockedRays, escaped, again, why[kNoOwnTree], why[kTie], M.refWalks, why[kLeaf], mismatches, glowHits / n, again / n);
  printf("  per bounce ray: closest-hit walk %.2f node visits %.2f triangle tests | any-hit walk %.2f node visits %.2f triangle tests\n", closest.nodes / n, closest.tris / n,
         anyhit.nodes / n, anyhit.tris / n);
  printf("  envelope over the %d rays of a tile (%llu tiles): closest-hit walk %.2f node visits %.2f triangle tests | any-hit walk %.2f node visits %.2f triangle tests\n",
         raysPerTile, groups, closestEnv.nodes / g, closestEnv.tris / g, anyEnv.nodes / g, anyEnv.tris / g);
  return mismatches ? 1 : 0;
}

int main(int argc, char **argv)
{
  int rc = 0;
  if (argc >= 4 && !strcmp(argv[1], "rays") && atoi(argv[2]) >= 1)
    for (int i = 3; i < argc; ++i) rc |= RaysOf(argv[i], atoi(argv[2]));
  else if (argc == 3 && !strcmp(argv[1], "predicate")) {
    Scene s;
    if (!s.Load(argv[2])) return 1;
    printf("%s lastCastQuery=%d glowMask=%u resident=%d\n", argv[2], (int) s.t.plan.lastCastQuery, s.t.plan.lastCastGlow, (int) s.t.plan.resident);
  } else {
    printf("usage: last_cast_check rays <rays per tile> <blob>... | predicate <blob>\n");
    return 2;
  }
  printf(rc ? "last_cast_check: FAILED\n" : "last_cast_check: clean\n");
  return rc;
}
