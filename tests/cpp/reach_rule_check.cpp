// Host check of the leaf test by which hitMesh trusts the own tree's answer (refReaches / refLeafReached, qa_kernel.h and
// qa_tilecull.h; built by tests/test_cast_cost_host.py with -fsanitize=address,undefined, no GPU):
//   reach_rule_check <rays per tile> <blob>...
// For every 8x8 tile of the blob's frame: random sub-pixel camera rays, and from every camera hit on a mesh one cosine-distributed
// bounce ray.  Every ray that passes a mesh's bounds test is a closest-hit query of that mesh: the closest accepted triangle by
// brute force over all of them (the reference's inside test, restated from hitTriangleZ), the reference's walk restated from
// walkBVH<false>, and the leaf test in both forms - strict (entry < t, before) and at the found distance (entry <= t, now).
// Wherever the new form trusts the answer and no second triangle is accepted at the same distance, the reference's walk must
// return the same element at the same distance, bit for bit.  One line per mesh node; exit code 1 on a mismatch.
#define main tile_cull_check_main   // the scene loader of the tile lists' check
#include "tile_cull_check.cpp"
#undef main

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

struct Tally { unsigned long long queries = 0, hits = 0, ties = 0, oldRewalks = 0, newRewalks = 0, entryEqual = 0, trusted = 0, mismatches = 0; };

// One closest-hit query of a mesh, as hitMesh asks it with nothing held.  Returns the hit (node space) for the bounce ray.
static bool Query(const DMesh &m, const MeshTables &mt, const Ray &ray, Tally &T, float &tHit, uint32_t &elem)
{
  const f3 drcp = F3(1.f / ray.d.x, 1.f / ray.d.y, 1.f / ray.d.z);
  const float mb[6] = {m.bmin[0], m.bmin[1], m.bmin[2], m.bmax[0], m.bmax[1], m.bmax[2]};
  float entry, exit_;
  RefBox(ray, drcp, mb, entry, exit_);
  if (entry > QA_BIGFLOAT || entry > exit_) return false;   // Box::IntersectRay
  ++T.queries;
  // the closest accepted triangle over all of them, and whether a second one is accepted at that distance
  float best = QA_BIGFLOAT;
  uint32_t X = 0, atBest = 0;
  for (uint32_t e = 0; e < m.num_faces; ++e) {
    float t = QA_BIGFLOAT;
    if (!TriangleZ(mt.tris[e], ray, t)) continue;
    if (t < best) { best = t; X = e; atBest = 1; }
    else if (t == best) ++atBest;
  }
  if (!atBest) return false;   // (a miss is trusted by another rule: the normal list of hitMesh)
  ++T.hits;
  const bool tie = atBest > 1;
  T.ties += tie ? 1 : 0;
  const uint32_t leaf = mt.shade[X].pad;
  bool oldOk = true, newOk = true;
  if (leaf > 1) {
    RefBox(ray, drcp, mt.nodes[leaf].box, entry, exit_);
    oldOk = refLeafReached(entry, exit_, best, false);
    newOk = refLeafReached(entry, exit_, best, true);
    T.entryEqual += (entry == best && entry < exit_) ? 1 : 0;
  }
  if (!tie) {
    T.oldRewalks += oldOk ? 0 : 1;
    T.newRewalks += newOk ? 0 : 1;
    if (newOk) {
      ++T.trusted;
      float hz = QA_BIGFLOAT;
      uint32_t refElem = 0xFFFFFFFFu;
      const bool hit = RefWalk(mt, ray, drcp, hz, refElem);
      uint32_t a, b;
      memcpy(&a, &hz, 4);
      memcpy(&b, &best, 4);
      if (!hit || refElem != X || a != b) {
        if (T.mismatches++ < 5)
          printf("  mismatch: element %u at %.9g trusted, the reference walk returns %s element %u at %.9g\n", X, (double) best, hit ? "" : "NO HIT,", refElem, (double) hz);
      }
    }
  }
  tHit = best;
  elem = X;
  return true;
}

static int Reach(const char *path, int raysPerTile)
{
  Scene s;
  if (!s.Load(path)) return 1;
  const DCamera &cam = s.t.ds.cam;
  const int W = cam.width, H = cam.height;
  int bad = 0, nodes = 0;
  for (int k = 1; k < (int) s.h->num_instances; ++k) {
    if (s.inst[k].obj_type != QA_OBJ_MESH) continue;
    const DMesh &m = s.t.plan.meshes[s.inst[k].mesh];
    const MeshTables &mt = s.t.mesh[s.inst[k].mesh];
    if (!m.useFast) continue;
    ++nodes;
    const std::vector<int> chain = s.Chain(k);
    auto toNodeSpace = [&](Ray ray) {
      if (s.t.ds.rootIdentity) ray.d = (ray.p + ray.d) - ray.p;   // rootRay
      for (int a : chain) ray = toNode(s.inst[a], ray);
      return ray;
    };
    Tally camT, bncT;
    for (int Y0 = 0; Y0 < H; Y0 += 8)
      for (int X0 = 0; X0 < W; X0 += 8)
        for (int r = 0; r < raysPerTile; ++r) {
          const int px = X0 + (int) (g_rng % (unsigned) std::min(8, W - X0)), py = Y0 + (int) ((g_rng >> 8) % (unsigned) std::min(8, H - Y0));
          const f3 texpos = F3(Rnd(), Rnd(), 0.f) + F3((float) px, (float) py, 0.f);
          const f3 cpt = (ld3(cam.screenA) + ld3(cam.screenU) * texpos.x) + ld3(cam.screenV) * texpos.y;
          Ray world;
          world.p = ld3(cam.pos);
          world.d = normalize(cpt - world.p);
          const Ray ray = toNodeSpace(world);
          float t;
          uint32_t e;
          if (!Query(m, mt, ray, camT, t, e)) continue;
          // the hit in world space (Node::FromNodeCoords up the chain), the geometric normal turned against the ray
          f3 p = ray.p + ray.d * t, N = ld3(mt.tris[e].N);
          if (dot(N, ray.d) > 0) N = -N;
          for (size_t i = chain.size(); i-- > 0;) {
            const qa_instance &in = s.inst[chain[i]];
            p = mulMV(in.tm, p) + ld3(in.pos);
            N = normalize(mulTMV(in.itm, N));
          }
          // a cosine-distributed direction about N
          const f3 ax = qabs(N.x) < 0.5f ? F3(1, 0, 0) : F3(0, 1, 0);
          const f3 u = normalize(cross(ax, N)), v = cross(N, u);
          const float r1 = Rnd(), phi = 2.f * QA_PI * Rnd(), rad = qsqrt(r1);
          Ray bounce;
          bounce.p = p;
          bounce.d = normalize((u * (rad * cosf(phi)) + v * (rad * sinf(phi))) + N * qsqrt(qmax(0.f, 1.f - r1)));
          Query(m, mt, toNodeSpace(bounce), bncT, t, e);
        }
    for (int i = 0; i < 2; ++i) {
      const Tally &T = i ? bncT : camT;
      printf("%s node=%d rays=%s queries=%llu hits=%llu ties=%llu oldRewalks=%llu newRewalks=%llu entryEqualsT=%llu trusted=%llu mismatches=%llu\n", path, k,
             i ? "bounce" : "camera", T.queries, T.hits, T.ties, T.oldRewalks, T.newRewalks, T.entryEqual, T.trusted, T.mismatches);
      bad += T.mismatches ? 1 : 0;
    }
  }
  if (!nodes) { printf("%s: no mesh node with an own tree\n", path); return 1; }
  return bad ? 1 : 0;
}

int main(int argc, char **argv)
{
  if (argc < 3 || atoi(argv[1]) < 1) {
    printf("usage: reach_rule_check <rays per tile> <blob>...\n");
    return 2;
  }
  int rc = 0;
  for (int i = 2; i < argc; ++i) rc |= Reach(argv[i], atoi(argv[1]));
  printf(rc ? "reach_rule_check: FAILED\n" : "reach_rule_check: clean\n");
  return rc;
}
