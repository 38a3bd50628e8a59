// Host check of the own tree's slab step in its fma form (boxEntryExitPadFma, qa_tilecull.h; built by
// tests/test_cast_cost_host.py with -fsanitize=address,undefined, no GPU):
//   slab_form_check boxes <blob>...   random and adversarial rays (origins on box faces, direction components just above the
//                                     walk's 1e-7, origins far outside) against the leaf boxes of every mesh node's own tree.
//                                     The box widened by the ray's pad LESS what the header's analysis allows the arithmetic
//                                     (2.5e-7 of the largest coordinate involved) has an exact interval on the ray's line, taken
//                                     in double precision; whenever that interval is non-empty and begins at or before the
//                                     distance held, the fp32 fma form must pass the walk's test.  No omission allowed.
//   slab_form_check rays <blob>...    tile_cull_check's rays mode with the fma form as the walk's test: every leaf it passes for a
//                                     camera ray of a tile must be on the tile's list.
// One line per node; exit code 1 on an omission.
#include <cstdlib>
#define main tile_cull_check_main   // the scene loader and the list builder of the tile lists' check
#include "tile_cull_check.cpp"
#undef main

static float RndSigned() { return 2.f * Rnd() - 1.f; }

// [lo, hi] of the line o + t d inside the box widened by w, in double precision (every |d| component is >= 1e-7: no axis is open)
static bool ExactInterval(f3 o, f3 d, const float *box, double w, double &lo, double &hi)
{
  const double O[3] = {o.x, o.y, o.z}, D[3] = {d.x, d.y, d.z};
  lo = -1e300;
  hi = 1e300;
  for (int a = 0; a < 3; ++a) {
    const double t0 = ((double) box[a] - w - O[a]) / D[a], t1 = ((double) box[a + 3] + w - O[a]) / D[a];
    lo = std::max(lo, std::min(t0, t1));
    hi = std::min(hi, std::max(t0, t1));
  }
  return lo <= hi;
}

static int Boxes(const char *path)
{
  Scene s;
  if (!s.Load(path)) return 1;
  int bad = 0, nodes = 0;
  for (int k = 1; k < (int) s.h->num_instances; ++k) {
    if (s.inst[k].obj_type != QA_OBJ_MESH) continue;
    const DMesh &m = s.t.plan.meshes[s.inst[k].mesh];
    if (!m.useFast || !m.numLeaves) continue;
    ++nodes;
    const std::vector<DNode> &leaves = s.t.mesh[s.inst[k].mesh].leaves;
    const f3 lo = ld3(m.bmin), ext = ld3(m.bmax) - ld3(m.bmin);
    unsigned long long tests = 0, required = 0, passed = 0, omissions = 0, oldOmissions = 0;
    for (int r = 0; r < 60000; ++r) {
      Ray ray;
      const int kind = r % 6;
      // origin: in and around the bounds | on a face of a leaf box | far outside
      ray.p = lo + ext * F3(1.5f * Rnd() - 0.25f, 1.5f * Rnd() - 0.25f, 1.5f * Rnd() - 0.25f);
      if (kind == 1 || kind == 2) {
        const DNode &l = leaves[g_rng % leaves.size()];
        const int face = (int) ((g_rng >> 8) % 6u);
        float *c = face % 3 == 0 ? &ray.p.x : face % 3 == 1 ? &ray.p.y : &ray.p.z;
        *c = l.box[face];
        if (kind == 2) {   // inside the face's rectangle
          const f3 q = ld3(l.box) + (ld3(l.box + 3) - ld3(l.box)) * F3(Rnd(), Rnd(), Rnd());
          const float keep = *c;
          ray.p = q;
          *c = keep;
        }
      }
      if (kind == 3) ray.p = lo + ext * 0.5f + F3(RndSigned(), RndSigned(), RndSigned()) * (1e3f * m.absMax);
      if (kind == 4) ray.p = lo + ext * 0.5f + F3(RndSigned(), RndSigned(), RndSigned()) * (1e6f * m.absMax);
      // direction: unit length at random | one or two components just above the walk's threshold
      ray.d = normalize(F3(RndSigned(), RndSigned(), RndSigned()) + F3(1e-3f, 1e-3f, 1e-3f));
      if (kind == 5 || (r % 7) == 0) {
        const float tiny = (1.0000001e-7f + 1e-7f * Rnd() * ((r & 8) ? 1.f : 1e-3f)) * ((r & 16) ? 1.f : -1.f);
        if (r & 1) ray.d.x = tiny; else ray.d.y = tiny;
        if ((r & 6) == 6) ray.d.z = -tiny;
      }
      if (qabs(ray.d.x) < 1e-7f || qabs(ray.d.y) < 1e-7f || qabs(ray.d.z) < 1e-7f || !(dot(ray.d, ray.d) > 0)) continue;   // the walk's exact form
      const float oMax = qmax(qmax(qabs(ray.p.x), qabs(ray.p.y)), qabs(ray.p.z));
      const float pad = fastWalkPad(m.invH, m.absMax, oMax);
      const f3 pLo = ray.p + F3(pad, pad, pad), pHi = ray.p - F3(pad, pad, pad);
      const f3 drcp = F3(1.f / ray.d.x, 1.f / ray.d.y, 1.f / ray.d.z);
      const f3 cLo = slabRayTerm(pLo, drcp), cHi = slabRayTerm(pHi, drcp);
      for (const DNode &l : leaves) {
        ++tests;
        float bAbs = 0;
        for (int a = 0; a < 6; ++a) bAbs = qmax(bAbs, qabs(l.box[a]));
        const double allow = 2.5e-7 * ((double) qmax(oMax, bAbs) + pad);
        double tLo, tHi;
        float entry, exit_, e0, x0;
        boxEntryExitPadFma(cLo, cHi, drcp, ld3(l.box), ld3(l.box + 3), entry, exit_);
        boxEntryExitPadFast(pLo, pHi, drcp, ld3(l.box), ld3(l.box + 3), e0, x0);
        passed += entry <= exit_ ? 1 : 0;
        if (!((double) pad > allow) || !ExactInterval(ray.p, ray.d, l.box, (double) pad - allow, tLo, tHi)) continue;
        ++required;
        // the distance held: nothing yet | just where the reduced box begins (rounded up to a float) | inside it
        const float held[3] = {QA_BIGFLOAT, std::nextafterf((float) tLo, 3e38f), (float) (0.5 * (tLo + tHi))};
        for (int h = 0; h < 3; ++h) {
          if (!((double) held[h] >= tLo)) continue;
          if (!(entry <= held[h] && entry <= exit_)) {
            if (omissions++ < 5)
              printf("  omitted: o (%.9g, %.9g, %.9g) d (%.9g, %.9g, %.9g) box %.9g %.9g %.9g  %.9g %.9g %.9g held %.9g: entry %.9g exit %.9g, exact [%.17g, %.17g]\n", (double) ray.p.x,
                     (double) ray.p.y, (double) ray.p.z, (double) ray.d.x, (double) ray.d.y, (double) ray.d.z, (double) l.box[0], (double) l.box[1], (double) l.box[2], (double) l.box[3],
                     (double) l.box[4], (double) l.box[5], (double) held[h], (double) entry, (double) exit_, tLo, tHi);
          }
          oldOmissions += (e0 <= held[h] && e0 <= x0) ? 0 : 1;   // (the old form under the same question: reported, not required)
        }
      }
    }
    printf("%s node=%d leaves=%u boxTests=%llu passed=%llu required=%llu omissions=%llu oldFormOmissions=%llu\n", path, k, m.numLeaves, tests, passed, required, omissions, oldOmissions);
    bad += omissions ? 1 : 0;
  }
  if (!nodes) { printf("%s: no mesh node with a leaf table\n", path); return 1; }
  return bad ? 1 : 0;
}

// Rays() of tile_cull_check with the walk's fast form replaced by the fma form
static int RaysFma(const char *path)
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
    unsigned long long rays = 0, required = 0, omissions = 0, fmaOnly = 0;
    for (int Y0 = 0; Y0 < H; Y0 += 8)
      for (int X0 = 0; X0 < W; X0 += 8) {
        const TileList L = ListOf(s, k, chain, X0, Y0);
        for (int r = 0; r < 256; ++r) {
          const int px = X0 + (int) (g_rng % (unsigned) std::min(8, W - X0)), py = Y0 + (int) ((g_rng >> 8) % (unsigned) std::min(8, H - Y0));
          const f3 texpos = F3(Rnd(), Rnd(), 0.f) + F3((float) px, (float) py, 0.f);
          const f3 cpt = (ld3(cam.screenA) + ld3(cam.screenU) * texpos.x) + ld3(cam.screenV) * texpos.y;
          Ray ray;
          ray.p = ld3(cam.pos);
          ray.d = normalize(cpt - ray.p);
          if (s.t.ds.rootIdentity) ray.d = (ray.p + ray.d) - ray.p;
          for (int a : chain) ray = toNode(s.inst[a], ray);
          if (qabs(ray.d.x) < 1e-7f || qabs(ray.d.y) < 1e-7f || qabs(ray.d.z) < 1e-7f) continue;   // the exact form: tile_cull_check
          ++rays;
          const float oMax = qmax(qmax(qabs(ray.p.x), qabs(ray.p.y)), qabs(ray.p.z));
          const float pad = fastWalkPad(m.invH, m.absMax, oMax);
          const f3 pLo = ray.p + F3(pad, pad, pad), pHi = ray.p - F3(pad, pad, pad);
          const f3 drcp = F3(1.f / ray.d.x, 1.f / ray.d.y, 1.f / ray.d.z);
          const f3 cLo = slabRayTerm(pLo, drcp), cHi = slabRayTerm(pHi, drcp);
          for (size_t i = 0; i < leaves.size(); ++i) {
            float entry, exit_, e0, x0;
            boxEntryExitPadFma(cLo, cHi, drcp, ld3(leaves[i].box), ld3(leaves[i].box + 3), entry, exit_);
            if (!(entry <= exit_)) continue;
            ++required;
            boxEntryExitPadFast(pLo, pHi, drcp, ld3(leaves[i].box), ld3(leaves[i].box + 3), e0, x0);
            fmaOnly += e0 <= x0 ? 0 : 1;
            if (!((L.mask >> i) & 1ull)) {
              if (omissions++ < 5) printf("  omitted: tile (%d, %d) leaf %zu, ray through (%.9g, %.9g)\n", X0, Y0, i, (double) texpos.x, (double) texpos.y);
            }
          }
        }
      }
    printf("%s node=%d leaves=%u rays=%llu required=%llu passedByFmaFormOnly=%llu omissions=%llu\n", path, k, m.numLeaves, rays, required, fmaOnly, omissions);
    bad += omissions ? 1 : 0;
  }
  if (!nodes) { printf("%s: no mesh node with a leaf table\n", path); return 1; }
  return bad ? 1 : 0;
}

int main(int argc, char **argv)
{
  int rc = 0;
  if (argc >= 3 && !strcmp(argv[1], "boxes"))
    for (int i = 2; i < argc; ++i) rc |= Boxes(argv[i]);
  else if (argc >= 3 && !strcmp(argv[1], "rays"))
    for (int i = 2; i < argc; ++i) rc |= RaysFma(argv[i]);
  else {
    printf("usage: slab_form_check boxes <blob>... | rays <blob>...\n");
    return 2;
  }
  printf(rc ? "slab_form_check: FAILED\n" : "slab_form_check: clean\n");
  return rc;
}
