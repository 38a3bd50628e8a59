// Host check of the empty-tile test (qa_emptytile.h; built by tests/test_empty_tiles_host.py with -fsanitize=address,undefined,
// no GPU):
//   empty_tile_check rays <rays per tile> <blob>...   for every 8x8 tile of the blob's frame that tileIsEmpty calls empty: camera rays
//                                    through the four corners of the tile's pixel area (offsets 0 and the largest float below 1)
//                                    and through <rays per tile> random sample positions of its pixels (offsets in [0, 1), the
//                                    extremes now and then), taken through every node's chain as rootRay / localRay take them;
//                                    the node's first gate must turn every one of them away: the mesh's bounds test in either
//                                    form of the walk (boxEntryExit / boxEntryExitFast against h.z = QA_BIGFLOAT), hitPlane,
//                                    hitSphere's discriminant.  One line per blob; exit code 1 on a ray that passes a gate.
//   empty_tile_check mask <blob>     the frame's mask, one row of tiles per line
// The gates are restated from qa_kernel.h (a device-only header), as tests/cpp/last_cast_check.cpp restates the intersectors.
#define main tile_cull_check_main   // the scene loader of the tile lists' check
#include "tile_cull_check.cpp"
#undef main

#include <cstdlib>

#include "qa_emptytile.h"

#define QA_BIAS 0.005f   /* qa_kernel.h */

// boxEntryExit (qa_kernel.h): the reference's slab interval
static void BoxEntryExit(const Ray &ray, f3 drcp, f3 bmin, f3 bmax, float &entry, float &exit_)
{
  const f3 p0 = (-(ray.p - bmin)) * drcp;
  const f3 p1 = (-(ray.p - bmax)) * drcp;
  f3 t0, t1;
  slab(ray.d.x, p0.x, p1.x, t0.x, t1.x);
  slab(ray.d.y, p0.y, p1.y, t0.y, t1.y);
  slab(ray.d.z, p0.z, p1.z, t0.z, t1.z);
  entry = qmax(t0.x, qmax(t0.y, t0.z));
  exit_ = qmin(t1.x, qmin(t1.y, t1.z));
}
// boxEntryExitFast (qa_kernel.h)
static void BoxEntryExitFast(const Ray &ray, f3 drcp, f3 bmin, f3 bmax, float &entry, float &exit_)
{
  const f3 p0 = (bmin - ray.p) * drcp;
  const f3 p1 = (bmax - ray.p) * drcp;
  entry = __builtin_fmaxf(__builtin_fmaxf(__builtin_fminf(p0.x, p1.x), __builtin_fminf(p0.y, p1.y)), __builtin_fminf(p0.z, p1.z));
  exit_ = __builtin_fminf(__builtin_fminf(__builtin_fmaxf(p0.x, p1.x), __builtin_fmaxf(p0.y, p1.y)), __builtin_fmaxf(p0.z, p1.z));
}
// hitMesh's first lines (qa_kernel.h): does the ray get past Box::IntersectRay with nothing held (h.z = QA_BIGFLOAT)?
static bool MeshGatePasses(const Ray &ray, f3 bmin, f3 bmax)
{
  const f3 drcp = F3(1.f / ray.d.x, 1.f / ray.d.y, 1.f / ray.d.z);
  const bool nearZero = qabs(ray.d.x) < 1e-7f || qabs(ray.d.y) < 1e-7f || qabs(ray.d.z) < 1e-7f;
  float entry, exit_;
  BoxEntryExit(ray, drcp, bmin, bmax, entry, exit_);   // (the form a wave takes when any of its lanes has a near-zero component)
  bool pass = !(entry > QA_BIGFLOAT || entry > exit_);
  if (!nearZero) {
    BoxEntryExitFast(ray, drcp, bmin, bmax, entry, exit_);
    pass = pass || !(entry > QA_BIGFLOAT || entry > exit_);
  }
  return pass;
}
// hitPlane (qa_kernel.h) with nothing held
static bool PlaneHit(const Ray &ray)
{
  const f3 N = F3(0, 0, 1);
  const float dz = dot(ray.d, N);
  if (qabs(dz) < 1e-7f) return false;
  const float pz = dot(ray.p, N);
  const float t = -pz / dz;
  if (t <= QA_BIAS) return false;
  if (QA_BIGFLOAT > t) {
    const f3 p = ray.p + ray.d * t;
    if (qabs(p.x) > 1.f || qabs(p.y) > 1.f) return false;
    return true;
  }
  return false;
}
// hitSphere's first gate (qa_kernel.h): false = "delta < 0", the miss an empty tile promises
static bool SphereGatePasses(const Ray &ray)
{
  const float a = dot(ray.d, ray.d);
  const float b = 2.f * dot(ray.p, ray.d);
  const float c = dot(ray.p, ray.p) - 1;
  const float delta = b * b - 4 * a * c;
  return !(delta < 0);
}

struct HostNodes {
  const qa_instance *insts;
  const DMesh *meshes;
  const qa_instance &inst(int k) const { return insts[k]; }
  const DMesh &mesh(int i) const { return meshes[i]; }
};

static bool Empty(const Scene &s, int X0, int Y0)
{
  const HostNodes n = {s.inst, s.t.plan.meshes.data()};
  TileCone cone;
  return tileIsEmpty(n, s.t.ds.cam, s.t.ds.background, s.t.ds.num_inst, s.t.ds.rootIdentity != 0, (float) X0, (float) Y0, &cone);
}

static int RaysOfEmptyTiles(int perTile, const char *path)
{
  Scene s;
  if (!s.Load(path)) return 1;
  const DCamera &cam = s.t.ds.cam;
  const int W = cam.width, H = cam.height, N = (int) s.h->num_instances;
  std::vector<std::vector<int>> chains(N);
  int objects = 0;
  for (int k = 1; k < N; ++k)
    if (s.inst[k].obj_type != QA_OBJ_NONE) { chains[k] = s.Chain(k); ++objects; }
  const float last = std::nextafterf(1.f, 0.f);
  unsigned long long tiles = 0, empty = 0, rays = 0, passed = 0;
  for (int Y0 = 0; Y0 < H; Y0 += 8)
    for (int X0 = 0; X0 < W; X0 += 8) {
      ++tiles;
      if (!Empty(s, X0, Y0)) continue;
      ++empty;
      const int nx = std::min(8, W - X0), ny = std::min(8, H - Y0);
      for (int r = -4; r < perTile; ++r) {
        f3 texpos;
        if (r < 0) {   // the corners of the tile's pixel area
          const bool right = (r & 1) != 0, low = (r & 2) != 0;
          texpos = F3(right ? last : 0.f, low ? last : 0.f, 0.f) + F3((float) (X0 + (right ? nx - 1 : 0)), (float) (Y0 + (low ? ny - 1 : 0)), 0.f);
        } else {
          const int px = X0 + (int) (g_rng % (unsigned) nx), py = Y0 + (int) ((g_rng >> 8) % (unsigned) ny);
          texpos = F3(Rnd(), Rnd(), 0.f) + F3((float) px, (float) py, 0.f);
        }
        // qa_integrate_lastcast section B (src/renderers/renderer.cpp:312-328), then rootRay and localRay
        const f3 cpt = (ld3(cam.screenA) + ld3(cam.screenU) * texpos.x) + ld3(cam.screenV) * texpos.y;
        Ray world;
        world.p = ld3(cam.pos);
        world.d = normalize(cpt - world.p);
        if (s.t.ds.rootIdentity) world.d = (world.p + world.d) - world.p;
        ++rays;
        for (int k = 1; k < N; ++k) {
          const int type = s.inst[k].obj_type;
          if (type == QA_OBJ_NONE) continue;
          Ray ray = world;
          for (int a : chains[k]) ray = toNode(s.inst[a], ray);
          bool pass;
          if (type == QA_OBJ_MESH) {
            const DMesh &m = s.t.plan.meshes[s.inst[k].mesh];
            pass = MeshGatePasses(ray, ld3(m.bmin), ld3(m.bmax));
          } else if (type == QA_OBJ_PLANE) pass = PlaneHit(ray);
          else pass = SphereGatePasses(ray);
          if (pass && passed++ < 5)
            printf("  a gate passes: tile (%d, %d) node %d type %d, ray through (%.9g, %.9g)\n", X0, Y0, k, type, (double) texpos.x, (double) texpos.y);
        }
      }
    }
  const bool variant = s.t.plan.resident && s.t.plan.lastCastQuery && s.t.ds.num_lights == 0;
  printf("%s frame=%dx%d objects=%d variant=%d tileListBytes=%zu tiles=%llu empty=%llu rays=%llu passed=%llu\n", path, W, H, objects, variant ? 1 : 0,
         s.t.plan.tileListBytes, tiles, empty, rays, passed);
  return passed ? 1 : 0;
}

static int Mask(const char *path)
{
  Scene s;
  if (!s.Load(path)) return 1;
  for (int Y0 = 0; Y0 < s.t.ds.cam.height; Y0 += 8) {
    for (int X0 = 0; X0 < s.t.ds.cam.width; X0 += 8) putchar(Empty(s, X0, Y0) ? '#' : '.');
    putchar('\n');
  }
  return 0;
}

int main(int argc, char **argv)
{
  int rc = 0;
  if (argc >= 4 && !strcmp(argv[1], "rays"))
    for (int i = 3; i < argc; ++i) rc |= RaysOfEmptyTiles(atoi(argv[2]), argv[i]);
  else if (argc == 3 && !strcmp(argv[1], "mask"))
    rc = Mask(argv[2]);
  else {
    printf("usage: empty_tile_check rays <rays per tile> <blob>... | mask <blob>\n");
    return 2;
  }
  printf(rc ? "empty_tile_check: FAILED\n" : "empty_tile_check: clean\n");
  return rc;
}
