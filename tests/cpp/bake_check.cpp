// bake_check.cpp — the host half of qaray_amd/csrc/hip/qa_bake_dev.h, stand-alone under AddressSanitizer + UBSan
// (tests/test_bake_host.py builds and runs it).  Every buffer lives on the heap at exactly the size the loops may touch, so a step
// outside one is reported.  Checked here:
//   - the map of a jittered 5x4-cell chart under a scaled, translated node at 1x1, 16x16, 17x16, 19x13 and 64x64 texels: every
//     plane of exactly width * height entries; a covered texel's face is in range, its weights put the sample back (in double) and
//     its point lies on the face; an uncovered one holds zeros; no sample strictly inside the chart is left uncovered,
//   - faces with a vt of -1, a vt beyond the array, a NaN texture vertex and zero area are void and read nothing,
//   - the tile counts at the limit and beyond it, charts on other tiles, the texmap's transform, the material filter, the plane,
//   - the gutter fill against loops written out in place, radius 0 .. 8, pictures down to 1x1.
// Prints "bake_check: clean" and returns 0, or the first failures and 1.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <limits>
#include <memory>
#include <vector>

#include "qa_bake_dev.h"

using namespace qa;

static int g_fail = 0;
#define CHECK(cond, ...)                                   \
  do {                                                     \
    if (!(cond)) {                                         \
      if (++g_fail <= 20) { printf("FAIL %s:%d: %s: ", __FILE__, __LINE__, #cond); printf(__VA_ARGS__); printf("\n"); } \
    }                                                      \
  } while (0)

struct Lcg {
  uint64_t s;
  explicit Lcg(uint64_t seed) : s(seed * 2862933555777941757ull + 3037000493ull) {}
  uint32_t next() { s = s * 6364136223846793005ull + 1442695040888963407ull; return (uint32_t) (s >> 32); }
  float unit() { return (float) (next() & 0xFFFFFF) / 16777216.0f; }
};

// a chart of nx x ny cells over [u0, u1] x [v0, v1] in heap arrays of exactly their size
struct Chart {
  uint32_t nf, nv;
  std::unique_ptr<qa_face[]> faces;
  std::unique_ptr<float[]> vertices, normals, texcoords;
  Chart(uint32_t nx, uint32_t ny, float u0, float u1, float v0, float v1, bool jitter)
  {
    nv = (nx + 1) * (ny + 1);
    nf = 2 * nx * ny;
    faces.reset(new qa_face[nf]);
    vertices.reset(new float[3 * nv]);
    normals.reset(new float[3 * nv]);
    texcoords.reset(new float[2 * nv]);
    Lcg rng(nx * 131 + ny);
    for (uint32_t j = 0; j <= ny; ++j)
      for (uint32_t i = 0; i <= nx; ++i) {
        float u = (float) i / nx, w = (float) j / ny;
        if (jitter && i > 0 && i < nx && j > 0 && j < ny) { u += (rng.unit() - 0.5f) * 0.6f / nx; w += (rng.unit() - 0.5f) * 0.6f / ny; }
        const uint32_t k = j * (nx + 1) + i;
        texcoords[2 * k] = u0 + (u1 - u0) * u;
        texcoords[2 * k + 1] = v0 + (v1 - v0) * w;
        vertices[3 * k] = 4 * u - 2; vertices[3 * k + 1] = 4 * w - 2; vertices[3 * k + 2] = 0.25f * u * w;
        normals[3 * k] = 0.f; normals[3 * k + 1] = 0.6f; normals[3 * k + 2] = 0.8f;
      }
    uint32_t f = 0;
    for (uint32_t j = 0; j < ny; ++j)
      for (uint32_t i = 0; i < nx; ++i) {
        const int a = (int) (j * (nx + 1) + i), b = a + 1, c = a + (int) nx + 2, d = a + (int) nx + 1;
        const int tri[2][3] = {{a, b, c}, {a, d, c}};   // (the second with reversed winding)
        for (int t = 0; t < 2; ++t, ++f)
          for (int q = 0; q < 3; ++q) { faces[f].v[q] = faces[f].vn[q] = faces[f].vt[q] = tri[t][q]; faces[f].mtl = (int) (f % 2); }
      }
  }
  BakeSource source(int mtl = -1) const
  {
    BakeSource s = {};
    s.faces = faces.get(); s.vertices = vertices.get(); s.normals = normals.get(); s.texcoords = texcoords.get();
    s.numFaces = nf; s.numTexcoords = nv; s.mtl = mtl;
    return s;
  }
};

struct Planes {
  size_t n;
  std::unique_ptr<float[]> point, normal, bary;
  std::unique_ptr<int32_t[]> face;
  explicit Planes(size_t n_) : n(n_), point(new float[3 * n_]), normal(new float[3 * n_]), bary(new float[2 * n_]), face(new int32_t[n_]) {}
  BakePlanes out() { const BakePlanes o = {point.get(), normal.get(), face.get(), bary.get()}; return o; }
};

static std::unique_ptr<qa_instance[]> Nodes()
{
  std::unique_ptr<qa_instance[]> inst(new qa_instance[2]);
  memset(inst.get(), 0, 2 * sizeof(qa_instance));
  for (int k = 0; k < 2; ++k) {
    for (int d = 0; d < 3; ++d) inst[k].tm[4 * d] = inst[k].itm[4 * d] = 1.f;
    inst[k].parent = k - 1;
  }
  inst[1].tm[0] = 2.f; inst[1].itm[0] = 0.5f;
  inst[1].pos[0] = 1.f; inst[1].pos[2] = -3.f;
  return inst;
}

// -> covered texels
static uint32_t RunMap(const BakeSource &src, uint32_t W, uint32_t H, bool expectFull, const char *what)
{
  const std::unique_ptr<qa_instance[]> inst = Nodes();
  Planes p((size_t) W * H);
  const BakePlanes o = p.out();
  for (uint32_t iy = 0; iy < H; ++iy)
    for (uint32_t ix = 0; ix < W; ++ix) bakeTexel(src, inst.get(), 1, true, ix, iy, W, H, o);
  uint32_t covered = 0;
  for (uint32_t iy = 0; iy < H; ++iy)
    for (uint32_t ix = 0; ix < W; ++ix) {
      const size_t q = (size_t) iy * W + ix;
      const int32_t f = p.face[q];
      float sx, sy;
      bakeSample(ix, iy, W, H, sx, sy);
      if (f < 0) {
        CHECK(f == -1 && p.point[3 * q] == 0.f && p.point[3 * q + 2] == 0.f && p.normal[3 * q + 1] == 0.f && p.bary[2 * q] == 0.f && p.bary[2 * q + 1] == 0.f,
              "%s %ux%u texel %u,%u: an uncovered texel holds something", what, W, H, ix, iy);
        if (expectFull) CHECK(!(sx > 1e-6f && sx < 1.f - 1e-6f && sy > 1e-6f && sy < 1.f - 1e-6f), "%s %ux%u texel %u,%u: a crack", what, W, H, ix, iy);
        continue;
      }
      ++covered;
      CHECK((uint32_t) f < src.numFaces, "%s: face %d out of range", what, f);
      if ((uint32_t) f >= src.numFaces) continue;
      const BakeFace bf = bakeFaceSetup(src, (uint32_t) f);
      CHECK(bf.nm >= 1 && bf.nm <= QA_BAKE_MAX_TILES && bf.nn >= 1 && bf.nn <= QA_BAKE_MAX_TILES, "%s: a void face won", what);
      const double a = p.bary[2 * q], b = p.bary[2 * q + 1], c = 1.0 - a - b;
      CHECK(a >= -1e-5 && b >= -1e-5 && c >= -1e-5, "%s texel %u,%u: weights %.9g %.9g %.9g", what, ix, iy, a, b, c);
      const double u = a * bf.t0x + b * bf.t1x + c * bf.t2x - sx, v = a * bf.t0y + b * bf.t1y + c * bf.t2y - sy;
      CHECK(std::fabs(u - std::round(u)) < 2e-5 && std::fabs(v - std::round(v)) < 2e-5, "%s texel %u,%u: the weights give uv off the sample by %.3g %.3g", what, ix, iy,
            u - std::round(u), v - std::round(v));
      if (!src.plane) {
        // the point: node 1 of Nodes() is x -> 2 x + 1, z -> z - 3 over the identity root
        const qa_face &fc = src.faces[f];
        double loc[3];
        for (int k = 0; k < 3; ++k) loc[k] = a * src.vertices[3 * fc.v[0] + k] + b * src.vertices[3 * fc.v[1] + k] + c * src.vertices[3 * fc.v[2] + k];
        CHECK(std::fabs(p.point[3 * q] - (2 * loc[0] + 1)) < 1e-5 && std::fabs(p.point[3 * q + 1] - loc[1]) < 1e-5 && std::fabs(p.point[3 * q + 2] - (loc[2] - 3)) < 1e-5,
              "%s texel %u,%u: the point", what, ix, iy);
      }
      const double nl = std::sqrt((double) p.normal[3 * q] * p.normal[3 * q] + (double) p.normal[3 * q + 1] * p.normal[3 * q + 1] + (double) p.normal[3 * q + 2] * p.normal[3 * q + 2]);
      CHECK(std::fabs(nl - 1.0) < 4e-7, "%s texel %u,%u: normal length %.9g", what, ix, iy, nl);
    }
  return covered;
}

static void CheckDilate(uint32_t W, uint32_t H, uint32_t radius, uint32_t every)
{
  const size_t n = (size_t) W * H;
  std::unique_ptr<uint8_t[]> rgb(new uint8_t[3 * n]), out(new uint8_t[3 * n]);
  std::unique_ptr<int32_t[]> face(new int32_t[n]);
  Lcg rng(W * 7 + H * 3 + radius);
  for (size_t q = 0; q < n; ++q) {
    face[q] = (every && rng.next() % every == 0) ? (int32_t) (rng.next() % 5) : -1;
    for (int k = 0; k < 3; ++k) rgb[3 * q + k] = (uint8_t) rng.next();
  }
  for (uint32_t y = 0; y < H; ++y)
    for (uint32_t x = 0; x < W; ++x) bakeDilateTexel(rgb.get(), face.get(), W, H, radius, x, y, out.get());
  const int r = (int) radius;
  for (int y = 0; y < (int) H; ++y)
    for (int x = 0; x < (int) W; ++x) {
      size_t from = (size_t) y * W + x;
      if (face[from] < 0) {
        int best = 1 << 30;
        for (int dy = -r; dy <= r; ++dy)
          for (int dx = -r; dx <= r; ++dx) {
            const int yy = ((y + dy) % (int) H + (int) H) % (int) H, xx = ((x + dx) % (int) W + (int) W) % (int) W;
            if (face[(size_t) yy * W + xx] >= 0 && dx * dx + dy * dy < best) { best = dx * dx + dy * dy; from = (size_t) yy * W + xx; }
          }
      }
      const size_t q = (size_t) y * W + x;
      CHECK(out[3 * q] == rgb[3 * from] && out[3 * q + 1] == rgb[3 * from + 1] && out[3 * q + 2] == rgb[3 * from + 2], "fill %ux%u radius %u texel %d,%d", W, H, radius, x, y);
    }
}

int main()
{
  const uint32_t sizes[5][2] = {{1, 1}, {16, 16}, {17, 16}, {19, 13}, {64, 64}};
  {
    const Chart chart(5, 4, 0.f, 1.f, 0.f, 1.f, true);
    for (const auto &s : sizes) {
      const uint32_t covered = RunMap(chart.source(), s[0], s[1], true, "chart");
      CHECK(covered + s[0] + s[1] >= s[0] * s[1], "chart %ux%u: %u covered", s[0], s[1], covered);
    }
    // the material filter: the even faces, the odd faces, together everything
    const uint32_t even = RunMap(chart.source(0), 19, 13, false, "even"), odd = RunMap(chart.source(1), 19, 13, false, "odd");
    CHECK(even > 60 && odd > 60 && even + odd >= 19 * 13 - 32 && RunMap(chart.source(5), 19, 13, false, "none") == 0, "the material filter: %u + %u", even, odd);
  }
  {
    // other tiles: the same coverage wherever a half-tile chart is placed, and across a tile border
    const Chart up(3, 3, 1.25f, 1.75f, 1.25f, 1.75f, true), neg(3, 3, -0.75f, -0.25f, -1.5f, -1.0f, true), wide(3, 2, 0.5f, 2.5f, -0.25f, 0.5f, true);
    const uint32_t a = RunMap(up.source(), 32, 32, false, "up"), b = RunMap(neg.source(), 32, 32, false, "negative"), c = RunMap(wide.source(), 32, 32, false, "wide");
    CHECK(a >= 240 && a <= 290 && b >= 240 && b <= 290 && c > 700, "tiles: %u %u %u covered", a, b, c);
    // through a texmap: T = itm (uv - pos)
    BakeSource m = up.source();
    m.mapped = 1;
    memset(&m.map, 0, sizeof(m.map));
    m.map.itm[1] = 2.f; m.map.itm[3] = -0.5f; m.map.itm[8] = 1.f;   // a quarter turn with two scales
    m.map.pos[0] = 0.25f; m.map.pos[1] = -0.5f;
    CHECK(RunMap(m, 32, 16, false, "texmap") > 50, "texmap: nothing covered");
  }
  {
    // void faces: vt of -1, vt beyond the array, a NaN texture vertex, zero area.  Only face 4 is left to win
    Chart c(3, 1, 0.f, 1.f, 0.f, 1.f, false);
    c.faces[0].vt[1] = -1;
    c.faces[1].vt[2] = (int32_t) c.nv;
    c.faces[2].vt[0] = 0x7FFFFFFF;
    c.faces[3].vt[0] = c.faces[3].vt[1];
    for (uint32_t f = 0; f < 4; ++f) CHECK(bakeFaceSetup(c.source(), f).nm == 0 && !bakeFaceSetup(c.source(), f).over, "face %u is not void", f);
    c.texcoords[2 * c.faces[5].vt[1]] = std::numeric_limits<float>::quiet_NaN();
    CHECK(bakeFaceSetup(c.source(), 5).nm == 0, "a NaN texture vertex");
    RunMap(c.source(), 19, 13, false, "void faces");
  }
  {
    // the tile limit: a face over exactly 4 tiles is taken, one over 5 is reported and has no counts
    for (int tiles = 1; tiles <= 6; ++tiles) {
      Chart c(1, 1, 0.25f, tiles - 0.5f, 0.25f, 0.75f, false);
      const BakeFace bf = bakeFaceSetup(c.source(), 0);
      CHECK(tiles <= 4 ? (bf.nm == (uint32_t) tiles && bf.nn == 1 && !bf.over) : (bf.over && bf.nm == 0), "%d tiles: nm %u over %u", tiles, bf.nm, bf.over);
      CHECK(bakeOverTiles(c.source()) == (tiles > 4), "%d tiles: the refusal", tiles);
    }
    Chart far(1, 1, 3e9f, 3e9f + 1024.f, -5e9f, -5e9f + 2048.f, false);   // beyond the integers: still counted in floats
    CHECK(bakeOverTiles(far.source()), "a far chart's tiles");
  }
  {
    BakeSource plane = {};
    plane.plane = 1;
    plane.numFaces = 2;
    plane.mtl = -1;
    CHECK(RunMap(plane, 16, 16, true, "plane") == 256 && RunMap(plane, 19, 13, true, "plane") == 19 * 13, "the plane is covered everywhere");
    plane.mtl = 1;
    CHECK(RunMap(plane, 16, 16, false, "plane mtl 1") == 0, "the plane's faces have mtl 0");
  }
  // the sample convention
  float sx, sy;
  bakeSample(0, 0, 7, 5, sx, sy);
  CHECK(sx == 0.f && sy == 0.f, "sample 0 0");
  bakeSample(6, 4, 7, 5, sx, sy);
  CHECK(sx == 6.f / 7.f && sy == 1.f - 4.f / 5.f, "sample 6 4");
  CHECK(bakeWrap(-1, 5) == 4 && bakeWrap(-5, 5) == 0 && bakeWrap(7, 5) == 2 && bakeWrap(-8, 1) == 0 && bakeWrap(-9, 4) == 3, "wrap");

  const uint32_t pics[6][2] = {{1, 1}, {3, 5}, {5, 3}, {16, 16}, {19, 13}, {40, 33}};
  for (const auto &s : pics)
    for (uint32_t radius = 0; radius <= QA_BAKE_MAX_RADIUS; ++radius)
      for (uint32_t every : {0u, 1u, 3u, 40u}) CheckDilate(s[0], s[1], radius, every);

  if (g_fail) { printf("bake_check: %d failure(s)\n", g_fail); return 1; }
  printf("bake_check: clean\n");
  return 0;
}
