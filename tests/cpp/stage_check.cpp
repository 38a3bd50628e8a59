// stage_check.cpp — the layout half of qaray_amd/csrc/hip/qa_stage.h, stand-alone under AddressSanitizer + UBSan
// (tests/test_stage_host.py builds and runs it; no HIP header is on its include path).  The plane declarations of every host form
// that stages through qa_ctx::stageQuery are restated here in the order their call sites make them - Req for a plane the form's
// checks demand, Opt for one the caller may leave out - and laid out for every subset of the optional planes, at n = 1, 3 and 65
// (r = n and r = 3 n records for the radiance rays, m = 2 and d = 1 for the probes).  Checked for each:
//   - every plane starts on a multiple of 16 bytes and ends inside the total; the planes present are pairwise disjoint;
//   - an absent plane has no bytes and resolves to null, a present one to base + its offset; a heap buffer of exactly the total is
//     written plane by plane, so a byte outside it is reported;
//   - the total is at most what the form reserved before the carver, the formula written out as a literal, plus 16 bytes per plane.
// And once, the probes at n = 2^31 - 1, m = 128 with a cube: the total is the same sum in unsigned __int128 - nothing wrapped.
// Prints "stage_check: clean" and returns 0, or the first failures and 1.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <memory>

#include "qa_stage.h"

typedef unsigned __int128 u128;

static int g_fail = 0;
#define CHECK(cond, ...)                                   \
  do {                                                     \
    if (!(cond)) {                                         \
      if (++g_fail <= 20) { printf("FAIL %s:%d: %s: ", __FILE__, __LINE__, #cond); printf(__VA_ARGS__); printf("\n"); } \
    }                                                      \
  } while (0)

// A form's declarations: bit k of mask says whether its k-th optional plane was asked for
struct Decls {
  StageLayout lay;
  bool wanted[StageLayout::kMaxPlanes];
  size_t elem[StageLayout::kMaxPlanes], n[StageLayout::kMaxPlanes];
  unsigned mask = 0;
  int optional = 0;
  bool Plane(size_t elemSize, size_t count, bool want)
  {
    const int i = lay.Add(elemSize, count, want);
    wanted[i] = want; elem[i] = elemSize; n[i] = count;
    return want;
  }
  bool Req(size_t elemSize, size_t count) { return Plane(elemSize, count, true); }
  bool Opt(size_t elemSize, size_t count) { return Plane(elemSize, count, (mask >> optional++) & 1u); }
};

// ---- the host forms: their planes as declared, -> the bytes the form reserved before the carver
struct Sizes { size_t n, r, K, cells; };   // rays, points, pixels or texels; ray records; a probe's cube texels; its moment floats

static u128 CastRays(Decls &d, const Sizes &s)
{
  d.Req(4, 3 * s.n); d.Req(4, 3 * s.n);                                          // origins, dirs
  d.Opt(4, s.n); d.Opt(4, 3 * s.n); d.Opt(4, 3 * s.n); d.Opt(4, 2 * s.n);        // t, normal, point, ids
  return (u128) 60 * s.n;
}
static u128 Occluded(Decls &d, const Sizes &s)
{
  d.Req(4, 3 * s.n); d.Req(4, 3 * s.n); d.Req(4, s.n);                           // origins, dirs, tmax
  d.Req(1, s.n);                                                                 // out
  return (u128) 29 * s.n;
}
static u128 GBuffer(Decls &d, const Sizes &s)
{
  d.Opt(4, 3 * s.n); d.Opt(4, 3 * s.n); d.Opt(4, s.n); d.Opt(4, 2 * s.n);        // normal, albedo, depth, ids
  return (u128) 36 * s.n;
}
static u128 Matte(Decls &d, const Sizes &s)
{
  d.Opt(4, s.n);                                                                 // ns
  d.Opt(4, s.n); d.Opt(4, 3 * s.n); d.Opt(4, 3 * s.n); d.Opt(4, 3 * s.n);        // coverage, albedo, normal, backdrop
  return (u128) 44 * s.n;
}
static u128 IdMatte(Decls &d, const Sizes &s)
{
  d.Opt(4, s.n);                                                                 // ns
  d.Opt(4, 8 * s.n); d.Opt(4, 8 * s.n); d.Opt(4, s.n); d.Opt(4, s.n);            // ids, counts, other, samples
  return (u128) 76 * s.n;
}
static u128 AoRegion(Decls &d, const Sizes &s)
{
  d.Opt(4, s.n);                                                                 // ns
  d.Opt(4, s.n); d.Opt(4, s.n); d.Opt(4, s.n);                                   // open, rays, ao
  return (u128) 16 * s.n;
}
static u128 AoPoints(Decls &d, const Sizes &s)
{
  d.Req(4, 3 * s.n); d.Req(4, 3 * s.n); d.Opt(4, s.n);                           // points, normals, stream ids
  d.Opt(4, s.n); d.Opt(4, s.n);                                                  // open, ao
  return (u128) 36 * s.n;
}
static u128 BakeTexels(Decls &d, const Sizes &s)
{
  const bool point = d.Opt(4, 3 * s.n), normal = d.Opt(4, 3 * s.n), face = d.Opt(4, s.n), bary = d.Opt(4, 2 * s.n);
  return (u128) (point ? 12 * s.n : 0) + (normal ? 12 * s.n : 0) + (face ? 4 * s.n : 0) + (bary ? 8 * s.n : 0);
}
static u128 RadianceRays(Decls &d, const Sizes &s)
{
  d.Req(4, 3 * s.r); d.Req(4, 3 * s.r); d.Opt(4, 3 * s.r); d.Opt(4, 3 * s.r); d.Opt(4, 2 * s.r);   // origins, dirs, dx, dy, screen
  d.Opt(4, s.n);                                                                 // stream
  d.Req(4, 3 * s.n); d.Opt(4, s.n); d.Opt(4, s.n);                               // rgb, t, ns
  return ((u128) s.n * 6 + (u128) s.r * 14) * sizeof(float);
}
static u128 IrradiancePoints(Decls &d, const Sizes &s)
{
  d.Req(4, 3 * s.n); d.Req(4, 3 * s.n); d.Opt(4, s.n);                           // points, normals, stream ids
  d.Req(4, 3 * s.n); d.Opt(4, s.n);                                              // rgb, nsamples
  return (u128) s.n * 11 * sizeof(float);
}
// ProbeHost of qa_lightprobe.hip, as qa_probe_sh calls it (sh required, no moments) and as qa_probevis_sh does (sh optional)
static u128 Probe(Decls &d, const Sizes &s, bool vis)
{
  d.Req(4, 3 * s.n); d.Opt(4, s.n);                                              // points, stream ids
  vis ? d.Opt(4, 27 * s.n) : d.Req(4, 27 * s.n);                                 // sh
  const bool cube = d.Opt(4, 3 * s.K * s.n);
  d.Opt(4, s.n); d.Opt(4, s.n);                                                  // hits, tmin
  d.Plane(4, (vis ? s.cells : 0) * s.n, vis);                                    // moments
  return (u128) s.n * (33 + (vis ? s.cells : 0) + (cube ? 3 * s.K : 0)) * sizeof(float);
}
static u128 ProbeSh(Decls &d, const Sizes &s) { return Probe(d, s, false); }
static u128 ProbeVisSh(Decls &d, const Sizes &s) { return Probe(d, s, true); }

struct Form { const char *name; u128 (*declare)(Decls &, const Sizes &); };
static const Form kForms[] = {{"qa_gbuffer_region", GBuffer}, {"qa_matte_region", Matte}, {"qa_idmatte_region", IdMatte}, {"qa_ao_region", AoRegion},
                              {"qa_ao_points", AoPoints}, {"qa_cast_rays", CastRays}, {"qa_occluded", Occluded}, {"qa_bake_texels", BakeTexels},
                              {"qa_radiance_rays", RadianceRays}, {"qa_irradiance_points", IrradiancePoints}, {"qa_probe_sh", ProbeSh},
                              {"qa_probevis_sh", ProbeVisSh}};

static u128 Padded(const Decls &d)
{
  u128 sum = 0;
  for (int i = 0; i < d.lay.count; ++i)
    if (d.wanted[i]) sum += (((u128) d.elem[i] * d.n[i] + 15) / 16) * 16;
  return sum;
}

static void CheckOne(const Form &f, const Sizes &s, unsigned mask)
{
  Decls d;
  d.mask = mask;
  const u128 parent = f.declare(d, s);
  const StageLayout &L = d.lay;
  std::unique_ptr<unsigned char[]> buf(new unsigned char[L.total ? L.total : 1]);
  for (int i = 0; i < L.count; ++i) {
    CHECK(L.off[i] % 16 == 0 && L.off[i] + L.bytes[i] <= L.total, "%s n %zu mask %x plane %d", f.name, s.n, mask, i);
    if (!d.wanted[i] || d.n[i] == 0) {
      CHECK(L.bytes[i] == 0 && L.At(buf.get(), i) == nullptr, "%s n %zu mask %x plane %d", f.name, s.n, mask, i);
      continue;
    }
    CHECK(L.bytes[i] == d.elem[i] * d.n[i] && L.At(buf.get(), i) == buf.get() + L.off[i], "%s n %zu mask %x plane %d", f.name, s.n, mask, i);
    memset(L.At(buf.get(), i), i + 1, L.bytes[i]);
    for (int j = 0; j < i; ++j)
      CHECK(!L.bytes[j] || L.off[j] + L.bytes[j] <= L.off[i] || L.off[i] + L.bytes[i] <= L.off[j], "%s n %zu mask %x planes %d %d", f.name, s.n, mask, j, i);
  }
  // (every plane still holds its own fill: no plane written after it reached into it)
  for (int i = 0; i < L.count; ++i)
    for (size_t b = 0; b < L.bytes[i]; ++b)
      if (static_cast<unsigned char *>(L.At(buf.get(), i))[b] != i + 1) { CHECK(false, "%s n %zu mask %x plane %d byte %zu", f.name, s.n, mask, i, b); break; }
  CHECK((u128) L.total == Padded(d), "%s n %zu mask %x", f.name, s.n, mask);
  CHECK((u128) L.total <= parent + (u128) 16 * L.count, "%s n %zu mask %x: %zu bytes, the form reserved %zu", f.name, s.n, mask, L.total, (size_t) parent);
}

int main()
{
  int layouts = 0;
  const size_t counts[] = {1, 3, 65}, spp[] = {1, 3};
  for (const Form &f : kForms)
    for (size_t n : counts)
      for (size_t per : spp) {
        if (per > 1 && f.declare != RadianceRays) continue;
        const Sizes s = {n, n * per, 6 * 2 * 2, 12 * 1 * 1};   // m = 2, d = 1
        Decls probe;
        f.declare(probe, s);
        for (unsigned mask = 0; mask < (1u << probe.optional); ++mask, ++layouts) CheckOne(f, s, mask);
      }

  // the largest request the checks let through: every plane asked for
  const Sizes big = {0x7FFFFFFFull, 0x7FFFFFFFull, 6ull * 128 * 128, 12ull * 128 * 128};   // m = d = 128
  const Form large[] = {{"qa_probe_sh", ProbeSh}, {"qa_probevis_sh", ProbeVisSh}};
  for (const Form &f : large) {
    Decls d;
    d.mask = ~0u;
    const u128 parent = f.declare(d, big);
    CHECK((u128) d.lay.total == Padded(d), "%s at 2^31 - 1 probes wrapped", f.name);
    CHECK((d.lay.total >> 50) != 0 && (u128) d.lay.total <= parent + (u128) 16 * d.lay.count, "%s at 2^31 - 1 probes: %zu bytes", f.name, d.lay.total);
    for (int i = 0; i < d.lay.count; ++i) CHECK(d.lay.off[i] % 16 == 0 && d.lay.off[i] + d.lay.bytes[i] <= d.lay.total, "%s plane %d", f.name, i);
  }
  if (g_fail) { printf("stage_check: %d failure(s)\n", g_fail); return 1; }
  printf("stage_check: clean (%d layouts)\n", layouts);
  return 0;
}
