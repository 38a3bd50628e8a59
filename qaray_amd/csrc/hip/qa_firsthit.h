// qa_firsthit.h — one camera ray, one first hit: what the read-only passes over the resident scene share (qa_gbuffer.hip,
// qa_matte.hip, qa_ray_query.hip, the camera-ray hand-out of qa_radiance.hip).  Each helper restates text of the integrator body
// (qa_kernel_body.h: section B the camera ray, section C the reset of the hit, section D the hit's material; the bodies keep their
// own text, their register allocation is their speed: DESIGN.md 5) - the same float expressions on the same operands in the same
// order, the same random draws in the same order.  A change to one side is a change to the other.
//
// The interfaces are shaped by the kernels' resources (profiles/firsthit_unify_ab.txt).  The compiler simplifies a
// helper before it inlines it, and two nestings cost registers or scratch in the textured kernels however their arguments were
// passed: normalize() inside a camera-ray helper (+ 32 bytes of scratch in qa_gbuffer<RES, TEX>) and instAt() inside the material
// helper (+ 6 VGPRs in qa_gbuffer<!RES, TEX>, one occupancy step).  So camPoint returns the point and the kernel normalises, and
// hitMaterial takes the instance's material set from the kernel.  The material index and `white` travel as a pair.
#pragma once
#include "qa_kernel.h"

namespace qa {

#define QA_HIT_BACK 0x40000000   /* bit 30 of a material word: the hit is on a back face (QA_GBUFFER_BACKFACE of the C ABI) */

// dynamic LDS as qa_integrate lays it out: [resident scene image (RES) | traversal stacks (stackDepth x 256)]; -> the lane's stack
template <bool RES>
__device__ __forceinline__ uint32_t *sceneToLds(const DScene &sc, uint4 *dyn)
{
  if (RES) {
    for (uint32_t i = threadIdx.x; i < sc.residentVec4; i += QA_BLOCK) dyn[i] = sc.resident[i];
    __syncthreads();
  }
  return reinterpret_cast<uint32_t *>(dyn + (RES ? sc.residentVec4 : 0)) + threadIdx.x;
}
// the material table: in that image, or in global memory
template <bool RES>
__device__ __forceinline__ const uint4 *materialTable(const DScene &sc, const uint4 *dyn)
{
  return RES ? dyn + sc.resMaterials : reinterpret_cast<const uint4 *>(sc.mtl);
}
__device__ __forceinline__ TexTables texTables(const DScene &sc)
{
  TexTables tt;
  tt.blob = sc.blob;
  tt.texels = sc.texels;
  tt.texOff = sc.texOff;
  tt.texmap = sc.texmap;
  tt.tex = sc.tex;
  tt.filter = sc.texFilter;
  return tt;
}

// ---- the camera ray of (px, py, sample s): section B
// where sample s of the pixel lies on the image plane, in pixels (also where a miss looks the background's texmap up)
__device__ __forceinline__ f3 camTexpos(const float *halton, int s, int px, int py)
{
  const float hx = halton[2 * s], hy = halton[2 * s + 1];
  return F3(hx, hy, 0.f) + F3((float) px, (float) py, 0.f);
}
// the ray's origin: the camera's position, moved over the lens by two draws of the pixel's stream when dof > 0.1
// (SuperSamplerHalton::NewDofSample).  A pinhole camera draws nothing: callers that refuse a lens read cam.pos themselves
__device__ __forceinline__ f3 camLensPos(const DCamera &cam, uint32_t &rng)
{
  f3 campos = ld3(cam.pos);
  if (cam.dof > 0.1f) {
    const float r1 = rng1(rng), r2 = rng1(rng);
    const float r = cam.dof * qsqrt(r1);
    const float t = r2 * 2.f * QA_PI;
    campos = campos + (ld3(cam.screenX) * (r * qcosf(t)) + ld3(cam.screenY) * (r * qsinf(t)));
  }
  return campos;
}
// the point (x, y) of the image plane, x and y in pixels.  A sample's ray goes from the origin through the point of its texpos:
// d = normalize(point - origin); its differential rays (DiffRay x / y, TEX) through the points of x + QA_DX and of y + QA_DX
__device__ __forceinline__ f3 camPoint(const DCamera &cam, float x, float y)
{
  const f3 A = ld3(cam.screenA), U = ld3(cam.screenU), V = ld3(cam.screenV);
  return (A + U * x) + V * y;
}

// ---- the reset of a cast's records: section C (HitInfo::Init)
__device__ __forceinline__ void hitInit(Hit &h)
{
  h.z = QA_BIGFLOAT;
  h.node = -1;
  h.mtlID = 0;
  h.front = true;
  h.p = F3(0, 0, 0);
  h.N = F3(0, 0, 0);
}
__device__ __forceinline__ void texHitInit(TexHit &th)
{
  th.uvw = F3(0.5f, 0.5f, 0.5f);
  th.duvw0 = th.duvw1 = F3(0, 0, 0);
  th.hasTexture = false;
}

// ---- the hit's material: section D.  sets: DScene::mtlset; set: the hit instance's, instAt<RES>(sc, h.node).mtlset -> the index
// into the material table, or -1: the node has no material (black), or - `white` - a multi-material mesh whose face names none
// (MultiMtl::Shade returns (1, 1, 1))
__device__ __forceinline__ int hitMaterial(const qa_mtlset *sets, int set, int mtlID, bool &white)
{
  int mi = -1;
  white = false;
  if (set >= 0) {
    const qa_mtlset ms = sets[set];
    if (ms.multi) {
      if (mtlID >= 0 && mtlID < ms.count) mi = ms.first + mtlID;
      else white = true;
    } else mi = ms.first;
  }
  return mi;
}
// the material word of the ids planes: the index, -1 none, -2 white; bit 30 on a back face (a negative word has it anyway)
__device__ __forceinline__ int materialWord(int mi, bool white, bool front)
{
  int mword = mi < 0 ? (white ? -2 : -1) : mi;
  if (!front) mword = (int) ((uint32_t) mword | (uint32_t) QA_HIT_BACK);
  return mword;
}

// ---- the colour of a first hit: the diffuse colour shadeSurface would shade with, through its texture when TEX
// (shadeSurfaceTexFirst); and of a miss: the background a camera ray returns, through its texmap at texpos when TEX
template <bool TEX>
__device__ __forceinline__ f3 hitColor(const DScene &sc, const TexTables &tt, const uint4 *mtlTable, const TexHit &th, int mi, bool white)
{
  f3 kd;
  if (mi < 0) {
    kd = white ? F3(1, 1, 1) : F3(0, 0, 0);
  } else {
    const uint4 m0 = mtlTable[6 * (size_t) mi];
    kd = F3(asF(m0.x), asF(m0.y), asF(m0.z));
    if (TEX) kd = mtlSample(tt, th, kd, sc.mtlTex[8 * (size_t) mi]);
  }
  return kd;
}
template <bool TEX>
__device__ __forceinline__ f3 missColor(const DScene &sc, const TexTables &tt, const f3 texpos)
{
  f3 kd = ld3(sc.background);
  if (TEX) kd = texColorSample(tt, kd, sc.bgTexmap, F3(texpos.x / (float) sc.cam.width, texpos.y / (float) sc.cam.height, 0.f));
  return kd;
}

}  // namespace qa
