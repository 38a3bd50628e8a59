// qa_reproject.hip — temporal reprojection on the device and, from the same source, on the host: three forms that nest, each with its
// own generation of the C ABI in front of ONE rank-templated source.  Rank 0: the plain form of qa_reproject_dev.h
// (qa_reproject_device, qa_progressive_reproject_device, qa_test_reproject_host); rank 1: with a node's motion record ahead of the
// projection and a colour clamp behind the taps (qa_reproject_motion_dev.h, the *_motion_* entries); rank 2: with the luma's moments
// and the shortened length (qa_reproject_moments_dev.h, the *_moments_* entries).  An entry fills a ReprojectCall and names its rank;
// behind that there is one check, one launch, one kernel template, one progressive prologue and one host loop.
// The kernel: one pixel per thread on 16x16 tiles: the pixel's own 20 bytes (28 with ids), then a gather of up to four history
// taps of 20 bytes (28 with ids) around the point the old camera saw the pixel's surface at; 16 bytes are written.  Neighbouring
// lanes project to neighbouring history pixels (the map between two views of a surface is smooth), so the taps of a wave share their
// cache lines as a 2x2 filter's do: rank 0 uses no LDS, and no rank a working plane but the ids of a progressive frame; from rank 1
// on a tile stages the clamp's window of current colours in LDS with a halo.  tools/gpu_reproject_cost.py puts the traffic beside
// the measured times.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstddef>
#include <cstdint>
#include <cstring>
#include <vector>

#include "qa_ctx.h"
#include "qa_reproject_moments_dev.h"   // (and through it qa_reproject_motion_dev.h and qa_reproject_dev.h)

namespace qa {

#define QA_REPROJECT_TILE 16

// The current frame.  state = null: the plain buffers.  Else the progressive frame's slabs, resolved as qa_prog_resolve does
// (qa_progressive.hip; qa_denoise.hip's DenoiseSrc is the same rule): the running mean and samples so far of an unfinished pixel,
// the outputs of a finished one
struct ReprojectSrc {
  const float *rgb, *depth;
  const uint32_t *ns, *state;
  int W;
  __device__ __forceinline__ ReprojectPixel operator()(int x, int y) const
  {
    const size_t q = (size_t) y * (size_t) W + (size_t) x;
    ReprojectPixel p;
    p.z = depth[q];
    if (state) {
      const uint4 a = reinterpret_cast<const uint4 *>(state)[2 * q];
      if (!(a.y & 0x80000000u)) {
        p.r = __uint_as_float(a.z); p.g = __uint_as_float(a.w); p.b = __uint_as_float(state[8 * q + 4]);
        p.ns = a.y;
        return p;
      }
    }
    p.r = rgb[3 * q]; p.g = rgb[3 * q + 1]; p.b = rgb[3 * q + 2];
    p.ns = ns[q];
    return p;
  }
};

// The history planes / the ids planes of both frames, on the device and on the host
struct ReprojectHistory {
  const float *rgb, *depth, *length;
  int W;
  __host__ __device__ __forceinline__ void operator()(int x, int y, ReprojectTap &t) const
  {
    const size_t q = (size_t) y * (size_t) W + (size_t) x;
    t.length = length[q];
    t.z = depth[q];
    t.r = rgb[3 * q]; t.g = rgb[3 * q + 1]; t.b = rgb[3 * q + 2];
  }
};
struct ReprojectMomentPlane {
  const float2 *moments;   // 8-byte aligned: one vector load per tap
  int W;
  __host__ __device__ __forceinline__ void operator()(int x, int y, float *h) const
  {
    const float2 v = moments[(size_t) y * (size_t) W + (size_t) x];
    h[0] = v.x; h[1] = v.y;
  }
};
struct ReprojectIds {
  const int32_t *plane[2];   // current, history
  int W;
  __host__ __device__ __forceinline__ void operator()(int which, int x, int y, int *out) const
  {
    const size_t q = (size_t) y * (size_t) W + (size_t) x;
    out[0] = plane[which][2 * q]; out[1] = plane[which][2 * q + 1];
  }
};

#define QA_REPROJECT_MAX_RADIUS 3
#define QA_REPROJECT_MAX_SIDE (QA_REPROJECT_TILE + 2 * QA_REPROJECT_MAX_RADIUS)

// The clamp's window out of the tile's staged pixels: (x, y) is at most `radius` outside the tile, by the caller's loops
struct ReprojectStagedWin {
  const float4 *tile;
  int ox, oy, side;   // the region-local pixel of tile[0]; pixels per staged row
  __device__ __forceinline__ ReprojectWin operator()(int x, int y) const
  {
    const float4 v = tile[(y - oy) * side + (x - ox)];
    ReprojectWin q;
    q.r = v.x; q.g = v.y; q.b = v.z; q.cls = __float_as_uint(v.w);
    return q;
  }
};

// The clamp's staging for the tile at (bx, by), by all 256 threads of the block: with QA_REPROJECT_CLAMP the tile and its halo of
// clampRadius pixels go to `tile` (QA_REPROJECT_MAX_SIDE squared entries), and the block meets at a barrier
__device__ __forceinline__ ReprojectStagedWin reprojectStage(float4 *tile, const ReprojectSetup &S, const ReprojectMotionSetup &M, const ReprojectSrc &cur, int bx,
                                                             int by)
{
  ReprojectStagedWin win = {tile, bx, by, QA_REPROJECT_TILE};
  if (M.flags & QA_REPROJECT_CLAMP) {
    const int r = M.clampRadius, side = QA_REPROJECT_TILE + 2 * r;   // r is 1 .. 3: side * side <= the array's size
    win.ox = bx - r; win.oy = by - r; win.side = side;
    for (int e = (int) threadIdx.x; e < side * side; e += 256) {
      const int gx = win.ox + e % side, gy = win.oy + e / side;
      float4 v = make_float4(0.f, 0.f, 0.f, __uint_as_float(0u));
      if (gx >= 0 && gy >= 0 && gx < S.W && gy < S.H) {
        const ReprojectWin q = reprojectWinOf(cur(gx, gy));
        v = make_float4(q.r, q.g, q.b, __uint_as_float(q.cls));
      }
      tile[e] = v;
    }
    __syncthreads();
  }
  return win;
}

// What a launch hands its kernel, whatever its rank: a rank reads the members its form has
struct ReprojectArgs {
  ReprojectSetup S;
  ReprojectMotionSetup M;
  ReprojectMomentsSetup X;
  ReprojectSrc cur;
  ReprojectHistory hist;
  ReprojectMomentPlane mom;
  ReprojectIds ids;
  int withIds, withMoments;   // both ids planes are given; QA_REPROJECT_MOMENTS is set and the history has a moments plane
  float *outRgb, *outLength;
  float2 *outMoments;         // written with QA_REPROJECT_MOMENTS only (else they may be null)
  float *outVariance;
};

// The kernel of the form of rank FORM (reprojectPixel<FORM> of qa_reproject_moments_dev.h): one pixel per thread on 16x16 tiles.  From
// rank 1 on, with QA_REPROJECT_CLAMP the block first stages the current colour and class of its tile and a halo of clampRadius
// pixels (at radius 3: 22 x 22 x 16 B = 7744 B of LDS), a pixel outside the region as "does not contribute"; the window scans read
// LDS only.  Threads outside the region stage and wait with the others, then leave.  Rank 0 has no tile and no barrier.
template <int FORM>
__global__ __launch_bounds__(256) void qa_reproject_k(ReprojectArgs a)
{
  const int bx = (int) (blockIdx.x * QA_REPROJECT_TILE), by = (int) (blockIdx.y * QA_REPROJECT_TILE);
  ReprojectStagedWin win = {nullptr, bx, by, QA_REPROJECT_TILE};
  if constexpr (FORM >= 1) {
    __shared__ float4 tile[QA_REPROJECT_MAX_SIDE * QA_REPROJECT_MAX_SIDE];
    win = reprojectStage(tile, a.S, a.M, a.cur, bx, by);
  }
  const int x = bx + (int) (threadIdx.x & 15u), y = by + (int) (threadIdx.x >> 4);
  if (x >= a.S.W || y >= a.S.H) return;
  float o[3], om[2], var;
  const float len = reprojectPixel<FORM>(a.S, a.M, a.X, a.cur, a.hist, a.mom, a.ids, win, a.withIds != 0, a.withMoments != 0, x, y, o, om, var);
  const size_t q = (size_t) y * (size_t) a.S.W + (size_t) x;
  a.outRgb[3 * q] = o[0]; a.outRgb[3 * q + 1] = o[1]; a.outRgb[3 * q + 2] = o[2];
  a.outLength[q] = len;
  if constexpr (FORM >= 2) {
    if (a.M.flags & QA_REPROJECT_MOMENTS) {
      a.outMoments[q] = make_float2(om[0], om[1]);
      a.outVariance[q] = var;
    }
  }
}

}  // namespace qa

static bool Overlap(const void *a, size_t na, const void *b, size_t nb)
{
  const uintptr_t p = (uintptr_t) a, q = (uintptr_t) b;
  return a && b && p < q + nb && q < p + na;
}

// One call of any entry: the entry's own arguments in the order of its signature (what its form does not have stays null), then what
// the library adds.  The two narrower parameter structs widen into the third (WithParams)
struct ReprojectCall {
  const qa_camera *prev, *cur;
  int x0, y0, W, H;
  // the current frame.  Of a progressive frame (its slabs are the library's own) all four, and state, are null while the call is checked
  const float *rgb, *depth;
  const uint32_t *ns;
  const int32_t *ids;
  const float *hRgb, *hDepth, *hLength;   // the history
  const int32_t *hIds;
  const float *hMoments;
  const qa_node_motion *motion;
  int count;
  float *outRgb, *outLength, *outMoments, *outVariance;
  const uint32_t *state;   // a progressive frame's slabs (ReprojectSrc)
  bool progressive, noParams;
  qa_reproject_moments_params p;
};

static void WithParams(ReprojectCall &k, const qa_reproject_params *p)
{
  k.noParams = !p;
  if (p) k.p = {p->depth_tolerance, p->max_history, 0.f, 0.f, 0.f, 0, p->flags};
}
static void WithParams(ReprojectCall &k, const qa_reproject_motion_params *p)
{
  k.noParams = !p;
  if (p) k.p = {p->depth_tolerance, p->max_history, p->clamp_gamma, 0.f, 0.f, p->clamp_radius, p->flags};
}
static void WithParams(ReprojectCall &k, const qa_reproject_moments_params *p)
{
  k.noParams = !p;
  if (p) k.p = *p;
}

// The flags the entries of the form of rank `form` accept
static constexpr uint32_t FlagsOf(int form)
{
  return form == 0   ? 0u
         : form == 1 ? (QA_REPROJECT_MOTION | QA_REPROJECT_CLAMP)
                     : (QA_REPROJECT_MOTION | QA_REPROJECT_CLAMP | QA_REPROJECT_MOMENTS | QA_REPROJECT_SHORTEN);
}

// What every entry checks of its sizes, parameters and planes: the parameters and the entry's own flags, then the plain form's
// tests, then what QA_REPROJECT_MOTION and QA_REPROJECT_CLAMP add, then QA_REPROJECT_SHORTEN and QA_REPROJECT_MOMENTS
static int CheckReproject(const ReprojectCall &k, uint32_t allowedFlags)
{
  const qa_reproject_moments_params &p = k.p;
  const float *rgb = k.rgb, *outRgb = k.outRgb, *outLength = k.outLength;
  if (!k.progressive && (!rgb || !k.depth || !k.ns)) return Fail(QA_EINVAL, "null buffer");
  if (k.noParams) return Fail(QA_EINVAL, "null parameters");
  if (p.flags & ~allowedFlags) return Fail(QA_EINVAL, "unknown flags");
  if (!k.prev || !k.cur) return Fail(QA_EINVAL, "null camera");
  if (!k.hRgb || !k.hDepth || !k.hLength || !outRgb || !outLength) return Fail(QA_EINVAL, "null buffer");
  // (a side of 2^24 at most: pixel coordinates are exact floats)
  if (k.W < 1 || k.H < 1 || k.x0 < 0 || k.y0 < 0 || k.x0 > (1 << 24) - k.W || k.y0 > (1 << 24) - k.H) return Fail(QA_EINVAL, "bad frame size");
  if ((uint64_t) k.W * (uint64_t) k.H > 0x7FFFFFFFull) return Fail(QA_EINVAL, "too many pixels");
  if (!std::isfinite(p.depth_tolerance) || p.depth_tolerance < 0.f) return Fail(QA_EINVAL, "a depth_tolerance that is not finite or is negative");
  if (!std::isfinite(p.max_history) || !(p.max_history > 0.f)) return Fail(QA_EINVAL, "a max_history that is not finite and positive");
  const bool idsGiven = k.progressive ? k.hIds != nullptr : k.ids != nullptr;   // (a progressive frame computes its own when the history has them)
  if (idsGiven != (k.hIds != nullptr)) return Fail(QA_EINVAL, "one ids plane without the other");
  const size_t n = (size_t) k.W * (size_t) k.H;
  const struct { const void *p; size_t bytes; bool history; } in[] = {{rgb, 12 * n, false}, {k.depth, 4 * n, false}, {k.ns, 4 * n, false}, {k.ids, 8 * n, false},
                                                                     {k.hRgb, 12 * n, true}, {k.hDepth, 4 * n, true}, {k.hLength, 4 * n, true}, {k.hIds, 8 * n, true}};
  if (Overlap(outRgb, 12 * n, outLength, 4 * n)) return Fail(QA_EINVAL, "the outputs overlap");
  for (const auto &b : in) {
    if (b.history && (Overlap(outRgb, 12 * n, b.p, b.bytes) || Overlap(outLength, 4 * n, b.p, b.bytes)))
      return Fail(QA_EINVAL, "an output aliases a history plane");
    // a pixel reads only its own current pixel: the colour may be written where it was read, and nothing else may overlap
    const bool inPlace = b.p == rgb && outRgb == rgb;
    if (!b.history && !inPlace && Overlap(outRgb, 12 * n, b.p, b.bytes))
      return Fail(QA_EINVAL, "an output overlaps an input (only d_out_rgb == d_rgb is allowed)");
    if (!b.history && Overlap(outLength, 4 * n, b.p, b.bytes)) return Fail(QA_EINVAL, "an output overlaps an input (only d_out_rgb == d_rgb is allowed)");
  }
  const bool motionOn = (p.flags & QA_REPROJECT_MOTION) != 0u;
  const size_t motionBytes = motionOn ? (size_t) k.count * sizeof(qa_node_motion) : 0;
  if (motionOn) {
    if (!k.motion) return Fail(QA_EINVAL, "QA_REPROJECT_MOTION without a motion table");
    if (k.count < 1) return Fail(QA_EINVAL, "QA_REPROJECT_MOTION with a motion_count below 1");
    if ((uintptr_t) k.motion % alignof(qa_node_motion)) return Fail(QA_EINVAL, "a misaligned motion table");
    if (!idsGiven || !k.hIds) return Fail(QA_EINVAL, "QA_REPROJECT_MOTION needs both ids planes");
    if (Overlap(outRgb, 12 * n, k.motion, motionBytes) || Overlap(outLength, 4 * n, k.motion, motionBytes))
      return Fail(QA_EINVAL, "an output overlaps the motion table");
  }
  if (p.flags & QA_REPROJECT_CLAMP) {
    if (p.clamp_radius < 1 || p.clamp_radius > QA_REPROJECT_MAX_RADIUS) return Fail(QA_EINVAL, "a clamp_radius outside 1 .. 3");
    if (!std::isfinite(p.clamp_gamma) || p.clamp_gamma < 0.f) return Fail(QA_EINVAL, "a clamp_gamma that is not finite or is negative");
    if (rgb && outRgb == rgb) return Fail(QA_EINVAL, "QA_REPROJECT_CLAMP reads the neighbours' current colours: d_out_rgb == d_rgb is not allowed with it");
  }
  if (p.flags & QA_REPROJECT_SHORTEN) {
    if (!(p.flags & QA_REPROJECT_CLAMP)) return Fail(QA_EINVAL, "QA_REPROJECT_SHORTEN without QA_REPROJECT_CLAMP");
    if (!std::isfinite(p.shorten_rate) || p.shorten_rate < 0.f) return Fail(QA_EINVAL, "a shorten_rate that is not finite or is negative");
  }
  if (!(p.flags & QA_REPROJECT_MOMENTS)) return QA_OK;
  const float *hMoments = k.hMoments, *outMoments = k.outMoments, *outVariance = k.outVariance;
  if (!std::isfinite(p.min_frames) || !(p.min_frames >= 1.f)) return Fail(QA_EINVAL, "a min_frames that is not finite or is below 1");
  if (!outMoments || !outVariance) return Fail(QA_EINVAL, "QA_REPROJECT_MOMENTS without both d_out_moments and d_out_variance");
  if (hMoments && outMoments == hMoments) return Fail(QA_EINVAL, "d_out_moments is the history's moments plane");
  if ((uintptr_t) hMoments % 8 || (uintptr_t) outMoments % 8) return Fail(QA_EINVAL, "a moments plane that is not 8-byte aligned");
  // the two new outputs overlap nothing: no input, no history plane, no other output, not the motion table
  const struct { const void *p; size_t bytes; } other[] = {{rgb, 12 * n}, {k.depth, 4 * n}, {k.ns, 4 * n}, {k.ids, 8 * n}, {k.hRgb, 12 * n}, {k.hDepth, 4 * n},
                                                          {k.hLength, 4 * n}, {k.hIds, 8 * n}, {hMoments, 8 * n}, {outRgb, 12 * n}, {outLength, 4 * n},
                                                          {motionOn ? k.motion : nullptr, motionBytes}};
  if (Overlap(outMoments, 8 * n, outVariance, 4 * n)) return Fail(QA_EINVAL, "the outputs overlap");
  for (const auto &b : other)
    if (Overlap(outMoments, 8 * n, b.p, b.bytes) || Overlap(outVariance, 4 * n, b.p, b.bytes))
      return Fail(QA_EINVAL, "d_out_moments or d_out_variance overlaps another plane of the call");
  // and the old outputs stay clear of the history's moments
  if (Overlap(outRgb, 12 * n, hMoments, 8 * n) || Overlap(outLength, 4 * n, hMoments, 8 * n)) return Fail(QA_EINVAL, "an output aliases a history plane");
  return QA_OK;
}

static qa::ReprojectMotionSetup MotionSetup(const ReprojectCall &k)
{
  const bool on = (k.p.flags & QA_REPROJECT_MOTION) != 0u;
  return {on ? k.motion : nullptr, on ? k.count : 0, k.p.flags, (k.p.flags & QA_REPROJECT_CLAMP) ? k.p.clamp_radius : 0, k.p.clamp_gamma};
}

// A checked call on stream s, by the kernel of the entry's own rank (whatever the flags: qa_reproject_motion_device with flags 0
// still stages nothing and still runs the kernel that could)
template <int FORM>
static int LaunchReproject(const ReprojectCall &k, hipStream_t s)
{
  const int withIds = (k.ids && k.hIds) ? 1 : 0, withMoments = ((k.p.flags & QA_REPROJECT_MOMENTS) && k.hMoments) ? 1 : 0;
  const qa::ReprojectArgs args = {reprojectSetup(*k.prev, *k.cur, k.x0, k.y0, k.W, k.H, k.p.depth_tolerance, k.p.max_history),
                                  MotionSetup(k),
                                  {k.p.min_frames, k.p.shorten_rate},
                                  {k.rgb, k.depth, k.ns, k.state, k.W},
                                  {k.hRgb, k.hDepth, k.hLength, k.W},
                                  {reinterpret_cast<const float2 *>(k.hMoments), k.W},
                                  {{k.ids, k.hIds}, k.W},
                                  withIds, withMoments, k.outRgb, k.outLength, reinterpret_cast<float2 *>(k.outMoments), k.outVariance};
  const dim3 grid((unsigned) ((k.W + QA_REPROJECT_TILE - 1) / QA_REPROJECT_TILE), (unsigned) ((k.H + QA_REPROJECT_TILE - 1) / QA_REPROJECT_TILE)), block(256);
  hipLaunchKernelGGL(qa::qa_reproject_k<FORM>, grid, block, 0, s, args);
  HIP_TRY(hipGetLastError());
  return QA_OK;
}

// What the three qa_progressive_reproject*_device entries share: k holds the history, the outputs and the parameters; the current
// frame, its region and its camera are the context's
template <int FORM>
static int ProgressiveReproject(qa_ctx *c, ReprojectCall &k, void *hip_stream)
{
  int rc = ProgActive(c);
  if (rc != QA_OK) return rc;
  const qa_ctx::Progressive &f = c->prog;
  if (f.stale) return Fail(QA_EINVAL, "the frame's pixels are not the resident camera's (the scene was edited): qa_progressive_restart first");
  k.x0 = f.args.x0; k.y0 = f.args.y0; k.W = f.args.x1 - f.args.x0; k.H = f.args.y1 - f.args.y0;
  // the camera the frame was rendered from: the header's camera block of the resident blob, as qa_scene_edit_camera leaves it
  qa_camera cam;
  memcpy(&cam, c->hostBlob.data() + offsetof(qa_flat_header, screenA), sizeof(qa_camera));
  k.cur = &cam;
  k.progressive = true;
  if ((rc = CheckReproject(k, FlagsOf(FORM))) != QA_OK) return rc;
  HIP_TRY(hipSetDevice(c->device));
  hipStream_t s = StreamOf(c, hip_stream);
  HIP_TRY(f.done.WaitOn(s));
  int32_t *ids = nullptr;
  if (k.hIds) {
    // the current ids: the context's plane (it only grows; the old one may be in use on a stream of the caller's), every entry of
    // which the guide kernel writes on s before the reprojection reads it
    HIP_TRY(c->reprojectIds.Reserve((size_t) k.W * (size_t) k.H * 8, true));
    HIP_TRY(c->lastReproject.WaitOn(s));
    ids = static_cast<int32_t *>(c->reprojectIds.p);
    if ((rc = qa_progressive_gbuffer_device(c, nullptr, nullptr, nullptr, ids, hip_stream)) != QA_OK) return rc;
  }
  k.rgb = f.args.rgb; k.depth = f.args.depth; k.ns = f.args.ns; k.state = f.dState; k.ids = ids;
  if ((rc = LaunchReproject<FORM>(k, s)) != QA_OK) return rc;
  if (ids) HIP_TRY(c->lastReproject.Record(s));
  return QA_OK;
}

// The same source on the CPU, pixel after pixel (no GPU, no context): what the three qa_test_reproject*_host entries share
template <int FORM>
static int ReprojectOnHost(const ReprojectCall &k)
{
  if (int rc = CheckReproject(k, FlagsOf(FORM))) return rc;
  const int W = k.W, H = k.H;
  const ReprojectSetup S = reprojectSetup(*k.prev, *k.cur, k.x0, k.y0, W, H, k.p.depth_tolerance, k.p.max_history);
  const ReprojectMotionSetup M = MotionSetup(k);
  const ReprojectMomentsSetup X = {k.p.min_frames, k.p.shorten_rate};
  const float *rgb = k.rgb, *depth = k.depth;
  const uint32_t *ns = k.ns;
  const auto src = [=](int x, int y) {
    const size_t q = (size_t) y * (size_t) W + (size_t) x;
    ReprojectPixel px;
    px.r = rgb[3 * q]; px.g = rgb[3 * q + 1]; px.b = rgb[3 * q + 2]; px.z = depth[q]; px.ns = ns[q];
    return px;
  };
  const auto win = [=](int x, int y) {
    if (x < 0 || y < 0 || x >= W || y >= H) {
      const ReprojectWin none = {0.f, 0.f, 0.f, 0u};
      return none;
    }
    return reprojectWinOf(src(x, y));
  };
  const ReprojectHistory hist = {k.hRgb, k.hDepth, k.hLength, W};
  const ReprojectMomentPlane mom = {reinterpret_cast<const float2 *>(k.hMoments), W};
  const ReprojectIds id = {{k.ids, k.hIds}, W};
  const bool withMoments = (k.p.flags & QA_REPROJECT_MOMENTS) && k.hMoments;
  for (int y = 0; y < H; ++y)
    for (int x = 0; x < W; ++x) {
      const size_t q = (size_t) y * (size_t) W + (size_t) x;
      float o[3], om[2], var;
      k.outLength[q] = reprojectPixel<FORM>(S, M, X, src, hist, mom, id, win, k.ids != nullptr, withMoments, x, y, o, om, var);
      k.outRgb[3 * q] = o[0]; k.outRgb[3 * q + 1] = o[1]; k.outRgb[3 * q + 2] = o[2];
      if constexpr (FORM >= 2) {
        if (k.p.flags & QA_REPROJECT_MOMENTS) {
          k.outMoments[2 * q] = om[0]; k.outMoments[2 * q + 1] = om[1];
          k.outVariance[q] = var;
        }
      }
    }
  return QA_OK;
}

// A 3x4 affine map in double: x -> a x + t (a row-major)
struct Affine {
  double a[9], t[3];
};
static Affine Compose(const Affine &f, const Affine &g)   // f o g
{
  Affine r;
  for (int i = 0; i < 3; ++i) {
    for (int j = 0; j < 3; ++j) r.a[3 * i + j] = f.a[3 * i] * g.a[j] + f.a[3 * i + 1] * g.a[3 + j] + f.a[3 * i + 2] * g.a[6 + j];
    r.t[i] = f.a[3 * i] * g.t[0] + f.a[3 * i + 1] * g.t[1] + f.a[3 * i + 2] * g.t[2] + f.t[i];
  }
  return r;
}

extern "C" {

int qa_reproject_params_default(qa_reproject_params *p)
{
  if (!p) return Fail(QA_EINVAL, "null parameters");
  p->depth_tolerance = QA_REPROJECT_DEFAULT_DEPTH_TOLERANCE;
  p->max_history = QA_REPROJECT_DEFAULT_MAX_HISTORY;
  p->flags = 0u;
  return QA_OK;
}

int qa_reproject_device(qa_ctx *c, const qa_camera *prev_cam, const qa_camera *cur_cam, int x0, int y0, int width, int height, const float *d_rgb,
                        const float *d_depth, const uint32_t *d_ns, const int32_t *d_ids, const float *d_hist_rgb, const float *d_hist_depth,
                        const float *d_hist_length, const int32_t *d_hist_ids, const qa_reproject_params *p, float *d_out_rgb, float *d_out_length,
                        void *hip_stream)
{
  if (int rc = Enter(c)) return rc;
  ReprojectCall k = {prev_cam, cur_cam, x0, y0, width, height, d_rgb, d_depth, d_ns, d_ids, d_hist_rgb, d_hist_depth, d_hist_length, d_hist_ids,
                     nullptr, nullptr, 0, d_out_rgb, d_out_length};
  WithParams(k, p);
  if (int rc = CheckReproject(k, FlagsOf(0))) return rc;
  return LaunchReproject<0>(k, StreamOf(c, hip_stream));
}

int qa_progressive_reproject_device(qa_ctx *c, const qa_camera *prev_cam, const float *d_hist_rgb, const float *d_hist_depth, const float *d_hist_length,
                                    const int32_t *d_hist_ids, const qa_reproject_params *p, float *d_out_rgb, float *d_out_length, void *hip_stream)
{
  ReprojectCall k = {prev_cam, nullptr, 0, 0, 0, 0, nullptr, nullptr, nullptr, nullptr, d_hist_rgb, d_hist_depth, d_hist_length, d_hist_ids,
                     nullptr, nullptr, 0, d_out_rgb, d_out_length};
  WithParams(k, p);
  return ProgressiveReproject<0>(c, k, hip_stream);
}

int qa_test_reproject_host(const qa_camera *prev_cam, const qa_camera *cur_cam, int x0, int y0, int width, int height, const float *rgb, const float *depth,
                           const uint32_t *ns, const int32_t *ids, const float *hist_rgb, const float *hist_depth, const float *hist_length,
                           const int32_t *hist_ids, const qa_reproject_params *p, float *out_rgb, float *out_length)
{
  ReprojectCall k = {prev_cam, cur_cam, x0, y0, width, height, rgb, depth, ns, ids, hist_rgb, hist_depth, hist_length, hist_ids,
                     nullptr, nullptr, 0, out_rgb, out_length};
  WithParams(k, p);
  return ReprojectOnHost<0>(k);
}

int qa_reproject_motion_params_default(qa_reproject_motion_params *p)
{
  if (!p) return Fail(QA_EINVAL, "null parameters");
  p->depth_tolerance = QA_REPROJECT_DEFAULT_DEPTH_TOLERANCE;
  p->max_history = QA_REPROJECT_DEFAULT_MAX_HISTORY;
  p->clamp_gamma = QA_REPROJECT_DEFAULT_CLAMP_GAMMA;
  p->clamp_radius = QA_REPROJECT_DEFAULT_CLAMP_RADIUS;
  p->flags = 0u;
  return QA_OK;
}

int qa_reproject_node_motion(const qa_instance *prev, const qa_instance *cur, int count, qa_node_motion *out)
{
  if (!prev || !cur || !out) return Fail(QA_EINVAL, "null table");
  if (count < 1) return Fail(QA_EINVAL, "count below 1");
  for (int k = 0; k < count; ++k) {
    if (prev[k].parent != cur[k].parent || prev[k].subtree_end != cur[k].subtree_end || prev[k].depth != cur[k].depth)
      return Fail(QA_EINVAL, "the tables differ in parent, subtree_end or depth: not two states of one scene graph");
    if (cur[k].parent < -1 || cur[k].parent >= k) return Fail(QA_EINVAL, "a parent that does not precede its node (the table is in depth-first pre-order)");
  }
  // per node: Wprev(k), Wcur(k)^-1 and whether k or an ancestor differs
  std::vector<Affine> wPrev((size_t) count), wInv((size_t) count);
  std::vector<uint8_t> moved((size_t) count);
  for (int k = 0; k < count; ++k) {
    const qa_instance &a = prev[k], &b = cur[k];
    Affine lPrev, lInv;   // L_k of the previous table: tm p + pos;  L_k^-1 of the current one: itm (q - pos) = itm q - itm pos
    for (int i = 0; i < 3; ++i) {
      for (int j = 0; j < 3; ++j) {
        lPrev.a[3 * i + j] = (double) a.tm[3 * j + i];   // (tm and itm are column-major)
        lInv.a[3 * i + j] = (double) b.itm[3 * j + i];
      }
      lPrev.t[i] = (double) a.pos[i];
    }
    for (int i = 0; i < 3; ++i)
      lInv.t[i] = -(lInv.a[3 * i] * (double) b.pos[0] + lInv.a[3 * i + 1] * (double) b.pos[1] + lInv.a[3 * i + 2] * (double) b.pos[2]);
    bool differs = false;
    for (int i = 0; i < 9; ++i) differs = differs || !(a.tm[i] == b.tm[i]) || !(a.itm[i] == b.itm[i]);
    for (int i = 0; i < 3; ++i) differs = differs || !(a.pos[i] == b.pos[i]);
    const int parent = b.parent;
    wPrev[k] = parent < 0 ? lPrev : Compose(wPrev[parent], lPrev);
    wInv[k] = parent < 0 ? lInv : Compose(lInv, wInv[parent]);
    moved[k] = (uint8_t) (differs || (parent >= 0 && moved[parent]));
    qa_node_motion &o = out[k];
    memset(&o, 0, sizeof o);
    o.m[0] = o.m[4] = o.m[8] = 1.f;
    if (moved[k]) {
      const Affine m = Compose(wPrev[k], wInv[k]);
      for (int i = 0; i < 9; ++i) o.m[i] = (float) m.a[i];
      for (int i = 0; i < 3; ++i) o.m[9 + i] = (float) m.t[i];
      o.moved = 1u;
    }
  }
  return QA_OK;
}

int qa_reproject_motion_device(qa_ctx *c, const qa_camera *prev_cam, const qa_camera *cur_cam, int x0, int y0, int width, int height, const float *d_rgb,
                               const float *d_depth, const uint32_t *d_ns, const int32_t *d_ids, const float *d_hist_rgb, const float *d_hist_depth,
                               const float *d_hist_length, const int32_t *d_hist_ids, const qa_node_motion *d_motion, int motion_count,
                               const qa_reproject_motion_params *p, float *d_out_rgb, float *d_out_length, void *hip_stream)
{
  if (int rc = Enter(c)) return rc;
  ReprojectCall k = {prev_cam, cur_cam, x0, y0, width, height, d_rgb, d_depth, d_ns, d_ids, d_hist_rgb, d_hist_depth, d_hist_length, d_hist_ids,
                     nullptr, d_motion, motion_count, d_out_rgb, d_out_length};
  WithParams(k, p);
  if (int rc = CheckReproject(k, FlagsOf(1))) return rc;
  return LaunchReproject<1>(k, StreamOf(c, hip_stream));
}

int qa_progressive_reproject_motion_device(qa_ctx *c, const qa_camera *prev_cam, const float *d_hist_rgb, const float *d_hist_depth, const float *d_hist_length,
                                           const int32_t *d_hist_ids, const qa_node_motion *d_motion, int motion_count, const qa_reproject_motion_params *p,
                                           float *d_out_rgb, float *d_out_length, void *hip_stream)
{
  ReprojectCall k = {prev_cam, nullptr, 0, 0, 0, 0, nullptr, nullptr, nullptr, nullptr, d_hist_rgb, d_hist_depth, d_hist_length, d_hist_ids,
                     nullptr, d_motion, motion_count, d_out_rgb, d_out_length};
  WithParams(k, p);
  return ProgressiveReproject<1>(c, k, hip_stream);
}

int qa_test_reproject_motion_host(const qa_camera *prev_cam, const qa_camera *cur_cam, int x0, int y0, int width, int height, const float *rgb,
                                  const float *depth, const uint32_t *ns, const int32_t *ids, const float *hist_rgb, const float *hist_depth,
                                  const float *hist_length, const int32_t *hist_ids, const qa_node_motion *motion, int motion_count,
                                  const qa_reproject_motion_params *p, float *out_rgb, float *out_length)
{
  ReprojectCall k = {prev_cam, cur_cam, x0, y0, width, height, rgb, depth, ns, ids, hist_rgb, hist_depth, hist_length, hist_ids,
                     nullptr, motion, motion_count, out_rgb, out_length};
  WithParams(k, p);
  return ReprojectOnHost<1>(k);
}

int qa_reproject_moments_params_default(qa_reproject_moments_params *p)
{
  if (!p) return Fail(QA_EINVAL, "null parameters");
  p->depth_tolerance = QA_REPROJECT_DEFAULT_DEPTH_TOLERANCE;
  p->max_history = QA_REPROJECT_DEFAULT_MAX_HISTORY;
  p->clamp_gamma = QA_REPROJECT_DEFAULT_CLAMP_GAMMA;
  p->min_frames = QA_REPROJECT_DEFAULT_MIN_FRAMES;
  p->shorten_rate = QA_REPROJECT_DEFAULT_SHORTEN_RATE;
  p->clamp_radius = QA_REPROJECT_DEFAULT_CLAMP_RADIUS;
  p->flags = 0u;
  return QA_OK;
}

int qa_reproject_moments_device(qa_ctx *c, const qa_camera *prev_cam, const qa_camera *cur_cam, int x0, int y0, int width, int height, const float *d_rgb,
                                const float *d_depth, const uint32_t *d_ns, const int32_t *d_ids, const float *d_hist_rgb, const float *d_hist_depth,
                                const float *d_hist_length, const int32_t *d_hist_ids, const float *d_hist_moments, const qa_node_motion *d_motion,
                                int motion_count, const qa_reproject_moments_params *p, float *d_out_rgb, float *d_out_length, float *d_out_moments,
                                float *d_out_variance, void *hip_stream)
{
  if (int rc = Enter(c)) return rc;
  ReprojectCall k = {prev_cam, cur_cam, x0, y0, width, height, d_rgb, d_depth, d_ns, d_ids, d_hist_rgb, d_hist_depth, d_hist_length, d_hist_ids,
                     d_hist_moments, d_motion, motion_count, d_out_rgb, d_out_length, d_out_moments, d_out_variance};
  WithParams(k, p);
  if (int rc = CheckReproject(k, FlagsOf(2))) return rc;
  return LaunchReproject<2>(k, StreamOf(c, hip_stream));
}

int qa_progressive_reproject_moments_device(qa_ctx *c, const qa_camera *prev_cam, const float *d_hist_rgb, const float *d_hist_depth,
                                            const float *d_hist_length, const int32_t *d_hist_ids, const float *d_hist_moments,
                                            const qa_node_motion *d_motion, int motion_count, const qa_reproject_moments_params *p, float *d_out_rgb,
                                            float *d_out_length, float *d_out_moments, float *d_out_variance, void *hip_stream)
{
  ReprojectCall k = {prev_cam, nullptr, 0, 0, 0, 0, nullptr, nullptr, nullptr, nullptr, d_hist_rgb, d_hist_depth, d_hist_length, d_hist_ids,
                     d_hist_moments, d_motion, motion_count, d_out_rgb, d_out_length, d_out_moments, d_out_variance};
  WithParams(k, p);
  return ProgressiveReproject<2>(c, k, hip_stream);
}

int qa_test_reproject_moments_host(const qa_camera *prev_cam, const qa_camera *cur_cam, int x0, int y0, int width, int height, const float *rgb,
                                   const float *depth, const uint32_t *ns, const int32_t *ids, const float *hist_rgb, const float *hist_depth,
                                   const float *hist_length, const int32_t *hist_ids, const float *hist_moments, const qa_node_motion *motion,
                                   int motion_count, const qa_reproject_moments_params *p, float *out_rgb, float *out_length, float *out_moments,
                                   float *out_variance)
{
  ReprojectCall k = {prev_cam, cur_cam, x0, y0, width, height, rgb, depth, ns, ids, hist_rgb, hist_depth, hist_length, hist_ids,
                     hist_moments, motion, motion_count, out_rgb, out_length, out_moments, out_variance};
  WithParams(k, p);
  return ReprojectOnHost<2>(k);
}

}  // extern "C"
