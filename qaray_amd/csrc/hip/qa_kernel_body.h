// qa_kernel_body.h - the body of the per-lane megakernel (qa_kernel.h), included by its two entry points: qa_integrate and
// qa_integrate_rays, and a third, qa_integrate_points (qa_integrate_lastcast has a body of its own, qa_kernel_lastcast_body.h).  Not a header of its own: it is the text
// of a function whose parameters are `sc` and `rp`, with the template parameters RES, LIGHTS, TEX, AREA, STATS, PHOTON, the constants
// RAYS and POINTS and the ray batch `rb` (RayBatch; empty unless RAYS) in scope.  (A text include rather than an inline function, as qa_kernel_cs_body.h: the shipped
// instances keep exactly the code they had - through a function the kernel arguments are copied to scratch and the AREA variants
// spill a thousand registers.)
// RAYS (qa_integrate_rays; the opening comment of qa_radiance.hip is the specification): the paths start from the rays of `rb` and
// not from the camera.  Only the work items (section A), the start of a sample (B), the first ray's miss (C) and the output sites
// differ, each under `if constexpr (RAYS)`: with RAYS false the text below is the text the shipped kernels were compiled from.
// POINTS (qa_integrate_points, RAYS with it; the opening comment of qa_irradiance.hip is the specification): `rb` holds surface
// points and normals where a ray batch holds origins and directions, and a sample starts by shading its point instead of tracing
// a first segment - one block ahead of the sweep of section C, under `if constexpr (POINTS)`; with POINTS false the text is
// qa_integrate_rays'.
  extern __shared__ uint4 s_dyn[];
  SceneMem<RES> mem;
  mem.img = s_dyn;
  if (RES) {
    for (uint32_t i = threadIdx.x; i < sc.residentVec4; i += QA_BLOCK) s_dyn[i] = sc.resident[i];
    __syncthreads();
  }
  uint32_t *stack = reinterpret_cast<uint32_t *>(s_dyn + (RES ? sc.residentVec4 : 0)) + threadIdx.x;
  // per-lane sample accumulators (running mean + variance of SuperSamplerHalton) live in LDS: they
  // are touched once per sample, registers are better spent on the traversal
  float *acc = reinterpret_cast<float *>(stack + (size_t) sc.stackDepth * QA_BLOCK - threadIdx.x) + threadIdx.x;
  const uint4 *mtlTable = RES ? s_dyn + sc.resMaterials : reinterpret_cast<const uint4 *>(sc.mtl);
  // LDS-resident scenes have shallow stacks: their workgroups also keep the path's throughput and radiance, the pixel, its output
  // index and the sample index in LDS columns (QA_LANE_SLOTS_RES) - state touched at a handful of points of an iteration
  constexpr bool LCOLS = RES && !PHOTON;   // (a photon gather's stack is deep: those variants keep the registers)
  if (LCOLS)
    for (int i = QA_LANE_SLOTS; i < QA_LANE_SLOTS_RES; ++i) acc[i * QA_BLOCK] = 0.f;
#define QA_GET_T() (LCOLS ? F3(acc[6 * QA_BLOCK], acc[7 * QA_BLOCK], acc[8 * QA_BLOCK]) : path.T)
#define QA_GET_L() (LCOLS ? F3(acc[9 * QA_BLOCK], acc[10 * QA_BLOCK], acc[11 * QA_BLOCK]) : path.L)
#define QA_PUT_T(...) { const f3 v_ = (__VA_ARGS__); if (LCOLS) { acc[6 * QA_BLOCK] = v_.x; acc[7 * QA_BLOCK] = v_.y; acc[8 * QA_BLOCK] = v_.z; } else path.T = v_; }
#define QA_PUT_L(...) { const f3 v_ = (__VA_ARGS__); if (LCOLS) { acc[9 * QA_BLOCK] = v_.x; acc[10 * QA_BLOCK] = v_.y; acc[11 * QA_BLOCK] = v_.z; } else path.L = v_; }
#define QA_GET_Q() (LCOLS ? __float_as_uint(acc[13 * QA_BLOCK]) : q)
#define QA_GET_SIDX() (LCOLS ? __float_as_int(acc[14 * QA_BLOCK]) : sidx)
  // Tile lists for the camera rays (qa_tilecull.h): the wave's area behind the per-lane columns, when the launch made room for it.
  // With depth of field the camera rays of a tile share no origin.
  // (in the variant without lights only: the lit and textured resident variants pay for the shared text in spilled registers)
  constexpr bool TL = RES && !LIGHTS && !TEX && !AREA && !STATS && !PHOTON && !RAYS;   // (rays of a batch share no tile)
  uint32_t *tileList = nullptr;
  if constexpr (TL)
    if (rp.tile_lists > 0 && !(sc.cam.dof > 0.1f))
      tileList = reinterpret_cast<uint32_t *>(s_dyn + sc.residentVec4) + ((size_t) sc.stackDepth + QA_LANE_SLOTS_RES) * QA_BLOCK +
                 __builtin_amdgcn_readfirstlane(threadIdx.x / 64) * QA_TILE_LIST_DWORDS;

  // work items walk 8x8 pixel tiles (a wave starts on a compact screen patch); ragged right /
  // bottom tiles contain padding slots that are simply skipped.
  // A launch may own only every tile_row_step-th 8-row strip of the region (round-robin image
  // partition between GPUs, the reference's ThreadRender(tileStart=rank, step=size),
  // src/renderers/renderer.cpp:383-387); its outputs are packed strip after strip.
  const int rw = rp.x1 - rp.x0, rh = rp.y1 - rp.y0;
  const unsigned tilesX = (unsigned) (rw + 7) / 8;
  // Tiles in sample chunks (RenderParams::chunk_spp): a frame of few tiles per wave ends with waves idle while the last tiles finish
  // their hundreds of samples (1080p at 512 spp on 5 120 waves: 6.3 tiles of ~12 ms per wave, 11 % of the wave slots empty on
  // average).  A pixel's samples cannot be shared out - one random-number stream, one running variance - but they can be HANDED ON:
  // a work item is (chunk, tile), all tiles' chunk 0 first; at the end of a chunk every lane stores its pixel's state, the wave
  // publishes the tile's progress (agent-scope release), and whoever fetches (chunk + 1, tile) - a whole pass of the frame later -
  // reads the state back behind an acquire.  Same samples in the same order for every pixel: same bits.
  const unsigned numTiles = tilesX * (unsigned) rp.own_tile_rows;
  // (RAYS: a work item is 64 consecutive rays, lane = ray)
  const unsigned total = RAYS ? (rb.n + 63u) / 64u * 64u : numTiles * (rp.chunk_spp ? rp.num_chunks : 1u) * 64u;
  const unsigned lane = __lane_id();
  unsigned curTile = 0xFFFFFFFFu, curChunk = 0;   // (wave-uniform) the work item in hand
  int chunkEnd = 0x7FFFFFFF;                      // samples a pixel has when its chunk is complete

  DCounters cnt = {};
#ifdef QA_STAMPS
  __shared__ unsigned long long s_stamps[QA_BLOCK / 64][QA_NSTAMPS];
  cnt.sl = s_stamps[threadIdx.x / 64];
  if (__lane_id() < QA_NSTAMPS) cnt.sl[__lane_id()] = 0;
#endif
  QA_T(tKernel)
  TexTables tt;
  tt.blob = sc.blob;
  tt.texels = sc.texels;
  tt.texOff = sc.texOff;
  tt.texmap = sc.texmap;
  tt.tex = sc.tex;
  tt.filter = sc.texFilter;
  int nrec = 0;               // AREA: hits logged for the current path
  float *rec = sc.areaScratch + (size_t) blockIdx.x * QA_BLOCK + threadIdx.x;  // + (lvl*19+f) * recStride
  const size_t recStride = (size_t) gridDim.x * QA_BLOCK;
  RayDiff pathDiff;           // TEX: differential directions of the current ray
  pathDiff.dx = pathDiff.dy = F3(0, 0, 1);

  // pixel state
  int px = 0, py = 0;
  unsigned q = 0;           // output index of the pixel
  uint32_t rng = 1;
  int sidx = 0;
  Path path;
  path.primary = true;
  path.ray.p = F3(0, 0, 0);
  path.ray.d = F3(0, 0, 1);
  path.T = F3(0, 0, 0);
  path.L = F3(0, 0, 0);
  path.absorbMtl = -1;
  path.bounce = 0;
  path.fromDiffuse = false;
  f3 texpos = F3(0, 0, 0);

  bool alive = true, needPixel = true, needSample = false;

  for (;;) {
    QA_T(tA)
    // ---- A. tile fetch: a wave owns one 8x8 pixel tile at a time (lane = pixel).  Rays of one
    // tile are coherent and cost about the same, so background tiles (every ray misses the scene
    // bounds) never share a wave with expensive ones.  One atomic per wave and tile; lanes that
    // finish their pixel early wait for the rest of the tile (the spread is a few percent).
    const unsigned long long aliveMask = __ballot(alive);
    const unsigned long long want = __ballot(alive && needPixel);
    if (want && want == aliveMask) {
      if (rp.chunk_spp && curTile != 0xFFFFFFFFu) {
        // the chunk in hand is complete: every lane has stored its pixel's state (section E); publish it
        // (the state words are agent-scope atomic stores - written through, no line of them stays in this XCD's L2 - and this wave
        // has waited for all of them: no release fence, whose write-back of the L2's dirty lines - the spilled registers of every
        // wave of the XCD - cost 170 us per hand-over; MI355X_MICROARCH.md, inter-workgroup visibility)
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        if (lane == 0) __hip_atomic_store(rp.tile_progress + curTile, curChunk + 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        curTile = 0xFFFFFFFFu;
      }
      unsigned base = 0;
      const int leader = __ffsll((long long) want) - 1;
      if ((int) lane == leader) base = (*rp.stop_flag) ? total : atomicAdd(rp.work_counter, 64u);
      base = __shfl(base, leader);
      unsigned item = base / 64;   // (wave-uniform) tile, or chunk * numTiles + tile
      if (rp.chunk_spp && base < total) {
        curChunk = item / numTiles;
        item -= curChunk * numTiles;
        curTile = item;
        chunkEnd = (int) (rp.chunk_spp + curChunk * rp.chunk_tail);
        if (curChunk > 0) {
          // the tile's previous chunk was handed out a whole pass of the frame ago: this wait ends at once, except on frames of
          // fewer tiles than waves.  Its holder is a resident wave that waits for nothing this wave holds; the bound is a guard
          // against a lost update, not a path that is taken (a frame that hit it would fail every parity test).
          for (int spins = 0; spins < (1 << 22); ++spins) {
            if (__hip_atomic_load(rp.tile_progress + curTile, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) >= curChunk) break;
            __builtin_amdgcn_s_sleep(16);
          }
          __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
        }
      }
      if constexpr (TL) {
        if (tileList && base < total) {
          const unsigned tile = rp.tile_order ? rp.tile_order[item] : item;
          const unsigned otr = tile / tilesX;
          buildTileLists<RES>(sc, (uint32_t) rp.tile_lists, (float) (rp.x0 + (int) ((tile % tilesX) * 8)),
                              (float) (rp.y0 + (int) (((unsigned) rp.tile_row0 + otr * (unsigned) rp.tile_row_step) * 8)), tileList,
                              reinterpret_cast<TileCone *>(stack - lane));   // row 0 of the wave's stacks: no walk is under way
          // every lane that is alive asks for a pixel here: what it holds of its last path is dead, and saying so keeps those
          // registers out of the way of the list build (a lane starts its next path from section B)
          path.ray.p = F3(0, 0, 0);
          path.ray.d = F3(0, 0, 1);
          path.absorbMtl = -1;
          path.bounce = 0;
          path.fromDiffuse = false;
          path.primary = true;
          rng = 1;
          sidx = 0;
          px = py = 0;
          q = 0;
        }
      }
      if (alive) {
        const unsigned w = base + lane;
        if (base >= total) {
          alive = false;
        } else if constexpr (RAYS) {
          if (w < rb.n) {   // (else: padding lane of the last item - this lane sits it out)
            q = w;
            rng = qa_pixel_seed(rp.seed, rb.stream ? rb.stream[q] : (uint32_t) q);
            sidx = 0;
            for (int i = 0; i < 6; ++i) acc[i * QA_BLOCK] = 0.f;
            needSample = true;
            needPixel = false;
            if (LCOLS) {
              acc[13 * QA_BLOCK] = __uint_as_float(q);
              acc[14 * QA_BLOCK] = __int_as_float(sidx);
            }
          }
        } else {
          const unsigned in = w % 64;
          const unsigned tile = rp.tile_order ? rp.tile_order[item] : item;
          const unsigned otr = tile / tilesX;  // index among the strips this launch owns
          const unsigned tx = (tile % tilesX) * 8 + (in % 8);
          const unsigned ty = ((unsigned) rp.tile_row0 + otr * (unsigned) rp.tile_row_step) * 8 + (in / 8);
          if (tx < (unsigned) rw && ty < (unsigned) rh) {
            px = rp.x0 + (int) tx;
            py = rp.y0 + (int) ty;
            q = (otr * 8 + (in / 8)) * (unsigned) rw + tx;
            rng = qa_pixel_seed(rp.seed, (uint32_t) py * (uint32_t) sc.cam.width + (uint32_t) px);
            sidx = 0;
            for (int i = 0; i < 6; ++i) acc[i * QA_BLOCK] = 0.f;
            needSample = true;
            needPixel = false;
            if (rp.chunk_spp && curChunk > 0) {
              // the pixel as the previous chunk left it
              const unsigned long long *st = reinterpret_cast<const unsigned long long *>(rp.pix_state) + 4 * (size_t) q;
              const unsigned long long s0 = __hip_atomic_load(st, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT), s1 = __hip_atomic_load(st + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT),
                                       s2 = __hip_atomic_load(st + 2, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT), s3 = __hip_atomic_load(st + 3, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
              const uint4 a = make_uint4((uint32_t) s0, (uint32_t) (s0 >> 32), (uint32_t) s1, (uint32_t) (s1 >> 32));
              const uint4 b = make_uint4((uint32_t) s2, (uint32_t) (s2 >> 32), (uint32_t) s3, (uint32_t) (s3 >> 32));
              if (a.y & 0x80000000u) {   // finished in an earlier chunk: the lane sits this one out
                needSample = false;
                needPixel = true;
              } else {
                rng = a.x;
                sidx = (int) a.y;
                acc[0] = __uint_as_float(a.z); acc[QA_BLOCK] = __uint_as_float(a.w); acc[2 * QA_BLOCK] = __uint_as_float(b.x);
                acc[3 * QA_BLOCK] = __uint_as_float(b.y); acc[4 * QA_BLOCK] = __uint_as_float(b.z); acc[5 * QA_BLOCK] = __uint_as_float(b.w);
              }
            }
            if (LCOLS) {
              acc[12 * QA_BLOCK] = __uint_as_float((unsigned) px | ((unsigned) py << 16));
              acc[13 * QA_BLOCK] = __uint_as_float(q);
              acc[14 * QA_BLOCK] = __int_as_float(sidx);
            }
          }
          // else: padding slot of a ragged tile - this lane sits the tile out
        }
      }
    }
    if (!__any(alive)) break;

    // ---- B. start a sample: camera ray (src/renderers/renderer.cpp:312-328) ------------------
    // (qa_firsthit.h restates the camera ray of this section, the reset of section C and the material lookup of section D for the
    // read-only passes: camTexpos / camLensPos / camPoint, hitInit / texHitInit, hitMaterial.  A change here is a change there.)
    // sync_samples: lanes wait until the whole wave is between samples, so that the coherent
    // camera rays of a tile are traced together instead of next to incoherent secondary rays
    const bool goSample = !rp.sync_samples || (__ballot(needSample) == __ballot(alive && !needPixel));
    if (alive && needSample && goSample) {
      const int si = QA_GET_SIDX();
      if constexpr (RAYS) {
        // sample si of ray q: the caller's ray, used as given (no Halton term, no camera, no lens draws)
        const size_t ri = (rb.flags & QA_RAYS_PER_SAMPLE) ? (size_t) QA_GET_Q() * (size_t) rp.spp_max + (size_t) si : (size_t) QA_GET_Q();
        path.ray.p = F3(rb.o[3 * ri], rb.o[3 * ri + 1], rb.o[3 * ri + 2]);
        path.ray.d = F3(rb.d[3 * ri], rb.d[3 * ri + 1], rb.d[3 * ri + 2]);
        if (TEX) {
          // without differentials a ray of no width: DiffRay(pos, dir), x = y = c - the filter takes its unfiltered branch
          pathDiff.dx = pathDiff.dy = path.ray.d;
          if (rb.dx) {
            pathDiff.dx = F3(rb.dx[3 * ri], rb.dx[3 * ri + 1], rb.dx[3 * ri + 2]);
            pathDiff.dy = F3(rb.dy[3 * ri], rb.dy[3 * ri + 1], rb.dy[3 * ri + 2]);
          }
          texpos = F3(0, 0, 0);   // where a missed first ray looks the background texmap up (pixels)
          if (rb.screen) texpos = F3(rb.screen[2 * ri], rb.screen[2 * ri + 1], 0.f);
        }
      } else {
      const float hx = sc.halton[2 * si], hy = sc.halton[2 * si + 1];
      if (LCOLS) {
        const unsigned pxy = __float_as_uint(acc[12 * QA_BLOCK]);
        texpos = F3(hx, hy, 0.f) + F3((float) (int) (pxy & 0xFFFFu), (float) (int) (pxy >> 16), 0.f);
      } else {
        texpos = F3(hx, hy, 0.f) + F3((float) px, (float) py, 0.f);
      }
      const f3 A = ld3(sc.cam.screenA), U = ld3(sc.cam.screenU), V = ld3(sc.cam.screenV);
      const f3 cpt = (A + U * texpos.x) + V * texpos.y;
      f3 campos = ld3(sc.cam.pos);
      if (sc.cam.dof > 0.1f) {
        // SuperSamplerHalton::NewDofSample (src/scene/scene.cpp:104-111)
        const float r1 = rng1(rng), r2 = rng1(rng);
        const float r = sc.cam.dof * qsqrt(r1);
        const float t = r2 * 2.f * QA_PI;
        campos = campos + (ld3(sc.cam.screenX) * (r * qcosf(t)) + ld3(sc.cam.screenY) * (r * qsinf(t)));
      }
      path.ray.p = campos;
      path.ray.d = normalize(cpt - campos);
      if (TEX) {
        // DiffRay x / y: the same pixel sample shifted by DiffRay::dx / dy (renderer.cpp:314-317)
        const f3 xpt = (A + U * (texpos.x + QA_DX)) + V * texpos.y;
        const f3 ypt = (A + U * texpos.x) + V * (texpos.y + QA_DX);
        pathDiff.dx = normalize(xpt - campos);
        pathDiff.dy = normalize(ypt - campos);
      }
      }
      QA_PUT_T(F3(1, 1, 1))
      QA_PUT_L(F3(0, 0, 0))
      path.absorbMtl = -1;
      path.bounce = rp.max_bounce;
      path.fromDiffuse = false;
      path.primary = true;
      needSample = false;
      nrec = 0;
      QA_TALLY(cnt.samples);
    }

    QA_TACC(cnt.sl[1], tA)
    // ---- C. trace ----------------------------------------------------------------------------
    bool done = false;  // path finished in this iteration
    if (alive && !needPixel && !needSample) {
      Hit h;
      h.z = QA_BIGFLOAT;
      h.node = -1;
      h.mtlID = 0;
      h.front = true;
      h.p = F3(0, 0, 0);
      h.N = F3(0, 0, 0);
      TexHit th;
      th.uvw = F3(0.5f, 0.5f, 0.5f);   // HitInfo::Init (src/core/hitinfo.cpp:31-42)
      th.duvw0 = th.duvw1 = F3(0, 0, 0);
      th.hasTexture = false;
      bool sweep = true;   // the closest-hit sweep and shading; RAYS: not for a void first ray
      if constexpr (RAYS) {
        // a void first ray (a component that is not finite, or direction 0) is not walked and draws nothing from the stream: the
        // sample is black, and it counts
        const Ray &r0 = path.ray;
        const bool finite = isfinite(r0.p.x) && isfinite(r0.p.y) && isfinite(r0.p.z) && isfinite(r0.d.x) && isfinite(r0.d.y) && isfinite(r0.d.z);
        if (path.primary && !(finite && !(r0.d.x == 0.f && r0.d.y == 0.f && r0.d.z == 0.f))) {
          if (QA_GET_SIDX() == 0 && rp.depth) rp.depth[QA_GET_Q()] = QA_BIGFLOAT;
          done = true;
          sweep = false;
        }
      }
      if constexpr (POINTS) {
        // The first "hit" of a sample is the caller's point: path.ray holds (P, N) from section B, and nothing is traced to get there.
        // Section D on a white diffuse material seen along the normal (V = N, front face): the lobe draw, the point's direct light
        // (AREA: record 0 of the log, replayed last), one cosine-weighted bounce flagged fromDiffuse.  The bounce ray is swept below,
        // in the same turn; a sample that spawns none (max_bounce 0, the roulette) ends here.
        if (path.primary && sweep) {
          const f3 p = path.ray.p, N = path.ray.d;
          const uint4 white[6] = {make_uint4(0x3F800000u, 0x3F800000u, 0x3F800000u, 0u), make_uint4(0u, 0u, 0u, 0u), make_uint4(0u, 0u, 0u, 0u),
                                  make_uint4(0u, 0u, 0u, 0u), make_uint4(0u, 0u, 0u, 0u), make_uint4(0u, 0u, 0u, 0u)};
          const Surface sf = shadeSurface<false>(white, sc, tt, 0, N, N, true, th, path.bounce, path.fromDiffuse, rng);
          QA_PUT_L(QA_GET_L() + QA_GET_T() * sf.emission)
          if constexpr (PHOTON) {
            // section D's gather at the point itself (qa_integrate_points_pm): the point's path has fromDiffuse = false, so the
            // caustics map alone, ahead of the point's direct light or its log record; the heap is the lane's, as in section D
            if (sf.selDiffuse) {
              uint2 *heap = rp.heap + ((size_t) blockIdx.x * QA_BLOCK + threadIdx.x) * (QA_PHOTON_GATHER + 1);
              QA_PUT_L(QA_GET_L() + QA_GET_T() * photonGather(rp.pm[1], p, N, N, sf.kd, sf.ks, sf.gloss, stack, heap))
            }
          }
          if (LIGHTS && !AREA)
            QA_PUT_L(QA_GET_L() + QA_GET_T() * directLight<RES, STATS>(mem, sc, p, N, N, sf.kd, sf.ks, sf.gloss, stack, cnt, rng))
          if (AREA && nrec < QA_MAX_PATH) {
            const f3 pT = QA_GET_T();
            const float v[QA_REC_FLOATS] = {p.x, p.y, p.z, N.x, N.y, N.z, N.x, N.y, N.z, pT.x, pT.y, pT.z,
                                            sf.kd.x, sf.kd.y, sf.kd.z, sf.ks.x, sf.ks.y, sf.ks.z, sf.gloss};
            for (int f = 0; f < QA_REC_FLOATS; ++f) rec[(size_t) (nrec * QA_REC_FLOATS + f) * recStride] = v[f];
            ++nrec;
          }
          if (sf.spawn) {
            path.ray.d = normalize(sf.nextDir);
            if (TEX) pathDiff.dx = pathDiff.dy = path.ray.d;
            QA_PUT_T(QA_GET_T() * sf.bxdf)
            path.bounce -= 1;
            path.fromDiffuse = sf.nextFromDiffuse;
            path.primary = false;
          } else {
            done = true;
            sweep = false;
          }
        }
      }
      if (sweep) {
      QA_T(tC)
      const bool found = traceClosest<RES, TEX, STATS, TL>(mem, sc, path.ray, pathDiff, h, th, stack, cnt, tileList, path.primary);
      QA_TACC(cnt.sl[2], tC)
      if constexpr (RAYS) {
        if (path.primary && QA_GET_SIDX() == 0 && rp.depth) rp.depth[QA_GET_Q()] = found ? h.z : QA_BIGFLOAT;   // (t is optional)
      } else {
      if (path.primary && QA_GET_SIDX() == 0) rp.depth[QA_GET_Q()] = found ? h.z : QA_BIGFLOAT;
      }

      QA_T(tM)
      if (!found) {
        // background for camera rays (renderer.cpp:337-341), environment otherwise
        // (MtlBlinn_PhotonMap.cpp:249-251); textured versions: TEX kernel variants
        if constexpr (RAYS) {
          // QA_RADIANCE_MISS_ENVIRONMENT sends a missed first ray to the environment by direction, as a bounce ray
          const bool asCamera = path.primary && !(rb.flags & QA_RAYS_MISS_ENVIRONMENT);
          f3 c = asCamera ? ld3(sc.background) : ld3(sc.environment);
          if (TEX) {
            if (asCamera)
              c = texColorSample(tt, c, sc.bgTexmap, F3(texpos.x / (float) sc.cam.width, texpos.y / (float) sc.cam.height, 0.f));
            else
              c = sampleEnvironment(tt, c, sc.envTexmap, path.ray.d);
          }
          QA_PUT_L(QA_GET_L() + QA_GET_T() * c)
        } else {
        f3 c = path.primary ? ld3(sc.background) : ld3(sc.environment);
        if (TEX) {
          if (path.primary)
            c = texColorSample(tt, c, sc.bgTexmap, F3(texpos.x / (float) sc.cam.width, texpos.y / (float) sc.cam.height, 0.f));
          else
            c = sampleEnvironment(tt, c, sc.envTexmap, path.ray.d);
        }
        QA_PUT_L(QA_GET_L() + QA_GET_T() * c)
        }
        done = true;
        QA_TACC(cnt.sl[10], tM)
      } else {
        // ---- D. shade: MtlBlinn_PhotonMap::Shade (MtlBlinn_PhotonMap.cpp:256-500) -----------
        // Beer-Lambert attenuation of everything this hit returns, when the ray arrives from
        // inside (ComputeSecondaryRay :244-248)
        if (!path.primary && !h.front && path.absorbMtl >= 0) {
          const uint4 ab = mtlTable[6 * (size_t) path.absorbMtl + 5];
          const f3 att = F3(qexpf(-asF(ab.x) * h.z), qexpf(-asF(ab.y) * h.z), qexpf(-asF(ab.z) * h.z));
          QA_PUT_T(QA_GET_T() * att)
        }
        const qa_instance &in = instAt<RES>(sc, h.node);
        int mi = -1;
        bool white = false;
        if (in.mtlset >= 0) {
          const qa_mtlset ms = sc.mtlset[in.mtlset];
          if (ms.multi) {
            if (h.mtlID >= 0 && h.mtlID < ms.count) mi = ms.first + h.mtlID;
            else white = true;  // MultiMtl::Shade returns (1,1,1) (materials.h:70-76)
          } else mi = ms.first;
        }
        if (mi < 0) {
          if (white) QA_PUT_L(QA_GET_L() + QA_GET_T())
          done = true;
        } else {
          const f3 V = -path.ray.d;
          const f3 N = h.N;
          const f3 p = h.p;
          QA_TACC(cnt.sl[11], tM)
          QA_T(tD)
          const Surface sf = shadeSurface<TEX>(mtlTable, sc, tt, mi, N, V, h.front, th, path.bounce, path.fromDiffuse, rng);
          QA_TACC(cnt.sl[4], tD)
          QA_PUT_L(QA_GET_L() + QA_GET_T() * sf.emission)
          const f3 sampleDiffuse = sf.kd, sampleSpecular = sf.ks;
          const float glossSpec = sf.gloss;
          const bool spawn = sf.spawn;
          const f3 nextDir = sf.nextDir, bxdf = sf.bxdf;
          const bool nextFromDiffuse = sf.nextFromDiffuse;

          if (PHOTON && sf.selDiffuse) {
            // this lane's heap: QA_PHOTON_GATHER + 1 consecutive elements of the scratch slab (the top levels of
            // a heap share a cache line that way: 10 - 12 % faster than slot-major columns)
            uint2 *heap = rp.heap + ((size_t) blockIdx.x * QA_BLOCK + threadIdx.x) * (QA_PHOTON_GATHER + 1);
            if (path.fromDiffuse)
              QA_PUT_L(QA_GET_L() + QA_GET_T() * photonGather(rp.pm[0], p, N, V, sampleDiffuse, sampleSpecular, glossSpec, stack, heap))
            QA_PUT_L(QA_GET_L() + QA_GET_T() * photonGather(rp.pm[1], p, N, V, sampleDiffuse, sampleSpecular, glossSpec, stack, heap))
          }

          // direct lighting (:481-498)
          if (LIGHTS && !AREA) {
            QA_T(tL)
            QA_PUT_L(QA_GET_L() + QA_GET_T() * directLight<RES, STATS>(mem, sc, p, N, V, sampleDiffuse, sampleSpecular, glossSpec, stack, cnt, rng))
            QA_TACC(cnt.sl[5], tL)
          }
          if (AREA && nrec < QA_MAX_PATH) {
            const f3 pT = QA_GET_T();
            const float v[QA_REC_FLOATS] = {p.x, p.y, p.z, N.x, N.y, N.z, V.x, V.y, V.z, pT.x, pT.y, pT.z,
                                            sampleDiffuse.x, sampleDiffuse.y, sampleDiffuse.z,
                                            sampleSpecular.x, sampleSpecular.y, sampleSpecular.z, glossSpec};
            for (int f = 0; f < QA_REC_FLOATS; ++f) rec[(size_t) (nrec * QA_REC_FLOATS + f) * recStride] = v[f];
            ++nrec;
          }

          QA_T(tS)
          if (spawn) {
            // ComputeSecondaryRay (:226-254): DiffRay(pos, dir).Normalize()
            path.ray.p = p;
            path.ray.d = normalize(nextDir);
            if (TEX) pathDiff.dx = pathDiff.dy = path.ray.d;  // DiffRay(pos, dir): x = y = c (ray.h:57-63)
            QA_PUT_T(QA_GET_T() * bxdf)
            path.absorbMtl = mi;
            path.bounce -= 1;
            path.fromDiffuse = nextFromDiffuse;
            path.primary = false;
          } else {
            done = true;
          }
          QA_TACC(cnt.sl[12], tS)
        }
      }
#ifdef QA_STAMPS
      if (!__any(path.primary)) QA_TACC(cnt.sl[20], tM)   // the part behind the sweep of casts in a wave without a camera ray
#endif
      }
    }

    // ---- E. sample finished: SuperSamplerHalton::Accumulate / Loop (scene.cpp:92-121) ---------
    QA_T(tE)
#ifdef QA_STAMPS
    if (lane == 0) cnt.sl[8] += 1;
#endif
    if (alive && done) {
      if (AREA) {
        for (int lvl = nrec - 1; lvl >= 0; --lvl) {
          float v[QA_REC_FLOATS];
          for (int f = 0; f < QA_REC_FLOATS; ++f) v[f] = rec[(size_t) (lvl * QA_REC_FLOATS + f) * recStride];
          const f3 d = directLight<RES, STATS>(mem, sc, F3(v[0], v[1], v[2]), F3(v[3], v[4], v[5]), F3(v[6], v[7], v[8]),
                                               F3(v[12], v[13], v[14]), F3(v[15], v[16], v[17]), v[18], stack, cnt, rng);
          QA_PUT_L(QA_GET_L() + F3(v[9], v[10], v[11]) * d)
        }
        nrec = 0;
      }
      if (LCOLS) sidx = QA_GET_SIDX();
      const unsigned qo = QA_GET_Q();
      const f3 pL = QA_GET_L();
      const float inv = (float) (sidx + 1);
      f3 mean = F3(acc[0], acc[QA_BLOCK], acc[2 * QA_BLOCK]);
      f3 cstd = F3(0, 0, 0);
      const f3 dc = (pL - mean) / inv;
      mean = mean + dc;
      acc[0] = mean.x; acc[QA_BLOCK] = mean.y; acc[2 * QA_BLOCK] = mean.z;
      // The running variance decides one thing - whether a pixel past sppMin takes another sample (below) - and is no output: with
      // sppMin == sppMax (every BASELINE config) nothing reads it, and its three correctly rounded divisions per sample are not made
      // (Cornell box + 1.5 %).  In the variants without lights only: the lit LDS-resident kernel lost 8 % to the changed register
      // allocation around this branch (project3_sphere 18 500 -> 16 900), profiles/round03/experiments.txt 32.
      if (LIGHTS || rp.spp_min < rp.spp_max) {
        cstd = F3(acc[3 * QA_BLOCK], acc[4 * QA_BLOCK], acc[5 * QA_BLOCK]);
        if (sidx > 0) cstd = cstd + ((dc * dc) * inv - cstd / (float) sidx);
        acc[3 * QA_BLOCK] = cstd.x; acc[4 * QA_BLOCK] = cstd.y; acc[5 * QA_BLOCK] = cstd.z;
      }
      ++sidx;
      if (LCOLS) acc[14 * QA_BLOCK] = __int_as_float(sidx);
      const bool more = sidx < rp.spp_min ||
                        (sidx < rp.spp_max && (cstd.x > 0.005f || cstd.y > 0.001f || cstd.z > 0.005f));
      if (more) {
        if (rp.chunk_spp && sidx >= chunkEnd) {
          // the chunk's last sample of this pixel: its state waits for whoever takes the tile's next chunk
          unsigned long long *st = reinterpret_cast<unsigned long long *>(rp.pix_state) + 4 * (size_t) qo;
#define QA_PAIR(lo, hi) ((unsigned long long) (lo) | ((unsigned long long) (hi) << 32))
          __hip_atomic_store(st, QA_PAIR(rng, (uint32_t) sidx), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
          __hip_atomic_store(st + 1, QA_PAIR(__float_as_uint(mean.x), __float_as_uint(mean.y)), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
          __hip_atomic_store(st + 2, QA_PAIR(__float_as_uint(mean.z), __float_as_uint(cstd.x)), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
          __hip_atomic_store(st + 3, QA_PAIR(__float_as_uint(cstd.y), __float_as_uint(cstd.z)), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
#undef QA_PAIR
          needPixel = true;
        } else {
          needSample = true;
        }
      } else {
        rp.rgb[3 * qo + 0] = mean.x;
        rp.rgb[3 * qo + 1] = mean.y;
        rp.rgb[3 * qo + 2] = mean.z;
        if constexpr (RAYS) {
          if (rp.ns) rp.ns[qo] = (uint32_t) sidx;   // (optional)
        } else {
        rp.ns[qo] = (uint32_t) sidx;
        }
        if (rp.chunk_spp)   // (later chunks of the tile skip this pixel)
          __hip_atomic_store(reinterpret_cast<unsigned long long *>(rp.pix_state) + 4 * (size_t) qo, 0x80000000ull << 32, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        QA_TALLY(cnt.pixels);
        needPixel = true;
      }
    }
    QA_TACC(cnt.sl[7], tE)
  }

  // ---- counters: wave reduction, one atomic per wave and counter -----------------------------
  unsigned long long v[6] = {cnt.samples, cnt.casts_normal, cnt.casts_shadow, cnt.bvh_nodes, cnt.tri_tests, cnt.pixels};
  unsigned long long *dst = reinterpret_cast<unsigned long long *>(rp.counters);
  for (int i = 0; i < 6; ++i) {
    unsigned long long x = v[i];
#ifdef QA_LANE_TALLIES
    for (int off = 32; off > 0; off >>= 1) x += __shfl_down(x, off);
#endif
    if (lane == 0 && x) atomicAdd(&dst[i], x);
  }
#ifdef QA_STAMPS
  if (lane == 0) {
    cnt.sl[0] = __builtin_readcyclecounter() - tKernel;
    cnt.sl[9] = 1;
    for (int i = 0; i < QA_NSTAMPS; ++i) atomicAdd(&dst[6 + i], cnt.sl[i]);
  }
#endif
