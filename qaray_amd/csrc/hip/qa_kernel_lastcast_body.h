// qa_kernel_lastcast_body.h - the body of qa_integrate_lastcast (qa_kernel.h): qa_kernel_body.h for the scenes of PlanLastCast, where
// a path is always camera ray, diffuse hit, one bounce ray, end.  A text include like qa_kernel_body.h, with `sc`, `rp` and RES in
// scope.  The general body runs such a path as two turns of its per-lane state machine (needSample / done / primary / fromDiffuse as
// exec masks, throughput and radiance through six LDS columns); here ONE turn of the loop runs one whole sample of every lane that
// holds a pixel:
//   A  tile and chunk fetch, hand-over, tile lists, ragged tiles, stop_flag: the text of qa_kernel_body.h section A; and between
//      the fetch and the hand-over's wait, a tile that no camera ray can hit anything from is written in closed form (qa_emptytile.h)
//   B  camera ray (DoF draws included)
//   C  trip 1 of a two-trip loop over (ray, primary): closest-hit sweep of the camera ray, depth at sample 0, miss or shading;
//      between the trips the bounce rays ask which emitter they meet (lastCastQuery); trip 2, the closest-hit sweep and shading once
//      more, is for the bounce rays whose query says "ask again" and for all of them under option last_cast = 0 - the wave skips it
//      when no lane asks.  (A loop and not a second copy of the sweep and the shading: one call site each for traceClosest,
//      shadeSurface and lastCastQuery - the second copy costs 900 scalar instructions and 16 more spilled registers.)
//   E  the sample's end: running mean / variance, hand-over or output
// Same float expressions in the same order on the same operands, same random draws in the same order: same bits as the general body
// (tests/test_gpu_lastcast_straight.py and tests/test_gpu_last_cast.py compare this kernel's frames with the counting kernel's, which
// is the general body).  Throughput and radiance are registers that die inside the turn; LDS
// columns 6 to 11 hold nothing of a lane's (the launch keeps their room: the layout is shared; their first 256 bytes carry the meshes'
// leaf-pair bytes, below).  Option sync_samples has no effect: the lanes
// of a wave move in lockstep by construction.  No material of these scenes has reflective or refractive lobes (PlanLastCast), so
// shadeSurface is compiled without them (LOBES = false).
  extern __shared__ uint4 s_dyn[];
  SceneMem<RES> mem;
  mem.img = s_dyn;
  static_assert(RES, "the last-cast query belongs to the resident variant without lights");
  for (uint32_t i = threadIdx.x; i < sc.residentVec4; i += QA_BLOCK) s_dyn[i] = sc.resident[i];
  // The start of column 6 holds the leaf-pair bytes of the scene's meshes, QA_TILE_LEAF_CAP each (DMesh::leafPairs; qa_kernel.h
  // sweepLeaves reads them): 256 of the 6 144 bytes this kernel leaves alone, so the launch's LDS size is what it was
  static_assert(QA_KARG_MESH * QA_TILE_LEAF_CAP <= 6 * QA_BLOCK * sizeof(uint32_t), "the leaf-pair bytes live in columns 6 to 11");
  uint32_t *const leafPairWords = reinterpret_cast<uint32_t *>(s_dyn + sc.residentVec4) + ((size_t) sc.stackDepth + 6) * QA_BLOCK;
  for (int mi = 0; mi < QA_KARG_MESH; ++mi) {
    const DMesh &pm = sc.meshv[mi];
    if (pm.leafPairs && threadIdx.x < QA_TILE_LEAF_CAP / 4)
      leafPairWords[mi * (QA_TILE_LEAF_CAP / 4) + threadIdx.x] = reinterpret_cast<const uint32_t *>(sc.resident + pm.resLeaves + 4 * (size_t) pm.numLeaves)[threadIdx.x];
  }
  __syncthreads();
  uint32_t *stack = reinterpret_cast<uint32_t *>(s_dyn + sc.residentVec4) + threadIdx.x;
  // per-lane sample accumulators (columns 0 - 5), the pixel (12), its output index (13) and the sample index (14) live in LDS
  float *acc = reinterpret_cast<float *>(stack + (size_t) sc.stackDepth * QA_BLOCK - threadIdx.x) + threadIdx.x;
  const uint4 *mtlTable = s_dyn + sc.resMaterials;
  for (int i = 12; i < QA_LANE_SLOTS_RES; ++i) acc[i * QA_BLOCK] = 0.f;
  // Tile lists for the camera rays (qa_tilecull.h); with depth of field the camera rays of a tile share no origin
  constexpr bool TL = true;
  uint32_t *tileList = nullptr;
  if (rp.tile_lists > 0 && !(sc.cam.dof > 0.1f))
    tileList = reinterpret_cast<uint32_t *>(s_dyn + sc.residentVec4) + ((size_t) sc.stackDepth + QA_LANE_SLOTS_RES) * QA_BLOCK +
               __builtin_amdgcn_readfirstlane(threadIdx.x / 64) * QA_TILE_LIST_DWORDS;

  // work items: qa_kernel_body.h (8x8 pixel tiles, lane = pixel; (chunk, tile) with RenderParams::chunk_spp)
  const int rw = rp.x1 - rp.x0, rh = rp.y1 - rp.y0;
  const unsigned tilesX = (unsigned) (rw + 7) / 8;
  const unsigned numTiles = tilesX * (unsigned) rp.own_tile_rows;
  const unsigned total = numTiles * (rp.chunk_spp ? rp.num_chunks : 1u) * 64u;
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
  RayDiff pathDiff;           // (TEX only: never read here)
  pathDiff.dx = pathDiff.dy = F3(0, 0, 1);

  // what a lane carries from one turn to the next: its random stream, and whether it holds a pixel
  uint32_t rng = 1;
  bool alive = true, needPixel = true;
  // n samples, casts or pixels at once, by QA_TALLY's rule (section A: the derived samples of an empty tile)
#ifdef QA_WAVE_TALLIES
#define QA_TALLY_N(x, n) (x) += (unsigned long long) (n) * (unsigned long long) __popcll(__ballot(1))
#else
#define QA_TALLY_N(x, n) (x) += (unsigned long long) (n)
#endif
#ifdef QA_STAMPS
  // diagnostic builds ask of every tile, whatever the option says: slot 15 = cycles of the turns of tiles the test calls empty, 16 = those turns
  bool tileEmpty = false;   // (wave-uniform) the tile in hand
#define QA_EMPTY_ASK true
#else
#define QA_EMPTY_ASK (rp.empty_tiles != 0)
#endif

  for (;;) {
    QA_T(tA)
    // ---- A. tile fetch (qa_kernel_body.h section A) --------------------------------------------
    const unsigned long long aliveMask = __ballot(alive);
    const unsigned long long want = __ballot(alive && needPixel);
    if (want && want == aliveMask) {
      if (rp.chunk_spp && curTile != 0xFFFFFFFFu) {
        // the chunk in hand is complete: every lane has stored its pixel's state (section E); publish it
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
      }
      // ---- a tile no camera ray can hit anything from (qa_emptytile.h) is finished here, in closed form: every sample of every pixel
      // is the background.  The item that starts the tile's pixels writes them; the tile's later chunks are nothing but this test.
      // Decided BEFORE the progress wait below: the answer depends on the scene, the camera and the tile alone, so every item of a
      // tile decides alike in a launch, no item of an empty tile ever publishes progress - and none ever waits for it.
      if (tileList && QA_EMPTY_ASK && base < total) {
        const unsigned tile = rp.tile_order ? rp.tile_order[item] : item;
        const unsigned otr = tile / tilesX;
        const bool emptyTile = __builtin_amdgcn_readfirstlane((int) tileIsEmpty(
            EmptyTileScene<RES>{sc}, sc.cam, sc.background, sc.num_inst, sc.rootIdentity != 0, (float) (rp.x0 + (int) ((tile % tilesX) * 8)),
            (float) (rp.y0 + (int) (((unsigned) rp.tile_row0 + otr * (unsigned) rp.tile_row_step) * 8)), reinterpret_cast<TileCone *>(stack - lane)));
#ifdef QA_STAMPS
        tileEmpty = emptyTile;
#endif
        if (emptyTile && rp.empty_tiles) {
          if (alive && (!rp.chunk_spp || curChunk == 0)) {
            const unsigned tx = (tile % tilesX) * 8 + (lane % 8);
            const unsigned ty = ((unsigned) rp.tile_row0 + otr * (unsigned) rp.tile_row_step) * 8 + (lane / 8);
            if (tx < (unsigned) rw && ty < (unsigned) rh) {   // (padding lanes of a ragged tile write nothing)
              const unsigned q = (otr * 8 + (lane / 8)) * (unsigned) rw + tx;
              // sample 0 as sections C and E form it: L = 0 + 1 * background, mean = 0 + (L - 0) / 1; no later sample moves it
              const f3 L0 = F3(0, 0, 0) + F3(1, 1, 1) * ld3(sc.background);
              const f3 mean = F3(0, 0, 0) + (L0 - F3(0, 0, 0)) / 1.f;
              rp.rgb[3 * q + 0] = mean.x;
              rp.rgb[3 * q + 1] = mean.y;
              rp.rgb[3 * q + 2] = mean.z;
              rp.depth[q] = QA_BIGFLOAT;
              rp.ns[q] = (uint32_t) rp.spp_min;
              // the frame holds these samples and casts: derived, not traced
              QA_TALLY_N(cnt.samples, rp.spp_min);
              QA_TALLY_N(cnt.casts_normal, rp.spp_min);
              QA_TALLY_N(cnt.pixels, 1);
            }
          }
          curTile = 0xFFFFFFFFu;   // nothing to publish
          continue;                // every lane that is alive still asks for a pixel: the next turn fetches
        }
      }
      // ---- the hand-over's wait: a later chunk of a tile starts when the chunk before it has published its pixels' state
      if (rp.chunk_spp && base < total && curChunk > 0) {
        // (the bound is a guard against a lost update, not a path that is taken: qa_kernel_body.h)
        for (int spins = 0; spins < (1 << 22); ++spins) {
          if (__hip_atomic_load(rp.tile_progress + curTile, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) >= curChunk) break;
          __builtin_amdgcn_s_sleep(16);
        }
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
      }
      if (tileList && base < total) {
        const unsigned tile = rp.tile_order ? rp.tile_order[item] : item;
        const unsigned otr = tile / tilesX;
        buildTileLists<RES>(sc, (uint32_t) rp.tile_lists, (float) (rp.x0 + (int) ((tile % tilesX) * 8)),
                            (float) (rp.y0 + (int) (((unsigned) rp.tile_row0 + otr * (unsigned) rp.tile_row_step) * 8)), tileList,
                            reinterpret_cast<TileCone *>(stack - lane));   // row 0 of the wave's stacks: no walk is under way
        rng = 1;   // (every lane that is alive asks for a pixel here: its stream is dead)
      }
      if (alive) {
        const unsigned w = base + lane;
        if (base >= total) {
          alive = false;
        } else {
          const unsigned in = w % 64;
          const unsigned tile = rp.tile_order ? rp.tile_order[item] : item;
          const unsigned otr = tile / tilesX;  // index among the strips this launch owns
          const unsigned tx = (tile % tilesX) * 8 + (in % 8);
          const unsigned ty = ((unsigned) rp.tile_row0 + otr * (unsigned) rp.tile_row_step) * 8 + (in / 8);
          if (tx < (unsigned) rw && ty < (unsigned) rh) {
            const int px = rp.x0 + (int) tx, py = rp.y0 + (int) ty;
            const unsigned q = (otr * 8 + (in / 8)) * (unsigned) rw + tx;
            int sidx = 0;
            rng = qa_pixel_seed(rp.seed, (uint32_t) py * (uint32_t) sc.cam.width + (uint32_t) px);
            for (int i = 0; i < 6; ++i) acc[i * QA_BLOCK] = 0.f;
            needPixel = false;
            if (rp.chunk_spp && curChunk > 0) {
              // the pixel as the previous chunk left it
              const unsigned long long *st = reinterpret_cast<const unsigned long long *>(rp.pix_state) + 4 * (size_t) q;
              const unsigned long long s0 = __hip_atomic_load(st, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT), s1 = __hip_atomic_load(st + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT),
                                       s2 = __hip_atomic_load(st + 2, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT), s3 = __hip_atomic_load(st + 3, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
              const uint4 a = make_uint4((uint32_t) s0, (uint32_t) (s0 >> 32), (uint32_t) s1, (uint32_t) (s1 >> 32));
              const uint4 b = make_uint4((uint32_t) s2, (uint32_t) (s2 >> 32), (uint32_t) s3, (uint32_t) (s3 >> 32));
              if (a.y & 0x80000000u) {   // finished in an earlier chunk: the lane sits this one out
                needPixel = true;
              } else {
                rng = a.x;
                sidx = (int) a.y;
                acc[0] = __uint_as_float(a.z); acc[QA_BLOCK] = __uint_as_float(a.w); acc[2 * QA_BLOCK] = __uint_as_float(b.x);
                acc[3 * QA_BLOCK] = __uint_as_float(b.y); acc[4 * QA_BLOCK] = __uint_as_float(b.z); acc[5 * QA_BLOCK] = __uint_as_float(b.w);
              }
            }
            acc[12 * QA_BLOCK] = __uint_as_float((unsigned) px | ((unsigned) py << 16));
            acc[13 * QA_BLOCK] = __uint_as_float(q);
            acc[14 * QA_BLOCK] = __int_as_float(sidx);
          }
          // else: padding slot of a ragged tile - this lane sits the tile out
        }
      }
    }
    if (!__any(alive)) break;

    const bool active = alive && !needPixel;   // this lane holds a pixel: the turn runs one sample of it
    Ray ray;
    ray.p = F3(0, 0, 0);
    ray.d = F3(0, 0, 1);
    f3 T = F3(0, 0, 0), L = F3(0, 0, 0);   // throughput, and the radiance this sample has gathered
    int bounce = 0;
    bool fromDiffuse = false;

    // ---- B. start the sample: camera ray (src/renderers/renderer.cpp:312-328) -------------------
    if (active) {
      const int si = __float_as_int(acc[14 * QA_BLOCK]);
      const float hx = sc.halton[2 * si], hy = sc.halton[2 * si + 1];
      const unsigned pxy = __float_as_uint(acc[12 * QA_BLOCK]);
      const f3 texpos = F3(hx, hy, 0.f) + F3((float) (int) (pxy & 0xFFFFu), (float) (int) (pxy >> 16), 0.f);
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
      ray.p = campos;
      ray.d = normalize(cpt - campos);
      T = F3(1, 1, 1);
      L = F3(0, 0, 0);
      bounce = rp.max_bounce;
      fromDiffuse = false;
      QA_TALLY(cnt.samples);
    }
    QA_TACC(cnt.sl[1], tA)

    // ---- C. the sample's two rays ---------------------------------------------------------------
    bool go = active;      // the lane's ray in hand takes the closest-hit sweep and shading
    bool primary = true;   // (wave-uniform) the rays in hand are camera rays
#pragma nounroll
    for (int trip = 0; trip < 2; ++trip) {
      if (go) {
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
        go = false;   // (until the hit spawns a ray)
        QA_T(tC)
        const bool found = traceClosest<RES, false, false, TL>(mem, sc, ray, pathDiff, h, th, stack, cnt, tileList, primary);
        QA_TACC(cnt.sl[2], tC)
        if (primary && __float_as_int(acc[14 * QA_BLOCK]) == 0) rp.depth[__float_as_uint(acc[13 * QA_BLOCK])] = found ? h.z : QA_BIGFLOAT;

        QA_T(tM)
        if (!found) {
          // background for camera rays (renderer.cpp:337-341), environment otherwise (MtlBlinn_PhotonMap.cpp:249-251)
          const f3 c = primary ? ld3(sc.background) : ld3(sc.environment);
          L = L + T * c;
          QA_TACC(cnt.sl[10], tM)
        } else {
          // ---- D. shade: MtlBlinn_PhotonMap::Shade (MtlBlinn_PhotonMap.cpp:256-500) -----------
          // (No Beer-Lambert attenuation of a ray that arrives from inside, ComputeSecondaryRay :244-248: PlanLastCast refuses every
          // material whose absorption is not +0 or -0, so the factor would be qexpf(-+0 * h.z) with h.z finite and positive - exactly
          // 1.0f - and T * 1.0f has T's bits: tests/cpp/absorb_identity_check.cpp.  The material a ray was spawned from is not kept.)
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
            if (white) L = L + T;
          } else {
            const f3 V = -ray.d;
            const f3 N = h.N;
            const f3 p = h.p;
            QA_TACC(cnt.sl[11], tM)
            QA_T(tD)
            const Surface sf = shadeSurface<false, DScene, false>(mtlTable, sc, tt, mi, N, V, h.front, th, bounce, fromDiffuse, rng);
            QA_TACC(cnt.sl[4], tD)
            L = L + T * sf.emission;
            QA_T(tS)
            if (sf.spawn) {
              // ComputeSecondaryRay (:226-254): DiffRay(pos, dir).Normalize()
              ray.p = p;
              ray.d = normalize(sf.nextDir);
              T = T * sf.bxdf;
              bounce -= 1;
              fromDiffuse = sf.nextFromDiffuse;
              go = true;
            }
            QA_TACC(cnt.sl[12], tS)
          }
        }
#ifdef QA_STAMPS
        if (!primary) QA_TACC(cnt.sl[20], tM)   // the part behind the sweep of casts in a wave without a camera ray
#endif
      }
      if (trip) break;
      primary = false;
      // ---- between the trips: every ray that is no camera ray is its path's last (PlanLastCast): which emitter does it meet?
      if (sc.lastCast && go) {
        QA_T(tQ)
        bool drawn;
        int emitSet;
        go = !lastCastQuery<RES>(mem, sc, ray, stack, cnt, drawn, emitSet, reinterpret_cast<const uint8_t *>(s_dyn + sc.residentVec4) + ((size_t) sc.stackDepth + 6) * QA_BLOCK * sizeof(uint32_t));
        if (!go) {
          QA_TALLY(cnt.casts_normal);
          // the products, not their values for a finite throughput: a hit that does not emit adds T * 0
          f3 c = ld3(sc.environment);
          if (drawn) {
            (void) rng1(rng);   // RandomSelectMtl's draw at the hit; nothing is spawned from a diffuse bounce's hit
            c = F3(0, 0, 0);
            if (emitSet >= 0) {
              const uint4 m2 = mtlTable[6 * (size_t) sc.mtlset[emitSet].first + 2];
              c = F3(asF(m2.x), asF(m2.y), asF(m2.z));
            }
          }
          L = L + T * c;
        }
        QA_TACC(cnt.sl[21], tQ)
#ifdef QA_STAMPS
        {
          const unsigned long long asked = __ballot(go);   // lanes whose query said "ask again"
          if ((int) __lane_id() == __ffsll((long long) __ballot(1)) - 1) cnt.sl[23] += (unsigned long long) __popcll(asked);
        }
#endif
      }
      if (!__any(go)) break;
    }

    // ---- E. sample finished: SuperSamplerHalton::Accumulate / Loop (scene.cpp:92-121) ---------
    QA_T(tE)
#ifdef QA_STAMPS
    if (lane == 0) cnt.sl[8] += 1;
#endif
    if (active) {
      int sidx = __float_as_int(acc[14 * QA_BLOCK]);
      const unsigned qo = __float_as_uint(acc[13 * QA_BLOCK]);
      const f3 pL = L;
      const float inv = (float) (sidx + 1);
      f3 mean = F3(acc[0], acc[QA_BLOCK], acc[2 * QA_BLOCK]);
      f3 cstd = F3(0, 0, 0);
      const f3 dc = (pL - mean) / inv;
      mean = mean + dc;
      acc[0] = mean.x; acc[QA_BLOCK] = mean.y; acc[2 * QA_BLOCK] = mean.z;
      // the running variance only decides whether a pixel past sppMin takes another sample (qa_kernel_body.h)
      if (rp.spp_min < rp.spp_max) {
        cstd = F3(acc[3 * QA_BLOCK], acc[4 * QA_BLOCK], acc[5 * QA_BLOCK]);
        if (sidx > 0) cstd = cstd + ((dc * dc) * inv - cstd / (float) sidx);
        acc[3 * QA_BLOCK] = cstd.x; acc[4 * QA_BLOCK] = cstd.y; acc[5 * QA_BLOCK] = cstd.z;
      }
      ++sidx;
      acc[14 * QA_BLOCK] = __int_as_float(sidx);
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
        }
      } else {
        rp.rgb[3 * qo + 0] = mean.x;
        rp.rgb[3 * qo + 1] = mean.y;
        rp.rgb[3 * qo + 2] = mean.z;
        rp.ns[qo] = (uint32_t) sidx;
        if (rp.chunk_spp)   // (later chunks of the tile skip this pixel)
          __hip_atomic_store(reinterpret_cast<unsigned long long *>(rp.pix_state) + 4 * (size_t) qo, 0x80000000ull << 32, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        QA_TALLY(cnt.pixels);
        needPixel = true;
      }
    }
    QA_TACC(cnt.sl[7], tE)
#ifdef QA_STAMPS
    if (tileEmpty) {
      QA_TACC(cnt.sl[15], tA)
      if (lane == 0) cnt.sl[16] += 1;
    }
#endif
  }
#undef QA_TALLY_N
#undef QA_EMPTY_ASK

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
