// qa_kernel_cs_body.h - the body of the cooperative megakernel (qa_kernel_cs.h), included by its two entry points: qa_integrate_cs and
// qa_integrate_cs_resume.  Not a header of its own: it is the text of a function whose parameters are `sc` and `rp`, with the template
// parameters LIGHTS, TEX, CULL, MANY, AREA and the constant CHUNK in scope.  (A text include rather than an inline function: the
// shipped instances keep exactly the code they had - their register allocation is what their speed hangs on)
  extern __shared__ uint4 s_dyn[];
  const unsigned lane = __lane_id();
  CsLds L;
  {
    const uint32_t poolCap = (sc.csPoolLimit && sc.csPoolLimit < sc.csItems) ? sc.csPoolLimit : sc.csItems;   // (a limit below the LDS there is: tests of the overflow path)
    const uint32_t wave = (uint32_t) __builtin_amdgcn_readfirstlane((int) (threadIdx.x / 64));                   // (wave-uniform: the pointers stay in scalar registers)
    uint32_t *base = reinterpret_cast<uint32_t *>(s_dyn) + wave * CsLdsWords(sc.csItems, sc.csSlots);
    L.rays = reinterpret_cast<uint4 *>(base);                     // 16-byte aligned: first
    L.res = base + 8u * sc.csSlots;                               // 8-byte aligned keys
    L.flags = L.res + QA_CS_RES_WORDS;
    L.items = L.flags + 64;
    L.capItems = poolCap;
    L.slots = sc.csSlots;
  }
  float *acc = reinterpret_cast<float *>(L.items + sc.csItems) + lane;   // + i * 64
  // The path's throughput and the sample's radiance live in LDS too (columns 6 - 11): they are touched at a handful of points of an
  // iteration and would otherwise be six more registers alive through every sweep and every round (- 19 / - 34 spilled registers in the
  // untextured / textured kernels); the pool gives up 256 items and 16 ray slots for them.
#define QA_PT() F3(acc[6 * 64], acc[7 * 64], acc[8 * 64])
#define QA_PL() F3(acc[9 * 64], acc[10 * 64], acc[11 * 64])
#define QA_SET_PT(v) { const f3 t_ = (v); acc[6 * 64] = t_.x; acc[7 * 64] = t_.y; acc[8 * 64] = t_.z; }
#define QA_SET_PL(v) { const f3 t_ = (v); acc[9 * 64] = t_.x; acc[10 * 64] = t_.y; acc[11 * 64] = t_.z; }
  // ... and so do the pixel (x | y << 16), its output index and the sample index (columns 12 - 14): read at the sample's start and end
#define QA_PXY() __float_as_uint(acc[12 * 64])
#define QA_Q() __float_as_uint(acc[13 * 64])
#define QA_SIDX() __float_as_int(acc[14 * 64])
  // (lanes that hold no pixel - padding lanes of ragged tiles, lanes before their first tile - still run the wave's code: their sample
  // index is an index into the Halton table in csRayDiff / csTexPos, so every column starts from zero)
  for (int i = 0; i < QA_CS_LANE_SLOTS; ++i) acc[i * 64] = 0.f;
  const uint4 *mtlTable = reinterpret_cast<const uint4 *>(sc.mtl);

  const int rw = rp.x1 - rp.x0, rh = rp.y1 - rp.y0;
  const unsigned tilesX = (unsigned) (rw + 7) / 8;
  // tiles in sample chunks (qa_integrate, section A: RenderParams::chunk_spp)
  const unsigned numTiles = tilesX * (unsigned) rp.own_tile_rows;
  const unsigned total = numTiles * ((CHUNK && rp.chunk_spp) ? rp.num_chunks : 1u) * 64u;
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

  // per-lane state: pixel (x | y << 16, output index, RNG stream, sample index) and path (ray, throughput, radiance, state word)
  uint32_t rng = 1;
  Ray ray;
  ray.p = F3(0, 0, 0);
  ray.d = F3(0, 0, 1);
  uint32_t pst = QA_PST_PRIMARY;
  bool alive = true, needPixel = true, needSample = false;
  uint32_t nrec = 0;       // AREA: hits logged for the current path
  // BATCH (the textured and the many-light variants; compiled into the others it costs C4 and C5 1 %): sync_samples >= 2, below
  constexpr bool BATCH = !AREA && (TEX || MANY);
  bool awaiting = false;   // AREA: the path has ended, its lights have not been evaluated yet; BATCH: ... it waits for others to finish

  for (;;) {
    QA_T(tA)
    // ---- A. tile fetch (qa_integrate, section A)
    const unsigned long long aliveMask = __ballot(alive);
    const unsigned long long want = __ballot(alive && needPixel);
    if (want && want == aliveMask) {
      if (CHUNK && rp.chunk_spp && curTile != 0xFFFFFFFFu) {
        // the chunk in hand is complete: every lane stores what it holds (agent-scope atomic stores), the wave waits for them, publishes
        csChunkSaveAll(rp.pix_state, acc, rng);
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        if (lane == 0) __hip_atomic_store(rp.tile_progress + curTile, curChunk + 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        curTile = 0xFFFFFFFFu;
      }
      unsigned base = 0;
      const int leader = __ffsll((long long) want) - 1;
      if ((int) lane == leader) base = (*rp.stop_flag) ? total : atomicAdd(rp.work_counter, 64u);
      base = __shfl(base, leader);
      unsigned item = base / 64;   // (wave-uniform) tile, or chunk * numTiles + tile
      if (CHUNK && rp.chunk_spp && base < total) {
        curChunk = item / numTiles;
        item -= curChunk * numTiles;
        curTile = item;
        chunkEnd = csChunkBegin(rp.tile_progress, curTile, curChunk, rp.chunk_spp, rp.chunk_tail);
      }
      if (alive) {
        const unsigned w = base + lane;
        if (base >= total) {
          alive = false;
        } else {
          const unsigned in = w % 64;
          const unsigned tile = rp.tile_order ? rp.tile_order[item] : item;
          const unsigned otr = tile / tilesX;
          const unsigned tx = (tile % tilesX) * 8 + (in % 8);
          const unsigned ty = ((unsigned) rp.tile_row0 + otr * (unsigned) rp.tile_row_step) * 8 + (in / 8);
          if (tx < (unsigned) rw && ty < (unsigned) rh) {
            const uint32_t px = (uint32_t) rp.x0 + tx, py = (uint32_t) rp.y0 + ty;
            acc[12 * 64] = __uint_as_float(px | (py << 16));
            acc[13 * 64] = __uint_as_float((otr * 8 + (in / 8)) * (unsigned) rw + tx);
            rng = qa_pixel_seed(rp.seed, py * (uint32_t) sc.cam.width + px);
            acc[14 * 64] = __int_as_float(0);
            for (int i = 0; i < 6; ++i) acc[i * 64] = 0.f;
            needSample = true;
            needPixel = false;
            if (CHUNK && rp.chunk_spp && curChunk > 0) {
              bool finished;
              const uint32_t r = csChunkRestore(rp.pix_state, QA_Q(), acc, &finished);
              if (finished) {   // (finished in an earlier chunk: the lane sits this one out)
                needSample = false;
                needPixel = true;
                acc[13 * 64] = __uint_as_float(0xFFFFFFFFu);
              } else rng = r;
            }
          } else if (CHUNK) {
            acc[13 * 64] = __uint_as_float(0xFFFFFFFFu);   // (a padding lane of a ragged tile holds nothing: csChunkSaveAll)
          }
        }
      }
    }
    if (!__any(alive)) break;

    // ---- B. start a sample (qa_integrate, section B; src/renderers/renderer.cpp:312-328)
    const bool goSample = !rp.sync_samples || (BATCH && rp.sync_samples != 1) || (__ballot(needSample) == __ballot(alive && !needPixel));
    const bool starting = alive && needSample && goSample;
    cnt.samples += (unsigned long long) __popcll(__ballot(starting));   // (wave-uniform tallies: no registers per lane)
    if (starting) {
      const f3 texpos = csTexPos(sc, QA_PXY(), QA_SIDX());
      const f3 A = ld3(sc.cam.screenA), U = ld3(sc.cam.screenU), V = ld3(sc.cam.screenV);
      const f3 cpt = (A + U * texpos.x) + V * texpos.y;
      f3 campos = ld3(sc.cam.pos);
      if (sc.cam.dof > 0.1f) {
        const float r1 = rng1(rng), r2 = rng1(rng);
        const float r = sc.cam.dof * qsqrt(r1);
        const float t = r2 * 2.f * QA_PI;
        campos = campos + (ld3(sc.cam.screenX) * (r * qcosf(t)) + ld3(sc.cam.screenY) * (r * qsinf(t)));
      }
      ray.p = campos;
      ray.d = normalize(cpt - campos);
      QA_SET_PT(F3(1, 1, 1))
      QA_SET_PL(F3(0, 0, 0))
      pst = QA_PST_PRIMARY | (uint32_t) (rp.max_bounce & 0xFF);
      needSample = false;
    }
    QA_TACC(cnt.sl[1], tA)
    // ---- C. trace (qa_integrate, section C)
    const bool act = alive && !needPixel && !needSample && !((AREA || BATCH) && awaiting);
    bool done = false;
    Hit h;
    TexHit th;
    QA_T(tC)
    const bool found = csTraceClosest<TEX, CULL>(sc, L, act, ray, (pst & QA_PST_PRIMARY) != 0, acc, h, th, cnt);
    QA_TACC(cnt.sl[2], tC)
    QA_T(tD)

    // ---- D. shade up to the lights (qa_integrate, section D)
    bool lit = false;
    int mi = -1;
    f3 V = F3(0, 0, 1), N = F3(0, 0, 1), p = F3(0, 0, 0);
    Surface sf;
    sf.emission = sf.kd = sf.ks = sf.nextDir = sf.bxdf = F3(0, 0, 0);
    sf.gloss = 0.f;
    sf.spawn = sf.nextFromDiffuse = sf.selDiffuse = false;
    if (act) {
      const bool primary = (pst & QA_PST_PRIMARY) != 0;
      if (primary && QA_SIDX() == 0) rp.depth[QA_Q()] = found ? h.z : QA_BIGFLOAT;
      if (!found) {
        f3 c = primary ? ld3(sc.background) : ld3(sc.environment);
        if (TEX) {
          if (primary) {
            const f3 texpos = csTexPos(sc, QA_PXY(), QA_SIDX());
            c = texColorSample(tt, c, sc.bgTexmap, F3(texpos.x / (float) sc.cam.width, texpos.y / (float) sc.cam.height, 0.f));
          } else
            c = sampleEnvironment(tt, c, sc.envTexmap, ray.d);
        }
        QA_SET_PL(QA_PL() + QA_PT() * c)
        done = true;
      } else {
        const int absorbMtl = QA_PST_ABSORB(pst);
        if (!primary && !h.front && absorbMtl >= 0) {
          const uint4 ab = mtlTable[6 * (size_t) absorbMtl + 5];
          const f3 att = F3(qexpf(-asF(ab.x) * h.z), qexpf(-asF(ab.y) * h.z), qexpf(-asF(ab.z) * h.z));
          QA_SET_PT(QA_PT() * att)
        }
        const qa_instance &in = sc.inst[h.node];
        bool white = false;
        if (in.mtlset >= 0) {
          const qa_mtlset ms = sc.mtlset[in.mtlset];
          if (ms.multi) {
            if (h.mtlID >= 0 && h.mtlID < ms.count) mi = ms.first + h.mtlID;
            else white = true;
          } else mi = ms.first;
        }
        if (mi < 0) {
          if (white) QA_SET_PL(QA_PL() + QA_PT())
          done = true;
        } else {
          V = -ray.d;
          N = h.N;
          p = h.p;
          // (shadeSurface inline: as a function of its own - tried for the untextured variants - its results come back through
          // memory or a block of registers that the caller spills: C4 3 790 vs 4 510, C5 1 590 vs 1 690 Msamples/s at 16 spp)
          sf = shadeSurface<TEX>(mtlTable, sc, tt, mi, N, V, h.front, th, QA_PST_BOUNCE(pst), (pst & QA_PST_FROM_DIFFUSE) != 0, rng);
          QA_SET_PL(QA_PL() + QA_PT() * sf.emission)
          lit = true;
        }
      }
    }
    QA_TACC(cnt.sl[4], tD)
    // ---- direct lighting, first half: the lights' terms as if unshadowed; then the path moves on to its next segment (or
    // ends) BEFORE the shadow queries, so that the surface is dead while the wave sweeps the scene for them: what is kept is
    // the shading point (= the next ray's origin), the throughput the lights are weighted with, and three values per light
    QA_T(tE)
    CsTerms terms;
    terms.c0 = terms.c1 = terms.c2 = terms.c3 = F3(0, 0, 0);
    f3 litT = F3(0, 0, 0);
    if (AREA) {
      // log the hit: position, normal, view direction, throughput, sampled colours, glossiness (qa_kernel.h's record)
      if (lit && nrec < QA_MAX_PATH) {
        const size_t stride = (size_t) gridDim.x * QA_BLOCK;
        float *rec = sc.areaScratch + (size_t) blockIdx.x * QA_BLOCK + threadIdx.x + (size_t) nrec * QA_REC_FLOATS * stride;
        const f3 pT = QA_PT();
        const float v[QA_REC_FLOATS] = {p.x, p.y, p.z, N.x, N.y, N.z, V.x, V.y, V.z, pT.x, pT.y, pT.z, sf.kd.x, sf.kd.y, sf.kd.z, sf.ks.x, sf.ks.y, sf.ks.z, sf.gloss};
#pragma unroll
        for (int f = 0; f < QA_REC_FLOATS; ++f) rec[(size_t) f * stride] = v[f];
        ++nrec;
      }
    } else if (LIGHTS) {
      if (__any(lit)) {
        QA_T(tLt)
        terms = csLightTerms(sc, lit, 0, p, N, V, sf.kd, sf.ks, sf.gloss);
        if (MANY && lit) {
          // more lights than one batch: the surface waits in the slab (column f of this lane: csSurf[f * lanes + lane id])
          const size_t stride = (size_t) gridDim.x * QA_BLOCK;
          float *sv = sc.csSurf + (size_t) blockIdx.x * QA_BLOCK + threadIdx.x;
          const float v[13] = {N.x, N.y, N.z, V.x, V.y, V.z, sf.kd.x, sf.kd.y, sf.kd.z, sf.ks.x, sf.ks.y, sf.ks.z, sf.gloss};
#pragma unroll
          for (int f = 0; f < 13; ++f) sv[f * stride] = v[f];
        }
        QA_TACC(cnt.sl[18], tLt)
      }
    }
    if (lit) {
      litT = QA_PT();
      ray.p = p;
      if (sf.spawn) {
        // ComputeSecondaryRay (:226-254): DiffRay(pos, dir).Normalize()
        ray.d = normalize(sf.nextDir);
        QA_SET_PT(litT * sf.bxdf)
        pst = (uint32_t) ((QA_PST_BOUNCE(pst) - 1) & 0xFF) | (sf.nextFromDiffuse ? QA_PST_FROM_DIFFUSE : 0u) | ((uint32_t) (mi + 1) << 16);
      } else {
        done = true;
      }
    }
    // ---- second half: the whole wave walks the shadow rays of its lit lanes
    if (LIGHTS && !AREA) {
      if (__any(lit)) {
        QA_T(tL)
        int li = 0;
        uint32_t nb = 0;
        uint32_t occl = csShadowBatch<CULL>(sc, L, lit, csTermsNeed(terms) | (sc.walkZeroTerms ? 15u : 0u), ray.p, li, nb, cnt);
        f3 dl = csLightSum(F3(0, 0, 0), terms, nb, occl);
        if (MANY) {
          // the further batches of a scene with many lights: surface back from the slab, terms, shadow queries, sum - in table order
          while (li < sc.num_lights) {
            const int li0 = li;
            const size_t stride = (size_t) gridDim.x * QA_BLOCK;
            const float *sv = sc.csSurf + (size_t) blockIdx.x * QA_BLOCK + threadIdx.x;
            float v[13];
#pragma unroll
            for (int f = 0; f < 13; ++f) v[f] = lit ? sv[f * stride] : 0.f;
            terms = csLightTerms(sc, lit, li0, ray.p, F3(v[0], v[1], v[2]), F3(v[3], v[4], v[5]), F3(v[6], v[7], v[8]), F3(v[9], v[10], v[11]), v[12]);
            occl = csShadowBatch<CULL>(sc, L, lit, csTermsNeed(terms) | (sc.walkZeroTerms ? 15u : 0u), ray.p, li, nb, cnt);
            if (!nb) break;   // (only ambient lights were left)
            dl = csLightSum(dl, terms, nb, occl);
          }
        }
        if (lit) QA_SET_PL(QA_PL() + litT * dl)
        QA_TACC(cnt.sl[5], tL)
      }
    }

    // sync_samples >= 2: finished paths wait until that many of the wave's have gathered (or every lane's has): sections E and B
    // then run for a group of lanes instead of a few lanes in nearly every iteration
    if (BATCH && rp.sync_samples >= 2) {
      awaiting = awaiting || (alive && done);
      done = false;
      const unsigned long long aw = __ballot(awaiting);
      if (aw && (__popcll(aw) >= rp.sync_samples || aw == __ballot(alive && !needPixel))) {
        done = awaiting;
        awaiting = false;
      }
    }
    // ---- AREA: the lights of the paths that have ended, once the whole wave is between samples
    if (AREA) {
      awaiting = awaiting || (alive && done);
      done = false;
      if (__any(awaiting) && __ballot(awaiting) == __ballot(alive && !needPixel)) {
        QA_T(tL)
        uint32_t maxrec = 0;
        for (uint32_t b = 0; b < 4u; ++b) if (__any(awaiting && ((nrec >> b) & 1u))) maxrec |= 1u << b;   // (an upper bound of the wave's deepest log)
        const size_t stride = (size_t) gridDim.x * QA_BLOCK;
        const float *rec0 = sc.areaScratch + (size_t) blockIdx.x * QA_BLOCK + threadIdx.x;
        const float normCoefDI = 1.f / (float) sc.num_lights;
        for (uint32_t lvl = maxrec < QA_MAX_PATH ? maxrec : QA_MAX_PATH; lvl-- > 0;) {
          const bool on = awaiting && nrec > lvl;
          if (!__any(on)) continue;
          float v[QA_REC_FLOATS];
#pragma unroll
          for (int f = 0; f < QA_REC_FLOATS; ++f) v[f] = on ? rec0[((size_t) lvl * QA_REC_FLOATS + f) * stride] : 0.f;
          const f3 hp = F3(v[0], v[1], v[2]), hN = F3(v[3], v[4], v[5]), hV = F3(v[6], v[7], v[8]);
          f3 sum = F3(0, 0, 0);
          // directLight + illuminate of qa_kernel.h, the shadow queries done by the wave
          for (int li = 0; li < sc.num_lights; ++li) {
            const qa_light l = ldTable(sc.light + li);
            if (l.type == QA_LIGHT_AMBIENT) continue;
            f3 I;
            if (l.type != QA_LIGHT_DIRECT && l.size > 0.01f) {
              // area light: 16 shadow rays towards points of a ball around the light, 64 as soon as the running estimate is a
              // penumbra value (src/lights/lights.cpp:52-65,88-100) - four at a time: the first 16 always exist, and whether the
              // other 48 do is decided by then
              int spp = 16, ns = 0;
              float inshadow = 0.0f;
              for (;;) {
                const bool more = on && ns < spp;
                if (!__any(more)) break;
                CsRays4 rq;
                f3 dir0 = F3(0, 0, 1), dir1 = dir0, dir2 = dir0, dir3 = dir0;
                if (more) {
                  dir0 = (ld3(l.position) + uniformBall(rng, l.size)) - hp;
                  dir1 = (ld3(l.position) + uniformBall(rng, l.size)) - hp;
                  dir2 = (ld3(l.position) + uniformBall(rng, l.size)) - hp;
                  dir3 = (ld3(l.position) + uniformBall(rng, l.size)) - hp;
                }
                rq.d0 = normalize(dir0); rq.t0 = length(dir0);
                rq.d1 = normalize(dir1); rq.t1 = length(dir1);
                rq.d2 = normalize(dir2); rq.t2 = length(dir2);
                rq.d3 = normalize(dir3); rq.t3 = length(dir3);
                const uint32_t occl = csShadowRays<CULL>(sc, L, more ? 15u : 0u, 4u, hp, rq, cnt);
                if (more) {
#define QA_CS_FOLD(S, DIR)                                                                                                   \
                  {                                                                                                            \
                    const float shadowed = ((occl >> S) & 1u) ? 0.0f : 1.0f;                                                   \
                    inshadow += (shadowed - inshadow) * inverseSquareFalloff(DIR) / (float) (ns + 1);                          \
                    ns++;                                                                                                      \
                    if (inshadow > 0.f && inshadow < 1.f) spp = 64;                                                            \
                  }
                  QA_CS_FOLD(0, dir0)
                  QA_CS_FOLD(1, dir1)
                  QA_CS_FOLD(2, dir2)
                  QA_CS_FOLD(3, dir3)
#undef QA_CS_FOLD
                }
              }
              I = ld3(l.intensity) * inshadow;
              if (l.type == QA_LIGHT_SPOT) I = I * spotAttenuation(l, hp);
            } else {
              CsRays4 rq;
              rq.d1 = rq.d2 = rq.d3 = F3(0, 0, 1);
              rq.t1 = rq.t2 = rq.t3 = 0.f;
              f3 dir = F3(0, 0, 1);
              if (l.type == QA_LIGHT_DIRECT) {
                rq.d0 = normalize(-ld3(l.direction));
                rq.t0 = QA_BIGFLOAT;
              } else {
                dir = ld3(l.position) - hp;
                rq.d0 = normalize(dir);
                rq.t0 = length(dir);
              }
              // (a surface facing away from the light - cosNL = 0 - gets the same zero whether the light is occluded or not: its shadow
              // ray is counted and not walked, csShadowBatch)
              const bool walk = on && (sc.walkZeroTerms || qmax(0.f, dot(hN, normalize(-lightDirection(l, hp)))) != 0.f);
              cnt.casts_shadow += (unsigned long long) __popcll(__ballot(on && !walk));
              const uint32_t occl = csShadowRays<CULL>(sc, L, walk ? 1u : 0u, 1u, hp, rq, cnt);
              const float shadowed = (occl & 1u) ? 0.0f : 1.0f;
              if (l.type == QA_LIGHT_DIRECT) I = ld3(l.intensity) * shadowed;
              else {
                I = (ld3(l.intensity) * shadowed) * inverseSquareFalloff(dir);
                if (l.type == QA_LIGHT_SPOT) I = I * spotAttenuation(l, hp);
              }
            }
            const f3 intensity = I * normCoefDI;
            const f3 Ld = normalize(-lightDirection(l, hp));
            const f3 H = normalize(hV + Ld);
            const float cosNL = qmax(0.f, dot(hN, Ld));
            const float cosNH = qmax(0.f, dot(hN, H));
            const f3 brdf = F3(v[12], v[13], v[14]) + F3(v[15], v[16], v[17]) * qpowf(cosNH, v[18]);
            sum = sum + (intensity * cosNL) * brdf;
          }
          if (on) QA_SET_PL(QA_PL() + F3(v[9], v[10], v[11]) * sum)
        }
        QA_TACC(cnt.sl[5], tL)
        done = awaiting;
        awaiting = false;
        nrec = 0;
      }
    }
    // ---- E. sample finished (qa_integrate, section E; scene.cpp:92-121)
    bool pixelDone = false;
    if (alive && done) {
      int sidx = QA_SIDX();
      const float inv = (float) (sidx + 1);
      f3 mean = F3(acc[0], acc[64], acc[2 * 64]);
      f3 cstd = F3(0, 0, 0);
      const f3 dc = (QA_PL() - mean) / inv;
      mean = mean + dc;
      acc[0] = mean.x; acc[64] = mean.y; acc[2 * 64] = mean.z;
      if (rp.spp_min < rp.spp_max) {   // (the running variance is read by the "another sample?" test below alone: qa_integrate, section E)
        cstd = F3(acc[3 * 64], acc[4 * 64], acc[5 * 64]);
        if (sidx > 0) cstd = cstd + ((dc * dc) * inv - cstd / (float) sidx);
        acc[3 * 64] = cstd.x; acc[4 * 64] = cstd.y; acc[5 * 64] = cstd.z;
      }
      ++sidx;
      acc[14 * 64] = __int_as_float(sidx);
      const bool more = sidx < rp.spp_min || (sidx < rp.spp_max && (cstd.x > 0.005f || cstd.y > 0.001f || cstd.z > 0.005f));
      if (more) {
        if (CHUNK && rp.chunk_spp && sidx >= chunkEnd) {
          needPixel = true;   // the chunk's last sample of this pixel: its state goes to the next chunk's wave when the tile is handed on (section A)
        } else {
          needSample = true;
        }
      } else {
        const uint32_t q = QA_Q();
        rp.rgb[3 * q + 0] = mean.x;
        rp.rgb[3 * q + 1] = mean.y;
        rp.rgb[3 * q + 2] = mean.z;
        rp.ns[q] = (uint32_t) sidx;
        if (CHUNK) acc[13 * 64] = __uint_as_float(q | 0x80000000u);   // (finished: csChunkSaveAll tells the tile's later chunks)
        pixelDone = true;
        needPixel = true;
      }
    }
    cnt.pixels += (unsigned long long) __popcll(__ballot(pixelDone));
    QA_TACC(cnt.sl[7], tE)
#ifdef QA_STAMPS
    if (lane == 0) cnt.sl[8] += 1;
#endif
  }

  // the tallies are per wave: one lane adds them
  unsigned long long *dst = reinterpret_cast<unsigned long long *>(rp.counters);
  if (lane == 0) {
    if (cnt.samples) atomicAdd(&dst[0], cnt.samples);
    if (cnt.casts_normal) atomicAdd(&dst[1], cnt.casts_normal);
    if (cnt.casts_shadow) atomicAdd(&dst[2], cnt.casts_shadow);
    if (cnt.pixels) atomicAdd(&dst[5], cnt.pixels);
  }
#ifdef QA_STAMPS
  if (lane == 0) {
    cnt.sl[0] = __builtin_readcyclecounter() - tKernel;
    cnt.sl[9] = 1;
    for (int i = 0; i < QA_NSTAMPS; ++i) atomicAdd(&dst[6 + i], cnt.sl[i]);
  }
#endif
