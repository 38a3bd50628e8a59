/* qaray_hip.h — C ABI of the MI355X hot path (libqaray_hip.so, gfx950 only).
 *
 * The reference has no FFI: its hot path is reached through in-process C++ virtual calls
 * (SURVEY.md §8b).  This header is the boundary a maintainer of the reference would bind from
 * Renderer::ThreadRender; each entry point names the reference interface it stands in for
 * (paths in the reference repo).  Plain pointers and sizes only; one host thread per context;
 * every call returns QA_OK (0) or a negative QA_E* code (include/qaray_host.h) and never throws.
 * The library owns all device memory behind the opaque handle; callers own every buffer they
 * pass in.  There is NO CPU fallback: without a gfx950 device qa_ctx_create fails.
 *
 *   qa_ctx_create / destroy        Renderer::Renderer / Terminate      src/renderers/renderer.cpp:67-70,293-298
 *   qa_scene_upload                Renderer::ComputeScene (scene side)  src/renderers/renderer.cpp:71-113
 *   qa_scene_upload_device         same, blob already in HBM (after an RCCL broadcast); the
 *                                  reference instead re-parses the XML on every rank
 *                                                                       src/renderers/Renderer_MPI.cpp:54
 *   qa_scene_edit_*, qa_scene_download   (no counterpart: the reference loads a scene once per process; what a viewer built on
 *                                  Renderer_GUI would need to move the camera or a light without a reload)
 *   qa_render_region[_device]      Renderer::ThreadRender -> PixelRender over a pixel region:
 *                                  camera ray, Scene::TraceNodeNormal, Material::Shade,
 *                                  Light::Illuminate/GenLight::Shadow, SuperSamplerHalton
 *                                                                       src/renderers/renderer.cpp:302-423
 *   qa_render_strips_device        Renderer_MPI's rank-strided ThreadRender (every rank renders
 *                                  tiles rank, rank+size, ...)          src/renderers/renderer.cpp:383-387
 *   qa_request_stop / qa_clear_stop   tasking::signal_stop / signal_start  src/tasking/parallel_for.cpp:70-73
 *   qa_photon_maps_build / clear   the photon-map block of Renderer::ComputeScene with
 *                                  RendererParam::usePhotonMap (-use-photon-map): photon tracing,
 *                                  power scaling, kd-tree; afterwards qa_render_* shade with
 *                                  Scene::usePhotonMap = true        src/renderers/renderer.cpp:114-291,
 *                                                                       src/materials/MtlBlinn_PhotonMap.cpp:349-458
 *   qa_progressive_*               Renderer_GUI's progressive display: BeginRender starts the render
 *                                  threads, the window shows renderImage while it fills, StopRender
 *                                  signals the stop            src/renderers/Renderer_GUI.cpp:37-97
 *   qa_display_device,             renderImage's 8-bit products: the tail of PixelRender (LinearToSRGB, clamp, round) and
 *   qa_progressive_display*        FrameBuffer::ComputeZBufferImage / ComputeSampleCountImage, computed where the frame
 *                                  is; what Renderer_GUI shows of renderImage   src/fb/framebuffer.cpp:62-107,
 *                                                                       src/renderers/renderer.cpp:34-39,347-365
 *   qa_denoise_device,             (no counterpart: the reference shows its previews unfiltered; an edge-avoiding a-trous
 *   qa_progressive_denoise*        filter for the few-sample previews of an interactive session)
 *   qa_gbuffer_region*,            (no counterpart: what the camera ray of a pixel's first sample sees - depth, normal, diffuse
 *   qa_progressive_gbuffer_device  colour, node and material - for picking in a viewer and as guides for a preview filter)
 *   qa_matte_region*,              (no counterpart: the same over the camera rays of all of a pixel's samples - coverage, mean
 *   qa_progressive_matte_device,   albedo, normal and backdrop - and the straight-alpha RGBA picture made from them)
 *   qa_matte_rgba_device
 *   qa_idmatte_region*,            (no counterpart: which nodes or materials those samples' rays meet and how many samples each takes,
 *   qa_progressive_idmatte_device, ranked per pixel - an anti-aliased matte per object, as compositing asks of a renderer - and the
 *   qa_idmatte_select_device       coverage plane of a chosen set of ids made from it)
 *   qa_cast_rays*, qa_occluded*,   (no counterpart: Scene::TraceNodeNormal / TraceNodeShadow for rays of the caller's, and the camera
 *   qa_camera_rays_device          rays PixelRender starts from, handed out)       src/scene/scene.cpp:35-74
 *   qa_ao_region*, qa_ao_points*,  (no counterpart: ambient occlusion - how many of K short rays over the facing side of what a pixel's
 *   qa_progressive_ao_device       samples see, or of points of the caller's, meet nothing within a radius)
 *   qa_bake_texels*,               (no counterpart: the reference bakes nothing - the surface point of a node behind every texel of
 *   qa_bake_dilate_device          a texture laid over it, and the gutter fill of a baked picture)
 *   qa_denoise_guided_device,      (no counterpart: the preview filter with those normal and albedo planes as two more
 *   qa_progressive_denoise_guided* edge-stopping guides)
 *   qa_denoise_variance_device     (no counterpart: that filter with a per-pixel variance of the caller's in place of its spatial guess)
 *   qa_reproject_device,           (no counterpart: the reference renders every frame from nothing; the accumulated frame of
 *   qa_progressive_reproject_device   an earlier camera carried into the frame of the camera as it now stands)
 *   qa_reproject_motion_device,    (no counterpart: the same with the history of a node that moved fetched from where the node
 *   qa_progressive_reproject_motion_device,   was, and a clamp of the history to the current frame's neighbourhood)
 *   qa_reproject_node_motion
 *   qa_reproject_moments_device,   (no counterpart: the same carrying the first two luma moments of every pixel, for a per-pixel
 *   qa_progressive_reproject_moments_device   variance of the accumulated colour, and shortening the history the clamp moved)
 *   qa_radiance_rays*,             (no counterpart: PixelRender's path - Scene::TraceNodeNormal, Material::Shade, the lights - started
 *   qa_camera_sample_rays_device   from rays of the caller's instead of the camera ray, and the camera rays of every sample handed
 *                                  out)                                 src/renderers/renderer.cpp:312-341
 *   qa_irradiance_points*          (no counterpart: MtlBlinn_PhotonMap::Shade of a white diffuse hit at a surface point of the
 *                                  caller's - its lights, one diffuse bounce, the path behind it - with no ray leading there)
 *   qa_probe_sh*, qa_probe_shade_device,   (no counterpart: PixelRender's path along the directions of a cube map around a point in
 *   qa_probe_grid_shade_device     free space, projected onto spherical harmonics - the light a moving object there receives)
 *   qa_probevis_sh*,               (no counterpart: the distances those rays travelled as two moments per direction cell, and a grid
 *   qa_probevis_grid_shade_device  shading that weighs each probe by whether it sees the shading point - no light through walls)
 *   qa_reflprobe_prefilter_device, (no counterpart: a probe's cube map convolved with Phong lobes into a chain of ever smaller cube
 *   qa_reflprobe_shade_device,     maps, and the lookup of a direction at a level in it, in one probe or blended over a grid's cell -
 *   qa_reflprobe_grid_shade_device what a glossy Blinn material sees of its surroundings)
 *   qa_get_counters               (no counterpart: the reference only prints wall-clock)
 *   qa_get_kernel_time             Renderer::StartTimer/StopTimer       src/renderers/renderer.cpp:42-63
 */
#ifndef QARAY_HIP_H
#define QARAY_HIP_H

#include <stdint.h>

#include "qa_flat_scene.h" /* the records qa_scene_edit_* take */
#include "qa_photon.h"
#include "qaray_host.h" /* QA_OK / QA_E* */

#ifdef __cplusplus
extern "C" {
#endif

typedef struct qa_ctx qa_ctx;

typedef struct qa_counters {
  uint64_t samples;        /* camera paths started (1 sample = 1 iteration of PixelRender's loop) */
  uint64_t casts_normal;   /* closest-hit casts: camera + secondary rays */
  uint64_t casts_shadow;   /* any-hit casts */
  uint64_t bvh_nodes;      /* BVH nodes popped (only counted by stats launches, else 0) */
  uint64_t tri_tests;      /* triangle tests   (only counted by stats launches, else 0) */
  uint64_t pixels;         /* pixels completed */
} qa_counters;

/* flags for qa_render_region* */
#define QA_RENDER_STATS 1u  /* also count BVH nodes / triangle tests (slower kernel variant) */

int qa_ctx_create(int device_id, qa_ctx **out);
int qa_ctx_destroy(qa_ctx *ctx);

/* Upload a flattened scene (include/qa_flat_scene.h) from host memory / adopt a copy of one that
 * already sits in device memory.  Replaces any previous scene of the context. */
int qa_scene_upload(qa_ctx *ctx, const void *host_blob, uint64_t nbytes);
int qa_scene_upload_device(qa_ctx *ctx, const void *device_blob, uint64_t nbytes);

/* Scene edits: the camera, lights, materials and node transforms of the resident scene, rewritten in place.  After an edit the
 * context is in the state qa_scene_upload of the edited blob would leave it in - same kernel plan, same qa_get_kernel_name, same
 * bits in every later frame - but no mesh or texture table is rebuilt, copied or reallocated: the edited records go into the
 * resident blob (host and device copy) and the few tables derived from them are built again on the host (qa_scene_build.h
 * RebuildSceneSide) and copied over their device copies.  Records are those of include/qa_flat_scene.h; `first`, `n` select
 * records [first, first + n) of the blob's table.
 *   qa_scene_edit_camera     the header's camera block (screenA/U/V/X/Y, cam_pos, dof).  The image size cannot change.
 *   qa_scene_edit_lights     every field may change (a point light may become an area light, any light an ambient one ...)
 *   qa_scene_edit_materials  colours, glossiness, ior, absorption, kill.  QA_EINVAL when a record's texmap references differ
 *                            from the resident ones (texture tables are not rebuilt)
 *   qa_scene_edit_instances  tm, itm, pos.  QA_EINVAL when a record changes obj_type, mesh, mtlset, parent, subtree_end or depth
 * (Texmaps, texture colours, texels and the backdrop colours: the texture edits below.)
 * An edit that changes the plan (area lights appear or go, the shadow-casting lights cross QA_CS_LIGHT_BATCH, the root node
 * stops being the identity ...) selects the integrator again, and allocates the per-thread slab the new plan needs if no earlier
 * plan of this scene did; no other edit allocates device memory.  An edit that a fresh upload would refuse returns that upload's
 * code; QA_EINVAL: null argument, first + n beyond the table; QA_ENOSCENE: no scene.  A refused edit changes nothing.
 * Edits are ordered with the context's stream and never wait for the device: the copies leave pinned staging asynchronously and
 * the scene record is passed by value at launch, so a frame already enqueued renders the old scene and the next one the new.
 * (The staging is a ring: an edit waits for an earlier EDIT's copies only when the ring wraps.)
 * A progressive frame becomes stale: qa_progressive_advance returns QA_EINVAL until qa_progressive_restart or a new
 * qa_progressive_begin, while read / display / status keep serving the old frame's pixels.  The photon maps do not depend on
 * the camera: qa_scene_edit_camera keeps them; the other edits drop them as an upload does (their memory is released by the next
 * upload, build, clear or qa_ctx_destroy).
 *   qa_scene_download        the resident blob as it now stands (nbytes: its size, also when out is NULL or capacity too small,
 *                            which returns QA_EINVAL)
 *   qa_get_scene_stats       [0] mesh-table builds (calls of the per-mesh builder) since the context was created, [1] scene
 *                            device allocations since then, [2] bytes copied to the device by the last upload or edit,
 *                            [3] edits applied since the last upload
 * No reference counterpart: the reference loads a scene once per process (Renderer_GUI has no scene editing). */
int qa_scene_edit_camera(qa_ctx *ctx, const qa_camera *camera);
int qa_scene_edit_lights(qa_ctx *ctx, uint32_t first, uint32_t n, const qa_light *lights);
int qa_scene_edit_materials(qa_ctx *ctx, uint32_t first, uint32_t n, const qa_material *materials);
int qa_scene_edit_instances(qa_ctx *ctx, uint32_t first, uint32_t n, const qa_instance *instances);
int qa_scene_download(qa_ctx *ctx, void *out, uint64_t capacity, uint64_t *nbytes);
int qa_get_scene_stats(qa_ctx *ctx, uint64_t out[4]);

/* Texture edits of the resident scene: the same contract as the edits above - afterwards the context is where qa_scene_upload of
 * the edited blob would leave it (same plan, same qa_get_kernel_name, same bits in every later frame, qa_scene_download returns the
 * edited blob byte for byte), no mesh tree is rebuilt, no table reallocated, and a refused edit changes nothing.  The kernels read
 * qa_texmap and qa_texture records straight from the resident device blob and get the two backdrop colours by value at launch, so
 * the record edits are blob writes; the one derived table, the float texels (16 bytes per texel, byte / 255.0f), is recomputed for
 * the edited rectangle on the device.
 *   qa_scene_edit_texmaps   itm, pos and texture.  texture must be in -1 .. num_textures - 1 (QA_EINVAL otherwise, as an upload
 *                           says): this is how a viewer swaps the image a map shows among the resident textures - the material
 *                           side keeps its texmap references (qa_scene_edit_materials)
 *   qa_scene_edit_textures  color1 and color2 (a checker's colours).  QA_EINVAL when a record changes type, width, height or
 *                           off_texels: the texel table is not laid out again
 *   qa_scene_edit_backdrop  the colours of the header's background and environment; either pointer may be NULL (stays as it
 *                           is).  QA_EINVAL when a record's texmap differs from the resident one
 *   qa_scene_edit_texels    texels [x0, x1) x [y0, y1) of file texture `texture` <- rows of RGB8, row_stride_bytes apart.  The
 *                           bytes go into the resident blob (host and device copy) and the rectangle's float entries are made
 *                           again by a kernel.  The source leaves through the pinned edit ring in slices of 64 KB (the ring does
 *                           not grow with the texture): 3 bytes per texel cross the link.  Only enqueues on the context's stream;
 *                           waits for an earlier edit only when the ring wraps.  QA_EINVAL: a checker texture, a texture beyond
 *                           the table, an empty rectangle or one beyond the texture, a stride below 3 * (x1 - x0), a null source
 *   qa_scene_edit_texels_device   the same with the source in device memory: nothing crosses the link.  hip_stream is the stream
 *                           the source was produced on (NULL: the caller guarantees that it is ready): the context's stream waits
 *                           for it before the kernel runs, and hip_stream waits for the kernel afterwards, so the caller may
 *                           overwrite the source on that stream right after the call.  The host copy of the blob is brought up
 *                           to date lazily: qa_scene_download first fetches the bytes of the textures edited this way from the
 *                           device blob (and then synchronises); nothing else reads texels on the host
 * Side effects as for the other non-camera edits: a progressive frame goes stale until qa_progressive_restart, the photon maps
 * are dropped (photon tracing samples textures), and a frame on a stream of the caller's is ordered behind the edit.
 * qa_get_scene_stats [2] after a texel edit: the RGB8 bytes staged (host variant), 0 (device variant).
 * No reference counterpart (the reference loads its textures once per process). */
int qa_scene_edit_texmaps(qa_ctx *ctx, uint32_t first, uint32_t n, const qa_texmap *texmaps);
int qa_scene_edit_textures(qa_ctx *ctx, uint32_t first, uint32_t n, const qa_texture *textures);
int qa_scene_edit_backdrop(qa_ctx *ctx, const qa_texcolor *background, const qa_texcolor *environment);
int qa_scene_edit_texels(qa_ctx *ctx, uint32_t texture, int x0, int y0, int x1, int y1, const uint8_t *rgb8, uint64_t row_stride_bytes);
int qa_scene_edit_texels_device(qa_ctx *ctx, uint32_t texture, int x0, int y0, int x1, int y1, const uint8_t *d_rgb8,
                                uint64_t row_stride_bytes, void *hip_stream);

/* Render pixels [x0,x1) x [y0,y1) of the scene's image.  Outputs are region-local, row-major:
 * rgb (y1-y0)*(x1-x0)*3 floats of LINEAR mean radiance (sRGB/quantisation stay in FrameBuffer),
 * depth: hit distance of sample 0 (1e30 on a miss), nsamples: samples taken (0 = pixel skipped
 * because a stop was requested).  Pixel (i,j) always uses RNG stream qa_pixel_seed(seed,
 * j*width+i) (include/qa_seed.h), so any partition of the image gives identical pixels.
 * 1 <= spp_min <= spp_max: spp_min samples always, up to spp_max while the running variance
 * exceeds the reference's thresholds (SuperSamplerHalton::Loop, src/scene/scene.cpp:92-97).
 * The host variant synchronises and copies back; the device variant writes device buffers and
 * only enqueues work on `hip_stream` (a hipStream_t; NULL = the context's own non-blocking stream -
 * note that NULL is also the handle of the legacy default stream, which therefore cannot be
 * selected: consumers on other streams must wait for qa_synchronize or pass their own stream). */
int qa_render_region(qa_ctx *ctx, int x0, int y0, int x1, int y1, int spp_min, int spp_max,
                     int max_bounce, uint32_t seed, uint32_t flags, float *rgb, float *depth,
                     uint32_t *nsamples);
int qa_render_region_device(qa_ctx *ctx, int x0, int y0, int x1, int y1, int spp_min, int spp_max,
                            int max_bounce, uint32_t seed, uint32_t flags, float *d_rgb,
                            float *d_depth, uint32_t *d_nsamples, void *hip_stream);
/* Image-space partition between GPUs.  The region is cut into horizontal strips of QA_STRIP_ROWS
 * (8) pixel rows; this call renders strips first_strip, first_strip + strip_step, ... (rank r of
 * n: first_strip = r, strip_step = n), i.e. the reference's round-robin tile ownership
 *   tasking::parallel_for(tileStart = mpiRank, tileStop, tileStep = mpiSize)   src/renderers/renderer.cpp:383-387
 * Outputs are PACKED strip after strip: row (k*8 + i) of the buffers is row
 * y0 + (first_strip + k*strip_step)*8 + i of the image; buffers hold qa_strip_count()*8 rows of
 * (x1-x0) pixels (rows of a ragged last strip that fall below y1 keep nsamples = 0). */
#define QA_STRIP_ROWS 8
int qa_render_strips_device(qa_ctx *ctx, int x0, int y0, int x1, int y1, int first_strip, int strip_step,
                            int spp_min, int spp_max, int max_bounce, uint32_t seed, uint32_t flags,
                            float *d_rgb, float *d_depth, uint32_t *d_nsamples, void *hip_stream);
int qa_strip_count(int y0, int y1, int first_strip, int strip_step);
/* Which 8x8 tiles of such a launch does the frame finish in closed form, because no camera ray of theirs can hit anything (option
 * "empty_tiles"; qaray_amd/csrc/hip/qa_emptytile.h)?  One byte per tile, 1 = empty, strip after strip as above: (x1-x0+7)/8 tiles per
 * strip, qa_strip_count() strips.  The decision the frame's kernel takes, by the same device function; all zero where a frame of
 * this context with its current options takes none (another kernel, the option off, depth of field, no tile lists).  Nothing of it
 * is read back inside a frame.  Only enqueues on hip_stream, ordered as the read-only passes are: behind the context's last frame
 * and last edit, and a later edit waits for it.  qa_test_empty_tiles_host: the same from the host build of that header, for a context with default
 * options (no GPU and no context needed).  No reference counterpart. */
int qa_empty_tiles_device(qa_ctx *ctx, int x0, int y0, int x1, int y1, int first_strip, int strip_step, uint8_t *d_mask, void *hip_stream);
int qa_test_empty_tiles_host(const void *blob, int x0, int y0, int x1, int y1, int first_strip, int strip_step, uint8_t *mask);
/* Wait for everything enqueued by this context. */
int qa_synchronize(qa_ctx *ctx);

/* Photon / caustics maps (the reference's -use-photon-map mode).  qa_photon_maps_build traces
 * photons from the scene's point lights on the GPU - one RNG stream per emission, see
 * include/qa_photon.h - keeps the first params->*.size of them in the reference's order, scales
 * their powers by 1 / emitted rays, balances each map into cyPhotonMap's kd-tree and leaves both
 * resident in HBM; from then on qa_render_* shade with Scene::usePhotonMap = true (a DIFFUSE
 * selection gathers 100 nearest photons from the caustics map, and from the photon map instead of
 * bouncing after a diffuse bounce).  The maps live until qa_photon_maps_clear or the next scene
 * upload.  Deterministic in (scene, params, seed): every rank of a multi-GPU job builds the same maps.
 * Errors: QA_EUNSUPPORTED when the scene has no point light or a map cannot be filled within
 * QA_PHOTON_MAX_EMISSIONS (the reference divides by zero / loops forever in these cases).
 * qa_photon_maps_info: numOfEmittedRays and loop iterations per map ([0] photon, [1] caustics);
 * qa_photon_maps_download: the balanced records as they sit in HBM, size + 1 entries, [0] unused
 * ([1..size] is byte-compatible with the reference's photonmap.dat / caustics.dat dumps). */
int qa_photon_maps_build(qa_ctx *ctx, const qa_photon_params *params, uint32_t seed);
int qa_photon_maps_clear(qa_ctx *ctx);
int qa_photon_maps_info(qa_ctx *ctx, uint64_t emitted[2], uint64_t emissions[2]);
int qa_photon_maps_download(qa_ctx *ctx, int which, qa_photon *out, uint64_t capacity);

int qa_request_stop(qa_ctx *ctx);
int qa_clear_stop(qa_ctx *ctx);

/* Progressive frames: an image resident in HBM whose sample count is raised in passes (1, 4, 16, ... spp), with a preview
 * between passes and a stop / resume at any point.  The final image is bit-identical to the one-shot frame of the same
 * arguments: every pixel takes the same samples in the same order, its state (RNG state, samples taken, running mean and
 * variance: 32 bytes) waiting in device memory between passes.  One frame per context.
 *   qa_progressive_begin    validates like qa_render_region (same codes) and allocates the frame's slabs (52 bytes per pixel,
 *                           4 + 4 per 8x8 tile); renders nothing.  flags: QA_RENDER_STATS.  Ends the previous frame, if any.
 *   qa_progressive_advance  one launch of the megakernel (never the staged pipeline) that brings every unfinished pixel to
 *                           min(spp_target, spp_max) samples; a pixel may finish earlier by the adaptive rule of spp_min /
 *                           spp_max.  Enqueues on hip_stream (NULL = the context's stream, as for qa_render_region_device).  A
 *                           target at or below the frame's level is a no-op; at or below the last pass's target the call first
 *                           asks the device for the level (synchronises).  qa_request_stop during a pass: tiles in hand finish
 *                           the pass, the others keep their level; a later pass to the same or a higher target completes them.
 *   qa_progressive_read     the preview (synchronises), region-local like qa_render_region: finished pixels' final mean and
 *   qa_progressive_read_device   sample count, the running mean and the samples so far of the others (rgb 0, ns 0 where none was
 *                           taken); depth is sample 0's hit distance (1e30 before it).  The device variant only enqueues.
 *   qa_progressive_status   (synchronises) spp_reached: the lowest level of the frame's tiles; pixels_finished: pixels done
 *                           for good (spp_max or the adaptive rule); tiles_behind: tiles below the last pass's target (non-zero
 *                           after a stop).  Any pointer may be NULL.
 *   qa_progressive_end      frees the frame (also done by qa_ctx_destroy).
 *   qa_progressive_restart  starts the current frame again after a scene edit (or at any time): same region, spp, bounce, seed,
 *                           flags and slabs, every pixel's state fresh and every tile at level 0, as after qa_progressive_begin.
 *                           Validates like qa_progressive_begin against the edited scene; frees and allocates nothing; only
 *                           enqueues on the context's stream.
 * qa_scene_upload*,qa_photon_maps_build and qa_photon_maps_clear end the frame: a later advance / read / status returns
 * QA_EINVAL and qa_last_error says why.  qa_render_* frames between passes do not disturb it, and qa_set_option /
 * qa_set_pipeline may change between passes (same bits). */
int qa_progressive_begin(qa_ctx *ctx, int x0, int y0, int x1, int y1, int spp_min, int spp_max, int max_bounce, uint32_t seed,
                         uint32_t flags);
int qa_progressive_advance(qa_ctx *ctx, int spp_target, void *hip_stream);
int qa_progressive_read(qa_ctx *ctx, float *rgb, float *depth, uint32_t *nsamples);
int qa_progressive_read_device(qa_ctx *ctx, float *d_rgb, float *d_depth, uint32_t *d_nsamples, void *hip_stream);
int qa_progressive_status(qa_ctx *ctx, int *spp_reached, uint64_t *pixels_finished, uint64_t *tiles_behind);
int qa_progressive_end(qa_ctx *ctx);
int qa_progressive_restart(qa_ctx *ctx);

/* Passes over some of a progressive frame's tiles: the caller's choice, or the noisiest first.  A pass changes when a pixel takes
 * its samples, never which: the finished frame keeps the one-shot frame's bits.  The region's 8x8 tiles are counted row-major from
 * its top left corner, tiles_x = (x1 - x0 + 7) / 8 a row (qa_progressive_tile_count); a mask has one byte per tile, non-zero =
 * selected.
 *   qa_progressive_advance_tiles         qa_progressive_advance(T = min(spp_target, spp_max)) restricted to the mask: the selected
 *   qa_progressive_advance_tiles_device  tiles whose level is below T end at T, nothing else takes a sample (an empty choice still
 *                           launches and takes none).  The tiles are chosen on the device, in the frame's tile order; both
 *                           variants only enqueue on hip_stream: the host variant copies its mask to pinned memory first (and
 *                           waits there for its own previous copy alone), the device variant's mask must stay valid until the
 *                           pass has run.  Afterwards qa_progressive_status counts the tiles left below T as behind, and a
 *                           qa_progressive_advance to T (or above) completes them.  Refuses as qa_progressive_advance does
 *                           (no frame, a stale frame, spp_target < 1) and a null mask: QA_EINVAL.
 *   qa_progressive_tile_levels[_device]  per tile, the samples every unfinished pixel of it has (uint32).  The host forms of this
 *   qa_progressive_tile_error[_device]   and the next synchronise, the device forms only enqueue.  The error (float): the mean
 *                           over the tile's 64 slots of the estimated variance of each live pixel's mean in its worst channel
 *                           (running variance / samples taken; finished pixels and slots outside the region count 0), summed in
 *                           a fixed order; +inf while a live pixel has fewer than 2 samples; 0 where all are finished.  The
 *                           opening comment of qaray_amd/csrc/hip/qa_prog_error_dev.h is the exact rule.
 *   qa_progressive_advance_adaptive      one pass to T over the noisiest tiles: of the candidates (level < T and error > min_error;
 *                           min_error 0 leaves finished tiles out) the max_tiles of greatest error, +inf first, equal errors by
 *                           ascending tile index; max_tiles 0: every candidate.  Error map, selection and pass are enqueued on
 *                           hip_stream and nothing is read back.  QA_EINVAL also for a min_error that is negative or a NaN.
 *   qa_progressive_adaptive_info         (synchronises) of the last adaptive pass: out[0] tiles selected, out[1] candidates,
 *                           out[2] the bits of the smallest selected error (0: none selected), out[3] the bits of the largest
 *                           finite error among the candidates (0: none).  All 0 before the first such pass of the frame.
 *   qa_progressive_state    (synchronises) the frame's state slab, 8 words per pixel of the region, row-major: RNG state,
 *                           samples taken | bit 31 finished, the running mean (3 floats) and variance (3 floats).
 * A frame begun with spp_min == spp_max keeps no variance: qa_progressive_tile_error* and qa_progressive_advance_adaptive return
 * QA_EUNSUPPORTED on it (begin with spp_min < spp_max for the estimate); levels and masked passes work on every frame.
 * qa_test_tile_error_host / qa_test_tile_select_host: the error map of a state slab and the selection rule on the CPU, compiled
 * from the kernels' source (no context, no GPU); mask gets 1 / 0 per tile, info (may be NULL) qa_progressive_adaptive_info's words. */
int qa_progressive_tile_count(qa_ctx *ctx, int *tiles_x, int *tiles_y);
int qa_progressive_advance_tiles(qa_ctx *ctx, int spp_target, const uint8_t *tile_mask, void *hip_stream);
int qa_progressive_advance_tiles_device(qa_ctx *ctx, int spp_target, const uint8_t *d_tile_mask, void *hip_stream);
int qa_progressive_tile_levels(qa_ctx *ctx, uint32_t *levels);
int qa_progressive_tile_levels_device(qa_ctx *ctx, uint32_t *d_levels, void *hip_stream);
int qa_progressive_tile_error(qa_ctx *ctx, float *error);
int qa_progressive_tile_error_device(qa_ctx *ctx, float *d_error, void *hip_stream);
int qa_progressive_advance_adaptive(qa_ctx *ctx, int spp_target, uint32_t max_tiles, float min_error, void *hip_stream);
int qa_progressive_adaptive_info(qa_ctx *ctx, uint64_t out[4]);
int qa_progressive_state(qa_ctx *ctx, uint32_t *state);
int qa_test_tile_error_host(const uint32_t *state, int width, int height, float *error);
int qa_test_tile_select_host(const float *error, const uint32_t *levels, uint32_t tiles, uint32_t target, uint32_t max_tiles, float min_error,
                             uint8_t *mask, uint64_t info[4]);

/* The FrameBuffer's 8-bit products of a frame of float results, computed on the device: byte for byte what the host FrameBuffer
 * (Deposit + ComputeZBufferImage + ComputeSampleCountImage) makes of the same floats.  Per pixel:
 *   color     3 bytes: LinearToSRGB when use_srgb, MIN(1, .), MAX(0, .), roundf(c * 255)
 *   count     (uint8_t) (255.f * ns / spp_max)
 *   zimg      0 where depth == 1e30, else (uint8_t) ((zmax - z) / (zmax - zmin) * 255)
 *   countimg  (uint8_t) (255 * (count - smin) / (smax - smin)) in integers; 0 everywhere when smax == smin
 *   mask      ns != 0
 * A float becomes a byte as the host library's x86-64 build does it: NaN and |x| >= 2^31 give 0, else the low byte of the truncated
 * int.  A pixel with ns == 0 was skipped (stop request): colour 0, count 0, mask 0 and depth 0.0f, as FrameBuffer::Init leaves it.
 * stats: zmin (from 1e30 down) and zmax (from 0 up) over the depths other than 1e30, NaNs never counting; smin (from 255) and smax
 * (from 0) over the count bytes; a zero zmin is reported as +0.
 *   qa_display_device               npix pixels of plain device buffers -> device buffers.  Only enqueues on hip_stream (NULL = the
 *                                   context's stream, as for qa_render_region_device): a statistics kernel and an encode kernel.
 *   qa_progressive_display          the progressive frame's products straight from its slabs - finished pixels' outputs, the running
 *   qa_progressive_display_device   mean and samples so far of the others, exactly the floats qa_progressive_read returns, which are
 *                                   never written out.  spp_max is the frame's.  The host variant copies back 3 + 1 + 1 + 1 + 1
 *                                   bytes per pixel at most, and synchronises; the device variant only enqueues.
 * Every output pointer may be NULL (not wanted).  QA_EINVAL: npix == 0, spp_max < 1, a null source buffer; on a frame that has
 * ended, what the other qa_progressive_* calls return.  The frame is not changed.  The statistics block (32 bytes) and the host
 * variant's staging are allocated on first use and freed with the context. */
typedef struct qa_display_stats { float zmin, zmax; uint32_t smin, smax; } qa_display_stats;
int qa_display_device(qa_ctx *ctx, const float *d_rgb, const float *d_depth, const uint32_t *d_nsamples, uint64_t npix, int spp_max,
                      int use_srgb, uint8_t *d_color, uint8_t *d_count, uint8_t *d_zimg, uint8_t *d_countimg, uint8_t *d_mask,
                      qa_display_stats *d_stats, void *hip_stream);
int qa_progressive_display(qa_ctx *ctx, int use_srgb, uint8_t *color, uint8_t *count, uint8_t *zimg, uint8_t *countimg, uint8_t *mask,
                           qa_display_stats *stats);
int qa_progressive_display_device(qa_ctx *ctx, int use_srgb, uint8_t *d_color, uint8_t *d_count, uint8_t *d_zimg, uint8_t *d_countimg,
                                  uint8_t *d_mask, qa_display_stats *d_stats, void *hip_stream);

/* A filtered copy of a frame of float results: an edge-avoiding a-trous wavelet filter (Dammertz et al. 2010) guided by the frame's
 * own colour and by sample 0's hit distance, for the 1 - 8 spp previews between a scene edit and a converged frame.  The header
 * comment of qaray_amd/csrc/hip/qa_denoise_dev.h is its specification.  Per pixel:
 *   void   ns == 0, or a colour component or the depth not finite: weighs nothing, comes out as it went in (its bits)
 *   miss   depth == 1e30: filtered among miss pixels only
 *   hit    everything else: filtered among hit pixels, the weight falling with the depth difference measured in local slopes
 * and in every class with the luma difference measured in standard deviations of the 3x3 neighbourhood.  `iterations` passes of a
 * 5x5 kernel at steps 1, 2, 4, ...; iterations == 0 copies the input's bits.  qa_denoise_params_default: iterations 5,
 * sigma_color 4, sigma_depth 1, flags 0.  The result is for display only: no rendered frame changes, and the filter never
 * writes its inputs or the progressive frame's slabs.
 *   qa_denoise_device               width x height pixels of plain device buffers (row-major, as qa_render_region_device fills them)
 *                                   -> d_out_rgb, 3 floats per pixel; d_out_rgb == d_rgb is allowed.  Only enqueues on hip_stream
 *                                   (NULL = the context's stream, as for qa_render_region_device): a guide kernel and one kernel
 *                                   per iteration.
 *   qa_progressive_denoise          the progressive frame's preview filtered straight from its slabs: exactly the floats
 *   qa_progressive_denoise_device   qa_progressive_read returns go in, which are never written out.  The host variant copies back
 *                                   12 bytes per pixel and synchronises; the device variant only enqueues.  A stale frame (after a
 *                                   scene edit) is served as qa_progressive_read serves it.  As for qa_progressive_display_device
 *                                   and _read_device, a call on a stream of the caller's waits for the frame's last pass, but a
 *                                   later advance / restart / read on another stream does not wait for the filter: the caller
 *                                   orders it behind that stream (with iterations == 0 the call also writes the frame's preview
 *                                   buffers for depth and sample count, which qa_progressive_read fills on the context's stream).
 * QA_EINVAL: a null buffer or params, width or height < 1, iterations outside 0 .. 6, a sigma that is not finite or not positive,
 * flags other than 0; on a frame that has ended, what the other qa_progressive_* calls return.  The working planes (40 bytes per
 * pixel of the largest frame filtered so far) are allocated on first use, grow when a larger frame arrives (the call that grows
 * them waits for the device) and are freed with the context; they are not scene memory and qa_get_scene_stats does not count
 * them.  The 8-bit picture of a filtered preview is qa_display_device of the result with the frame's depth and sample counts. */
typedef struct qa_denoise_params { int iterations; float sigma_color, sigma_depth; uint32_t flags; } qa_denoise_params;
int qa_denoise_params_default(qa_denoise_params *params);
int qa_denoise_device(qa_ctx *ctx, const float *d_rgb, const float *d_depth, const uint32_t *d_nsamples, int width, int height,
                      const qa_denoise_params *params, float *d_out_rgb, void *hip_stream);
int qa_progressive_denoise(qa_ctx *ctx, const qa_denoise_params *params, float *rgb);
int qa_progressive_denoise_device(qa_ctx *ctx, const qa_denoise_params *params, float *d_rgb, void *hip_stream);

/* First-hit guide planes ("G-buffer") of pixels [x0,x1) x [y0,y1): per pixel one cast, the camera ray of the pixel's sample 0
 * exactly as qa_render_region builds it from (seed, pixel) - Halton offset, depth-of-field draws, texture differentials - through
 * the integrators' own closest-hit and texture code.  Region-local, row-major planes; every pointer may be NULL (not wanted), but
 * not all of them:
 *   depth   1 float    the hit distance, 1e30 on a miss: bit for bit the depth plane qa_render_region writes for the same seed
 *   normal  3 floats   the world-space unit normal of the hit as the integrator shades it (geometric side: not flipped towards
 *                      the viewer; on a mesh the normal interpolated between the face's vertex normals, which is the face's
 *                      own where the face is planar and its vertices are not shared with a tilted neighbour); 0, 0, 0 on a miss
 *   albedo  3 floats   the diffuse colour the integrator shades the hit with (the material's diffuse, through its texture where it
 *                      has one); 0 for a node without material, 1 for a multi-material mesh whose face names no material; on a
 *                      miss the background the camera ray returns (textured where the scene's background is)
 *   ids     2 int32    the hit's node index (qa_instance) and material index (qa_material); material -1: none, -2: the white
 *                      case above; bit 30 (QA_GBUFFER_BACKFACE) of a material word >= 0 is set when the ray hit a back
 *                      face (QA_GBUFFER_MATERIAL(word) gives the index again; a negative word stays as it is); -1, -1 on a miss
 * The kernel only reads the scene: no frame, progressive frame or counter (qa_get_counters) changes.  Codes as qa_render_region_device:
 * QA_ENOSCENE, QA_EINVAL for an empty region, one outside the image or no plane at all.  Ordered as a frame is: the device variant only
 * enqueues on hip_stream (NULL = the context's stream), behind the context's last frame and last edit, and a later edit waits for it;
 * the host variant copies back and synchronises.
 *   qa_progressive_gbuffer_device   the planes of the progressive frame's region and seed, computed afresh from the scene as it
 *                                   now stands on each call: after an edit and qa_progressive_restart they show the edited scene */
#define QA_GBUFFER_BACKFACE 0x40000000
#define QA_GBUFFER_MATERIAL(word) ((word) < 0 ? (word) : ((word) & ~QA_GBUFFER_BACKFACE))
int qa_gbuffer_region_device(qa_ctx *ctx, int x0, int y0, int x1, int y1, uint32_t seed, float *d_normal, float *d_albedo,
                             float *d_depth, int32_t *d_ids, void *hip_stream);
int qa_gbuffer_region(qa_ctx *ctx, int x0, int y0, int x1, int y1, uint32_t seed, float *normal, float *albedo, float *depth,
                      int32_t *ids);
int qa_progressive_gbuffer_device(qa_ctx *ctx, float *d_normal, float *d_albedo, float *d_depth, int32_t *d_ids, void *hip_stream);

/* Matte planes of pixels [x0,x1) x [y0,y1): the camera rays of ALL of a pixel's samples, each exactly as qa_render_region builds it
 * (Halton pair of the sample, texture differentials) and as qa_gbuffer_region casts sample 0, reduced per pixel in sample order (the
 * opening comment of qaray_amd/csrc/hip/qa_matte_dev.h is the specification).  A pixel takes samples 0 .. n - 1: n = spp, or with a
 * d_ns plane (region-local, one uint32 per pixel: a frame's sample counts) n = min(ns, spp); n = 0 writes 0 to every plane of the
 * pixel.  Region-local, row-major planes; every pointer may be NULL (not wanted), but not all of them:
 *   coverage  1 float    (float) hits / (float) n: the fraction of the samples' camera rays that hit something - a frame's alpha
 *   albedo    3 floats   the running mean (m += (x - m) / (s + 1), a frame's own rule) of what qa_gbuffer_region's albedo plane holds
 *                        for each sample's ray: bit for bit the frame of the scene's "emission := diffuse" twin at n samples and no bounce
 *   normal    3 floats   the running mean of the hit normals over the samples that hit (the divisor counts hits); 0 when none does;
 *                        not normalised
 *   backdrop  3 floats   the same mean as albedo's of the backdrop colour on a miss and 0 on a hit: the part of a frame's colour that
 *                        came from camera rays which met nothing; rgb - backdrop is the premultiplied foreground
 * With spp = 1 and no ns plane, albedo and normal are qa_gbuffer_region's bits and coverage is 0 or 1.
 * The kernel only reads the scene: no frame, progressive frame or counter (qa_get_counters) changes.  Codes: QA_ENOSCENE; QA_EINVAL
 * for an empty region, one outside the image, spp = 0 or no plane at all; QA_EUNSUPPORTED for a camera with depth of field (dof > 0.1),
 * as qa_camera_sample_rays_device.  A refused call writes nothing.  Ordered as qa_gbuffer_region_device: the device variants only
 * enqueue on hip_stream (NULL = the context's stream), behind the context's last frame and last edit, and a later edit waits for
 * them; the host variant (ns and the planes in host memory) copies and synchronises.
 *   qa_progressive_matte_device   the planes of the progressive frame's region, n = the samples each pixel holds now (read from the
 *                                 frame's slabs as qa_progressive_read reads them), from the scene as it now stands
 *   qa_matte_rgba_device          npix pixels of device buffers -> 4 bytes each, straight (unassociated) alpha as PNG stores it:
 *                                 ns == 0 gives 0, 0, 0, 0; else a = coverage, per component c = a > 0 ? (rgb - backdrop) / a : 0, the
 *                                 colour byte of c as qa_display_device makes it (sRGB when srgb != 0) and the alpha byte that of a
 *                                 without sRGB.  Non-finite values end as those bytes do (a NaN: byte 0).  Only enqueues. */
int qa_matte_region_device(qa_ctx *ctx, int x0, int y0, int x1, int y1, uint32_t spp, const uint32_t *d_ns, float *d_coverage,
                           float *d_albedo, float *d_normal, float *d_backdrop, void *hip_stream);
int qa_matte_region(qa_ctx *ctx, int x0, int y0, int x1, int y1, uint32_t spp, const uint32_t *ns, float *coverage, float *albedo,
                    float *normal, float *backdrop);
int qa_progressive_matte_device(qa_ctx *ctx, float *d_coverage, float *d_albedo, float *d_normal, float *d_backdrop, void *hip_stream);
int qa_matte_rgba_device(qa_ctx *ctx, const float *d_rgb, const float *d_backdrop, const float *d_coverage, const uint32_t *d_ns,
                         uint64_t npix, int srgb, uint8_t *d_rgba, void *hip_stream);

/* Id matte of pixels [x0,x1) x [y0,y1): per pixel, which nodes (key = QA_IDMATTE_NODE) or materials (QA_IDMATTE_MATERIAL) the camera
 * rays of ALL its samples meet and how many samples each takes (the opening comment of qaray_amd/csrc/hip/qa_idmatte_dev.h is the
 * specification).  The samples are qa_matte_region's: a pixel takes samples 0 .. n - 1, n = spp, or with a d_ns plane n = min(ns, spp).
 * The key of a hit is word 0 of qa_gbuffer_region's ids for that ray (the node), or QA_GBUFFER_MATERIAL(word 1) (the material, back-face
 * bit cleared; -1 and -2 for hits without a material as documented there); a miss has none.  A pixel has QA_IDMATTE_SLOTS slots:
 * in sample order a hit adds 1 to the slot that holds its key, else takes the first free slot, else - the table is full - adds 1 to
 * `other`.  At the end the occupied slots are ordered by count descending, equal counts by id ascending; free slots follow with id
 * QA_IDMATTE_EMPTY (no key has that value) and count 0.  Region-local, row-major planes; every pointer may be NULL (not wanted), but
 * not all of them; ids and counts are written 16 bytes at a time and must be 16-byte aligned:
 *   ids      8 int32    the slots' ids
 *   counts   8 uint32   the slots' sample counts
 *   other    1 uint32   the samples that hit something while the table was full of other ids
 *   samples  1 uint32   n; sum(counts) + other is the number of samples that hit, n = 0 gives empties and zeros
 * The kernel only reads the scene: no frame, progressive frame or counter (qa_get_counters) changes.  Codes as qa_matte_region_device:
 * QA_ENOSCENE; QA_EINVAL for an empty region, one outside the image, spp = 0, a key that is neither of the two, a misaligned plane or
 * no plane at all; QA_EUNSUPPORTED for a camera with depth of field (dof > 0.1).  A refused call writes nothing.  Ordered as
 * qa_matte_region_device: the device variants only enqueue on `stream` (a hipStream_t; NULL = the context's stream), behind the context's last
 * frame and last edit, and a later edit waits for them; the host variant (ns and the planes in host memory) copies and synchronises.
 *   qa_progressive_idmatte_device   the planes of the progressive frame's region, n = the samples each pixel holds now, from the
 *                                   scene as it now stands (as qa_progressive_matte_device)
 *   qa_idmatte_select_device        npix pixels of device planes and m <= QA_IDMATTE_MAX_SELECT ids in HOST memory (copied before the
 *                                   call returns; NULL when m = 0) -> one float per pixel in d_out: (float) c / (float) n, c the integer
 *                                   sum of the counts of the slots whose id is in the list, 0 where n = 0; and / or its 8-bit grey
 *                                   picture in d_bytes, the byte qa_display_device makes of that value without sRGB (either may be NULL,
 *                                   not both).  Touches no state of the context; only enqueues.  QA_EINVAL for npix = 0 or
 *                                   > 2^31 - 1, a NULL plane or m above the limit. */
#define QA_IDMATTE_SLOTS 8
#define QA_IDMATTE_EMPTY INT32_MIN
#define QA_IDMATTE_NODE 0
#define QA_IDMATTE_MATERIAL 1
#define QA_IDMATTE_MAX_SELECT 256
int qa_idmatte_region_device(qa_ctx *ctx, int x0, int y0, int x1, int y1, uint32_t spp, const uint32_t *d_ns, int key, int32_t *d_ids,
                             uint32_t *d_counts, uint32_t *d_other, uint32_t *d_samples, void *stream);
int qa_idmatte_region(qa_ctx *ctx, int x0, int y0, int x1, int y1, uint32_t spp, const uint32_t *ns, int key, int32_t *ids,
                      uint32_t *counts, uint32_t *other, uint32_t *samples);
int qa_progressive_idmatte_device(qa_ctx *ctx, int key, int32_t *d_ids, uint32_t *d_counts, uint32_t *d_other, uint32_t *d_samples,
                                  void *stream);
int qa_idmatte_select_device(qa_ctx *ctx, const int32_t *d_ids, const uint32_t *d_counts, const uint32_t *d_samples, uint64_t npix,
                             const int32_t *select, uint32_t m, float *d_out, uint8_t *d_bytes, void *stream);

/* Ambient occlusion of pixels [x0,x1) x [y0,y1), and of points of the caller's: how much of the hemisphere over a surface point is
 * open within `radius`, as a count of open rays (the opening comment of qaray_amd/csrc/hip/qa_ao_dev.h is the specification: the
 * counter-based direction generator, the facing normal, the counters).  A pixel takes the camera rays of samples first .. first + n - 1
 * as qa_matte_region builds them: n = spp, or with a d_ns plane (region-local, one uint32 per pixel) n = min(max(ns - first, 0), spp).
 * Each is cast as qa_cast_rays casts; from every hit K rays go out from the hit point, cosine-weighted about the normal turned
 * towards the camera ray, with the counters s * K + k of the pixel's stream (y * width + x, as qa_camera_sample_rays_device's
 * d_stream), each tested as qa_occluded tests a ray with tmax = radius (bias 0.005 included).  Region-local, row-major planes; every
 * pointer may be NULL (not wanted), but not all of them:
 *   open  1 uint32   the rays that met nothing
 *   rays  1 uint32   the samples that hit something, times K
 *   ao    1 float    rays ? (float) open / (float) rays : 1; a pixel with n = 0 writes 0, 0, 1
 * The counts are integers and do not depend on the order in which rays are cast: the call equals the composition
 * qa_camera_sample_rays_device -> qa_cast_rays_device -> qa_test_ao_face_normal_host / qa_test_ao_directions_host ->
 * qa_occluded_device on every pixel (tests/test_gpu_ao.py).
 *   qa_progressive_ao_device   the planes of the progressive frame's region with the frame's seed, first = 0 and n = the samples each
 *                              pixel holds now, from the scene as it now stands (as qa_progressive_matte_device)
 *   qa_ao_points_device        n points [n][3] with unit normals [n][3], world space, fp32: point i casts the K rays of the counters
 *                              first + k of stream i, or d_stream_ids[i], about its normal as given.  d_open [n] uint32 and / or
 *                              d_ao [n] float = (float) open / (float) K.  A point with a component (its normal's included) that is
 *                              not finite, or with normal (0, 0, 0), is void: not walked, open = K, ao = 1.  n == 0 is QA_OK and
 *                              launches nothing; n > 2^31 - 1, a NULL array or no output are QA_EINVAL as for the ray queries.
 * The kernels only read the scene: no frame, progressive frame, counter (qa_get_counters) or kernel-time record changes.  Codes:
 * QA_ENOSCENE; QA_EINVAL for an empty region, one outside the image, spp = 0, K = 0 or K > QA_AO_MAX_RAYS, (first + spp) * K (points:
 * first + K) beyond 32 bits, a radius that is NaN or <= 0.005 (+inf is allowed: unbounded, taken as 1e30) or no plane at all;
 * QA_EUNSUPPORTED for a camera with depth of field (dof > 0.1; the points form answers).  A refused call writes nothing.  Ordered as
 * qa_matte_region_device: the device variants only enqueue on `stream` (a hipStream_t; NULL = the context's stream), behind the
 * context's last frame and last edit, and a later edit waits for them; the progressive form first waits for the frame's last pass;
 * the host variants (arrays in host memory) copy and synchronise.
 *   qa_ao_grey_device          npix floats of a device plane -> one byte each in d_bytes: the plane's 8-bit grey picture, the byte
 *                              qa_display_device makes of the value without sRGB.  Touches no state of the context; only enqueues.
 *                              QA_EINVAL for npix = 0 or > 2^31 - 1 or a NULL buffer. */
#define QA_AO_MAX_RAYS 256
int qa_ao_region_device(qa_ctx *ctx, int x0, int y0, int x1, int y1, uint32_t first, uint32_t spp, const uint32_t *d_ns, uint32_t K,
                        float radius, uint32_t seed, uint32_t *d_open, uint32_t *d_rays, float *d_ao, void *stream);
int qa_ao_region(qa_ctx *ctx, int x0, int y0, int x1, int y1, uint32_t first, uint32_t spp, const uint32_t *ns, uint32_t K, float radius,
                 uint32_t seed, uint32_t *open, uint32_t *rays, float *ao);
int qa_progressive_ao_device(qa_ctx *ctx, uint32_t K, float radius, uint32_t *d_open, uint32_t *d_rays, float *d_ao, void *stream);
int qa_ao_points_device(qa_ctx *ctx, uint64_t n, const float *d_points, const float *d_normals, const int32_t *d_stream_ids,
                        uint32_t first, uint32_t K, float radius, uint32_t seed, uint32_t *d_open, float *d_ao, void *stream);
int qa_ao_grey_device(qa_ctx *ctx, const float *d_ao, uint64_t npix, uint8_t *d_bytes, void *stream);
int qa_ao_points(qa_ctx *ctx, uint64_t n, const float *points, const float *normals, const int32_t *stream_ids, uint32_t first,
                 uint32_t K, float radius, uint32_t seed, uint32_t *open, float *ao);

/* Bake maps: which surface point of a node lies behind each texel of a width x height texture laid over it, so that a lightmap or an
 * occlusion map of an object can be made with the point queries above and written back with qa_scene_edit_texels_device (the opening
 * comment of qaray_amd/csrc/hip/qa_bake_dev.h is the specification: the texel's sample, the inside rule and why charts have no cracks,
 * the tiles, what a covered texel holds).  node: an instance index; a mesh with texture vertices or a plane (the built-in pair of
 * faces); texmap: an index into the scene's texmaps whose transform the texture vertices go through as the renderer's lookup sends
 * them, or -1 for the raw (u, v); mtl: only the faces with this qa_face::mtl, or -1 for all.  Row-major planes [height][width], row 0
 * the top row as stored; every pointer may be NULL (not wanted), but not all of them:
 *   point   3 floats   the surface point, world space
 *   normal  3 floats   the interpolated shading normal, world space, unit (NaN where the mesh's normals cancel), never flipped
 *   face    1 int32    the blob's face id (0 / 1 for a plane), -1 where no face covers the texel; the other planes then hold zeros
 *   bary    2 floats   the weights of the face's first two vertices
 * One sample per texel; where charts overlap the lowest face wins.  The kernel only reads the scene: no frame, progressive frame,
 * counter (qa_get_counters) or kernel-time record changes.  Codes: QA_ENOSCENE; QA_EINVAL for a width or height of 0 or above 8192, no
 * plane at all, a node out of range or without an object, a mesh without texture vertices, a texmap out of range or without a
 * texture; QA_EUNSUPPORTED for a sphere node, for a map under which a face spans more than 4 tiles of the texture along an axis, and
 * for a scene whose traversal stacks leave less than 15 KB of a workgroup's 64 KB of LDS (a stack depth near 50): the map's face
 * chunk sits beside the dynamic LDS every scene kernel is launched with.
 * A refused call writes nothing.  Ordered as qa_ao_points_device: the device variant only enqueues on `stream` (a hipStream_t; NULL =
 * the context's stream), behind the context's last frame and last edit, and a later edit waits for it; the host variant copies and
 * synchronises.
 *   qa_bake_dilate_device   the gutter fill of a baked RGB8 picture [height][width][3]: a texel with d_face >= 0 keeps its bytes,
 *                           another takes those of the nearest covered texel within `radius` (<= 8) texels per axis, wrapping at
 *                           the borders as the lookup wraps; ties go to dy ascending, then dx ascending; with none in reach it keeps
 *                           its own.  d_out must not overlap d_rgb8.  Touches no state of the context; only enqueues.  QA_EINVAL for
 *                           a NULL buffer, a bad size or radius, or an overlap. */
int qa_bake_texels_device(qa_ctx *ctx, int node, int texmap, int mtl, uint32_t width, uint32_t height, float *d_point, float *d_normal,
                          int32_t *d_face, float *d_bary, void *stream);
int qa_bake_texels(qa_ctx *ctx, int node, int texmap, int mtl, uint32_t width, uint32_t height, float *point, float *normal, int32_t *face,
                   float *bary);
int qa_bake_dilate_device(qa_ctx *ctx, const uint8_t *d_rgb8, const int32_t *d_face, uint32_t width, uint32_t height, uint32_t radius,
                          uint8_t *d_out, void *stream);

/* Ray queries: n rays of the caller's against the resident scene, through the integrators' own closest-hit and shadow walks (the
 * opening comment of qa_ray_query.hip is the specification).  Ray i has origin origins[3i .. 3i+2] and direction dirs[3i .. 3i+2],
 * world space, fp32, contiguous.  The direction is used as given and NOT normalised: t is the parameter along it (the hit is at
 * origin + t * direction).  A query meets exactly what a path segment of qa_render_region with that ray meets, bias included (a
 * hit with t <= 0.005 is not seen).  A ray with a component that is not finite, or with direction (0, 0, 0), is void: it is not
 * walked and answers as a miss / as not occluded.
 *   qa_cast_rays_device   the closest hit of every ray.  Outputs, each may be NULL (not wanted) but not all of them:
 *                           d_t       [n] float        the parameter of the hit, QA_RAY_MISS (1e30) on a miss
 *                           d_ids     [n][2] int32     node and material word as the ids of qa_gbuffer_region (-1, -1 on a miss;
 *                                                      QA_GBUFFER_BACKFACE, QA_GBUFFER_MATERIAL apply)
 *                           d_normal  [n][3] float     the world-space unit normal as the integrator shades it (geometric side); 0 on a miss
 *                           d_point   [n][3] float     the hit point in world space as the integrator continues from it; 0 on a miss
 *                         Only enqueues on hip_stream (NULL = the context's stream).
 *   qa_cast_rays          the same from and to host memory, through a staging buffer of the call's own that only grows (60 bytes
 *                         per ray of the largest batch so far, freed with the context); synchronises.
 *   qa_occluded_device    d_out[i] (uint8) = 1 if ray i meets a surface at 0.005 < t < d_tmax[i], else 0: what a shadow ray of that
 *                         length answers.  A tmax that is NaN or <= 0.005 gives 0; one above 1e30, +inf included, counts as 1e30.
 *   qa_occluded           the same from and to host memory (staging: 29 bytes per ray); synchronises.
 *   qa_camera_rays_device origin and direction (unit) of the camera ray of sample 0 of every pixel of [x0,x1) x [y0,y1), exactly as
 *                         qa_render_region builds it from (seed, pixel) - Halton offset, depth-of-field draws - into two
 *                         [(y1-y0)*(x1-x0)][3] float arrays, region-local and row-major.  qa_cast_rays of them gives the depth plane
 *                         of qa_render_region and the ids and normal planes of qa_gbuffer_region bit for bit.
 * The kernels only read the scene: no frame, progressive frame, counter or kernel time changes.  Ordered as qa_gbuffer_region_device:
 * behind the context's last frame and last edit; a later edit waits for them.  Codes: QA_ENOSCENE without a scene; n == 0 is
 * QA_OK and launches nothing (the arrays may then be NULL); QA_EINVAL for n > 2^31 - 1, a NULL ray array (or d_tmax), no output at
 * all, and for qa_camera_rays_device a NULL array or a region that qa_render_region refuses.  Every mesh is walked per lane (no
 * cooperative walks), rays are taken in the caller's order (not sorted), and no texture is looked up at the hit. */
#define QA_RAY_MISS 1.0e30f
int qa_cast_rays_device(qa_ctx *ctx, uint64_t n, const float *d_origins, const float *d_dirs, float *d_t, int32_t *d_ids,
                        float *d_normal, float *d_point, void *hip_stream);
int qa_cast_rays(qa_ctx *ctx, uint64_t n, const float *origins, const float *dirs, float *t, int32_t *ids, float *normal, float *point);
int qa_occluded_device(qa_ctx *ctx, uint64_t n, const float *d_origins, const float *d_dirs, const float *d_tmax, uint8_t *d_out,
                       void *hip_stream);
int qa_occluded(qa_ctx *ctx, uint64_t n, const float *origins, const float *dirs, const float *tmax, uint8_t *out);
int qa_camera_rays_device(qa_ctx *ctx, int x0, int y0, int x1, int y1, uint32_t seed, float *d_origins, float *d_dirs, void *hip_stream);

/* The filter above, guided by the first-hit planes as well (the GUIDED FORM section of qa_denoise_dev.h is the specification).  A
 * pixel whose 3x3 neighbourhood agrees on the guides (normals within 11.5 degrees, albedo components within 0.3, one class) also
 * weighs its taps by the normals' angle (1 - n_p . n_q over sigma_normal) and by the largest albedo difference (over 0.02); a pixel
 * on an edge of the guides, which sample 0 describes from one side only, is filtered as the unguided filter does it.  Colours are
 * never divided by the albedo.  flags names the planes given: a plane's pointer is NULL if and only if its bit is clear; with
 * flags == 0 the result is qa_denoise_device's bit for bit.  qa_denoise_guided_params_default: iterations 5, sigma_color 4,
 * sigma_depth 1, sigma_normal 0.1, both guides.  The progressive variants compute the frame's planes themselves
 * (qa_progressive_gbuffer_device, from the scene as it now stands) for the bits set in flags.  Codes, streams, aliasing
 * (d_out_rgb == d_rgb) and memory as for the unguided calls; the working planes are 72 bytes per pixel, and 96 for a progressive
 * frame.  QA_EINVAL also for unknown flag bits, a plane that disagrees with its bit and a sigma_normal that is not finite and
 * positive. */
#define QA_DENOISE_GUIDE_NORMAL 1u
#define QA_DENOISE_GUIDE_ALBEDO 2u
typedef struct qa_denoise_guided_params { int iterations; float sigma_color, sigma_depth, sigma_normal; uint32_t flags; } qa_denoise_guided_params;
int qa_denoise_guided_params_default(qa_denoise_guided_params *params);
int qa_denoise_guided_device(qa_ctx *ctx, const float *d_rgb, const float *d_depth, const uint32_t *d_nsamples, const float *d_normal,
                             const float *d_albedo, int width, int height, const qa_denoise_guided_params *params, float *d_out_rgb,
                             void *hip_stream);
int qa_progressive_denoise_guided(qa_ctx *ctx, const qa_denoise_guided_params *params, float *rgb);
int qa_progressive_denoise_guided_device(qa_ctx *ctx, const qa_denoise_guided_params *params, float *d_rgb, void *hip_stream);

/* The guided filter above with a variance plane of the caller's (the VARIANCE FORM section of qa_denoise_dev.h is the
 * specification): d_variance, 1 float per pixel, an estimate of the variance of the pixel's luma from the frames behind it - the
 * d_out_variance plane of qa_reproject_moments_device (below).  Pass 0 of the filter estimates a pixel's variance from the 3x3 luma
 * window of the one frame it is given, which cannot tell texture on a converged surface from noise; with QA_DENOISE_GUIDE_VARIANCE
 * = 4 a pixel whose plane value is finite and >= 0 takes variance_scale x the (1, 2, 1) x (1, 2, 1) mean of such values among the
 * pixels of its class in its 3x3 window instead, and every other pixel (the plane says -1, "none") keeps the spatial estimate.  Only
 * pass 0 changes: one more kernel in place of the old pass 0, the iterations run as they are.  With the flag clear, or a plane of -1
 * everywhere, the result is qa_denoise_guided_device's bit for bit.  qa_denoise_variance_params_default: the guided defaults,
 * variance_scale 4 (DESIGN.md 4k has the sweep), all three flags.  QA_EINVAL: everything qa_denoise_guided_device refuses, a
 * variance_scale that is not finite and positive, a variance plane that disagrees with its flag.  The variance is of the luma only;
 * there are no progressive variants (a viewer filters the accumulated buffers of the reprojection). */
#define QA_DENOISE_GUIDE_VARIANCE 4u
typedef struct qa_denoise_variance_params {
  int      iterations;
  float    sigma_color, sigma_depth, sigma_normal, variance_scale;
  uint32_t flags;
} qa_denoise_variance_params;
int qa_denoise_variance_params_default(qa_denoise_variance_params *params);
int qa_denoise_variance_device(qa_ctx *ctx, const float *d_rgb, const float *d_depth, const uint32_t *d_nsamples, const float *d_normal,
                               const float *d_albedo, const float *d_variance, int width, int height,
                               const qa_denoise_variance_params *params, float *d_out_rgb, void *hip_stream);

/* Temporal reprojection: the accumulated frame of an EARLIER camera (the history) carried into the frame just rendered from the
 * camera as it now stands, so that a camera move keeps the samples of the surface points both cameras see.  The header comment of
 * qaray_amd/csrc/hip/qa_reproject_dev.h is its specification.  Both frames cover pixels [x0, x0 + width) x [y0, y0 + height) of the
 * image, region-local and row-major.  Per pixel, from the depth of sample 0 (the depth plane of qa_render_region / qa_gbuffer_region)
 * and the two qa_camera records, the point the pixel shows is projected into the old camera; the four history pixels around it are
 * blended bilinearly, each counting only when it holds history (length > 0), is finite, has the pixel's class (miss / hit), lies
 * within depth_tolerance (relative) of the depth the old camera must have seen the point at, and - when both ids planes are given -
 * carries the pixel's node and material ids.  With history c_h of effective sample count L = min(length, max_history):
 *   out = c_h + (c - c_h) * ns / (L + ns),  out_length = L + ns          without:  out = c (its bits),  out_length = ns
 * A pixel with ns == 0 or a colour or depth that is not finite passes through with length 0.  Equal cameras reproject every pixel
 * onto itself, exactly.  The caller keeps out_rgb, out_length and the current frame's depth (and ids) as the next history.
 * Limits: no neighbourhood colour clamp, no per-pixel variance, no moving objects (the ids catch an edited node only if its id
 * changes: reset the history after any edit that is not a camera move), a pinhole lens (the lens draw of dof > 0.1 is ignored).
 * qa_reproject_motion_device and qa_progressive_reproject_motion_device (below) lift the first and the third of these.
 *   qa_reproject_device               plain device buffers: the current frame (d_ids may be NULL), the history (d_hist_ids NULL if
 *                                     and only if d_ids is) -> d_out_rgb (3 floats per pixel), d_out_length (1).  d_out_rgb ==
 *                                     d_rgb is allowed (a pixel reads only its own current pixel); no other overlap of an output
 *                                     with an input or the other output is, and none with a history plane.  One kernel; only enqueues on
 *                                     hip_stream (NULL = the context's stream, as for qa_render_region_device).  No scene is needed.
 *   qa_progressive_reproject_device   the current frame is the progressive frame's preview straight from its slabs - the floats
 *                                     qa_progressive_read returns - with the frame's region and the resident scene's camera; with
 *                                     d_hist_ids the current ids are computed by qa_progressive_gbuffer_device on hip_stream into a
 *                                     plane of the context (8 bytes per pixel of the largest frame so far; the call that grows it
 *                                     waits for the device).  Waits for the frame's last pass as qa_progressive_denoise_device
 *                                     does.  QA_EINVAL on a stale frame (its pixels are not the resident camera's).  The frame is
 *                                     not changed.
 * qa_reproject_params_default: depth_tolerance 0.05, max_history 64, flags 0.  QA_EINVAL: a null camera, params or plane, width or
 * height < 1, a negative origin or a side beyond 2^24, one ids plane without the other, a depth_tolerance that is not finite or is
 * negative, a max_history that is not finite and positive, flags other than 0, an aliased output as above. */
typedef struct qa_reproject_params { float depth_tolerance, max_history; uint32_t flags; } qa_reproject_params;
int qa_reproject_params_default(qa_reproject_params *params);
int qa_reproject_device(qa_ctx *ctx, const qa_camera *prev_cam, const qa_camera *cur_cam, int x0, int y0, int width, int height,
                        const float *d_rgb, const float *d_depth, const uint32_t *d_nsamples, const int32_t *d_ids,
                        const float *d_hist_rgb, const float *d_hist_depth, const float *d_hist_length, const int32_t *d_hist_ids,
                        const qa_reproject_params *params, float *d_out_rgb, float *d_out_length, void *hip_stream);
int qa_progressive_reproject_device(qa_ctx *ctx, const qa_camera *prev_cam, const float *d_hist_rgb, const float *d_hist_depth,
                                    const float *d_hist_length, const int32_t *d_hist_ids, const qa_reproject_params *params,
                                    float *d_out_rgb, float *d_out_length, void *hip_stream);

/* Reprojection that follows moved nodes and clamps stale history: the calls above with two additions, each behind a flag of
 * qa_reproject_motion_params; with flags 0 they return the bits of the calls above.  The header comment of
 * qaray_amd/csrc/hip/qa_reproject_motion_dev.h is the specification.
 *   QA_REPROJECT_MOTION   d_motion: a table of motion_count records qa_node_motion, one per node of the scene (word 0 of an id is
 *                         the node's index).  m is a 3x3 matrix (row-major, m[0 .. 8]) and a translation (m[9 .. 11]) taking a world
 *                         point of the current scene to where the same point of the node lay in the scene the history was rendered
 *                         from; moved == 0: the node and its ancestors stand where they stood (m is not read).  A hit pixel of a
 *                         moved node is taken through m before it is projected into the old camera, also when the cameras are
 *                         equal; the ids test then finds the object where it was, and what it uncovered gets no history.  An id
 *                         outside [0, motion_count) is an unmoved node.  Both ids planes are required.
 *   QA_REPROJECT_CLAMP    a pixel's history colour is clamped, per component, to mean +- clamp_gamma * standard deviation of the
 *                         CURRENT frame's pixels within clamp_radius (1 .. 3) of it that are not void and have its class; a window
 *                         of one such pixel clamps nothing.  History that a light, material or texture edit, a slid shadow or
 *                         reflection has made wrong leaves within a few frames, not at 1 / max_history.  The length is not changed.
 *                         The window reads the neighbours' current colours: d_out_rgb == d_rgb is refused with this flag.
 * qa_reproject_node_motion builds the table on the host (no GPU, no context) from the instance tables of the previous and the
 * current scene (`count` records each, as qa_scene_download's blob holds them or as the caller edited them): record k is
 * Wprev(k) o Wcur(k)^-1 with W(k)(p) = W(parent(k))(tm_k p + pos_k), the inverse through the itm chain, composed in double and
 * rounded once; moved = 0 and the exact identity where tm, itm and pos of k and of all its ancestors compare equal.  QA_EINVAL: a
 * null table, count < 1, tables whose parent, subtree_end or depth differ, a parent that is not -1 .. k - 1.
 *   qa_reproject_motion_device               as qa_reproject_device; d_motion is a device pointer the caller uploaded (NULL is
 *                                            allowed when QA_REPROJECT_MOTION is clear).  One kernel; only enqueues.
 *   qa_progressive_reproject_motion_device   as qa_progressive_reproject_device (the stale-frame refusal and the context's ids
 *                                            plane included); QA_REPROJECT_MOTION requires d_hist_ids.
 * qa_reproject_motion_params_default: depth_tolerance 0.05, max_history 64, clamp_radius 1, clamp_gamma 1, flags 0 (DESIGN.md 4j has
 * the measurements behind the two clamp values).  QA_EINVAL: everything the calls above refuse; unknown flag bits;
 * QA_REPROJECT_MOTION with a null table, motion_count < 1 or without both ids planes; QA_REPROJECT_CLAMP with a clamp_radius outside
 * 1 .. 3, a clamp_gamma that is not finite or is negative, or d_out_rgb == d_rgb; an output overlapping the motion table. */
#define QA_REPROJECT_MOTION 1u
#define QA_REPROJECT_CLAMP  2u
typedef struct qa_reproject_motion_params {
  float    depth_tolerance, max_history, clamp_gamma;
  int32_t  clamp_radius;
  uint32_t flags;
} qa_reproject_motion_params;
typedef struct qa_node_motion {
  float    m[12];
  uint32_t moved;
  uint32_t pad[3];
} qa_node_motion;
int qa_reproject_motion_params_default(qa_reproject_motion_params *params);
int qa_reproject_node_motion(const qa_instance *prev, const qa_instance *cur, int count, qa_node_motion *out);
int qa_reproject_motion_device(qa_ctx *ctx, const qa_camera *prev_cam, const qa_camera *cur_cam, int x0, int y0, int width, int height,
                               const float *d_rgb, const float *d_depth, const uint32_t *d_nsamples, const int32_t *d_ids,
                               const float *d_hist_rgb, const float *d_hist_depth, const float *d_hist_length, const int32_t *d_hist_ids,
                               const qa_node_motion *d_motion, int motion_count, const qa_reproject_motion_params *params,
                               float *d_out_rgb, float *d_out_length, void *hip_stream);
int qa_progressive_reproject_motion_device(qa_ctx *ctx, const qa_camera *prev_cam, const float *d_hist_rgb, const float *d_hist_depth,
                                           const float *d_hist_length, const int32_t *d_hist_ids, const qa_node_motion *d_motion,
                                           int motion_count, const qa_reproject_motion_params *params, float *d_out_rgb,
                                           float *d_out_length, void *hip_stream);

/* Reprojection that carries luminance moments and shortens clamped history: the motion calls above with two more flags of
 * qa_reproject_moments_params; with neither they return the bits of the motion calls.  The header comment of
 * qaray_amd/csrc/hip/qa_reproject_moments_dev.h is the specification.
 *   QA_REPROJECT_MOMENTS  d_hist_moments (2 floats per pixel, 8-byte aligned; NULL: nobody has moment history) holds the accumulated
 *                         first and second moment of the luma (0.2126, 0.7152, 0.0722).  They are fetched with the colour taps and
 *                         blended with the frame's luma l and l * l at the colour's rate k = ns / (L + ns) into d_out_moments (the
 *                         next call's d_hist_moments).  d_out_variance (1 float) is max(o2 - o1 * o1, 0) * k, the variance of the
 *                         accumulated colour's luma, for a pixel that has moment history and out_length >= min_frames * ns; else
 *                         -1, "none", as it is on the first frame, after a disocclusion and on a void pixel.  It is a plane for
 *                         qa_denoise_variance_device.  Exact for frames of equal weight; once max_history caps the length it
 *                         overstates by up to 2x; it does not see the clamp (the moments are not clamped); the threshold counts
 *                         samples, not frames.  With the flag clear the two outputs are not written and may be NULL.
 *   QA_REPROJECT_SHORTEN  only with QA_REPROJECT_CLAMP.  Where the clamp moved the history colour by d (largest component) against a
 *                         box of half-width s = clamp_gamma * sigma (largest component), the history's length enters the
 *                         accumulation as L / (1 + shorten_rate * d / (s + 1e-4)): wrong history stops weighing on the frames
 *                         that follow.  A history inside the box keeps its length, bit for bit.
 * qa_reproject_moments_params_default: the motion call's defaults, min_frames 4, shorten_rate 4, flags 0 (DESIGN.md 4k has the
 * sweep behind shorten_rate).  QA_EINVAL: everything the motion calls refuse; unknown flag bits; QA_REPROJECT_SHORTEN without
 * QA_REPROJECT_CLAMP or with a shorten_rate that is not finite or is negative; QA_REPROJECT_MOMENTS with a min_frames that is not
 * finite or is below 1, without both output planes, with d_out_moments == d_hist_moments, with a moments plane that is not 8-byte
 * aligned, or with one of the two outputs overlapping any other plane of the call.  Not in the CLI, distributed.py or bench.py. */
#define QA_REPROJECT_MOMENTS 4u
#define QA_REPROJECT_SHORTEN 8u
typedef struct qa_reproject_moments_params {
  float    depth_tolerance, max_history, clamp_gamma, min_frames, shorten_rate;
  int32_t  clamp_radius;
  uint32_t flags;
} qa_reproject_moments_params;
int qa_reproject_moments_params_default(qa_reproject_moments_params *params);
int qa_reproject_moments_device(qa_ctx *ctx, const qa_camera *prev_cam, const qa_camera *cur_cam, int x0, int y0, int width, int height,
                                const float *d_rgb, const float *d_depth, const uint32_t *d_nsamples, const int32_t *d_ids,
                                const float *d_hist_rgb, const float *d_hist_depth, const float *d_hist_length, const int32_t *d_hist_ids,
                                const float *d_hist_moments, const qa_node_motion *d_motion, int motion_count,
                                const qa_reproject_moments_params *params, float *d_out_rgb, float *d_out_length, float *d_out_moments,
                                float *d_out_variance, void *hip_stream);
int qa_progressive_reproject_moments_device(qa_ctx *ctx, const qa_camera *prev_cam, const float *d_hist_rgb, const float *d_hist_depth,
                                            const float *d_hist_length, const int32_t *d_hist_ids, const float *d_hist_moments,
                                            const qa_node_motion *d_motion, int motion_count, const qa_reproject_moments_params *params,
                                            float *d_out_rgb, float *d_out_length, float *d_out_moments, float *d_out_variance,
                                            void *hip_stream);

/* Counters accumulated since the last reset (synchronises the context first). */
int qa_get_counters(qa_ctx *ctx, qa_counters *out);
int qa_reset_counters(qa_ctx *ctx);
/* Sum of the integrator kernel's durations (HIP events recorded around each launch, on the
 * stream it was launched on) and the number of launches since the last reset; synchronises. */
int qa_get_kernel_time(qa_ctx *ctx, double *total_ms, uint64_t *launches);
int qa_reset_kernel_time(qa_ctx *ctx);

/* Which integrator the uploaded scene runs on, e.g. "qa_integrate<RES=1,LIGHTS=0,TEX=0,AREA=0>" (one persistent
 * megakernel, LDS-resident scene), "qa_integrate_cs<LIGHTS=1,TEX=1>" (megakernel with cooperative mesh walks) or
 * "staged: wf_logic + wf_cull + wf_trace + wf_redo (n tile groups)".  Before the first frame after an upload (or after
 * qa_set_pipeline / qa_set_option) this is the plan; afterwards it names what the LAST qa_render_* call launched,
 * including "+ photon-map gathers" / "counting variant" for those frames.  Valid until the next call on the context. */
const char *qa_get_kernel_name(qa_ctx *ctx);
/* Diagnostics of the staged integrator since the last qa_reset_counters (synchronises):
 * [0] passes, [1] closest-hit rays, [2] shadow rays, [3] BVH jobs queued, [4] rays repeated exactly,
 * [5] jobs finished, [6] node steps, [7] leaf steps, [8] triangle tests, [9] hits that failed the order check,
 * [10] jobs suspended by the step budget, [11] lane slots used in traversal rounds, [12] traversal rounds (waves).
 * Lane utilisation of the traversal = [11] / (64 * [12]); geometry bytes = [6] * 64 + [8] * 48. */
#define QA_STAGED_STATS 13
int qa_get_staged_stats(qa_ctx *ctx, uint64_t out[QA_STAGED_STATS]);

/* Scenes whose geometry does not fit LDS can run on two integrators that return the same bits: the persistent
 * megakernel (for scenes without area lights with cooperative mesh walks: the whole wave walks its mesh queries from a pool
 * of (ray, node) items in LDS, qa_kernel_cs.h) and the staged pipeline (logic / cull / trace / redo stages exchanging rays
 * through queues in HBM, qa_wf.h).  QA_PIPE_AUTO (the default) and QA_PIPE_MEGA run the megakernel - the faster integrator
 * on every scene measured; QA_PIPE_STAGED runs the staged pipeline, which is kept as an independent bitwise cross-check.
 * Scenes the staged pipeline cannot take (LDS-resident scenes, area lights, photon maps, QA_RENDER_STATS frames, > 4
 * non-ambient lights, > 31 nodes) always run on the megakernel, whatever the mode. */
#define QA_PIPE_MEGA 0
#define QA_PIPE_STAGED 1
#define QA_PIPE_AUTO 2
int qa_set_pipeline(qa_ctx *ctx, int mode);

/* Options an embedding application or a test may set (the product library reads no environment variable of its own;
 * the developer knobs of the A/B scripts exist only in builds made with -DQA_DEV_KNOBS):
 *   "coop"           1 (default) / 0: cooperative mesh walks where the scene allows them; 0 = every lane walks its own ray
 *   "cs_cull"        1 (default) / 0: the cooperative kernel skips scene-graph nodes whose bounds a wave's rays all miss; 0 = every
 *                    node is visited as the reference does (same bits either way: A/B tests)
 *   "cs_force_exact" tests: bit 0 / bit 1 send every closest-hit / shadow query of the cooperative kernel to its exact sequential
 *                    walks (the path a tie, a failed order check or a full pool takes); same bits, much slower
 *   "walk_zero_terms" tests: 1 = the shadow ray of a light whose term is zero in every component whatever the ray finds (the surface
 *                    faces away from the light) is walked all the same, as the reference does; 0 (default) = counted, not walked
 *                    (same bits, same counters)
 *   "last_cast"      -1 (default) / 1: LDS-resident scenes without lights, reflective or refractive lobes and absorption whose only
 *                    emitters are planes and spheres - a path's last ray asks which emitter it meets (an any-hit sweep in place of the
 *                    closest-hit search, no hit details, no shading); 0: the same kernel runs the closest-hit sweep (same bits, same
 *                    counters; tests and A/B runs)
 *   "leaf_sweep"     -1 (default) / 1: where "last_cast" applies, the any-hit query of a mesh with a leaf table (an own tree of 2 - 64
 *                    leaves) tests every leaf box once, all lanes at the same leaf, and then each lane the triangles of its own
 *                    candidates, instead of walking the tree; 0: it walks the tree (same bits, same counters; tests and A/B runs)
 *   "cs_pool_limit"  n > 0: upper bound for the pool of the cooperative walks (tests: forces the overflow path); 0 = none
 *   "sync_samples"   -1 (default: per scene) / 0 / 1: a wave starts the next samples of its 64 pixels together; n >= 2 (cooperative
 *                    kernel; elsewhere like 1): finished paths wait until n of the wave's have gathered.  Taken without effect where
 *                    "last_cast" applies: that kernel runs one whole sample of every lane per turn of its loop
 *   "chunk_spp"      -1 (default: per frame) / 0 / n: the per-lane kernels hand a tile's samples out in chunks - n samples first, then
 *   "chunk_tail"     chunks of this many (0: an eighth of the frame's spp) - so that a frame of few tiles per wave ends on small work
 *                    items; a pixel's state waits in device memory between chunks (same samples in the same order: same bits)
 *   "tile_lists"     -1 (default: on, limit 8) / 0 / n: LDS-resident scenes without depth of field - a wave lists, once per tile,
 *                    the leaves of every mesh's own tree its camera rays can enter, and those rays test the listed triangles
 *                    instead of walking the tree; a mesh whose list for a tile is longer than n leaves is walked (same bits)
 *   "empty_tiles"    -1 (default) / 1: where "last_cast" and "tile_lists" apply, a one-shot frame finishes the 8x8 tiles whose camera
 *                    rays can hit nothing - every node's bounds lie outside the tile's pyramid - in closed form: rgb = background,
 *                    depth = QA_BIGFLOAT, nsamples = spp_min; their samples and casts are counted as the frame holds them, derived
 *                    and not traced.  0: every tile is traced (same bits, same counters; tests and A/B runs)
 *   "tile_order"     1 (default) / 0: tiles handed out centre-first
 *   "progressive_tile_limit"  tests: n > 0 = a progressive pass takes at most n tiles, then ends as if stopped; 0 (default) = none
 *   "staged_groups"  1 (default) .. 8 tile groups of the staged pipeline, each on its own stream; more than one only pays
 *                    when the process started the HIP runtime with GPU_MAX_HW_QUEUES >= 8
 *   "verbose"        1: tree statistics and launch shapes on stderr at upload
 * Unknown names return QA_EINVAL. */
int qa_set_option(qa_ctx *ctx, const char *name, long long value);

/* Test support: fills the private (scratch) segment of every wave slot of the device with `pattern`, on every stream this context
 * launches on, and waits.  A frame rendered afterwards must not depend on the pattern: one that does reads scratch memory it never
 * wrote (the compiler hazard of DESIGN.md 5b; tests/test_gpu_parity.py renders with several patterns).  No reference counterpart. */
int qa_debug_scrub_scratch(qa_ctx *ctx, uint32_t pattern);

/* Launch geometry (0 = library default). blocks_per_cu * CUs persistent workgroups of `threads`. */
int qa_set_launch_config(qa_ctx *ctx, int blocks_per_cu, int threads_per_block);

const char *qa_last_error(void);

/* Self-test hooks for the device math library (qaray_amd/csrc/hip/qa_device_math.h): the device
 * sinf/cosf evaluated on the GPU, and the same source compiled for the host (fn: 0 sinf, 1 cosf,
 * 2 powf(x,y), 3 expf). */
int qa_test_sincosf_device(const float *x, int n, float *s, float *c);
int qa_test_math_device(int fn, const float *x, const float *y, int n, float *out);
int qa_test_math_host(int fn, const float *x, const float *y, int n, float *out);

/* Self-test hooks for the texture path (qaray_amd/csrc/hip/qa_texture_dev.h): n queries of one op, 16 floats in and 9 out per query.
 * in: [0..2] a, [3..5] b, [6..8] c, [9..11] d, [12..14] e, [15] flag; out: three vectors r0, r1, r2 (zero where an op has fewer).
 *   op 0 tileClamp(a)                          4 mtlSample(hit {uvw a, duvw b, c, hasTexture flag}, colour d, texmap index)
 *   op 1 textureSample(texture index, a)       5 sampleEnvironment(colour b, texmap index, direction a)
 *   op 2 textureSampleFiltered(index, a, b, c) 6 texPlane(o a, dx b, dy c, p d) -> uvw, duvw0, duvw1
 *   op 3 texColorSample(colour b, texmap index, uvw a)   7 texSphere(o a, dx b, dy c, p d, N e) -> uvw, duvw0, duvw1
 *   op 8 texTriangle(element index & 0xFFFFF of mesh index >> 20, o a, dx b, dy c, barycentrics d.x, d.y) -> uvw, duvw0, duvw1
 *   op 9 the float -> int conversion of the texel lookups (x86 semantics) of a.x: the int's bits in r0.x
 * The device hook reads the tables of the scene uploaded into ctx, the host hook builds them from blob on the CPU (no GPU needed;
 * ops 0 and 9 read no table, and blob may be null). */
int qa_test_texture_device(qa_ctx *ctx, int op, int index, int n, const float *in, float *out);
int qa_test_texture_host(const void *blob, int op, int index, int n, const float *in, float *out);

/* Self-test hook for the 8-bit products (qaray_amd/csrc/hip/qa_display_dev.h): the source of qa_display_device's kernels compiled
 * for the host, pixel after pixel over host arrays (no GPU and no context needed). */
int qa_test_display_host(const float *rgb, const float *depth, const uint32_t *nsamples, uint64_t npix, int spp_max, int use_srgb,
                         uint8_t *color, uint8_t *count, uint8_t *zimg, uint8_t *countimg, uint8_t *mask, qa_display_stats *stats);

/* Self-test hooks for the matte planes (qaray_amd/csrc/hip/qa_matte_dev.h): the source of qa_matte_region_device's and
 * qa_matte_rgba_device's kernels compiled for the host (no GPU and no context needed).  accumulate: one pixel's n samples - values
 * [n][3] (what the albedo plane of qa_gbuffer_region would hold for each ray), normals [n][3] (read where hit[s] != 0), hit [n] ->
 * coverage [1], albedo [3], normal [3], backdrop [3]; an output may be NULL.  rgba: npix pixels over host arrays -> rgba [npix][4]. */
int qa_test_matte_accumulate_host(const float *values, const float *normals, const uint8_t *hit, uint32_t n, float *coverage,
                                  float *albedo, float *normal, float *backdrop);
int qa_test_matte_rgba_host(const float *rgb, const float *backdrop, const float *coverage, const uint32_t *nsamples, uint64_t npix,
                            int srgb, uint8_t *rgba);

/* Self-test hooks for the id matte (qaray_amd/csrc/hip/qa_idmatte_dev.h): the source of qa_idmatte_region_device's and
 * qa_idmatte_select_device's kernels compiled for the host (no GPU and no context needed).  accumulate: one pixel's n samples - hit
 * [n] flags and keys [n] (read where hit[s] != 0) -> the ranked table ids [8], counts [8], other [1]; an output may be NULL.
 * select: npix pixels over host arrays and a list of m ids -> out [npix]. */
int qa_test_idmatte_accumulate_host(const uint8_t *hit, const int32_t *keys, uint32_t n, int32_t *ids, uint32_t *counts, uint32_t *other);
int qa_test_idmatte_select_host(const int32_t *ids, const uint32_t *counts, const uint32_t *samples, uint64_t npix, const int32_t *select,
                                uint32_t m, float *out);

/* Self-test hooks for the ambient occlusion (qaray_amd/csrc/hip/qa_ao_dev.h): the source of qa_ao_region_device's and
 * qa_ao_points_device's kernels compiled for the host (no GPU and no context needed).  directions: `count` rays - stream [count],
 * c [count], the unit normals n [count][3] -> d [count][3].  face_normal: N [count][3] and camera-ray directions d [count][3] ->
 * n [count][3].  sphere: the generator's inner step for the same keys -> the sphere points s [count][3] and whether all attempts
 * failed, fallback [count] (either may be NULL).  direction_from: the outer step from sphere points given directly. */
int qa_test_ao_directions_host(uint32_t seed, const uint32_t *stream, const uint32_t *c, const float *n, uint64_t count, float *d);
int qa_test_ao_face_normal_host(const float *N, const float *d, uint64_t count, float *n);
int qa_test_ao_sphere_host(uint32_t seed, const uint32_t *stream, const uint32_t *c, uint64_t count, float *s, uint8_t *fallback);
int qa_test_ao_direction_from_host(const float *n, const float *s, uint64_t count, float *d);

/* Self-test hooks for the bake maps (qaray_amd/csrc/hip/qa_bake_dev.h): the source of qa_bake_texels_device's and
 * qa_bake_dilate_device's kernels compiled for the host (no GPU and no context needed).  texels: the call on a flat scene blob of
 * nbytes in host memory, every refusal but QA_ENOSCENE included; dilate: the fill over host arrays. */
int qa_test_bake_texels_host(const void *blob, uint64_t nbytes, int node, int texmap, int mtl, uint32_t width, uint32_t height, float *point,
                             float *normal, int32_t *face, float *bary);
int qa_test_bake_dilate_host(const uint8_t *rgb8, const int32_t *face, uint32_t width, uint32_t height, uint32_t radius, uint8_t *out);

/* Self-test hook for the texel conversion (qaray_amd/csrc/hip/qa_texel_dev.h): the source of qa_scene_edit_texels' kernel and of an
 * upload's texel table compiled for the host: h rows of w RGB8 texels, `stride` bytes apart -> w * h entries {r, g, b, 0} / 255.0f
 * of 4 floats (no GPU and no context needed). */
int qa_test_texels_host(const uint8_t *rgb8, int w, int h, uint64_t stride, float *out4);

/* Self-test hook for the filter (qaray_amd/csrc/hip/qa_denoise_dev.h): the source of qa_denoise_device's kernels compiled for the
 * host, pixel after pixel over host arrays (no GPU and no context needed); out_rgb == rgb is allowed. */
int qa_test_denoise_host(const float *rgb, const float *depth, const uint32_t *nsamples, int width, int height,
                         const qa_denoise_params *params, float *out_rgb);
int qa_test_denoise_guided_host(const float *rgb, const float *depth, const uint32_t *nsamples, const float *normal, const float *albedo,
                                int width, int height, const qa_denoise_guided_params *params, float *out_rgb);

int qa_test_denoise_variance_host(const float *rgb, const float *depth, const uint32_t *nsamples, const float *normal, const float *albedo,
                                  const float *variance, int width, int height, const qa_denoise_variance_params *params, float *out_rgb);

/* Self-test hook for the reprojection (qaray_amd/csrc/hip/qa_reproject_dev.h): the source of qa_reproject_device's kernel compiled
 * for the host, pixel after pixel over host arrays, arguments in the same order (no GPU and no context needed). */
int qa_test_reproject_host(const qa_camera *prev_cam, const qa_camera *cur_cam, int x0, int y0, int width, int height, const float *rgb,
                           const float *depth, const uint32_t *nsamples, const int32_t *ids, const float *hist_rgb, const float *hist_depth,
                           const float *hist_length, const int32_t *hist_ids, const qa_reproject_params *params, float *out_rgb,
                           float *out_length);
/* The same for qa_reproject_motion_device (qaray_amd/csrc/hip/qa_reproject_motion_dev.h), the motion table in host memory. */
int qa_test_reproject_motion_host(const qa_camera *prev_cam, const qa_camera *cur_cam, int x0, int y0, int width, int height, const float *rgb,
                                  const float *depth, const uint32_t *nsamples, const int32_t *ids, const float *hist_rgb,
                                  const float *hist_depth, const float *hist_length, const int32_t *hist_ids, const qa_node_motion *motion,
                                  int motion_count, const qa_reproject_motion_params *params, float *out_rgb, float *out_length);
/* The same for qa_reproject_moments_device (qaray_amd/csrc/hip/qa_reproject_moments_dev.h). */
int qa_test_reproject_moments_host(const qa_camera *prev_cam, const qa_camera *cur_cam, int x0, int y0, int width, int height, const float *rgb,
                                   const float *depth, const uint32_t *nsamples, const int32_t *ids, const float *hist_rgb, const float *hist_depth,
                                   const float *hist_length, const int32_t *hist_ids, const float *hist_moments, const qa_node_motion *motion,
                                   int motion_count, const qa_reproject_moments_params *params, float *out_rgb, float *out_length,
                                   float *out_moments, float *out_variance);

/* Radiance queries: n rays of the caller's path-traced on the resident scene by the integrator of qa_render_region, started from
 * the rays instead of the camera (qa_integrate_rays: qa_kernel_body.h sections A and B under RAYS; the opening comment of
 * qaray_amd/csrc/hip/qa_radiance.hip is the specification).  Ray arrays as for the ray queries above: [records][3] floats, world
 * space, contiguous; the direction is used as given and NOT normalised (shading assumes unit length, as for a camera ray).
 *   qa_radiance_params          spp >= 1 samples per ray (fixed: no adaptive stop), max_bounce >= 0 as qa_render_region's, seed, flags:
 *     QA_RADIANCE_PER_SAMPLE      every ray array holds n * spp records, sample s of ray q starts from record q * spp + s; without it
 *                                 n records, every sample of ray q starts from record q
 *     QA_RADIANCE_MISS_ENVIRONMENT a first ray that misses takes the environment by direction, as a bounce ray does; without it
 *                                 the background, as a frame's camera ray does
 *     QA_RADIANCE_PHOTON_MAPS     (bit 3; qa_irradiance_points* take it too) the batch runs with Scene::usePhotonMap = true, exactly
 *                                 as a frame does once qa_photon_maps_build has run: diffuse hits gather from the caustics map, and
 *                                 from the photon map behind a diffuse bounce (qa_integrate_rays_pm / qa_integrate_points_pm).  The
 *                                 gathers draw no random number.  Opt-in: a frame changes silently when maps are built, a batch says
 *                                 what it wants - without the flag a context whose maps are built refuses the batch
 *                                 (QA_EUNSUPPORTED), with it a context without maps does (QA_ENOSCENE, "no photon maps built")
 *   qa_radiance_params_default  spp 1, max_bounce 5, seed 0x51A7A7, flags 0.  Needs no context.
 *   qa_radiance_rays_device     d_dx, d_dy: the ray's differential directions for the texture filter, both or neither (NULL: a ray
 *                               of no width, the first hit's textures are looked up unfiltered); d_screen: [records][2] the position
 *                               in pixels at which a missed first ray looks a background texmap up (NULL: required only when the
 *                               background has a texmap and QA_RADIANCE_MISS_ENVIRONMENT is not set); d_stream: [n] uint32, ray q
 *                               draws from the random-number stream of pixel index d_stream[q] (NULL: q).  Outputs by ray: d_rgb
 *                               [n][3] the mean of the spp samples; d_t [n] (may be NULL) the parameter of sample 0's first hit,
 *                               QA_RAY_MISS on a miss; d_nsamples [n] uint32 (may be NULL): zeroed first, spp for a finished ray,
 *                               0 for one that qa_request_stop left unfinished.  A void ray (a component that is not finite, or
 *                               direction (0, 0, 0)) is not walked and draws no random number: its sample is black, and counts.
 *                               Only enqueues on hip_stream (NULL = the context's stream).
 *   qa_radiance_rays            the same from and to host memory through a staging buffer of the call's own that only grows (24 bytes
 *                               per ray and 56 per record of the largest batch so far, freed with the context); synchronises.
 *   qa_camera_sample_rays_device  samples [first, first + count) of the camera rays of every pixel of [x0,x1) x [y0,y1) exactly as
 *                               qa_render_region builds them (qa_kernel_body.h section B): record (pixel, k) at pixel * count + k,
 *                               pixels region-local and row-major; d_stream [pixels] = y * width + x.  Each output may be NULL, not
 *                               all.  Handed to qa_radiance_rays_device with QA_RADIANCE_PER_SAMPLE (first 0, count spp) they give
 *                               qa_render_region's rgb, depth and nsamples bit for bit.  Sample 0's origins and directions are
 *                               qa_camera_rays_device's.  QA_EUNSUPPORTED for a camera with dof > 0.1: its lens draws come from
 *                               the pixel's stream in the middle of a path sequence, and no ray array can carry them.
 * Ordered as a frame: behind the context's last frame and last edit, one at a time per context; qa_get_counters and
 * qa_get_kernel_time move as for a frame of n * spp samples; qa_get_kernel_name, progressive frames and frames rendered before and
 * after are untouched.  Codes: QA_ENOSCENE without a scene; n == 0 is QA_OK and launches nothing; QA_EINVAL for n > 2^31 - 1 (and
 * for (n + 63) / 64 * 64 >= 0xF0000000: the work counter is 32 bits), a NULL ray array, rgb or params, spp < 1, max_bounce < 0,
 * unknown flag bits, one of d_dx / d_dy without the other, a textured background without d_screen and without
 * QA_RADIANCE_MISS_ENVIRONMENT; QA_EUNSUPPORTED for area lights with max_bounce > 7 (as qa_render_region) and while photon maps
 * are built unless QA_RADIANCE_PHOTON_MAPS is set; QA_ENOSCENE for QA_RADIANCE_PHOTON_MAPS without maps.  A refused call writes
 * nothing.  Every mesh is walked per lane, rays are taken in the caller's order. */
#define QA_RADIANCE_PER_SAMPLE       1u
#define QA_RADIANCE_MISS_ENVIRONMENT 2u
#define QA_RADIANCE_PHOTON_MAPS      8u
typedef struct qa_radiance_params { int spp, max_bounce; uint32_t seed, flags; } qa_radiance_params;
int qa_radiance_params_default(qa_radiance_params *params);
int qa_radiance_rays_device(qa_ctx *ctx, uint64_t n, const float *d_origins, const float *d_dirs, const float *d_dx, const float *d_dy,
                            const float *d_screen, const uint32_t *d_stream, const qa_radiance_params *params, float *d_rgb, float *d_t,
                            uint32_t *d_nsamples, void *hip_stream);
int qa_radiance_rays(qa_ctx *ctx, uint64_t n, const float *origins, const float *dirs, const float *dx, const float *dy,
                     const float *screen, const uint32_t *stream, const qa_radiance_params *params, float *rgb, float *t,
                     uint32_t *nsamples);
int qa_camera_sample_rays_device(qa_ctx *ctx, int x0, int y0, int x1, int y1, int first, int count, float *d_origins, float *d_dirs,
                                 float *d_dx, float *d_dy, float *d_screen, uint32_t *d_stream, void *hip_stream);

/* Irradiance queries: the light arriving at n surface points of the caller's, path-traced on the resident scene by the integrator
 * of qa_render_region started from the points (qa_integrate_points: qa_kernel_body.h under POINTS; the opening comment of
 * qaray_amd/csrc/hip/qa_irradiance.hip is the specification).  d_points, d_normals: [n][3] floats, world space, contiguous; the
 * normal is used as given and NOT normalised.  Point q is shaded spp times as a hit there on a white diffuse material would be:
 * the direct light at the point, one cosine-weighted bounce, the integrator as it stands behind it; a bounce that misses takes the
 * environment.  kd * rgb is what a frame shows for a diffuse surface of colour kd at the point: the values are not scaled by pi,
 * and every light weighs 1 / num_lights.  params: a qa_radiance_params whose flags are 0 or QA_RADIANCE_PHOTON_MAPS (the point then
 * gathers from the caustics map ahead of its direct light, and the paths behind its bounce gather as a frame's do: the opening
 * comment of qaray_amd/csrc/hip/qa_irradiance_pm.hip); d_stream: [n] uint32, point q draws from
 * the random-number stream of pixel index d_stream[q] (NULL: q).  Outputs by point: d_rgb [n][3] the mean of the spp samples;
 * d_nsamples [n] uint32 (may be NULL): zeroed first, spp for a finished point, 0 for one that qa_request_stop left unfinished.  A
 * void point (a component of the point or the normal that is not finite, or normal (0, 0, 0)) draws no random number: its samples
 * are black, and count.  The device form only enqueues on stream (NULL = the context's stream); qa_irradiance_points is the same
 * from and to host memory through the queries' staging buffer (44 bytes per point), and synchronises.
 * Ordered as a frame, as qa_radiance_rays_device: behind the context's last frame and last edit; qa_get_counters and
 * qa_get_kernel_time move as for n * spp samples whose first segment casts nothing; frames before and after are untouched.
 * Codes: QA_ENOSCENE without a scene; n == 0 is QA_OK and launches nothing; QA_EINVAL for n > 2^31 - 1 (and for
 * (n + 63) / 64 * 64 >= 0xF0000000), a NULL point or normal array, rgb or params, spp < 1, max_bounce < 0, any other flag bit;
 * QA_EUNSUPPORTED for area lights with max_bounce > 7 and while photon maps are built unless QA_RADIANCE_PHOTON_MAPS is set;
 * QA_ENOSCENE for QA_RADIANCE_PHOTON_MAPS without maps.  A refused call writes nothing. */
int qa_irradiance_points_device(qa_ctx *ctx, uint64_t n, const float *d_points, const float *d_normals, const uint32_t *d_stream,
                                const qa_radiance_params *params, float *d_rgb, uint32_t *d_nsamples, void *stream);
int qa_irradiance_points(qa_ctx *ctx, uint64_t n, const float *points, const float *normals, const uint32_t *stream_ids,
                         const qa_radiance_params *params, float *rgb, uint32_t *nsamples);

/* Light probes: the light arriving at n points in free space - where a moving object, a character or a particle will be - as the
 * nine coefficients per colour of the real spherical harmonics of order 2, and their evaluation at shading points (the opening
 * comment of qaray_amd/csrc/hip/qa_lightprobe_dev.h is the specification of every number below).  A probe holds what a camera at
 * its point would see in every direction: emitters, the environment, and the surfaces around it under their own direct and bounced
 * light.  It does NOT hold the direct term of point, spot and directional lights at the point itself - no ray can meet them; a shader
 * adds them analytically, as it does for any dynamic object.
 *   qa_probe_params             m: the probe is a cube map of m x m texels per face, 1 <= m <= 128, K = 6 m^2 directions through the
 *                               texel centres, each weighted by its texel's solid angle; spp, max_bounce, seed as qa_radiance_params';
 *                               flags: QA_PROBE_JITTER (the directions are jittered inside their texels by counter-based words of
 *                               (seed, the probe's stream id, k)) and QA_RADIANCE_PHOTON_MAPS (passed through to the rays), every
 *                               other bit is refused; chunk_rays: the probes are traced max(1, chunk_rays / K) at a time (0: 2^20
 *                               rays), which bounds the scratch and changes no result.
 *   qa_probe_params_default     m 16, spp 1, max_bounce 5, seed 0x51A7A7, flags 0, chunk_rays 0.  Needs no context.
 *   qa_probe_sh_device          d_points [n][3] floats, world space; d_stream [n] uint32 the probe's stream id S (NULL: its index).
 *                               Ray (q, k) is a ray of qa_radiance_rays_device from point q along direction k with
 *                               QA_RADIANCE_MISS_ENVIRONMENT, spp samples and the random-number stream of pixel index
 *                               (S * K + k) mod 2^32.  Outputs by probe: d_sh [n][9][3] the coefficients (order: 1; y, z, x; xy, yz,
 *                               3z^2 - 1, xz, x^2 - y^2), the projection normalised by 4 pi over the summed weights; d_cube
 *                               [n][6][m][m][3] (may be NULL) the rays' rgb, faces +x, -x, +y, -y, +z, -z; d_hits [n] uint32 (may be
 *                               NULL) the rays with t < QA_RAY_MISS; d_tmin [n] (may be NULL) the least t - a probe inside a wall or
 *                               against one shows there.  A probe with a component that is not finite is void: all outputs 0,
 *                               d_tmin QA_RAY_MISS.  A result depends on the point, S, m, flags, seed, spp and max_bounce alone.
 *                               Only enqueues on stream (NULL = the context's stream); the rays of a chunk live in a scratch buffer
 *                               of the context's that only grows (44 bytes per ray of the largest chunk so far).
 *   qa_probe_sh                 the same from and to host memory through the queries' staging buffer (132 bytes per probe, and the
 *                               cube when asked for); synchronises.
 *   qa_probe_shade_device       shading point i takes probe d_index[i] (int32; NULL: i) of d_sh [probes][9][3] and its normal
 *                               d_normals[i] (unit length assumed) -> d_rgb [n][3] = max(0, sum_c A_c sh_c Y_c(N)), A = 1, 2/3, 1/4 by
 *                               band: the units of qa_irradiance_points, not scaled by pi, kd * rgb is a diffuse colour.  An index
 *                               outside [0, probes) is clamped into it (the array is the device's: nothing is refused by content); a
 *                               normal that is not finite shades to 0.  Needs no scene; only enqueues.
 *   qa_probe_grid_shade_device  the same from a regular grid: origin[3], spacing[3] > 0, counts[3] >= 1 in host memory, probe
 *                               (iz * ny + iy) * nx + ix of d_sh at origin + (ix, iy, iz) * spacing; the point's 27 coefficients
 *                               are interpolated trilinearly (x, then y, then z) between the probes of its cell, points outside
 *                               the grid take the nearest cell's edge.  A point or normal that is not finite shades to 0.
 * qa_probe_sh_device is ordered as its chunks are, as qa_radiance_rays_device: behind the context's last frame and last edit, and a
 * later edit waits for it; qa_get_counters moves as for n * K * spp samples, qa_get_kernel_time by one launch per chunk.  The two
 * shading calls read only the caller's arrays and order nothing.
 * Codes: qa_probe_sh*: QA_ENOSCENE without a scene; n == 0 is QA_OK and launches nothing; QA_EINVAL for n > 2^31 - 1, a NULL point
 * array, sh or params, m outside 1 .. 128, an unknown flag bit, and whatever qa_radiance_rays_device refuses of a chunk: more than
 * 2^31 - 1 rays in one chunk (the limit is per chunk, not per batch), spp < 1, max_bounce < 0; QA_EUNSUPPORTED for area lights with
 * max_bounce > 7 and while photon maps are built unless QA_RADIANCE_PHOTON_MAPS is set; QA_ENOSCENE for that flag without maps.
 * The shading calls: QA_EINVAL for n > 2^31 - 1, a NULL array, probes == 0, probes < n without an index, a grid whose origin or
 * spacing is not finite, spacing <= 0, a count < 1 or more than 2^31 - 1 probes.  A refused call writes nothing. */
#define QA_PROBE_JITTER 16u
typedef struct qa_probe_params { int m, spp, max_bounce; uint32_t seed, flags; uint64_t chunk_rays; } qa_probe_params;
int qa_probe_params_default(qa_probe_params *params);
int qa_probe_sh_device(qa_ctx *ctx, uint64_t n, const float *d_points, const uint32_t *d_stream, const qa_probe_params *params,
                       float *d_sh, float *d_cube, uint32_t *d_hits, float *d_tmin, void *stream);
int qa_probe_sh(qa_ctx *ctx, uint64_t n, const float *points, const uint32_t *stream_ids, const qa_probe_params *params, float *sh,
                float *cube, uint32_t *hits, float *tmin);
int qa_probe_shade_device(qa_ctx *ctx, uint64_t n, const float *d_sh, uint64_t probes, const float *d_normals, const int32_t *d_index,
                          float *d_rgb, void *stream);
int qa_probe_grid_shade_device(qa_ctx *ctx, uint64_t n, const float *d_sh, const float *origin, const float *spacing,
                               const int32_t *counts, const float *d_points, const float *d_normals, float *d_rgb, void *stream);
/* Self-test hooks for the light probes (qaray_amd/csrc/hip/qa_lightprobe_dev.h): the source of the kernels above compiled for the
 * host (no GPU and no context needed).  directions: n probes with stream ids stream [n] -> d [n][K][3], w [n][K], ray_stream [n][K]
 * (each may be NULL, not all); flags: 0 or QA_PROBE_JITTER.  project: one probe's K rays - d [K][3], w [K], rgb [K][3], t [K] - reduced
 * as the wave reduces them -> sh [27], hits [1], tmin [1] (the last two may be NULL).  shade, grid_shade: the calls over host arrays. */
int qa_test_probe_directions_host(int m, uint32_t seed, uint32_t flags, const uint32_t *stream, uint64_t n, float *d, float *w,
                                  uint32_t *ray_stream);
int qa_test_probe_project_host(uint64_t K, const float *d, const float *w, const float *rgb, const float *t, float *sh, uint32_t *hits,
                               float *tmin);
int qa_test_probe_shade_host(uint64_t n, const float *sh, uint64_t probes, const float *normals, const int32_t *index, float *rgb);
int qa_test_probe_grid_shade_host(uint64_t n, const float *sh, const float *origin, const float *spacing, const int32_t *counts,
                                  const float *points, const float *normals, float *rgb);

/* Probe visibility: the distances a probe's rays travelled, kept as two moments per direction cell, and a grid shading that weighs
 * each of a cell's eight probes by whether it can see the shading point - so that a wall between them stops the light (the opening
 * comment of qaray_amd/csrc/hip/qa_probevis_dev.h is the specification of every number below).  No ray is traced beyond those of
 * qa_probe_sh_device.
 *   qa_probevis_params            d: the moments are a cube map of d x d cells per face, 1 <= d <= m and m % d == 0, each pooling
 *                                 (m / d)^2 texels; dmax > 0, finite: a ray's t is clamped to it (a miss becomes dmax); normal_bias,
 *                                 finite: the shading point is moved by normal_bias * N before the visibility test.
 *   qa_probevis_params_default    d 8, dmax 0, normal_bias 0.  dmax 0 is refused below: the caller sets it (ProbeGrid of the Python
 *                                 layer takes 1.5 |spacing|).  Needs no context.
 *   qa_probevis_sh_device         qa_probe_sh_device and, from the same rays, d_moments [n][6][d][d][2] (mean of t, mean of t^2 per
 *                                 cell; +0 for a void probe).  d_moments is required, d_sh may be NULL here; d_cube, d_hits, d_tmin
 *                                 as there.  The outputs it shares with qa_probe_sh_device have that call's bits.
 *   qa_probevis_sh                the same from and to host memory.
 *   qa_probevis_grid_shade_device qa_probe_grid_shade_device with d_moments [probes][6][d][d][2] of the grid's probes: the eight
 *                                 probes of the point's cell are weighed by trilinear weight x wrapped cosine x Chebyshev visibility
 *                                 and normalised.  d says the layout of d_moments (1 .. 128); of params only normal_bias is read.
 * qa_probevis_sh_device is ordered, counted and refused exactly as qa_probe_sh_device on the same arguments (one more kernel per
 * chunk pools the chunk's t before the next chunk overwrites it: qa_get_kernel_time counts the chunks as before), and QA_EINVAL
 * also for NULL vis params or d_moments, d < 1, d > m, m % d != 0, dmax <= 0 or not finite, normal_bias not finite.  The shading
 * call reads only the caller's arrays and orders nothing; QA_EINVAL as qa_probe_grid_shade_device and for NULL d_moments or params,
 * d outside 1 .. 128, normal_bias not finite.  A refused call writes nothing. */
typedef struct qa_probevis_params { int d; float dmax, normal_bias; } qa_probevis_params;
int qa_probevis_params_default(qa_probevis_params *params);
int qa_probevis_sh_device(qa_ctx *ctx, uint64_t n, const float *d_points, const uint32_t *d_stream, const qa_probe_params *params,
                          const qa_probevis_params *vis, float *d_sh, float *d_cube, uint32_t *d_hits, float *d_tmin, float *d_moments,
                          void *stream);
int qa_probevis_sh(qa_ctx *ctx, uint64_t n, const float *points, const uint32_t *stream_ids, const qa_probe_params *params,
                   const qa_probevis_params *vis, float *sh, float *cube, uint32_t *hits, float *tmin, float *moments);
int qa_probevis_grid_shade_device(qa_ctx *ctx, uint64_t n, const float *d_sh, const float *d_moments, int d, const float *origin,
                                  const float *spacing, const int32_t *counts, const float *d_points, const float *d_normals,
                                  const qa_probevis_params *params, float *d_rgb, void *stream);
/* Self-test hooks (qaray_amd/csrc/hip/qa_probevis_dev.h compiled for the host; no GPU and no context needed).  moments: one probe's
 * K = 6 m^2 hit parameters t -> out [6][d][d][2].  grid_shade: the call above over host arrays. */
int qa_test_probevis_moments_host(int m, int d, float dmax, const float *t, float *out);
int qa_test_probevis_grid_shade_host(uint64_t n, const float *sh, const float *moments, int d, const float *origin, const float *spacing,
                                     const int32_t *counts, const float *points, const float *normals,
                                     const qa_probevis_params *params, float *rgb);

/* Reflection probes: a probe's cube map (d_cube of qa_probe_sh_device) prefiltered for glossy reflection - convolved with Phong lobes
 * of decreasing sharpness into a chain of ever smaller cube maps - and the lookup of a direction at a level of that chain (the opening
 * comment of qaray_amd/csrc/hip/qa_reflprobe_dev.h is the specification of every number below).  No ray is traced here.
 *   qa_reflprobe_layout            m: the cube's texels per face edge, a power of two in 1 .. 128, lg = log2 m; levels: 1 .. lg + 1.
 *                                  Level l has res[l] = m >> l texels per face edge and starts at texel offset[l] of a probe's chain;
 *                                  level 0 is the cube itself, level l >= 1 the cube convolved with max(0, dot)^(2^squarings[l]),
 *                                  squarings[l] = max(0, 2 (lg - l) - 1) (squarings[0] = 0: nothing is convolved there); *texels = T,
 *                                  the chain's texels.  The three arrays hold `levels` entries; each output may be NULL.  Needs no
 *                                  context.
 *   qa_reflprobe_prefilter_device  d_cube [n][6][m][m][3] -> d_chain [n][T][3]: level 0 copied bit for bit, every texel of the others
 *                                  the lobe-weighted, solid-angle-weighted mean of all 6 m^2 source texels, summed in ascending order.
 *                                  A NaN texel reaches exactly the outputs whose lobe covers it; zeros stay zeros.
 *   qa_reflprobe_shade_device      lookup i takes probe d_index[i] (int32; NULL: i; clamped into [0, probes)) of d_chain
 *                                  [probes][T][3], the direction d_dirs[i] (any length) and the level d_level[i] (a float, clamped to
 *                                  [0, levels - 1]) -> d_rgb [n][3]: bilinear inside the direction's face (coordinates clamp at the
 *                                  face's edge), linear between the two levels.  A direction that is zero or not finite, or a level
 *                                  that is NaN, answers 0.
 *   qa_reflprobe_grid_shade_device the same from a regular grid (as qa_probe_grid_shade_device's: origin, spacing, counts in host
 *                                  memory, d_chain in the grid's order): the lookups in the eight probes of the point's cell blended
 *                                  trilinearly (x, then y, then z); a point on a probe takes that probe's answer.  A point that is not
 *                                  finite answers 0.  No parallax correction, no visibility weighting.
 * The three device calls read and write only arrays of the caller's and order nothing, as qa_probe_shade_device; they need no scene
 * and only enqueue on stream (NULL = the context's stream).  A caller who prefilters a cube that qa_probe_sh_device is still writing
 * puts both on one stream.
 * Codes: n == 0 is QA_OK and launches nothing; QA_EINVAL for a NULL array, an m that is not a power of two in 1 .. 128, levels outside
 * 1 .. lg + 1, n or probes beyond 2^31 - 1, probes == 0, probes < n without an index, or a bad grid (as qa_probe_grid_shade_device).  A
 * refused call writes nothing. */
int qa_reflprobe_layout(int m, int levels, uint32_t *offset, uint32_t *res, uint32_t *squarings, uint64_t *texels);
int qa_reflprobe_prefilter_device(qa_ctx *ctx, uint64_t n, const float *d_cube, int m, int levels, float *d_chain, void *stream);
int qa_reflprobe_shade_device(qa_ctx *ctx, uint64_t n, const float *d_chain, uint64_t probes, int m, int levels, const float *d_dirs,
                              const float *d_level, const int32_t *d_index, float *d_rgb, void *stream);
int qa_reflprobe_grid_shade_device(qa_ctx *ctx, uint64_t n, const float *d_chain, int m, int levels, const float *origin,
                                   const float *spacing, const int32_t *counts, const float *d_points, const float *d_dirs,
                                   const float *d_level, float *d_rgb, void *stream);
/* Self-test hooks (qaray_amd/csrc/hip/qa_reflprobe_dev.h compiled for the host; no GPU and no context needed): the three calls above
 * over host arrays, refusing what they refuse. */
int qa_test_reflprobe_prefilter_host(uint64_t n, const float *cube, int m, int levels, float *chain);
int qa_test_reflprobe_shade_host(uint64_t n, const float *chain, uint64_t probes, int m, int levels, const float *dirs, const float *level,
                                 const int32_t *index, float *rgb);
int qa_test_reflprobe_grid_shade_host(uint64_t n, const float *chain, int m, int levels, const float *origin, const float *spacing,
                                      const int32_t *counts, const float *points, const float *dirs, const float *level, float *rgb);

#ifdef __cplusplus
}
#endif
#endif /* QARAY_HIP_H */
