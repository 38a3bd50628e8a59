"""Cross-stream ordering of a context's shared buffers: one case per dependency of DESIGN.md "Streams: who waits for whom".

Every case makes one stream late (stream_order_util.hold) and checks that the call on the other stream really waited for it - by the
order of two events, and by the bits of both results against the same two calls run serially on one stream - and that the case was
not vacuous: the two streams run side by side (the module's control), and the hold still ran when the consumer was submitted.

Frames are 64x48 at 4 spp (48 tiles), queries 256 rays.  Producer and consumer take different seeds or inputs, so that a swapped or
shared buffer shows.  Outputs are filled with a pattern on the call's own stream first, and the serial run's tensors are kept until
the comparison, so that memory the allocator hands out again cannot hold the right answer by accident.

qaray_amd.hip does not hand out the context's own stream.  Where a case needs it late (an edit's copies behind a hold, a frame on
another stream right after), a texel edit from device memory is what holds it: the context's stream waits for the caller's there."""
import functools

import numpy as np
import pytest

import stream_order_util as U

pytestmark = pytest.mark.gpu

W, H, SPP = 64, 48, 4
REGION = (0, 0, W, H)
SMALL = (0, 0, 40, 24)
RAYS, RAYS2 = (0, 0, 16, 16), (24, 16, 40, 32)   # 256 camera rays each
BOX12, BOX3, OBJECT7, TEXTURES = "example_project12_box.xml", "example_project3_box.xml", "example_project7_object.xml", "custom_textures.xml"

RUN = {}   # case name -> its function (a, b): the names and their order are stream_order_util.CASES'


def case(fn):
    RUN[fn.__name__] = fn
    return fn


# ---- plumbing

@functools.lru_cache(maxsize=None)
def _blob(scene):
    from conftest import ensure_assets
    from qaray_amd.host import load_scene_blob
    ensure_assets()
    return load_scene_blob(scene, size=(W, H))


def blob_of(scene):
    return _blob(scene).copy()


def new_ctx(scene, options=(), **more):
    """A fresh context with `scene` uploaded -> the state ordered() hands to a case's calls"""
    from qaray_amd import hip
    c = hip.Context(0)
    for name, value in options:
        c.set_option(name, value)
    blob = blob_of(scene)
    c.upload_scene(blob)
    st = {"ctx": c, "blob": blob, "close": c.close}
    st.update(more)
    return st


def filled(s, shape, dtype):
    """An output tensor, filled with a pattern on stream s (the call that writes it follows on s)"""
    import torch
    with torch.cuda.stream(s):
        return torch.full(shape, 0x5A if dtype == torch.uint8 else -7777, dtype=dtype, device=torch.device("cuda", 0))


def frame(c, s, region=REGION, spp=SPP, seed=1, stats=False):
    import torch
    h, w = region[3] - region[1], region[2] - region[0]
    out = {"rgb": filled(s, (h, w, 3), torch.float32), "depth": filled(s, (h, w), torch.float32), "ns": filled(s, (h, w), torch.int32)}
    c.render_region_device(region, spp, out["rgb"], out["depth"], out["ns"], seed=seed, stats=stats, stream=s.cuda_stream)
    return out


def frame_of(seed=1, region=REGION, spp=SPP, stats=False):
    return lambda st, s: frame(st["ctx"], s, region, spp, seed, stats)


def gbuffer(c, s, region=REGION, seed=3):
    import torch
    h, w = region[3] - region[1], region[2] - region[0]
    return c.gbuffer_device(region, seed=seed, normal=filled(s, (h, w, 3), torch.float32), albedo=filled(s, (h, w, 3), torch.float32),
                            depth=filled(s, (h, w), torch.float32), ids=filled(s, (h, w, 2), torch.int32), stream=s.cuda_stream)


def warm_frame(st, s, then=None):
    """What a context does on its first frame only (the Halton table, the tile order's upload and its synchronize) happens here, not
    behind the hold; then the producer's own first call"""
    frame(st["ctx"], s, seed=9)
    if then:
        then(st, s)


def warmed(then=None):
    return lambda st, s: warm_frame(st, s, then)


def with_rays(st):
    """Two sets of 256 camera rays (device and host), and their tmax"""
    import torch
    c = st["ctx"]
    for k, region in (("1", RAYS), ("2", RAYS2)):
        o, d = c.camera_rays_device(region, seed=3)
        c.synchronize()
        st["o" + k], st["d" + k] = o, d
        st["ho" + k], st["hd" + k] = o.cpu().numpy(), d.cpu().numpy()
    st["tmax"] = torch.full((256,), 6.0, dtype=torch.float32, device=o.device)
    torch.cuda.synchronize()
    return st


# ---- frame <-> frame

def _frame_frame(name, scene, a, b, options=(), consumer=None, blocking=False, stats=False):
    def warm(st, s):
        warm_frame(st, s)
        if stats:
            frame(st["ctx"], s, seed=9, stats=True)   # (the counting kernel's first launch)
            s.synchronize()
            st["ctx"].reset_counters()
    finish = (lambda st: st["ctx"].counters()) if stats else None
    return U.ordered(name, lambda: new_ctx(scene, options), frame_of(1, stats=stats), consumer or frame_of(2, stats=stats), a, b, blocking=blocking, warm=warm,
                     finish=finish)


def _differ(x, y, what):
    assert U.differences(x, y), f"{what}: the two results are the same, so the case could not tell them apart"


@case
def frame_frame_box12(a, b):
    p, c, _ = _frame_frame("frame_frame_box12", BOX12, a, b)
    _differ(p, c, "seeds 1 and 2")


@case
def frame_frame_box3(a, b):
    _frame_frame("frame_frame_box3", BOX3, a, b)


@case
def frame_frame_object7(a, b):
    _frame_frame("frame_frame_object7", OBJECT7, a, b)


@case
def frame_frame_chunked(a, b):
    # pixState, tileProgress and the work ring are shared by the two frames and zeroed again by the second
    _frame_frame("frame_frame_chunked", BOX12, a, b, options=(("chunk_spp", 2), ("chunk_tail", 1)))


@case
def frame_frame_reshaped(a, b):
    # the tile order is rebuilt (freed, allocated, uploaded) for b's frame while a's frame, which reads the old one, is held
    _frame_frame("frame_frame_reshaped", BOX12, a, b, consumer=frame_of(2, region=SMALL), blocking=True)


@case
def frame_frame_halton_grows(a, b):
    # 128 samples want a longer Halton table than the 64 entries a's frame reads: freed and allocated under it
    _frame_frame("frame_frame_halton_grows", BOX12, a, b, options=(("chunk_spp", 0),), consumer=frame_of(2, spp=128), blocking=True)


@case
def frame_frame_stats(a, b):
    for scene in (BOX12, BOX3, OBJECT7):
        _, _, counters = _frame_frame("frame_frame_stats " + scene, scene, a, b, stats=True)
        assert counters["samples"] >= 2 * W * H * SPP, counters   # (both frames counted; the serial run's sum was compared in ordered)


@case
def frame_strips(a, b):
    import torch
    from qaray_amd import hip

    def strips(st, s):
        rows = hip.strip_count(0, H, 0, 2) * 8
        out = {"rgb": filled(s, (rows, W, 3), torch.float32), "depth": filled(s, (rows, W), torch.float32), "ns": filled(s, (rows, W), torch.int32)}
        st["ctx"].render_strips_device(REGION, 0, 2, SPP, out["rgb"], out["depth"], out["ns"], seed=1, stream=s.cuda_stream)
        return out
    # (b's whole frame has another tile order than a's strips: it is rebuilt, which blocks)
    U.ordered("frame_strips", lambda: new_ctx(BOX12), strips, frame_of(2), a, b, blocking=True)


# ---- frame <-> the read-only passes, both ways

def _pass_case(name, call, a, b):
    setup = lambda: with_rays(new_ctx(BOX3))   # noqa: E731
    U.ordered(name + " frame->pass", setup, frame_of(1), call, a, b, warm=warmed(call))
    U.ordered(name + " pass->frame", setup, call, frame_of(2), a, b, warm=warmed(call))


@case
def frame_gbuffer(a, b):
    _pass_case("frame_gbuffer", lambda st, s: gbuffer(st["ctx"], s), a, b)


@case
def frame_matte(a, b):
    _pass_case("frame_matte", lambda st, s: st["ctx"].matte_device(REGION, SPP, stream=s.cuda_stream), a, b)


@case
def frame_cast_rays(a, b):
    _pass_case("frame_cast_rays", lambda st, s: st["ctx"].cast_rays_device(st["o1"], st["d1"], stream=s.cuda_stream), a, b)


@case
def frame_occluded(a, b):
    import torch
    _pass_case("frame_occluded", lambda st, s: st["ctx"].occluded_device(st["o1"], st["d1"], st["tmax"], out=filled(s, (256,), torch.uint8), stream=s.cuda_stream), a, b)


@case
def frame_radiance_rays(a, b):
    _pass_case("frame_radiance_rays", lambda st, s: st["ctx"].radiance_rays_device(st["o1"], st["d1"], spp=2, seed=5, stream=s.cuda_stream), a, b)


@case
def frame_camera_rays(a, b):
    _pass_case("frame_camera_rays", lambda st, s: st["ctx"].camera_rays_device(RAYS, seed=3, stream=s.cuda_stream), a, b)


@case
def frame_camera_sample_rays(a, b):
    _pass_case("frame_camera_sample_rays", lambda st, s: st["ctx"].camera_sample_rays_device(RAYS, 0, 2, stream=s.cuda_stream), a, b)


# ---- edits: the held frame is the old scene's, what follows the edit is the new scene's

def _quartered_light(blob):
    from qaray_amd import hip
    lights = hip.blob_table(blob, "lights")
    k = int(np.flatnonzero(lights["type"] != 0)[0])   # (the first light after the ambient one, which the integrator does not use)
    new = lights[k:k + 1].copy()
    new["intensity"] *= np.float32(0.25)
    return (k, lights[k:k + 1].copy()), (k, new)


def _moved_camera(blob):
    from qaray_amd import hip
    cam = hip.blob_camera(blob).copy()
    new = cam.copy()
    shift = np.array([0.5, 0.25, 0.0], np.float32)
    new["cam_pos"] = cam["cam_pos"] + shift   # (the eye and the screen's corner move together: the same view from another place)
    new["screenA"] = cam["screenA"] + shift
    return cam, new


def _moved_node(blob):
    from qaray_amd import hip
    inst = hip.blob_table(blob, "instances")
    k = len(inst) - 1
    new = inst[k:k + 1].copy()
    new["pos"] = new["pos"] + np.array([1.5, 0.5, 1.0], np.float32)
    return (k, inst[k:k + 1].copy()), (k, new)


# kind -> (records_of(blob) -> (the records as they stand, the edited records), apply(ctx, records))
EDITS = {"lights": (_quartered_light, lambda c, r: c.edit_lights(*r)),
         "camera": (_moved_camera, lambda c, r: c.edit_camera(r)),
         "instances": (_moved_node, lambda c, r: c.edit_instances(*r))}


def _edit_case(name, kind, a, b):
    """The edit is applied while the frame it must wait for is held on a"""
    records_of, apply = EDITS[kind]

    def setup():
        st = new_ctx(BOX3)
        st["old"], st["new"] = records_of(st["blob"])
        return st

    def warm(st, s):
        warm_frame(st, s)
        apply(st["ctx"], st["old"])   # (an edit that changes nothing: the pinned ring is made here)
        gbuffer(st["ctx"], s)

    def consumer(st, s):
        apply(st["ctx"], st["new"])
        return {"frame": frame(st["ctx"], s, seed=2), "gbuffer": gbuffer(st["ctx"], s)}

    old, new, again = U.ordered(name, setup, frame_of(1), consumer, a, b, warm=warm, finish=lambda st: st["ctx"].render_region(REGION, SPP, seed=1))
    # the same frame as the held one, of the edited scene: it differs, so a held frame that had run on the new tables would show
    _differ([old["rgb"]], [again[0]], name + ": the frame before and after the edit")


@case
def edit_lights(a, b):
    _edit_case("edit_lights", "lights", a, b)


@case
def edit_camera(a, b):
    _edit_case("edit_camera", "camera", a, b)


@case
def edit_instances(a, b):
    _edit_case("edit_instances", "instances", a, b)


def _file_texture(st):
    """The state's first file texture, its texels as they stand on the host and as a device tensor"""
    import torch
    from qaray_amd import hip
    tex = hip.blob_table(st["blob"], "textures")
    st["tex"] = int(np.flatnonzero(tex["type"] == hip.QA_TEX_FILE)[0])
    st["texels_old"] = hip.blob_texels(st["blob"], st["tex"]).copy()
    st["same"] = torch.from_numpy(st["texels_old"]).to("cuda:0")
    return st


@case
def edit_under_held_context_stream(a, b):
    # The other direction: the edit's own copies are late, because the context's stream is.  The library does not hand that stream
    # out, but a texel edit from device memory makes it wait for the caller's stream (texSource): behind the hold on a, it holds the
    # context's stream, the next edit's copies queue up behind it, and a frame on b right after must still be the edited scene's
    for kind, (records_of, apply) in EDITS.items():
        def setup():
            st = _file_texture(new_ctx(TEXTURES))
            st["old"], st["new"] = records_of(st["blob"])
            st["before"] = st["ctx"].render_region(REGION, SPP, seed=2)
            return st

        def hold_the_context(st, s):
            st["ctx"].edit_texels(st["tex"], st["same"], stream=s.cuda_stream)   # (the texels as they are)

        def warm(st, s):
            warm_frame(st, s)
            apply(st["ctx"], st["old"])
            hold_the_context(st, s)
            gbuffer(st["ctx"], s)

        def consumer(st, s):
            apply(st["ctx"], st["new"])
            return {"frame": frame(st["ctx"], s, seed=2), "gbuffer": gbuffer(st["ctx"], s)}

        _, new, before = U.ordered("edit_under_held_context_stream " + kind, setup, hold_the_context, consumer, a, b, warm=warm, finish=lambda st: st["before"])
        _differ([new["frame"]["rgb"]], [before[0]], kind + ": the frame before and after the edit")


@case
def edit_after_empty_tiles(a, b):
    # qa_empty_tiles_device reads the instance and mesh tables: an edit after it waits for it, as for every read-only pass
    import torch

    def setup():
        st = new_ctx(BOX12)
        st["old"], st["new"] = _moved_node(st["blob"])
        return st

    def mask(st, s):
        m = filled(s, (H // 8, W // 8), torch.uint8)
        st["ctx"].empty_tiles_device(REGION, m, stream=s.cuda_stream)
        return m

    def warm(st, s):
        warm_frame(st, s)
        st["ctx"].edit_instances(*st["old"])
        mask(st, s)

    def consumer(st, s):
        st["ctx"].edit_instances(*st["new"])
        return mask(st, s)
    U.ordered("edit_after_empty_tiles", setup, mask, consumer, a, b, warm=warm)


@case
def edit_texels_device(a, b):
    # the source is produced on a behind the hold and overwritten on a right after the call: the next frame on b sees the new
    # texels, and the overwrite does not reach the texture.  The reference is an upload of the blob with the texels edited on the host
    import torch
    from qaray_amd import hip

    def setup():
        st = new_ctx(TEXTURES)
        tex = hip.blob_table(st["blob"], "textures")
        st["tex"] = int(np.flatnonzero(tex["type"] == hip.QA_TEX_FILE)[0])
        st["texels"] = (255 - hip.blob_texels(st["blob"], st["tex"])).astype(np.uint8)
        st["new"] = torch.from_numpy(st["texels"]).to("cuda:0")
        st["src"] = torch.zeros_like(st["new"])
        return st

    def warm(st, s):
        warm_frame(st, s)
        with torch.cuda.stream(s):
            st["src"].copy_(torch.from_numpy(hip.blob_texels(st["blob"], st["tex"]).copy()).to("cuda:0"))
        st["ctx"].edit_texels(st["tex"], st["src"], stream=s.cuda_stream)   # (the texels as they are: what a first device edit sets up)

    def producer(st, s):
        with torch.cuda.stream(s):
            st["src"].copy_(st["new"])
        st["ctx"].edit_texels(st["tex"], st["src"], stream=s.cuda_stream)
        with torch.cuda.stream(s):
            st["src"].zero_()
        return None

    def serial(st, s):
        edited = st["blob"].copy()
        hip.blob_texels(edited, st["tex"])[...] = st["texels"]
        before = U._host(frame(st["ctx"], s, seed=2))
        st["ctx"].upload_scene(edited)
        after = frame(st["ctx"], s, seed=2)
        torch.cuda.synchronize()
        _differ(before, U._host(after), "the frame before and after the texel edit")
        return None, after
    U.ordered("edit_texels_device", setup, producer, frame_of(2), a, b, warm=warm, serial=serial,
              finish=lambda st: hip.blob_texels(st["ctx"].download_scene(), st["tex"]).copy())


# ---- the progressive frame

def _progressive(spp=16, spp_max=None):
    def setup():
        import torch
        st = new_ctx(BOX12)
        frame(st["ctx"], torch.cuda.current_stream(), seed=9)   # (the context's first frame, on its own stream: the tile order of this shape)
        st["ctx"].synchronize()
        st["p"] = st["ctx"].progressive(REGION, spp, spp_max=spp_max, seed=1)
        st["ctx"].synchronize()
        return st
    return setup


def _advance(target):
    def call(st, s):
        st["p"].advance(target, stream=s.cuda_stream)
    return call


def _prog_state(st):
    return {"read": st["p"].read(), "levels": st["p"].tile_levels()}


@case
def progressive_readers(a, b):
    import torch

    def read_device(st, s):
        out = {"rgb": filled(s, (H, W, 3), torch.float32), "depth": filled(s, (H, W), torch.float32), "ns": filled(s, (H, W), torch.int32)}
        st["p"].read_device(out["rgb"], out["depth"], out["ns"], stream=s.cuda_stream)
        return out
    U.ordered("progressive_readers read()", _progressive(), _advance(4), lambda st, s: st["p"].read(), a, b, blocking=True, warm=False)
    readers = {"read_device": read_device,
               "gbuffer_device": lambda st, s: st["p"].gbuffer_device(stream=s.cuda_stream),
               "denoise_device": lambda st, s: st["p"].denoise_device(out=filled(s, (H, W, 3), torch.float32), stream=s.cuda_stream),
               "denoise_guided_device": lambda st, s: st["p"].denoise_guided_device(out=filled(s, (H, W, 3), torch.float32), stream=s.cuda_stream),
               "display_device": lambda st, s: st["p"].display_device(stream=s.cuda_stream),
               "matte_device": lambda st, s: st["p"].matte_device(stream=s.cuda_stream),
               "tile_levels_device": lambda st, s: st["p"].tile_levels_device(out=filled(s, (H // 8, W // 8), torch.int32), stream=s.cuda_stream)}
    for name, call in readers.items():
        # (warm: the reader once on the fresh frame - the planes and blocks it makes on first use)
        U.ordered("progressive_readers " + name, _progressive(), _advance(4), call, a, b, warm=call, finish=_prog_state)


@case
def progressive_advance_advance(a, b):
    U.ordered("progressive_advance_advance", _progressive(), _advance(4), _advance(8), a, b, warm=False, finish=_prog_state)


@case
def progressive_one_shot_between(a, b):
    # a one-shot frame between two passes shares the launch plumbing (the Halton table, the tile order, the work ring) with them
    def consumer(st, s):
        out = frame(st["ctx"], s, seed=2)
        st["p"].advance(8, stream=s.cuda_stream)
        return out
    U.ordered("progressive_one_shot_between", _progressive(), _advance(4), consumer, a, b, warm=False, finish=_prog_state)


@case
def progressive_tile_passes(a, b):
    import torch
    half = np.zeros((H // 8, W // 8), np.uint8)
    half[:, ::2] = 1

    def tiles_device(st, s):
        with torch.cuda.stream(s):
            st["mask"] = torch.from_numpy(half).to("cuda:0")
        st["p"].advance_tiles(12, st["mask"], stream=s.cuda_stream)
    passes = {"advance_tiles": lambda st, s: st["p"].advance_tiles(12, half, stream=s.cuda_stream),
              "advance_tiles_device": tiles_device,
              "advance_adaptive": lambda st, s: st["p"].advance_adaptive(12, fraction=0.5, stream=s.cuda_stream),
              "tile_error_device": lambda st, s: st["p"].tile_error_device(out=filled(s, (H // 8, W // 8), torch.float32), stream=s.cuda_stream)}

    def first_use(st, s):
        # the slabs of the selective passes (device and pinned memory) and the error map's kernel are made on first use: here, by
        # a pass over half the tiles, not behind the hold
        st["p"].advance_tiles(4, 1 - half, stream=s.cuda_stream)
        st["p"].tile_error_device(stream=s.cuda_stream)
    for name, call in passes.items():
        U.ordered("progressive_tile_passes " + name, _progressive(4, 16), _advance(8), call, a, b, warm=first_use, finish=_prog_state)


# ---- display, denoise, reproject: two calls with different inputs

def _two_frames(region=REGION, small=None, guides=False):
    """A context and two frames of it (seeds 1 and 2) as device tensors; small: frame 1 is of that region instead"""
    def setup():
        import torch
        st = new_ctx(BOX12)
        c = st["ctx"]
        cur = torch.cuda.current_stream()
        st["f1"], st["f2"] = frame(c, cur, small or region, seed=1), frame(c, cur, region, seed=2)
        if guides:
            st["g"] = gbuffer(c, cur, region)
            n = (region[3] - region[1]) * (region[2] - region[0])
            st["variance"] = ((torch.arange(n, device="cuda:0") % 7).to(torch.float32) / 7.0).reshape(region[3] - region[1], region[2] - region[0])
        c.synchronize()
        torch.cuda.synchronize()
        return st
    return setup


@case
def display_display(a, b):
    def call(which):
        return lambda st, s: st["ctx"].display_device(st[which]["rgb"], st[which]["depth"], st[which]["ns"], SPP, stream=s.cuda_stream)
    p, c, _ = U.ordered("display_display", _two_frames(), call("f1"), call("f2"), a, b)
    _differ(p, c, "the displays of two frames")


@case
def denoise_denoise(a, b):
    import torch

    def call(form, which):
        def run(st, s):
            f, c, out = st[which], st["ctx"], filled(s, (H, W, 3), torch.float32)
            if form == "plain":
                return c.denoise_device(f["rgb"], f["depth"], f["ns"], out=out, stream=s.cuda_stream)
            g = st["g"]
            if form == "guided":
                return c.denoise_guided_device(f["rgb"], f["depth"], f["ns"], normal=g["normal"], albedo=g["albedo"], out=out, stream=s.cuda_stream)
            return c.denoise_variance_device(f["rgb"], f["depth"], f["ns"], normal=g["normal"], albedo=g["albedo"], variance=st["variance"], out=out,
                                             stream=s.cuda_stream)
        return run
    for form in ("plain", "guided", "variance"):
        p, c, _ = U.ordered("denoise_denoise " + form, _two_frames(guides=True), call(form, "f1"), call(form, "f2"), a, b)
        _differ([p], [c], "the filtered frames")


@case
def denoise_planes_grow(a, b):
    # the second image is larger: the working planes are freed and allocated while the first filter, which uses the old ones, is held
    import torch

    def call(which, region):
        h, w = region[3] - region[1], region[2] - region[0]
        return lambda st, s: st["ctx"].denoise_device(st[which]["rgb"], st[which]["depth"], st[which]["ns"], out=filled(s, (h, w, 3), torch.float32),
                                                      stream=s.cuda_stream)
    U.ordered("denoise_planes_grow", _two_frames(small=SMALL), call("f1", SMALL), call("f2", REGION), a, b, blocking=True)


@case
def reproject_reproject(a, b):
    # the progressive forms with ids: the context's ids plane (lastReproject) and the guide pass that fills it (lastFrame)
    import torch
    from qaray_amd import hip

    def setup():
        st = _two_frames(guides=True)()
        c = st["ctx"]
        st["p"] = c.progressive(REGION, SPP, seed=3)
        st["p"].advance(SPP)
        c.synchronize()
        st["cam"] = hip.blob_camera(st["blob"]).copy()
        for k, length in (("f1", 1.0), ("f2", 3.0)):
            st[k]["length"] = torch.full((H, W), length, dtype=torch.float32, device="cuda:0")
        torch.cuda.synchronize()
        return st

    def call(form, which):
        def run(st, s):
            f = st[which]
            fn = {"plain": st["p"].reproject_device, "motion": st["p"].reproject_motion_device, "moments": st["p"].reproject_moments_device}[form]
            return fn((f["rgb"], f["depth"], f["length"]), st["cam"], hist_ids=st["g"]["ids"], out=filled(s, (H, W, 3), torch.float32),
                      out_length=filled(s, (H, W), torch.float32), stream=s.cuda_stream)
        return run
    for form in ("plain", "motion", "moments"):
        p, c, _ = U.ordered("reproject_reproject " + form, setup, call(form, "f1"), call(form, "f2"), a, b)
        _differ(p, c, "the reprojections of two histories")


# ---- the host forms under a held device form of the same unit

@case
def host_forms(a, b):
    import torch
    pairs = {
        "render_region": (frame_of(1), lambda st, s: st["ctx"].render_region(REGION, SPP, seed=2)),
        "cast_rays": (lambda st, s: st["ctx"].cast_rays_device(st["o1"], st["d1"], stream=s.cuda_stream), lambda st, s: st["ctx"].cast_rays(st["ho2"], st["hd2"])),
        "occluded": (lambda st, s: st["ctx"].occluded_device(st["o1"], st["d1"], st["tmax"], out=filled(s, (256,), torch.uint8), stream=s.cuda_stream),
                     lambda st, s: st["ctx"].occluded(st["ho2"], st["hd2"], 6.0)),
        "radiance_rays": (lambda st, s: st["ctx"].radiance_rays_device(st["o1"], st["d1"], spp=2, seed=5, stream=s.cuda_stream),
                          lambda st, s: st["ctx"].radiance_rays(st["ho2"], st["hd2"], spp=2, seed=6)),
        "gbuffer": (lambda st, s: gbuffer(st["ctx"], s), lambda st, s: st["ctx"].gbuffer(REGION, seed=4)),
        "matte": (lambda st, s: st["ctx"].matte_device(REGION, SPP, stream=s.cuda_stream), lambda st, s: st["ctx"].matte(SMALL, SPP)),
    }
    for name, (device_form, host_form) in pairs.items():
        U.ordered("host_forms " + name, lambda: with_rays(new_ctx(BOX3)), device_form, host_form, a, b, blocking=True, warm=warmed(device_form))


# ---- two contexts, then the lifetime cases

@case
def two_contexts(a, b):
    def setup():
        one, two = new_ctx(BOX12), new_ctx(BOX12)
        return {"one": one["ctx"], "two": two["ctx"], "close": lambda: (one["ctx"].close(), two["ctx"].close())}

    def warm(st, s):
        frame(st["one"], s, seed=9)
        frame(st["two"], s, seed=9)
    p, c, _ = U.ordered("two_contexts", setup, lambda st, s: frame(st["one"], s), lambda st, s: frame(st["two"], s), a, b, waits=False, warm=warm)
    assert not U.differences(p, c), "the same frame on two contexts differs"


@case
def upload_under_frame(a, b):
    def consumer(st, s):
        st["ctx"].upload_scene(st["next"])
        return frame(st["ctx"], s, seed=2)
    old, new, _ = U.ordered("upload_under_frame", lambda: new_ctx(BOX12, next=blob_of(BOX3)), frame_of(1), consumer, a, b, blocking=True)
    _differ([old["depth"]], [new["depth"]], "the two scenes")


@case
def close_under_frame(a, b):
    def consumer(st, s):
        st["ctx"].close()
        fresh = new_ctx(BOX12)
        try:
            return fresh["ctx"].render_region(REGION, SPP, seed=1)
        finally:
            fresh["ctx"].close()
    held, fresh, _ = U.ordered("close_under_frame", lambda: new_ctx(BOX12), frame_of(1), consumer, a, b, blocking=True)
    assert not U.differences([held["rgb"], held["depth"]], [fresh[0], fresh[1]]), "the fresh context's frame is not the held one's"


# ---- the tests

@pytest.fixture(scope="module")
def streams():
    """The two streams of the callers' - with the context's, three at a time - and the module's concurrency control"""
    import torch
    dev = torch.device("cuda", 0)
    a = torch.cuda.Stream(dev)
    U.calibrate(a)
    b = U.concurrency_control(a, [torch.cuda.Stream(dev) for _ in range(4)])
    yield a, b
    torch.cuda.synchronize()


def test_case_table_is_the_utilitys():
    assert list(RUN) == list(U.CASES)


@pytest.mark.parametrize("name", list(U.CASES))
def test_ordered(streams, name):
    RUN[name](*streams)
