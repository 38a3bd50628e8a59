"""Progressive frames (qa_progressive_*, Context.progressive): a resident image whose samples are raised in passes.

Every pixel takes the same samples in the same order as in a one-shot frame, its state waiting in device memory between
passes, so the preview after a pass to S samples IS the one-shot frame of S samples (spp_min == spp_max), bit for bit, and
the final frame is the one-shot frame of the same arguments - on every kernel family.  Counters summed over the passes
equal the one-shot frame's: a pass never takes a sample beyond its target (a re-issued target after a stop included)."""
import numpy as np
import pytest

from conftest import bits, ensure_assets, golden_blob, load_golden

pytestmark = pytest.mark.gpu

QA_EINVAL, QA_ENOSCENE, QA_EUNSUPPORTED = -1, -5, -6
CNT = ("samples", "casts_normal", "casts_shadow", "pixels")


@pytest.fixture(scope="module")
def ctx():
    from qaray_amd import hip
    c = hip.Context(0)
    yield c
    c.close()


def blob(scene, size):
    from qaray_amd.host import load_scene_blob
    ensure_assets()
    return load_scene_blob(scene, size=size)


def same(a, b):
    return all(np.array_equal(bits(x), bits(y)) for x, y in zip(a, b))


# scene, size, spp, what runs: every megakernel family
FAMILIES = {
    "box": ("example_project12_box.xml", (64, 64), 64, "qa_integrate<RES=1,LIGHTS=0"),
    "sphere": ("example_project3_sphere.xml", (64, 48), 32, "qa_integrate<"),
    "caustics_c4": ("example_project12_caustics_glossy.xml", (64, 48), 16, "qa_integrate_cs_resume<"),
    "tower_c5": ("trc_scene_tower.xml", (64, 48), 16, "qa_integrate_cs_resume<"),
    "object_textured": ("example_project7_object.xml", (80, 56), 16, "TEX=1"),
    "area_coop": ("example_project10_test.xml", (64, 48), 8, "qa_integrate_cs"),
    "area_per_lane": ("example_project10_test.xml", (64, 48), 8, "qa_integrate<RES=0"),
    "photon": ("custom_photon.xml", (64, 48), 8, "photon-map gathers"),
}


def targets(n):
    return sorted({s for s in (1, 2, 7, 8, 33, 64, 200, 512, 1024, n) if s <= n})


@pytest.mark.parametrize("case", sorted(FAMILIES))
def test_every_pass_is_the_one_shot_frame_of_its_samples(ctx, case):
    scene, size, n, kernel = FAMILIES[case]
    ctx.upload_scene(blob(scene, size))
    if case == "photon":
        ctx.build_photon_maps((2000, 20, 2.0), (300, 20, 3.0))
    ctx.set_option("coop", 0 if case == "area_per_lane" else 1)
    try:
        region = (0, 0) + size
        with ctx.progressive(region, n) as prog:
            for s in targets(n):
                prog.advance(s)
                frame = prog.read()
                assert kernel in ctx.kernel_name(), ctx.kernel_name()
                # (a one-shot frame between passes: it must not disturb the progressive one either)
                assert same(frame, ctx.render_region(region, s)), (case, s)
            st = prog.status()
            assert st["spp_reached"] == n and st["tiles_behind"] == 0 and st["pixels_finished"] == size[0] * size[1]
    finally:
        ctx.set_option("coop", 1)


@pytest.mark.parametrize("case", ["sphere", "caustics_c4", "tower_c5", "area_coop"])
def test_counters_summed_over_passes_equal_the_one_shot_frame(ctx, case):
    scene, size, n, _ = FAMILIES[case]
    ctx.upload_scene(blob(scene, size))
    region = (0, 0) + size
    ctx.reset_counters()
    one = ctx.render_region(region, n)
    c1 = ctx.counters()
    ctx.reset_counters()
    with ctx.progressive(region, n) as prog:
        for s in targets(n):
            prog.advance(s)
        frame = prog.read()
    c2 = ctx.counters()
    assert same(frame, one)
    assert all(c1[k] == c2[k] for k in CNT), (c1, c2)


def test_counting_frame_in_passes(ctx):
    """QA_RENDER_STATS frames: the traversal counters summed over the passes equal the one-shot counting frame's."""
    scene, size = "example_project12_box.xml", (64, 48)
    ctx.upload_scene(blob(scene, size))
    region = (0, 0) + size
    ctx.reset_counters()
    one = ctx.render_region(region, 16, stats=True)
    c1 = ctx.counters()
    ctx.reset_counters()
    with ctx.progressive(region, 16, stats=True) as prog:
        for s in (1, 5, 16):
            prog.advance(s)
        frame = prog.read()
    c2 = ctx.counters()
    assert "counting variant" in ctx.kernel_name()
    assert same(frame, one)
    assert c1 == c2 and c2["bvh_nodes"] > 0 and c2["tri_tests"] > 0


@pytest.mark.parametrize("name,passes", [("c2_box_1080p_crop_512spp", (64, 128, 320, 512)),
                                         ("c3_object_1080p_crop_256spp", (16, 100, 256)),
                                         ("c5_tower_4k_crop_2048spp", (256, 1024, 2048))])
def test_frames_built_in_passes_match_the_goldens(ctx, name, passes):
    rgb, depth, ns, meta = load_golden(name)
    ctx.upload_scene(golden_blob(meta))
    region = tuple(meta["crop"])
    ctx.reset_counters()
    with ctx.progressive(region, meta["spp_min"], spp_max=meta["spp_max"], max_bounce=meta["bounce"], seed=meta["seed"]) as prog:
        for s in passes:
            prog.advance(s)
        g_rgb, g_depth, g_ns = prog.read()
    cnt = ctx.counters()
    assert np.array_equal(g_ns, ns) and np.array_equal(bits(g_depth), bits(depth))
    assert (cnt["samples"], cnt["casts_normal"], cnt["casts_shadow"]) == (meta["samples"], meta["casts_normal"], meta["casts_shadow"])
    one = ctx.render_region(region, meta["spp_min"], max_bounce=meta["bounce"], seed=meta["seed"], spp_max=meta["spp_max"])
    assert same((g_rgb, g_depth, g_ns), one)
    if name.startswith("c2_"):
        assert np.array_equal(bits(g_rgb), bits(rgb))
    else:
        assert float(np.sqrt(np.mean((g_rgb.astype(np.float64) - rgb) ** 2))) <= 1e-6 and float(np.abs(g_rgb - rgb).max()) <= 1e-4


def test_adaptive_frame_in_passes(ctx):
    """spp_min < spp_max: pixels finish by the adaptive rule inside passes; the preview never shows more samples than the
    target, a finished pixel keeps its count, and the final frame is the golden's."""
    rgb, depth, ns, meta = load_golden("sphere_adaptive_64x48_4to32spp")
    ctx.upload_scene(golden_blob(meta))
    region = tuple(meta["crop"])
    prev = None
    with ctx.progressive(region, meta["spp_min"], spp_max=meta["spp_max"], max_bounce=meta["bounce"], seed=meta["seed"]) as prog:
        for s in (1, 2, 4, 5, 8, 16, 32, 64):
            prog.advance(s)
            f_rgb, f_depth, f_ns = prog.read()
            assert (f_ns <= min(s, meta["spp_max"])).all()
            if prev is not None:
                done = prev < min(prev_s, meta["spp_max"])   # stopped short of the target: finished for good
                assert np.array_equal(f_ns[done], prev[done])
                assert (f_ns >= prev).all()
            prev, prev_s = f_ns, s
    assert np.array_equal(f_ns, ns) and np.array_equal(bits(f_depth), bits(depth))
    assert float(np.sqrt(np.mean((f_rgb.astype(np.float64) - rgb) ** 2))) <= 1e-6
    one = ctx.render_region(region, meta["spp_min"], max_bounce=meta["bounce"], seed=meta["seed"], spp_max=meta["spp_max"])
    assert same((f_rgb, f_depth, f_ns), one)


@pytest.mark.parametrize("case", ["sphere", "caustics_c4"])
def test_torn_passes_complete_without_overshoot(ctx, case):
    """progressive_tile_limit: a pass takes at most n tiles, then ends as if stopped (the tiles in hand finish their pass)."""
    scene, size, _, _ = FAMILIES[case]
    ctx.upload_scene(blob(scene, size))
    region = (0, 0) + size
    tiles = (size[0] // 8) * (size[1] // 8)
    ref = {s: ctx.render_region(region, s) for s in (4, 16, 32)}
    ctx.reset_counters()
    ctx.render_region(region, 32)
    c1 = ctx.counters()
    ctx.reset_counters()
    try:
        with ctx.progressive(region, 32) as prog:
            # the first pass torn: tiles at level 0 and 4
            ctx.set_option("progressive_tile_limit", 10)
            prog.advance(4)
            st = prog.status()
            assert st["spp_reached"] == 0 and st["tiles_behind"] == tiles - 10
            f_rgb, f_depth, f_ns = prog.read()
            assert (f_ns == 4).sum() == 10 * 64 and (f_ns == 0).sum() == (tiles - 10) * 64
            assert (bits(f_depth)[f_ns == 0] == bits(np.float32(1e30))).all() and (f_rgb[f_ns == 0] == 0).all()
            # the same target again, torn again, then completed
            prog.advance(4)
            assert prog.status()["tiles_behind"] == tiles - 20
            ctx.set_option("progressive_tile_limit", 0)
            prog.advance(4)
            assert prog.status() == {"spp_reached": 4, "tiles_behind": 0, "pixels_finished": 0}
            assert same(prog.read(), ref[4])
            # a later pass torn: tiles at 4 and 16, then tiles at 4, 16 and 32
            ctx.set_option("progressive_tile_limit", 5)
            prog.advance(16)
            assert prog.status()["tiles_behind"] == tiles - 5 and prog.status()["spp_reached"] == 4
            prog.advance(32)
            st = prog.status()
            assert st["tiles_behind"] == tiles - 5 and st["spp_reached"] == 4 and st["pixels_finished"] == 5 * 64
            ctx.set_option("progressive_tile_limit", 0)
            prog.advance(16)   # re-issued below the highest target: the tiles at 32 take nothing
            assert prog.status()["tiles_behind"] == 0
            prog.advance(32)
            assert prog.status() == {"spp_reached": 32, "tiles_behind": 0, "pixels_finished": tiles * 64}
            frame = prog.read()
            prog.advance(32)   # at the frame's level: nothing happens
    finally:
        ctx.set_option("progressive_tile_limit", 0)
    c2 = ctx.counters()
    assert same(frame, ref[32])
    assert all(c1[k] == c2[k] for k in CNT), (c1, c2)


def test_stop_before_a_pass_moves_nothing(ctx):
    size = (64, 48)
    ctx.upload_scene(blob("example_project3_sphere.xml", size))
    region = (0, 0) + size
    one = ctx.render_region(region, 8)
    with ctx.progressive(region, 8) as prog:
        prog.advance(2)
        before = prog.read()
        ctx.reset_counters()
        ctx.request_stop()
        try:
            prog.advance(8)
            st = prog.status()
            assert st["spp_reached"] == 2 and st["tiles_behind"] == 48
            assert same(prog.read(), before)
            assert ctx.counters()["samples"] == 0
        finally:
            ctx.clear_stop()
        prog.advance(8)
        assert prog.status()["tiles_behind"] == 0
        assert same(prog.read(), one)


def test_one_shot_chunked_frames_and_option_changes_leave_the_frame_alone(ctx):
    size = (64, 48)
    ctx.upload_scene(blob("example_project12_caustics_glossy.xml", size))
    region = (0, 0) + size
    ref = {s: ctx.render_region(region, s) for s in (4, 8, 16)}
    try:
        with ctx.progressive(region, 16) as prog:
            prog.advance(4)
            a = prog.read()
            # a one-shot frame in small chunks (the context's own chunk slabs), then more passes with the cooperative walks off / on
            ctx.set_option("chunk_spp", 1)
            ctx.set_option("chunk_tail", 1)
            other = ctx.render_region(region, 8)
            ctx.set_option("chunk_spp", -1)
            ctx.set_option("chunk_tail", 0)
            assert same(other, ref[8])
            assert same(prog.read(), a)
            ctx.set_option("coop", 0)
            prog.advance(8)
            assert "qa_integrate<RES=0" in ctx.kernel_name()
            assert same(prog.read(), ref[8])
            ctx.set_option("coop", 1)
            ctx.set_pipeline("staged")   # progressive passes always run on the megakernel
            prog.advance(16)
            assert "qa_integrate_cs_resume<" in ctx.kernel_name(), ctx.kernel_name()
            assert same(prog.read(), ref[16])
    finally:
        ctx.set_option("chunk_spp", -1)
        ctx.set_option("chunk_tail", 0)
        ctx.set_option("coop", 1)
        ctx.set_pipeline("auto")


def test_read_device_equals_read(ctx):
    import torch
    size = (64, 48)
    ctx.upload_scene(blob("example_project12_box.xml", size))
    with ctx.progressive((0, 0) + size, 8) as prog:
        prog.advance(3)
        host = prog.read()
        rgb = torch.zeros((48, 64, 3), dtype=torch.float32, device="cuda")
        depth = torch.zeros((48, 64), dtype=torch.float32, device="cuda")
        ns = torch.zeros((48, 64), dtype=torch.int32, device="cuda")
        prog.read_device(rgb, depth, ns)
        ctx.synchronize()
        dev = (rgb.cpu().numpy(), depth.cpu().numpy(), ns.cpu().numpy().view(np.uint32))
    assert same(dev, host)


def test_lifetime_and_errors():
    from qaray_amd import hip
    c = hip.Context(0)
    try:
        with pytest.raises(hip.HipError) as e:
            c.progressive((0, 0, 8, 8), 4)
        assert e.value.code == QA_ENOSCENE
        box = blob("example_project12_box.xml", (64, 48))
        c.upload_scene(box)
        with pytest.raises(hip.HipError) as e:   # advance without begin
            hip.Progressive(c, (0, 0, 64, 48)).advance(4)
        assert e.value.code == QA_EINVAL
        for region in ((0, 0, 65, 48), (8, 8, 8, 16), (-1, 0, 8, 8)):
            with pytest.raises(hip.HipError) as e:
                c.progressive(region, 4)
            assert e.value.code == QA_EINVAL
        prog = c.progressive((0, 0, 64, 48), 4)
        prog.advance(2)
        c.upload_scene(box)   # a scene upload ends the frame
        with pytest.raises(hip.HipError) as e:
            prog.advance(4)
        assert e.value.code == QA_EINVAL and "scene" in str(e.value)
        with pytest.raises(hip.HipError) as e:
            prog.read()
        assert e.value.code == QA_EINVAL
        c.upload_scene(blob("example_project10_test.xml", (64, 48)))   # area lights: at most 7 bounces
        with pytest.raises(hip.HipError) as e:
            c.progressive((0, 0, 64, 48), 4, max_bounce=9)
        assert e.value.code == QA_EUNSUPPORTED
        c.upload_scene(blob("custom_photon.xml", (64, 48)))
        prog = c.progressive((0, 0, 64, 48), 4)
        prog.advance(1)
        c.build_photon_maps((2000, 20, 2.0), (300, 20, 3.0))   # so do the photon maps
        with pytest.raises(hip.HipError) as e:
            prog.advance(4)
        assert e.value.code == QA_EINVAL and "photon" in str(e.value)
    finally:
        c.close()


def test_frames_do_not_depend_on_scratch_contents():
    """a progressive frame rendered after the private segments were filled with two patterns is the same."""
    from qaray_amd import hip
    c = hip.Context(0)
    size = (96, 64)
    frames = []
    try:
        for scene in ("example_project12_caustics_glossy.xml", "example_project3_sphere.xml"):
            c.upload_scene(blob(scene, size))
            out = []
            for pattern in (0x00000000, 0xFFFFFFFF):
                c.scrub_scratch(pattern)
                with c.progressive((0, 0) + size, 8) as prog:
                    prog.advance(3)
                    prog.advance(8)
                    out.append(prog.read())
            frames.append(out)
    finally:
        c.close()
    for a, b in frames:
        assert same(a, b)


@pytest.mark.parametrize("scene", ["example_project12_box.xml", "example_project3_sphere.xml"])
def test_cli_progressive_writes_the_one_shot_images(tmp_path, scene):
    """qaray_hip -progressive N: passes of N spp, one line per pass; the final PNGs are the one-shot run's, byte for byte."""
    import os
    import subprocess
    from conftest import ROOT
    from qaray_amd.host import SCENES_DIR
    exe = os.path.join(ROOT, "qaray_amd", "lib", "qaray_hip")
    common = ["-batch", "-spp", "64", "-size", "96", "64", "-root", SCENES_DIR]
    outs = {}
    for mode, extra in (("one", []), ("prog", ["-progressive", "16"])):
        out = str(tmp_path / mode) + "_"
        r = subprocess.run([exe] + common + extra + ["-out", out, os.path.join(SCENES_DIR, scene)], stdout=subprocess.PIPE,
                           stderr=subprocess.STDOUT, text=True)
        assert r.returncode == 0, r.stdout
        outs[mode] = (out, r.stdout)
    passes = [l for l in outs["prog"][1].splitlines() if l.startswith("pass to ")]
    assert [l.split(":")[0] for l in passes] == ["pass to 16 spp", "pass to 32 spp", "pass to 48 spp", "pass to 64 spp"], outs["prog"][1]
    assert "64 spp reached" in passes[-1]
    for png in ("colorBuffer.png", "depthBuffer.png", "sampleBuffer.png"):
        with open(outs["one"][0] + png, "rb") as a, open(outs["prog"][0] + png, "rb") as b:
            assert a.read() == b.read(), png
    r = subprocess.run([exe] + common + ["-devices", "2", "-progressive", "16", os.path.join(SCENES_DIR, scene)], stdout=subprocess.PIPE,
                       stderr=subprocess.STDOUT, text=True)
    assert r.returncode != 0 and "-progressive" in r.stdout and "-devices" in r.stdout
