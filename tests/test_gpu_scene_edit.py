"""Scene edits (qa_scene_edit_*, Context.edit_*): the camera, lights, materials and node transforms of a resident scene.

After the edits that turn scene A into scene B the context must be exactly where upload_scene(B) leaves a fresh one - same
kernel plan and name, same bits in every later frame, on every kernel family and on the staged integrator - without a mesh build,
without a device allocation and with a few kilobytes copied.  Progressive frames go stale and restart in place; the photon maps
survive a camera edit and nothing else; a refused edit changes nothing."""
import numpy as np
import pytest

from conftest import bits, ensure_assets

import scene_edit_util as U

pytestmark = pytest.mark.gpu

QA_EINVAL, QA_ENOSCENE = -1, -5
CNT = ("samples", "casts_normal", "casts_shadow", "pixels")
# tests/test_gpu_parity.py's tolerances against the oracle (radiance scaled by the frame's largest value where that exceeds 1);
# the LDS-resident Cornell box is bit-exact there; photon frames: tests/test_gpu_photon.py's relative bound
RMSE_TOL, MAXABS_TOL, PHOTON_REL_MAX_TOL = 1e-6, 1e-4, 1e-6
PHOTON_MAPS = ((2000, 20, 2.0), (300, 20, 3.0))


@pytest.fixture(scope="module")
def ctx():
    from qaray_amd import hip
    c = hip.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def fresh():
    """The second context: only ever uploads."""
    from qaray_amd import hip
    c = hip.Context(0)
    yield c
    c.close()


def families():
    from test_gpu_progressive import FAMILIES
    return FAMILIES


FAMILY_NAMES = ["area_coop", "area_per_lane", "box", "caustics_c4", "object_textured", "photon", "sphere", "tower_c5"]


def blob_a(scene, size):
    from qaray_amd.host import load_scene_blob
    ensure_assets()
    return load_scene_blob(scene, size=size)


def same(a, b):
    return all(np.array_equal(bits(x), bits(y)) for x, y in zip(a, b))


def frame_and_counters(c, region, spp):
    c.reset_counters()
    f = c.render_region(region, spp)
    cnt = c.counters()
    return f, {k: cnt[k] for k in CNT}


def scene_side_bytes(blob):
    """What an edit may copy at most: the blob's sections that are neither mesh nor texture data, and the tables derived from them
    (CsInst 256 + CsCull 32 bytes per node, DMaterial 96 per material, the resident image of at most 40 KB)."""
    n = lambda at: int(blob[at:at + 4].view(np.uint32)[0])   # noqa: E731
    inst, mtlsets, mats, lights, texmaps = n(136), n(144), n(148), n(152), n(156)
    in_blob = 264 + inst * 112 + mtlsets * 16 + mats * 112 + lights * 64 + texmaps * 64
    return in_blob + inst * (256 + 32) + mats * 96 + 40 * 1024


def test_family_list_is_the_progressive_suites():
    assert FAMILY_NAMES == sorted(families())


@pytest.mark.parametrize("case", FAMILY_NAMES)
def test_edits_leave_the_context_where_an_upload_of_b_does(ctx, fresh, tmp_path, case):
    from oracle import binding as oracle
    scene, size, spp, kernel = families()[case]
    a = blob_a(scene, size)
    b, camera, records, _ = U.scene_b(scene, size, tmp_path)
    assert not np.array_equal(a, b) and len(a) == len(b)
    region = (0, 0) + size
    coop = 0 if case == "area_per_lane" else 1
    for c in (ctx, fresh):
        c.set_option("coop", coop)
    try:
        ctx.upload_scene(a)
        frame_a = ctx.render_region(region, spp)
        before = ctx.scene_stats()
        assert before[3] == 0 and before[2] >= len(a)
        bound = scene_side_bytes(a)
        ctx.edit_camera(camera)
        copied = [ctx.scene_stats()[2]]
        for which, fn in (("lights", ctx.edit_lights), ("materials", ctx.edit_materials), ("instances", ctx.edit_instances)):
            if which in records:
                fn(*records[which])
                copied.append(ctx.scene_stats()[2])
        after = ctx.scene_stats()
        print(case, "bytes copied per edit", copied, "bound", bound, "upload", before[2])
        assert after[0] == before[0], "an edit ran the per-mesh builder"
        assert after[1] == before[1], "an edit allocated device memory"
        assert all(0 < x <= bound for x in copied), (copied, bound)
        assert after[3] == len(copied)
        assert np.array_equal(ctx.download_scene(), b)

        fresh.upload_scene(b)
        assert ctx.kernel_name() == fresh.kernel_name()
        if case == "photon":
            ctx.build_photon_maps(*PHOTON_MAPS)
            fresh.build_photon_maps(*PHOTON_MAPS)
        f1, c1 = frame_and_counters(ctx, region, spp)
        f2, c2 = frame_and_counters(fresh, region, spp)
        # (FAMILIES names what a progressive pass launches; a one-shot frame runs the same variant without "_resume")
        assert kernel.replace("_resume", "") in ctx.kernel_name() and ctx.kernel_name() == fresh.kernel_name(), (ctx.kernel_name(), fresh.kernel_name())
        assert same(f1, f2), case
        assert c1 == c2
        assert not same(f1, frame_a), "the edits changed nothing"

        # the oracle on the blob the context hands back
        down = ctx.download_scene()
        if case == "photon":
            pp = oracle.photon_params(*PHOTON_MAPS)
            o_pm, o_cm, _, _ = oracle.photon_build(down, pp)
            o_rgb, o_depth, o_ns, o_cnt = oracle.render(down, region, spp, photon=(pp, o_pm, o_cm))
        else:
            o_rgb, o_depth, o_ns, o_cnt = oracle.render(down, region, spp)
        rgb, depth, ns = f1
        assert np.array_equal(ns, o_ns) and np.array_equal(bits(depth), bits(o_depth))
        assert (c1["samples"], c1["casts_normal"], c1["casts_shadow"]) == (o_cnt.samples, o_cnt.casts_normal, o_cnt.casts_shadow)
        finite = np.isfinite(o_rgb)
        assert np.isfinite(rgb).all() == finite.all()
        scale = max(1.0, float(np.abs(o_rgb[finite]).max()) if finite.any() else 1.0)
        err = float(np.nanmax(np.abs(rgb - o_rgb)))
        rms = float(np.sqrt(np.mean((np.nan_to_num(rgb).astype(np.float64) - np.nan_to_num(o_rgb)) ** 2)))
        print(case, "vs oracle: max abs", err, "rmse", rms, "scale", scale)
        if case == "box":
            assert np.array_equal(bits(rgb), bits(o_rgb))
        elif case == "photon":
            assert err <= PHOTON_REL_MAX_TOL * float(np.abs(o_rgb).max())
        else:
            assert err <= MAXABS_TOL * scale and rms <= RMSE_TOL * scale
    finally:
        for c in (ctx, fresh):
            c.set_option("coop", 1)


def first_point_light(blob):
    from qaray_amd import hip
    lights = hip.blob_table(blob, "lights")
    idx = [i for i in range(len(lights)) if lights[i]["type"] == U.QA_LIGHT_POINT]
    assert idx
    return idx[0], lights


@pytest.mark.parametrize("case", ["caustics_c4", "tower_c5"])
def test_plan_changing_edits(ctx, fresh, case):
    """A point light of a cooperative scene becomes an area light (the AREA variant and its hit-log slab), a point light again,
    then ambient (no shadow-casting light left): kernel name and frame are the fresh upload's every time."""
    scene, size, spp, _ = families()[case]
    a = blob_a(scene, size)
    region = (0, 0) + size
    ctx.upload_scene(a)
    builds, allocs = ctx.scene_stats()[:2]
    names = []
    work = a.copy()
    i, lights = first_point_light(work)
    steps = (("size", np.float32(0.75)), ("size", np.float32(0.0)), ("type", np.int32(U.QA_LIGHT_AMBIENT)))
    for k, (field, value) in enumerate(steps):
        lights[i][field] = value
        ctx.edit_lights(i, lights[i:i + 1])
        fresh.upload_scene(work)
        assert ctx.kernel_name() == fresh.kernel_name()
        assert same(ctx.render_region(region, spp), fresh.render_region(region, spp)), (case, field)
        assert ctx.kernel_name() == fresh.kernel_name()
        names.append(ctx.kernel_name())
        assert np.array_equal(ctx.download_scene(), work)
        # the area light's slab is the one allocation, made once
        assert ctx.scene_stats()[1] == allocs + 1
    assert "AREA=1" in names[0] and "AREA=1" not in names[1] and "AREA=1" not in names[2], names
    assert ctx.scene_stats()[0] == builds, "an edit ran the per-mesh builder"


@pytest.mark.parametrize("case", ["caustics_c4", "tower_c5", "object_textured"])
def test_edits_on_the_staged_integrator(ctx, fresh, tmp_path, case):
    scene, size, spp, _ = families()[case]
    a = blob_a(scene, size)
    b, camera, records, _ = U.scene_b(scene, size, tmp_path)
    region = (0, 0) + size
    try:
        for c in (ctx, fresh):
            c.set_pipeline("staged")
        ctx.upload_scene(a)
        frame_a = ctx.render_region(region, spp)
        assert "staged" in ctx.kernel_name()
        U.apply_edits(ctx, camera, records)
        fresh.upload_scene(b)
        assert ctx.kernel_name() == fresh.kernel_name()
        f1, c1 = frame_and_counters(ctx, region, spp)
        f2, c2 = frame_and_counters(fresh, region, spp)
        assert "staged" in ctx.kernel_name() and ctx.kernel_name() == fresh.kernel_name()
        assert same(f1, f2) and c1 == c2 and not same(f1, frame_a)
        # ... and the megakernel renders the same bits of the edited scene
        ctx.set_pipeline("mega")
        assert same(ctx.render_region(region, spp), f1)
    finally:
        for c in (ctx, fresh):
            c.set_pipeline("auto")


@pytest.mark.parametrize("case", ["box", "tower_c5"])
def test_progressive_frame_goes_stale_and_restarts_in_place(ctx, fresh, tmp_path, case):
    scene, size, spp, _ = families()[case]
    a = blob_a(scene, size)
    b, camera, records, _ = U.scene_b(scene, size, tmp_path)
    region = (0, 0) + size
    ctx.upload_scene(a)
    one_a = ctx.render_region(region, 4)
    fresh.upload_scene(b)
    want = fresh.render_region(region, spp)
    from qaray_amd import hip
    with ctx.progressive(region, spp) as prog:
        prog.advance(4)
        # enqueued right behind the pass, nothing waited for: the pass renders A
        ctx.edit_camera(camera)
        allocs = ctx.scene_stats()[1]
        with pytest.raises(hip.HipError) as e:
            prog.advance(8)
        assert e.value.code == QA_EINVAL and "edited" in str(e.value)
        assert same(prog.read(), one_a)
        assert prog.status()["spp_reached"] == 4
        prog.display()
        U.apply_edits(ctx, camera, records)
        assert same(prog.read(), one_a)
        prog.restart()
        st = prog.status()
        assert st == {"spp_reached": 0, "pixels_finished": 0, "tiles_behind": 0}, st
        assert not prog.read()[2].any()
        for s in (1, 4, spp):
            prog.advance(s)
        assert same(prog.read(), want)
        st = prog.status()
        assert st["spp_reached"] == spp and st["pixels_finished"] == size[0] * size[1]
        assert ctx.scene_stats()[1] == allocs
    assert same(ctx.render_region(region, spp), want)


def test_photon_maps_survive_a_camera_edit_only(ctx, fresh, tmp_path):
    from qaray_amd import hip
    scene, size, spp, _ = families()["photon"]
    a = blob_a(scene, size)
    b, camera, records, _ = U.scene_b(scene, size, tmp_path)
    region = (0, 0) + size
    ctx.upload_scene(a)
    ctx.build_photon_maps(*PHOTON_MAPS)
    info = ctx.photon_maps_info()
    maps = [ctx.download_photon_map(k).tobytes() for k in (0, 1)]
    ctx.edit_camera(camera)
    assert ctx.photon_maps_info() == info
    assert [ctx.download_photon_map(k).tobytes() for k in (0, 1)] == maps
    cam_only = a.copy()
    hip.blob_camera(cam_only)[...] = camera
    assert np.array_equal(ctx.download_scene(), cam_only)
    fresh.upload_scene(cam_only)
    fresh.build_photon_maps(*PHOTON_MAPS)
    f1 = ctx.render_region(region, spp)
    assert "photon-map gathers" in ctx.kernel_name()
    assert same(f1, fresh.render_region(region, spp))
    # a light edit drops the maps as an upload does (qa_photon_maps_clear's contract: Scene::usePhotonMap = false again):
    # the next frame renders without them, and the maps are gone
    ctx.edit_lights(*records["lights"])
    with pytest.raises(Exception, match="no photon maps"):
        ctx.photon_maps_info()
    light_only = cam_only.copy()
    i, rec = records["lights"]
    hip.blob_table(light_only, "lights")[i:i + 1] = rec
    fresh.upload_scene(light_only)
    f2 = ctx.render_region(region, spp)
    assert "photon-map gathers" not in ctx.kernel_name()
    assert same(f2, fresh.render_region(region, spp))
    # ... and can be built again for the edited scene
    ctx.build_photon_maps(*PHOTON_MAPS)
    fresh.build_photon_maps(*PHOTON_MAPS)
    assert ctx.photon_maps_info() == fresh.photon_maps_info()
    assert same(ctx.render_region(region, spp), fresh.render_region(region, spp))


def test_refused_edits_change_nothing(tmp_path):
    from qaray_amd import hip
    scene, size, spp, _ = families()["object_textured"]
    a = blob_a(scene, size)
    region = (0, 0) + size
    c = hip.Context(0)
    try:
        lights = hip.blob_table(a.copy(), "lights")
        with pytest.raises(hip.HipError) as e:
            c.edit_lights(0, lights[:1])
        assert e.value.code == QA_ENOSCENE
        with pytest.raises(hip.HipError) as e:
            c.edit_camera(hip.blob_camera(a.copy()))
        assert e.value.code == QA_ENOSCENE
        with pytest.raises(hip.HipError) as e:
            c.download_scene()
        assert e.value.code == QA_ENOSCENE
        c.upload_scene(a)
        frame_a = c.render_region(region, spp)
        stats = c.scene_stats()
        name = c.kernel_name()

        def refused(fn, first, records):
            with pytest.raises(hip.HipError) as e:
                fn(first, records)
            assert e.value.code == QA_EINVAL, e.value
            assert np.array_equal(c.download_scene(), a)
            assert c.scene_stats() == stats
            assert same(c.render_region(region, spp), frame_a)

        mats = hip.blob_table(a.copy(), "materials")
        textured = [i for i in range(len(mats)) if mats[i]["diffuse"]["texmap"] >= 0]
        assert textured
        m = mats[textured[0]:textured[0] + 1].copy()
        m[0]["diffuse"]["texmap"] = -1
        refused(c.edit_materials, textured[0], m)
        m = mats[:1].copy()
        m[0]["reflection"]["texmap"] = 0 if m[0]["reflection"]["texmap"] < 0 else -1
        refused(c.edit_materials, 0, m)
        inst = hip.blob_table(a.copy(), "instances")
        meshes = [k for k in range(len(inst)) if inst[k]["obj_type"] == 3]
        for field, value in (("mesh", inst[meshes[0]]["mesh"] + 1), ("parent", meshes[0] - 1 if inst[meshes[0]]["parent"] == 0 else 0),
                             ("obj_type", 1), ("depth", 2), ("mtlset", -1), ("subtree_end", len(inst))):
            r = inst[meshes[0]:meshes[0] + 1].copy()
            if r[0][field] == value:
                value = value + 1
            r[0][field] = value
            refused(c.edit_instances, meshes[0], r)
        refused(c.edit_lights, len(lights), lights[:1])
        refused(c.edit_lights, len(lights) - 1, lights[:2])
        refused(c.edit_instances, 0xFFFFFFFF, inst[:2])
        refused(c.edit_materials, len(mats) - 1, mats[:2])
        assert c.kernel_name() == name
    finally:
        c.close()


def test_frames_after_an_edit_do_not_depend_on_scratch_contents(tmp_path):
    from qaray_amd import hip
    scene, size, spp, _ = families()["tower_c5"]
    a = blob_a(scene, size)
    _, camera, records, _ = U.scene_b(scene, size, tmp_path)
    c = hip.Context(0)
    try:
        c.upload_scene(a)
        c.render_region((0, 0) + size, spp)
        U.apply_edits(c, camera, records)
        frames = []
        for pattern in (0x00000000, 0xFFFFFFFF):
            c.scrub_scratch(pattern)
            frames.append(c.render_region((0, 0) + size, spp))
        assert same(frames[0], frames[1]), c.kernel_name()
    finally:
        c.close()
