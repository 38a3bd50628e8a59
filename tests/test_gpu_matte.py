"""The matte planes (qa_matte_region*, qa_progressive_matte_device, qa_matte_rgba_device: qa_matte.hip) against the first-hit
planes, the CPU oracle's frames of the scene's two twins, the ray queries and the host build of qa_matte_dev.h.  Frames of 64x48,
the odd region (5, 3) - (52, 43), spp 1, 4 and 5.  Scenes: gbuffer_util's (one per <RES, TEX> instantiation), the sphere scene and
a teapot view from further back; matte_util.MATTE_SCENES says which must show silhouettes inside the region, and
needs_silhouettes() asserts that they do before a comparison relies on partly covered pixels."""
import functools
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT
from matte_util import (F32, MATTE_SCENES, MIN_PARTIAL, REGION, SIZE, SPHERES, SPPS, TEAPOT_FAR, bits, black_twin, emission_twin, linear_byte,
                        matte_blob, oracle_hits, rgba_edge_frames, running_mean_planes)

pytestmark = pytest.mark.gpu
QA_EINVAL = -1
QA_EUNSUPPORTED = -6
MISS = F32(1.0e30)
DOF_SCENE = "custom_softshadow.xml"
H, W = REGION[3] - REGION[1], REGION[2] - REGION[0]
PLANES = ("coverage", "albedo", "normal", "backdrop")
SCENE_IDS = [os.path.basename(s) for s in MATTE_SCENES]   # (two scenes are named by their path under tests/golden)


def fresh(blob):
    from qaray_amd import hip
    c = hip.Context(0)
    c.set_option("coop", 0)   # (kernel_name() then names qa_integrate<RES=..,TEX=..> for every scene)
    c.upload_scene(blob)
    return c


def same(a, b):
    return all(np.array_equal(bits(a[k]), bits(b[k])) for k in PLANES)


@functools.lru_cache(maxsize=None)
def blob_of(scene):
    return matte_blob(scene)


@functools.lru_cache(maxsize=None)
def twin_frame(scene, which, spp):
    """The oracle's frame (rgb, float32) of a twin of the scene at no bounce, computed once"""
    from oracle import binding as oracle
    twin = emission_twin(blob_of(scene)) if which == "emission" else black_twin(blob_of(scene))
    return oracle.render(twin, REGION, spp, max_bounce=0)[0].astype(F32)


@functools.lru_cache(maxsize=None)
def partial_mask(scene, spp):
    miss = oracle_hits(blob_of(scene), REGION, spp)
    return (miss > 0) & (miss < 1)


def needs_silhouettes(scene):
    """The condition without which the comparisons at 4 and 5 spp would pass on hit-or-miss pixels alone"""
    if MATTE_SCENES[scene]:
        n = int(partial_mask(scene, 5).sum())
        print(scene, "partly covered pixels at 5 spp:", n, "at 4 spp:", int(partial_mask(scene, 4).sum()))
        assert n >= MIN_PARTIAL, (scene, n)


@pytest.fixture(scope="module")
def planes():
    """scene -> dict: spp -> the four planes of REGION (host variant), "gbuffer" -> the first-hit planes, "rays" -> spp -> (hit
    [h, w, spp], normal [h, w, spp, 3]) of cast_rays_device over camera_sample_rays_device, "name" -> the kernel name"""
    out = {}
    for scene in MATTE_SCENES:
        c = fresh(blob_of(scene))
        try:
            d = {spp: c.matte(REGION, spp) for spp in SPPS}
            d["gbuffer"] = c.gbuffer(REGION)
            d["name"] = c.kernel_name()
            d["rays"] = {}
            for spp in SPPS[1:]:
                r = c.camera_sample_rays_device(REGION, 0, spp, outputs=("origins", "dirs"))
                hit = c.cast_rays_device(r["origins"].reshape(-1, 3), r["dirs"].reshape(-1, 3))
                c.synchronize()
                d["rays"][spp] = (hit["t"].cpu().numpy().reshape(H, W, spp) != MISS, hit["normal"].cpu().numpy().reshape(H, W, spp, 3))
            out[scene] = d
        finally:
            c.close()
    return out


def test_every_instantiation_is_reached_with_silhouettes(planes):
    seen = set()
    for scene in MATTE_SCENES:
        name = planes[scene]["name"]
        got = (int("RES=1" in name), int("TEX=1" in name))
        if MATTE_SCENES[scene]:
            needs_silhouettes(scene)
            seen.add(got)
    assert "RES=0" in planes[TEAPOT_FAR]["name"] and "TEX=0" in planes[TEAPOT_FAR]["name"]
    assert seen == {(0, 0), (0, 1), (1, 0), (1, 1)}, seen


@pytest.mark.parametrize("scene", list(MATTE_SCENES), ids=SCENE_IDS)
def test_one_sample_is_the_first_hit_planes(planes, scene):
    m, g = planes[scene][1], planes[scene]["gbuffer"]
    hit = g["depth"] != MISS
    assert np.array_equal(bits(m["albedo"]), bits(g["albedo"])) and np.array_equal(bits(m["normal"]), bits(g["normal"]))
    assert np.array_equal(m["coverage"], hit.astype(F32))
    assert np.array_equal(bits(m["backdrop"])[~hit], bits(g["albedo"])[~hit]) and not bits(m["backdrop"])[hit].any()


@pytest.mark.parametrize("spp", SPPS[1:])
@pytest.mark.parametrize("scene", list(MATTE_SCENES), ids=SCENE_IDS)
def test_albedo_is_the_emission_twins_frame(planes, scene, spp):
    needs_silhouettes(scene)
    want = twin_frame(scene, "emission", spp)
    got = planes[scene][spp]["albedo"]
    bad = np.argwhere(bits(got) != bits(want))
    assert len(bad) == 0, (scene, spp, len(bad), bad[:5])
    if MATTE_SCENES[scene]:   # ... on partly covered pixels too, which are neither the hit's nor the miss's colour
        part = partial_mask(scene, spp)
        assert part.sum() >= MIN_PARTIAL and np.array_equal(bits(got)[part], bits(want)[part])


@pytest.mark.parametrize("spp", SPPS[1:])
@pytest.mark.parametrize("scene", list(MATTE_SCENES), ids=SCENE_IDS)
def test_backdrop_is_the_black_twins_frame(planes, scene, spp):
    needs_silhouettes(scene)
    want = twin_frame(scene, "black", spp)
    got = planes[scene][spp]["backdrop"]
    assert np.array_equal(got, want), (scene, spp)
    nz = want != 0
    assert np.array_equal(bits(got)[nz], bits(want)[nz])
    cov = planes[scene][spp]["coverage"]
    assert not got[cov == 1].any()


@pytest.mark.parametrize("spp", SPPS[1:])
@pytest.mark.parametrize("scene", list(MATTE_SCENES), ids=SCENE_IDS)
def test_coverage_and_normal_are_the_ray_queries_reduced(planes, scene, spp):
    needs_silhouettes(scene)
    hit, normal = planes[scene]["rays"][spp]
    hits = hit.sum(axis=2)
    m = planes[scene][spp]
    assert np.array_equal(bits(m["coverage"]), bits(hits.astype(F32) / F32(spp))), scene
    assert np.array_equal((hits > 0) & (hits < spp), partial_mask(scene, spp))   # the oracle counts the same silhouettes
    want = running_mean_planes(np.moveaxis(normal, 2, 0), np.moveaxis(hit, 2, 0))
    assert np.array_equal(bits(m["normal"]), bits(want)), scene
    assert not bits(m["normal"])[hits == 0].any()


def test_an_ns_plane_gives_each_pixel_its_own_count(planes):
    import torch
    blob = blob_of(SPHERES)
    c = fresh(blob)
    try:
        ns = c.render_region(REGION, 4, spp_max=32)[2]
        counts = [int(k) for k in np.unique(ns)]
        print("sample counts of the adaptive frame:", counts)
        assert len(counts) >= 2 and min(counts) >= 4 and max(counts) <= 32
        got = c.matte(REGION, 32, ns=ns)
        for k in counts:
            at = c.matte(REGION, k)
            for p in PLANES:
                assert np.array_equal(bits(got[p])[ns == k], bits(at[p])[ns == k]), (k, p)
        # a synthetic plane: zeros, counts below spp, at it and far above it
        rng = np.random.default_rng(5)
        syn = rng.choice(np.array([0, 3, 5, 9, 2 ** 31, 2 ** 32 - 1], np.uint32), size=(H, W))
        host = c.matte(REGION, 5, ns=syn)
        dev = c.matte_device(REGION, 5, ns=torch.from_numpy(syn.view(np.int32)).cuda())
        c.synchronize()
        dev = {k: v.cpu().numpy() for k, v in dev.items()}
        assert same(host, dev)
        at3, at5 = c.matte(REGION, 3), planes[SPHERES][5]
        for p in PLANES:
            assert not bits(host[p])[syn == 0].any(), p
            assert np.array_equal(bits(host[p])[syn == 3], bits(at3[p])[syn == 3]), p
            assert np.array_equal(bits(host[p])[syn >= 5], bits(at5[p])[syn >= 5]), p
        assert same(c.matte(REGION, 5), at5)
    finally:
        c.close()


def test_progressive_matte_follows_the_frames_own_counts():
    c = fresh(blob_of(SPHERES))
    try:
        with c.progressive(REGION, 8) as prog:
            prog.advance(2)
            for limit, target in ((7, 5), (4, 8)):   # passes ended early: tiles at 2 and 5, then at 2, 5 and 8 (finished)
                c.set_option("progressive_tile_limit", limit)
                prog.advance(target)
                c.set_option("progressive_tile_limit", 0)
                ns = prog.read()[2]
                assert len(np.unique(ns)) >= 2, np.unique(ns)
                dev = prog.matte_device()
                c.synchronize()
                dev = {k: v.cpu().numpy() for k, v in dev.items()}
                assert same(dev, c.matte(REGION, 8, ns=ns)), target
            assert (ns == 8).any() and (ns == 2).any()
    finally:
        c.set_option("progressive_tile_limit", 0)
        c.close()


@pytest.mark.parametrize("scene", [SPHERES, "custom_textures.xml"])
def test_a_sub_region_cut_inside_a_tile_is_the_whole_regions_block(planes, scene):
    x0, y0 = REGION[0] + 3, REGION[1] + 5
    sub = (x0, y0, x0 + 27, y0 + 17)
    c = fresh(blob_of(scene))
    try:
        got = c.matte(sub, 5)
    finally:
        c.close()
    for p in PLANES:
        assert np.array_equal(bits(got[p]), bits(planes[scene][5][p][5:22, 3:30])), p


def test_after_edits_the_planes_are_those_of_the_edited_blob(planes):
    from qaray_amd import hip
    from qaray_amd.host import HostScene, SCENES_DIR
    blob = blob_of(SPHERES)
    hs = HostScene(os.path.join(SCENES_DIR, SPHERES), size=SIZE)
    cam0 = hip.blob_camera(blob)
    hs.set_camera(cam0["cam_pos"] + F32([3.0, 0.0, 2.0]), (0.0, 0.0, 5.0), up=(0, 0, 1))
    c = fresh(blob)
    try:
        c.edit_camera(hs.camera())
        mats = hip.blob_table(blob, "materials").copy()
        mats[0]["diffuse"]["color"] = F32([0.1, 0.7, 0.3])
        c.edit_materials(0, mats[0:1])
        bg = hip.blob_backdrop(blob)[0].copy()
        bg["color"] = F32([0.25, 0.5, 0.75])
        c.edit_backdrop(background=bg)
        got = c.matte(REGION, 5)
        edited = c.download_scene()
    finally:
        c.close()
        hs.close()
    c2 = fresh(edited)
    try:
        want = c2.matte(REGION, 5)
    finally:
        c2.close()
    assert same(got, want)
    old = planes[SPHERES][5]
    assert not np.array_equal(old["coverage"], want["coverage"]) and not np.array_equal(old["backdrop"], want["backdrop"])
    assert not np.array_equal(old["albedo"], want["albedo"])


def test_refusals_write_nothing_and_the_call_leaves_frames_and_counters_alone(planes):
    import torch
    from qaray_amd import hip
    L = hip.lib()
    c = fresh(blob_of(SPHERES))
    try:
        frame0 = c.render_region(REGION, 2)
        cnt0 = c.counters()
        t = {k: torch.full((H, W) if k == "coverage" else (H, W, 3), 7.0, dtype=torch.float32, device="cuda:0") for k in PLANES}
        ptr = [t[k].data_ptr() for k in PLANES]
        untouched = lambda: (c.synchronize(), torch.cuda.synchronize(), all(bool((v == 7).all()) for v in t.values()))[2]   # noqa: E731
        assert L.qa_matte_region_device(c._h, *REGION, 5, None, None, None, None, None, None) == QA_EINVAL      # no plane
        assert L.qa_matte_region_device(c._h, *REGION, 0, None, *ptr, None) == QA_EINVAL                          # spp = 0
        for bad in ((5, 3, 5, 43), (5, 3, 52, 3), (-1, 0, 10, 10), (0, 0, SIZE[0] + 1, 10), (0, 0, 10, SIZE[1] + 1)):
            assert L.qa_matte_region_device(c._h, *bad, 5, None, *ptr, None) == QA_EINVAL, bad
            with pytest.raises(hip.HipError) as e:
                c.matte(bad, 5)
            assert e.value.code == QA_EINVAL
        host = np.full(64, 7, F32)
        assert L.qa_matte_region(c._h, -1, 0, 1 << 30, 1 << 30, 5, None, host.ctypes.data, None, None, None) == QA_EINVAL   # (nothing is sized by it)
        assert L.qa_matte_region(c._h, 0, 0, 8, 8, 0, None, host.ctypes.data, None, None, None) == QA_EINVAL
        assert (host == 7).all() and untouched()
        # single planes are the full call's, and nothing a frame depends on moved
        for k in PLANES:
            one = c.matte_device(REGION, 5, **{k: t[k]})
            c.synchronize()
            assert list(one) == [k] and np.array_equal(bits(one[k].cpu().numpy()), bits(planes[SPHERES][5][k])), k
        assert c.counters() == cnt0
        frame1 = c.render_region(REGION, 2)
        assert all(np.array_equal(bits(a), bits(b)) for a, b in zip(frame0, frame1))
    finally:
        c.close()
    # a camera with depth of field
    d = fresh(matte_blob(DOF_SCENE))
    try:
        assert float(hip.blob_camera(matte_blob(DOF_SCENE))["dof"]) > 0.1
        t = torch.full((H, W), 7.0, dtype=torch.float32, device="cuda:0")
        with pytest.raises(hip.HipError) as e:
            d.matte_device(REGION, 5, coverage=t)
        assert e.value.code == QA_EUNSUPPORTED
        with pytest.raises(hip.HipError) as e:
            d.matte(REGION, 5)
        assert e.value.code == QA_EUNSUPPORTED
        with d.progressive(REGION, 2) as prog:
            prog.advance(1)
            with pytest.raises(hip.HipError) as e:
                prog.matte_device(coverage=t)
            assert e.value.code == QA_EUNSUPPORTED
        d.synchronize()
        torch.cuda.synchronize()
        assert bool((t == 7).all())
    finally:
        d.close()


@pytest.mark.parametrize("srgb", [True, False])
def test_rgba_device_is_the_host_functions_bytes(planes, srgb):
    import torch
    from qaray_amd import hip
    c = fresh(blob_of("custom_textures.xml"))
    try:
        up = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.int32) if a.dtype == np.uint32 else np.ascontiguousarray(a)).cuda()   # noqa: E731
        # a rendered frame with its own matte, adaptive counts included
        rgb, _, ns = c.render_region(REGION, 4, spp_max=8)
        m = c.matte(REGION, 8, ns=ns)
        got = c.rgba_device(up(rgb), up(m["backdrop"]), up(m["coverage"]), up(ns), srgb)
        c.synchronize()
        want = hip.matte_rgba_host(rgb, m["backdrop"], m["coverage"], ns, srgb)
        assert got.shape == (H, W, 4) and np.array_equal(got.cpu().numpy(), want)
        assert len(np.unique(want[..., 3])) >= 3 and (want[..., 3] == 255).any()   # silhouettes have alphas in between
        # the CPU test's edge frames; an output that is not dword-aligned takes the byte path
        for name, (e_rgb, e_back, e_cov, e_ns) in rgba_edge_frames().items():
            want = hip.matte_rgba_host(e_rgb, e_back, e_cov, e_ns, srgb)
            got = c.rgba_device(up(e_rgb), up(e_back), up(e_cov), up(e_ns), srgb)
            raw = torch.zeros(want.size + 1, dtype=torch.uint8, device="cuda:0")
            odd = c.rgba_device(up(e_rgb), up(e_back), up(e_cov), up(e_ns), srgb, out=raw[1:].view(want.shape))
            c.synchronize()
            assert np.array_equal(got.cpu().numpy(), want), name
            assert np.array_equal(odd.cpu().numpy(), want) and int(raw[0]) == 0, name
    finally:
        c.close()


def test_the_foreground_does_not_depend_on_the_backdrop():
    """rgb - backdrop of two frames that differ in the background colour alone: within 8 * spp * 2^-24 * M, M the largest component
    involved - three running means (rgb, backdrop, and the foreground they both carry) of at most spp roundings of at most one ulp of
    M each, doubled."""
    from qaray_amd import hip
    spp = 5
    blob = blob_of(SPHERES)
    c = fresh(blob)
    try:
        fg, big = [], 0.0
        for colour in ((0.25, 0.5, 0.75), (0.9, 0.1, 0.3)):
            bg = hip.blob_backdrop(blob)[0].copy()
            assert int(bg["texmap"]) < 0   # a plain background
            bg["color"] = F32(colour)
            c.edit_backdrop(background=bg)
            rgb = c.render_region(REGION, spp)[0]
            back = c.matte(REGION, spp)["backdrop"]
            assert (back != 0).any() and np.isfinite(rgb).all()
            fg.append(rgb.astype(np.float64) - back.astype(np.float64))
            big = max(big, float(np.abs(rgb).max()), float(np.abs(back).max()))
        err = float(np.abs(fg[0] - fg[1]).max())
        bound = 8 * spp * 2.0 ** -24 * big
        print("largest foreground difference", err, "bound", bound, "M", big)
        assert err <= bound, (err, bound)
    finally:
        c.close()


def test_cli_alpha_writes_a_fourth_image_and_leaves_the_three(tmp_path):
    from PIL import Image
    from qaray_amd.host import SCENES_DIR, load_scene_blob
    exe = os.path.join(ROOT, "qaray_amd", "lib", "qaray_hip")
    size = (48, 36)
    common = ["-batch", "-spp", "4", "-bounce", "5", "-size", str(size[0]), str(size[1]), "-root", SCENES_DIR]
    names = ("colorBuffer.png", "depthBuffer.png", "sampleBuffer.png")
    run = lambda args: subprocess.run([exe] + common + args, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)   # noqa: E731
    outs = {}
    for mode, extra in (("plain", []), ("alpha", ["-alpha"]), ("prog", ["-alpha", "-progressive", "2"])):
        outs[mode] = str(tmp_path / mode) + "_"
        r = run(extra + ["-out", outs[mode], os.path.join(SCENES_DIR, SPHERES)])
        assert r.returncode == 0, r.stdout
    assert not os.path.exists(outs["plain"] + "rgbaBuffer.png")
    for mode in ("alpha", "prog"):
        for png in names:
            with open(outs["plain"] + png, "rb") as a, open(outs[mode] + png, "rb") as b:
                assert a.read() == b.read(), (mode, png)
    img = Image.open(outs["alpha"] + "rgbaBuffer.png")
    assert img.mode == "RGBA" and img.size == size
    rgba = np.asarray(img)
    c = fresh(load_scene_blob(SPHERES, size=size))
    try:
        coverage = c.matte((0, 0) + size, 4)["coverage"]
    finally:
        c.close()
    assert np.array_equal(rgba[..., 3], linear_byte(coverage))
    assert ((rgba[..., 3] > 0) & (rgba[..., 3] < 255)).any()
    with open(outs["alpha"] + "rgbaBuffer.png", "rb") as a, open(outs["prog"] + "rgbaBuffer.png", "rb") as b:
        assert a.read() == b.read()
    r = run(["-alpha", "-devices", "1", os.path.join(SCENES_DIR, SPHERES)])
    assert r.returncode != 0 and "-alpha" in r.stdout and "-devices" in r.stdout
    r = run(["-alpha", "-out", str(tmp_path / "dof") + "_", os.path.join(SCENES_DIR, DOF_SCENE)])
    assert r.returncode != 0 and "-alpha" in r.stdout and "depth of field" in r.stdout
    assert not os.path.exists(str(tmp_path / "dof") + "_colorBuffer.png")
